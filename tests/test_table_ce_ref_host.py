"""Softmax cross-entropy over the full entity table (include/mgcn_hip.h (20)) without a GPU: the float64 reference of
tests/table_ce_ref.py against torch.nn.functional.cross_entropy with probability targets, the shards' statistics merged to the
whole row's, the measured ratio behind the bars, wrong conventions leaving the bars, the header and the exports, the argument
checks of the C ABI (all of which precede the first HIP call) and the refusals of the public surface."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as Fn

from . import cand_ce_ref as L
from . import dense_ref as R
from . import table_ce_ref as T
from .conftest import ROOT

NEW = ('mgcn_score_ce_tiles', 'mgcn_score_ce_partials', 'mgcn_score_ce_logits', 'mgcn_score_ce_finish')
F = ctypes.c_float


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('B,N,dim', [(8, 97, 7), (8, 33, 36), (5, 257, 4)])
def test_ref_table_ce_against_torch_cross_entropy(B, N, dim, eps):
    x, ent, bias, y = T.problem(B, N, dim, R.seed_of(81, B, N, dim))
    inv = 1.0 / B
    ref = T.ref_table_ce(x, ent, bias, y, eps, inv)
    xd, ed, bd = (t.double().requires_grad_(True) for t in (x, ent, bias))
    z = xd @ ed.t() + bd
    has = y.any(1)
    n_pos = y.sum(1).clamp(min=1)[:, None].double()
    q = (1.0 - eps) * y.double() / n_pos + eps / N
    assert float((q[has].sum(1) - 1.0).abs().max()) < 1e-12
    assert int(has.sum()) >= 2 and int((~has).sum()) >= 1 and int((y.sum(1) > 1).sum()) >= 1 and bool((y.sum(1) == N).any())
    total = Fn.cross_entropy(z[has], q[has], reduction='sum') * inv              # a row without a positive adds nothing, counts in B
    total.backward()
    assert abs(ref['loss'] - float(total.detach())) <= 1e-12 * max(1.0, abs(float(total.detach())))
    torch.testing.assert_close(ref['z'], z.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(ref['q'][has], q[has], rtol=0, atol=1e-15)
    torch.testing.assert_close(ref['dx'], xd.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref['d_ent'], ed.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref['d_bias'], bd.grad, rtol=1e-11, atol=1e-13)
    assert bool((ref['g'][~has] == 0).all()) and bool((ref['terms'][~has] == 0).all())
    assert float(ref['g'].sum(1)[has].abs().max()) < 1e-14                       # sum p = sum q = 1


@pytest.mark.parametrize('bounds', [[0, 97], [0, 31, 31, 97], [0, 33, 64, 97], [0, 0, 50, 97, 97]])
def test_shards_add_up_and_their_statistics_merge_to_the_whole_rows(bounds):
    B, N, dim, eps = 8, 97, 7, 0.1
    x, ent, bias, y = T.problem(B, N, dim, R.seed_of(82))
    whole = T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B)
    parts = [T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B, row0=a, n_local=e - a) for a, e in zip(bounds[:-1], bounds[1:])]
    assert abs(sum(p['loss'] for p in parts) - whole['loss']) <= 1e-12 * abs(whole['loss'])
    torch.testing.assert_close(sum(p['dx'] for p in parts), whole['dx'], rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(torch.cat([p['d_ent'] for p in parts]), whole['d_ent'], rtol=1e-12, atol=1e-15)     # (float64 sums in
    torch.testing.assert_close(torch.cat([p['d_bias'] for p in parts]), whole['d_bias'], rtol=1e-12, atol=1e-15)   # another blocking)
    stats = T.shard_stats64(x, ent, bias, y, bounds)
    for b in range(B):
        M, S, nl, npos = L.merge64(stats[b])
        assert (nl, npos) == (N, int(y[b].sum()))
        assert M == float(whole['M'][b]) and abs(S - float(whole['S'][b])) <= 1e-13 * float(whole['S'][b])
        # tiles of 32 inside a shard, then the shards: the same fold
        tiles = [T.shard_stats64(x[b:b + 1], ent[a:e], bias[a:e], y[b:b + 1, a:e], list(range(0, e - a, 32)) + [e - a])[0]
                 for a, e in zip(bounds[:-1], bounds[1:])]
        M2, S2, nl2, np2 = L.merge64([L.merge64(t) for t in tiles])
        assert (M2, nl2, np2) == (M, nl, npos) and abs(S2 - S) <= 1e-13 * S


def test_f32_emulation_agrees_with_the_reference_statistics():
    x, ent, bias, y = T.problem(8, 257, 36, R.seed_of(83))
    ref = T.ref_table_ce(x, ent, bias, y, 0.1, 1.0 / 8)
    M32, S32, lp32 = T.emul_lp_f32(ref['z'].float().numpy())
    assert float((torch.from_numpy(M32).double() - ref['M']).abs().max()) <= 2 * R.U * float(ref['M'].abs().max())
    assert float(((torch.from_numpy(S32).double() - ref['S']).abs() / ref['S']).max()) < 1e-5
    act = ref['act']
    assert float((torch.from_numpy(lp32).double() - ref['lp'])[act].abs().max()) < 1e-5


def test_measured_ratio_of_the_lse_term():
    worst, where = T.lse_worst()
    print('f32 tile-of-32-then-merge emulation: worst |err| / (u (1 + |lp|)) = %.3f at n, scale = %s (constant %.2f)' % (worst, where, T.C_LSE))
    assert worst <= T.C_LSE / 2, 'the emulation is within a factor 2 of C_LSE: re-measure LSE_RATIO_MEASURED (%.3f)' % worst
    assert worst >= T.LSE_RATIO_MEASURED / 2, 'LSE_RATIO_MEASURED went stale (%.3f measured)' % worst
    assert T.C_LSE == 4 * T.LSE_RATIO_MEASURED


def _ratios(ref, other, x, ent_shard, dim, inv, n_partials=8):
    """{quantity: worst |other - ref| / bar}."""
    _, rowbar = T.logit_bars(ref, dim)
    gb = T.g_bar(ref, rowbar, inv)
    dxb, deb, dbb = T.grad_bars(ref, x, ent_shard, rowbar, inv)
    return dict(g=float(((other['g'] - ref['g']).abs() / gb).max()),
                loss=abs(other['loss'] - ref['loss']) / T.loss_bar(ref, rowbar, inv, n_partials),
                dx=float(((other['dx'] - ref['dx']).abs() / dxb).max()),
                d_ent=float(((other['d_ent'] - ref['d_ent']).abs() / deb).max()),
                d_bias=float(((other['d_bias'] - ref['d_bias']).abs() / dbb).max()))


@pytest.mark.parametrize('convention', [c for c in T.CONVENTIONS if c != 'right'])
def test_wrong_conventions_leave_the_bars(convention):
    B, N, dim, eps, inv = 8, 97, 36, 0.1, 1.0 / 8
    x, ent, bias, y = T.problem(B, N, dim, R.seed_of(84))
    row0, n_local = (31, 40) if convention.startswith('local') else (0, N)          # a shard where the local quantities differ
    ref = T.ref_table_ce(x, ent, bias, y, eps, inv, row0=row0, n_local=n_local)
    sh = ent[row0:row0 + n_local]
    # the bars hold an f32 evaluation of the right convention (torch-CPU f32 log_softmax over the whole row) ...
    lp32 = torch.log_softmax((x @ ent.t() + bias).float(), 1).double()[:, row0:row0 + n_local]
    g32 = torch.where(ref['act'], (torch.exp(lp32) - ref['q']) * inv, torch.zeros_like(lp32))
    ok = dict(g=g32, loss=float((-(ref['q'] * torch.where(ref['act'], lp32, torch.zeros_like(lp32))) * inv).sum()),
              dx=g32 @ sh.double(), d_ent=g32.t() @ x.double(), d_bias=g32.sum(0))
    good = _ratios(ref, ok, x, sh, dim, inv)
    assert max(good.values()) <= 1.0, good
    # ... and every wrong convention leaves them by a wide factor
    bad = _ratios(ref, T.ref_table_ce(x, ent, bias, y, eps, inv, row0=row0, n_local=n_local, convention=convention), x, sh, dim, inv)
    print('%s: |wrong - right| / bar = %s' % (convention, ', '.join('%s %.3g' % kv for kv in sorted(bad.items()))))
    assert bad['g'] > 100 and bad['loss'] > 100 and max(bad['dx'], bad['d_ent'], bad['d_bias']) > 100, bad


def test_bars_are_positive():
    x, ent, bias, y = T.problem(8, 97, 36, R.seed_of(85))
    ref = T.ref_table_ce(x, ent, bias, y, 0.1, 1.0 / 8)
    zbar, rowbar = T.logit_bars(ref, 36)
    assert bool((zbar > 0).all()) and bool((rowbar[:, None] >= zbar).all())
    assert bool((T.lp_bar(ref, rowbar) > 0).all()) and bool((T.g_bar(ref, rowbar, 1.0 / 8) > 0).all()) and bool((T.lse_bar(ref, rowbar) > 0).all())
    assert T.loss_bar(ref, rowbar, 1.0 / 8, 16) > 0 and all(bool((b > 0).all()) for b in T.grad_bars(ref, x, ent, rowbar, 1.0 / 8))


def test_index_of_restates_the_known_tails(pkg):
    _, _, _, y = T.problem(8, 97, 4, R.seed_of(86))
    keys, ptr, tails = T.index_of(y)
    assert keys.tolist() == [b for b in range(8) if bool(y[b].any())] and ptr.numel() == keys.numel() + 1
    hit = R.ref_filter(torch.arange(8), keys, ptr, tails, 0, 97)
    assert torch.equal(hit.bool(), y)


def test_header_and_exports_name_the_new_entry_points(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    declared = set(re.findall(r'\b(mgcn_[a-z0-9_]+)\s*\(', header))
    handle = ctypes.CDLL(pkg._native.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._native.EXPORTS and hasattr(handle, name), name
    assert '(20) Softmax cross-entropy over the full entity table' in header
    lib = pkg._native.lib()
    assert lib.mgcn_abi_version() == 4
    assert [lib.mgcn_score_ce_tiles(n) for n in (-1, 0, 1, 32, 33, 2100)] == [0, 0, 1, 1, 2, 66]
    assert lib.mgcn_score_ce_partials(128, 40943) == 1280 * 2 and lib.mgcn_score_ce_partials(65, 33) == 4
    assert lib.mgcn_score_ce_partials(0, 33) == 0 and lib.mgcn_score_ce_partials(4, 0) == 0


def test_abi_argument_validation_without_a_gpu(pkg):
    """Every bad argument comes back as MGCN_EINVAL (1), a batch outside the acceptance rule as MGCN_EUNSUPPORTED (3), with a
    message before any HIP call; the fake pointers are never dereferenced."""
    lib = pkg._native.lib()
    N, P = None, 256

    def logits(batch=4, n=100, dim=8, x=P, ldx=8, ent=P, lde=8, bias=P, mask=P, ldm=4, z=P, ldz=4, stat=P, lds=4):
        return lib.mgcn_score_ce_logits(batch, n, dim, x, ldx, ent, lde, bias, mask, ldm, z, ldz, stat, lds, N)

    def finish(batch=4, n=100, z=P, ldz=4, mask=P, ldm=4, stat=P, eps=0.1, total=100, parts=P):
        return lib.mgcn_score_ce_finish(batch, n, z, ldz, mask, ldm, stat, F(eps), F(0.25), total, parts, N)

    big = (1 << 31) - 64
    cases = [
        (logits, 'score_ce_logits', [dict(x=N), dict(ent=N), dict(bias=N), dict(mask=N), dict(z=N), dict(stat=N), dict(ldx=7), dict(lde=7),
                                     dict(ldm=3), dict(ldz=3), dict(lds=3), dict(lds=1 << 40), dict(stat=P + 4), dict(batch=-1), dict(n=-1),
                                     dict(dim=0), dict(n=big, ldm=1 << 27), dict(batch=big, ldz=1 << 31, lds=1 << 31)]),
        (finish, 'score_ce_finish', [dict(z=N), dict(mask=N), dict(stat=N), dict(parts=N), dict(ldz=3), dict(ldm=3), dict(batch=-1),
                                     dict(n=-1), dict(eps=-0.5), dict(eps=1.5), dict(eps=float('nan')), dict(total=99), dict(total=0, n=0),
                                     dict(n=big, ldm=1 << 27, total=1 << 32), dict(batch=big, ldz=1 << 31)]),
    ]
    for fn, name, kws in cases:
        for kw in kws:
            rc = fn(**kw)
            msg = lib.mgcn_last_error().decode()
            assert rc == 1 and msg.startswith(name), (name, kw, rc, msg)
    for kw in (dict(batch=5, ldz=5, lds=5), dict(dim=6, ldx=6, lde=6), dict(x=P + 4), dict(ent=P + 4), dict(z=P + 4), dict(ldx=9), dict(lde=9),
               dict(ldz=5)):
        rc = logits(**kw)
        assert rc == 3 and lib.mgcn_last_error().decode().startswith('score_ce_logits'), (kw, rc)
    for fn in (logits, finish):
        for kw in (dict(batch=0), dict(n=0)):
            assert fn(**kw) == 0, (fn, kw)


def test_python_surface_needs_a_gpu_and_refuses_other_losses(pkg):
    nat = pkg._native
    x, ent, bias = torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(5)
    mask = torch.zeros((4, 1), dtype=torch.int32)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.score_ce_logits(x, ent, bias, mask)
    with pytest.raises(nat.NativeError, match='mask'):
        nat.score_ce_logits(x, ent, bias, mask[:3])
    with pytest.raises(nat.NativeError, match='stat'):
        nat.score_ce_finish(torch.zeros(5, 4), mask, torch.zeros(3, 4), 0.1, 5)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.score_ce_finish(torch.zeros(5, 4), mask, torch.zeros(4, 4), 0.1, 5)
    m = torch.tensor([[0, -1, -(1 << 31)], [5, 0, 0x0f0f0f0f]], dtype=torch.int32)
    assert nat.mask_popcount(m).tolist() == [33, 18] and nat.mask_popcount(m).dtype == torch.int32
    # the default everywhere is 'bce'
    for fn in (pkg.MGCN.forward_loss, pkg.harness.train_device_labels, pkg.captured.CapturedTrainStep.__init__, pkg.dist.train_step_sharded,
               pkg.dist.train_epoch_sharded):
        assert inspect.signature(fn).parameters['loss'].default == 'bce', fn
    # anything else is refused before any launch or collective: nothing here is on a GPU, and nothing is touched
    for bad in ('ce', 'Softmax', None, 1):
        with pytest.raises(nat.NativeError, match='loss must be'):
            pkg.MGCN.forward_loss(None, None, None, None, None, loss=bad)
        with pytest.raises(nat.NativeError, match='loss must be'):
            pkg.harness.train_device_labels(None, None, None, None, None, None, 4, loss=bad)
        with pytest.raises(nat.NativeError, match='loss must be'):
            pkg.dist.train_step_sharded(None, None, None, None, None, None, loss=bad)
        with pytest.raises(nat.NativeError, match='loss must be'):
            pkg.dist.train_epoch_sharded(None, None, None, None, None, None, 4, loss=bad)
        with pytest.raises(nat.NativeError, match='loss must be'):
            pkg.captured.CapturedTrainStep(None, None, None, None, loss=bad)._refuse(None)
    with pytest.raises(nat.NativeError, match='fused_loss'):
        pkg.harness.train_device_labels(None, None, None, None, None, None, 4, fused_loss=False, loss='softmax')
