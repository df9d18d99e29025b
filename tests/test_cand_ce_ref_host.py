"""Softmax cross-entropy over candidate lists (include/mgcn_hip.h (16)) without a GPU: the float64 reference of
tests/cand_ce_ref.py against torch.nn.functional.cross_entropy with probability targets, the merge's algebra (any cut of a row
into parts gives the row's statistic), the measured ratio behind the bars, the header and the exports, and the argument checks
of the C ABI (all of which precede the first HIP call)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as Fn

from . import cand_ce_ref as E
from . import dense_ref as R
from .conftest import ROOT

NEW = ('mgcn_cand_ce_partials', 'mgcn_cand_ce_logits', 'mgcn_cand_ce_merge', 'mgcn_cand_ce_finish')
F = ctypes.c_float


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('B,K,N,dim', [(8, 65, 97, 7), (8, 130, 97, 36), (5, 17, 33, 4)])
def test_ref_list_ce_against_torch_cross_entropy(B, K, N, dim, eps):
    x, ent, bias, cand, label = E.problem(B, K, N, dim, R.seed_of(71, B, K, N, dim))
    inv = 1.0 / B
    ref = E.ref_list_ce(x, ent, bias, cand, label, eps, inv)
    live, row = ref['live'], ref['row']
    xd, ed, bd = (t.double().requires_grad_(True) for t in (x, ent, bias))
    total, rows_with_a_term, multi = 0.0, 0, 0
    for b in range(B):
        lv = live[b]
        pos = label[b].bool() & lv
        if not bool(pos.any()):
            assert bool((ref['g'][b] == 0).all()) and bool((ref['terms'][b] == 0).all())     # no positive: nothing
            continue
        rows_with_a_term += 1
        multi += int(pos.sum()) > 1
        zb = (ed[row[b][lv]] * xd[b]).sum(1) + bd[row[b][lv]]
        q = (1.0 - eps) * pos[lv].double() / float(pos.sum()) + eps / float(lv.sum())
        assert abs(float(q.sum()) - 1.0) < 1e-12
        total = total + Fn.cross_entropy(zb[None], q[None]) * inv
        torch.testing.assert_close(ref['q'][b][lv], q, rtol=0, atol=1e-15)
        torch.testing.assert_close(ref['z'][b][lv], zb.detach(), rtol=1e-13, atol=1e-13)
    assert rows_with_a_term >= 2 and multi >= 1                                # shared mass among several known tails is exercised
    total.backward()
    assert abs(ref['loss'] - float(total.detach())) <= 1e-12 * max(1.0, abs(float(total.detach())))
    torch.testing.assert_close(ref['dx'], xd.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref['d_ent'], ed.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref['d_bias'], bd.grad, rtol=1e-11, atol=1e-13)
    assert bool((ref['g'][~live] == 0).all())
    # sum p = sum q = 1 on every row with a positive
    has = ref['n_pos'] > 0
    assert float(ref['g'].sum(1)[has].abs().max()) < 1e-14


def test_edge_rows_of_the_problem_builder():
    """problem() plants what the device grid needs, at a list of one chunk and of several."""
    for K in (63, 64, 65, 130, 257):
        x, ent, bias, cand, label = E.problem(8, K, 97, 4, R.seed_of(72, K))
        ref = E.ref_list_ce(x, ent, bias, cand, label, 0.1, 1.0 / 8)
        live, pos = ref['live'], label.bool() & ref['live']
        rows = {}
        for b in range(8):
            rows[b] = (int(live[b].sum()), int(pos[b].sum()))
        assert any(nl > 0 and npos == 0 for nl, npos in rows.values())                     # no positive
        assert any(nl == 0 for nl, _ in rows.values())                                     # all dead
        assert any(0 < nl < K and npos == nl for nl, npos in rows.values())                # all live positions positive, some dead
        last = min(64, K) - 1
        assert any(rows[b][0] == 1 and bool(live[b, last]) for b in rows)                  # only the last of a chunk
        if K > 64:
            assert any(rows[b][0] > 0 and not bool(live[b, :64].any()) for b in rows)      # the first chunk dead
        assert any(v >= 97 for v in cand.reshape(-1).tolist()) and (cand == -1).any() and (cand == 2 ** 62).any() and (cand == -2 ** 62).any()


def _close_stat(a, b):
    assert a[2:] == b[2:], (a, b)
    if a[0] == E.NINF or b[0] == E.NINF:
        assert a[:2] == b[:2] == (E.NINF, 0.0), (a, b)
        return
    assert a[0] == b[0], (a, b)
    assert abs(a[1] - b[1]) <= 1e-13 * abs(b[1]), (a, b)


@pytest.mark.parametrize('K,scale', [(1, 1.0), (65, 1.0), (130, 30.0), (257, 100.0)])
def test_any_cut_into_parts_merges_to_the_whole_row(K, scale):
    g = R.gen(R.seed_of(73, K))
    z = R.randn_scaled((K,), g, scale).double()
    live = torch.rand(K, generator=g) >= 0.2
    live[K // 2] = True
    pos = torch.rand(K, generator=g) < 0.3
    whole = E.stats64(z, live, pos)
    assert whole[2] == int(live.sum()) and whole[3] == int((pos & live).sum())
    cuts = [[0, K], [0, 0, K], [0, K, K], [0, 0, 0, K, K]]                     # one part; an empty first part; an empty last part
    cuts += [[0] + sorted(torch.randint(0, K + 1, (n,), generator=g).tolist()) + [K] for n in (1, 2, 5, 9)]
    cuts += [list(range(0, K, 64)) + [K]]                                      # the kernels' chunks
    for cut in cuts:
        parts = [E.stats64(z[a:b], live[a:b], pos[a:b]) for a, b in zip(cut[:-1], cut[1:])]
        _close_stat(E.merge64(parts), whole)
        # merging merged halves (chunks -> row, then rows of ranks -> global) is the same fold
        h = len(parts) // 2
        _close_stat(E.merge64([E.merge64(parts[:h]), E.merge64(parts[h:])]), whole)
    # a part whose positions are all dead contributes the empty statistic, wherever it stands
    dead = torch.zeros(K, dtype=torch.bool)
    assert E.stats64(z, dead, pos) == (E.NINF, 0.0, 0, 0)
    _close_stat(E.merge64([E.stats64(z, dead, pos), whole, E.stats64(z, dead, pos)]), whole)
    assert E.merge64([E.stats64(z, dead, pos)] * 3) == (E.NINF, 0.0, 0, 0)
    assert E.merge64([whole]) == whole                                          # one part: the identity


def test_f32_emulation_agrees_with_the_reference_statistics():
    x, ent, bias, cand, label = E.problem(8, 130, 97, 36, R.seed_of(74))
    ref = E.ref_list_ce(x, ent, bias, cand, label, 0.1, 1.0 / 8)
    M32, S32, lp32 = E.emul_lp_f32(ref['z'].float().numpy(), ref['live'].numpy())
    for b in range(8):
        if int(ref['n_live'][b]) == 0:
            assert M32[b] == -float('inf') and S32[b] == 0
            continue
        assert abs(float(M32[b]) - float(ref['M'][b])) <= 2 * R.U * abs(float(ref['M'][b]))
        assert abs(float(S32[b]) - float(ref['S'][b])) <= 1e-5 * float(ref['S'][b])
    act = ref['act']
    assert float((torch.from_numpy(lp32).double() - ref['lp'])[act].abs().max()) < 1e-5


def test_measured_ratio_of_the_lse_term():
    worst, where = E.lse_worst()
    print('f32 unit-then-merge emulation: worst |err| / (u (1 + |lp|)) = %.3f at K, scale = %s (constant %.2f)' % (worst, where, E.C_LSE))
    assert worst <= E.C_LSE / 2, 'the emulation is within a factor 2 of C_LSE: re-measure LSE_RATIO_MEASURED (%.3f)' % worst
    assert worst >= E.LSE_RATIO_MEASURED / 2, 'LSE_RATIO_MEASURED went stale (%.3f measured)' % worst
    assert E.C_LSE == 4 * E.LSE_RATIO_MEASURED


def test_bars_are_positive_and_scale_with_the_logits():
    x, ent, bias, cand, label = E.problem(8, 65, 97, 36, R.seed_of(75))
    ref = E.ref_list_ce(x, ent, bias, cand, label, 0.1, 1.0 / 8)
    zbar, rowbar = E.logit_bars(ref, 36)
    assert bool((E.lp_bar(ref, rowbar) > 0).all()) and bool((E.g_bar(ref, rowbar, 1.0 / 8) > 0).all())
    assert E.loss_bar(ref, rowbar, 1.0 / 8, 16) > 0
    # an f32 evaluation in another order (torch-CPU f32 log_softmax over the live subset) sits inside the lp bar
    lpb = E.lp_bar(ref, rowbar)
    for b in range(8):
        lv = ref['live'][b]
        if int(ref['n_pos'][b]) == 0:
            continue
        got = torch.log_softmax(ref['z'][b][lv].float(), 0).double()
        assert bool(((got - ref['lp'][b][lv]).abs() <= lpb[b][lv]).all())


def test_header_and_exports_name_the_new_entry_points(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    declared = set(re.findall(r'\b(mgcn_[a-z0-9_]+)\s*\(', header))
    handle = ctypes.CDLL(pkg._native.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._native.EXPORTS and hasattr(handle, name), name
    assert '(16) Softmax cross-entropy over per-query candidate lists' in header
    assert pkg._native.lib().mgcn_abi_version() == 4
    lib = pkg._native.lib()
    assert lib.mgcn_cand_ce_partials(128, 4096) == 128 * 64 and lib.mgcn_cand_ce_partials(3, 65) == 6
    assert lib.mgcn_cand_ce_partials(0, 65) == 0 and lib.mgcn_cand_ce_partials(3, 0) == 0
    assert lib.mgcn_cand_ce_partials(5, 257) == lib.mgcn_cand_bce_partials(5, 257)


def test_abi_argument_validation_without_a_gpu(pkg):
    """Every bad argument comes back as MGCN_EINVAL (1) with a message before any HIP call; the fake pointers are never
    dereferenced (every case fails validation or has nothing to do)."""
    lib = pkg._native.lib()
    N, P, Q = None, 256, 512

    def logits(batch=4, k=10, n=100, row0=0, dim=8, x=P, ldx=8, ent=P, lde=8, bias=P, cand=P, ldc=10, label=P, ldl=10, z=P, ldz=10, stat=P):
        return lib.mgcn_cand_ce_logits(batch, k, n, row0, dim, x, ldx, ent, lde, bias, cand, ldc, label, ldl, z, ldz, stat, N)

    def merge(batch=4, parts=3, src=P, row_stride=3, part_stride=1, out=Q):
        return lib.mgcn_cand_ce_merge(batch, parts, src, row_stride, part_stride, out, N)

    def finish(batch=4, k=10, n=100, row0=0, z=P, ldz=10, cand=P, ldc=10, label=P, ldl=10, stat=P, eps=0.1, g=P, ldg=10, parts=P):
        return lib.mgcn_cand_ce_finish(batch, k, n, row0, z, ldz, cand, ldc, label, ldl, stat, F(eps), F(0.25), g, ldg, parts, N)

    big = (1 << 31) - 64
    cases = [
        (logits, 'cand_ce_logits', [dict(x=N), dict(ent=N), dict(bias=N), dict(cand=N), dict(label=N), dict(z=N), dict(stat=N),
                                    dict(ldc=9), dict(ldl=9), dict(ldz=9), dict(ldx=7), dict(lde=7), dict(row0=-1), dict(batch=-1),
                                    dict(k=-1), dict(n=-1), dict(dim=0), dict(n=big), dict(batch=big),
                                    dict(k=big, ldc=1 << 31, ldl=1 << 31, ldz=1 << 31)]),
        (merge, 'cand_ce_merge', [dict(src=N), dict(out=N), dict(out=P), dict(batch=-1), dict(parts=0), dict(parts=-1), dict(row_stride=0),
                                  dict(part_stride=0), dict(row_stride=2), dict(row_stride=1, part_stride=3), dict(row_stride=1 << 40),
                                  dict(row_stride=5, part_stride=2), dict(batch=big), dict(parts=big, row_stride=1 << 32)]),
        (finish, 'cand_ce_finish', [dict(z=N), dict(cand=N), dict(label=N), dict(stat=N), dict(g=N), dict(parts=N), dict(ldz=9),
                                    dict(ldc=9), dict(ldl=9), dict(ldg=9), dict(row0=-1), dict(batch=-1), dict(k=-1), dict(n=-1),
                                    dict(eps=-0.5), dict(eps=1.5), dict(eps=float('nan')), dict(n=big), dict(batch=big),
                                    dict(k=big, ldz=1 << 31, ldc=1 << 31, ldl=1 << 31, ldg=1 << 31)]),
    ]
    for fn, name, kws in cases:
        for kw in kws:
            rc = fn(**kw)
            msg = lib.mgcn_last_error().decode()
            assert rc == 1 and msg.startswith(name), (name, kw, rc, msg)
    for fn in (logits, finish):
        for kw in (dict(batch=0), dict(k=0), dict(n=0)):
            assert fn(**kw) == 0, (fn, kw)
    assert merge(batch=0) == 0
    assert merge(batch=0, row_stride=1, part_stride=1) == 0


def test_python_surface_needs_a_gpu(pkg):
    nat = pkg._native
    x, ent, bias = torch.zeros(2, 8), torch.zeros(5, 8), torch.zeros(5)
    cand = torch.zeros((2, 3), dtype=torch.int64)
    label = torch.zeros((2, 3), dtype=torch.uint8)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.cand_ce_logits(x, ent, bias, cand, label)
    with pytest.raises(nat.NativeError, match='cand'):
        nat.cand_ce_logits(x, ent, bias, cand[:1], label)
    with pytest.raises(nat.NativeError, match='label'):
        nat.cand_ce_logits(x, ent, bias, cand, label[:, :2])
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.cand_ce_merge(torch.zeros(2, 3, 4))
    with pytest.raises(nat.NativeError, match='contiguous'):
        nat.cand_ce_merge(torch.zeros(2, 4))
    with pytest.raises(nat.NativeError, match='stat'):
        nat.cand_ce_finish(torch.zeros(2, 3), cand, label, torch.zeros(3, 4), 0.1, 5)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.cand_ce_finish(torch.zeros(2, 3), cand, label, torch.zeros(2, 4), 0.1, 5)
    empty = nat.cand_ce_empty_stat(3, 'cpu')
    m, s, nl, npos = nat.cand_ce_stat_fields(empty)
    assert bool((m == float('-inf')).all()) and bool((s == 0).all()) and nl.dtype == torch.int32 and not bool(nl.any()) and not bool(npos.any())
