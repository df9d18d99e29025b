"""Training on candidate lists (include/mgcn_hip.h (14)) without a GPU: the float64 reference of tests/cand_train_ref.py against
torch.nn.BCELoss + autograd, its numpy-f32 emulations of the two ordered sums against float64 within the standard summation
bound, _native.cand_plan and harness.sample_candidates on CPU tensors, the header and the exports, and the argument checks of
the C ABI (all of which precede the first HIP call)."""
import os
import re

import pytest
import torch

from . import cand_train_ref as C
from . import dense_ref as R
from .conftest import ROOT

NEW = ('mgcn_cand_labels', 'mgcn_cand_bce_partials', 'mgcn_cand_bce_fwd', 'mgcn_cand_bce_bwd_x', 'mgcn_cand_bce_bwd_ent')
DEAD = (-1, None, 2 ** 62, -2 ** 62)                  # None: N itself


def problem(B, K, N, dim, seed, row0=0, n_local=None, dead=True):
    g = R.gen(seed)
    n = N if n_local is None else n_local
    x, ent, bias = R.pm_uniform((B, dim), g), R.pm_uniform((n, dim), g), R.pm_uniform((n,), g)
    cand = C.lists(N, B, K, seed + 1)
    if dead:
        for i, v in enumerate(DEAD):
            cand[i % B, (3 * i + 1) % K] = N if v is None else v
    label = torch.rand((B, K), generator=g) < 0.3
    return x, ent, bias, cand, label


CASES = [(1, 1, 33, 4), (4, 15, 33, 7), (5, 65, 1000, 36), (36, 130, 33, 200), (4, 64, 1000, 36)]


@pytest.mark.parametrize('B,K,N,dim', CASES, ids=['%d-%d-%d-%d' % c for c in CASES])
def test_float64_reference_equals_bceloss_autograd_on_gathered_logits(B, K, N, dim):
    x, ent, bias, cand, label = problem(B, K, N, dim, R.seed_of(31, B, K, N, dim), dead=B * K > 4)
    hot, cold, inv = 0.9 + 1.0 / N, 1.0 / N, 1.0 / (B * K)
    ref = C.ref_list_bce(x, ent, bias, cand, label, hot, cold, inv)
    xd, ed, bd = (t.double().requires_grad_(True) for t in (x, ent, bias))
    live, row = ref['live'], ref['row']
    z = (ed[row] * xd[:, None, :]).sum(2) + bd[row]
    y = torch.where(label, torch.tensor(hot, dtype=torch.float64), torch.tensor(cold, dtype=torch.float64))
    loss = torch.nn.BCELoss(reduction='sum')(torch.sigmoid(z[live]), y[live]) * inv
    loss.backward()
    assert abs(ref['loss'] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    for got, want in ((ref['dx'], xd.grad), (ref['d_ent'], ed.grad), (ref['d_bias'], bd.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((ref['g'][~live] == 0).all())


@pytest.mark.parametrize('B,K,N,dim', CASES, ids=['%d-%d-%d-%d' % c for c in CASES])
def test_f32_emulations_within_the_summation_bound(B, K, N, dim):
    """|f32 sum - float64 sum| <= gamma_n sum |addends|, n the addends of that sum: derived, not chosen (cand_train_ref.gamma)."""
    x, ent, bias, cand, label = problem(B, K, N, dim, R.seed_of(32, B, K, N, dim), dead=B * K > 4)
    g = R.randn_scaled((B, K), R.gen(R.seed_of(33, B, K)), 1.0)
    g[0, 0] = 0.0
    live, row = C.live_rows(cand, 0, N)
    gd = torch.where(live, g.double(), torch.zeros((), dtype=torch.float64))
    rows = ent.double()[row]
    # dx: n = the live positions of the query
    dx64 = (gd[:, :, None] * rows).sum(1)
    mag = (gd.abs()[:, :, None] * rows.abs()).sum(1)
    n = live.sum(1).double().clamp(min=1)[:, None]
    err = (C.emul_dx_f32(g, cand, ent).double() - dx64).abs()
    assert bool((err <= C.gamma(n) * mag).all())
    # d_ent / d_bias: n = the occurrences of the row
    perm, n_live = C.loop_plan(cand, N)
    de, db = C.emul_ent_f32(g, cand, x, perm, n_live, N)
    fr, fg = row.reshape(-1), gd.reshape(-1)
    xr = x.double().repeat_interleave(K, 0)
    de64 = torch.zeros((N, dim), dtype=torch.float64).index_add_(0, fr, fg[:, None] * xr)
    dem = torch.zeros((N, dim), dtype=torch.float64).index_add_(0, fr, fg.abs()[:, None] * xr.abs())
    db64 = torch.zeros(N, dtype=torch.float64).index_add_(0, fr, fg)
    dbm = torch.zeros(N, dtype=torch.float64).index_add_(0, fr, fg.abs())
    cnt = torch.zeros(N, dtype=torch.float64).index_add_(0, fr, live.reshape(-1).double()).clamp(min=1)
    assert bool(((de.double() - de64).abs() <= C.gamma(cnt)[:, None] * dem).all())
    assert bool(((db.double() - db64).abs() <= C.gamma(cnt) * dbm).all())


def test_emulation_follows_a_bad_plan_without_leaving_the_checked_rows():
    B, K, N, dim = 3, 5, 9, 4
    x, ent, bias, cand, label = problem(B, K, N, dim, 77, dead=False)
    cand[1, 2] = -1
    g = R.randn_scaled((B, K), R.gen(78), 1.0)
    perm, n_live = C.loop_plan(cand, N)
    bad = torch.cat([torch.tensor([B * K + 3, -1, 7]), perm[:n_live], torch.tensor([2 ** 40])])   # 7 = (1, 2): a dead entry
    poison = torch.full((N, dim), 5.0)
    de, db = C.emul_ent_f32(g, cand, x, bad, bad.numel(), N, d_ent=poison, d_bias=torch.full((N,), 5.0))
    want_e, want_b = C.emul_ent_f32(g, cand, x, perm, n_live, N, d_ent=poison, d_bias=torch.full((N,), 5.0))
    assert torch.equal(de, want_e) and torch.equal(db, want_b)
    named = torch.zeros(N, dtype=torch.bool)
    named[cand[cand >= 0]] = True
    assert bool((de[~named] == 5.0).all()) and bool((db[~named] == 5.0).all())


@pytest.mark.parametrize('row0,n_local', [(0, 40), (0, 7), (13, 9), (39, 1), (5, 0)])
def test_cand_plan_on_cpu_equals_the_loop_builder(pkg, row0, n_local):
    nat = pkg._native
    N = 40
    cand = torch.randint(0, N, (6, 37), generator=R.gen(R.seed_of(34, row0, n_local)))
    cand[:, 5] = cand[:, 4]                           # duplicates inside a row
    cand[2] = cand[1]                                 # and across rows
    cand[0, 0], cand[3, 36], cand[4, 1], cand[5, 2], cand[5, 3] = -1, N, 2 ** 62, -2 ** 62, -2 ** 63
    perm, n_live = nat.cand_plan(cand, n_local, row0)
    want, want_live = C.loop_plan(cand, n_local, row0)
    assert perm.dtype == torch.int64 and n_live == want_live and torch.equal(perm, want)
    whole, total = nat.cand_plan(cand, n_local, row0, count=False)      # the same plan, its length for n_live
    assert total == cand.numel() and torch.equal(whole, perm)
    # a strided view of a wider block: the plan is that of the values
    wide = torch.full((6, 50), 2 ** 40, dtype=torch.int64)
    wide[:, 3:40] = cand
    p2, l2 = nat.cand_plan(wide[:, 3:40], n_local, row0)
    assert l2 == n_live and torch.equal(p2, perm)
    empty, none = nat.cand_plan(cand[:, :0], n_local, row0)
    assert empty.numel() == 0 and none == 0


def test_cand_plan_refuses_keys_that_overflow(pkg):
    nat = pkg._native
    cand = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(nat.NativeError, match='overflows'):
        nat.cand_plan(cand, 2 ** 61)
    with pytest.raises(nat.NativeError, match='int64'):
        nat.cand_plan(cand.int(), 5)
    with pytest.raises(nat.NativeError, match='>= 0'):
        nat.cand_plan(cand, 5, -1)


def test_sample_candidates_on_cpu(pkg):
    N, Rn = 50, 3
    g = R.gen(35)
    known = {}
    for _ in range(200):
        s, r, o = (int(v) for v in (torch.randint(0, N, (1,), generator=g), torch.randint(0, Rn, (1,), generator=g),
                                    torch.randint(0, N, (1,), generator=g)))
        known.setdefault((s, r), set()).add(o)
    index = pkg.dist.FilterIndex.from_known(known, Rn)
    pairs = sorted(known)
    q = torch.tensor([pairs[i % len(pairs)] for i in range(0, 3 * len(pairs), 3)] + [pairs[0]] * 40, dtype=torch.int64)
    gen = torch.Generator().manual_seed(5)
    state = gen.get_state()
    cand = pkg.harness.sample_candidates(q, index, N, 9, generator=gen)
    assert cand.shape == (q.size(0), 10) and cand.dtype == torch.int64
    assert bool(((cand >= 0) & (cand < N)).all())
    for (s, r), c in zip(q.tolist(), cand[:, 0].tolist()):
        assert c in known[(s, r)]
    if len(known[pairs[0]]) > 1:                      # forty draws for one query: more than one of its tails comes up
        assert len(set(cand[-40:, 0].tolist())) > 1
    gen.set_state(state)
    assert torch.equal(pkg.harness.sample_candidates(q, index, N, 9, generator=gen), cand)
    assert not torch.equal(pkg.harness.sample_candidates(q, index, N, 9, generator=gen), cand)
    assert pkg.harness.sample_candidates(q, index, N, 0, generator=gen).shape == (q.size(0), 1)
    labels = C.loop_labels(index.query_keys(q[:, 0], q[:, 1]), index.keys, index.ptr, index.tails, cand, 0, N)
    assert bool((labels[:, 0] == 1).all())
    with pytest.raises(ValueError, match='no known tail'):
        pkg.harness.sample_candidates(torch.tensor([[N + 1, 0]]), index, N, 3)
    empty = pkg.dist.FilterIndex.from_known({}, Rn)
    with pytest.raises(ValueError, match='no known tail'):
        pkg.harness.sample_candidates(q[:2], empty, N, 3)
    gen.set_state(state)                              # check=False: the same draw, without the test of the keys
    assert torch.equal(pkg.harness.sample_candidates(q, index, N, 9, generator=gen, check=False), cand)


def test_header_declares_and_library_exports_the_five_symbols(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    assert re.search(r'#define MGCN_ABI_VERSION 4\b', header)
    lib = pkg._native.lib()
    for n in NEW:
        assert n in pkg._native.EXPORTS and re.search(r'\b(int|int64_t) %s\(' % n, header) and hasattr(lib, n), n
    assert lib.mgcn_abi_version() == 4 == pkg._native.ABI_VERSION
    assert lib.mgcn_cand_bce_partials(5, 130) == 15 and lib.mgcn_cand_bce_partials(5, 64) == 5
    assert lib.mgcn_cand_bce_partials(0, 64) == 0 and lib.mgcn_cand_bce_partials(3, 0) == 0


def test_abi_argument_validation_without_a_gpu(pkg):
    """Every bad argument comes back as MGCN_EINVAL (1) with a message before any HIP call; the fake pointers are never
    dereferenced (every case fails validation or has nothing to do)."""
    lib = pkg._native.lib()
    N, P = None, 256

    def fwd(batch=4, k=10, n=100, row0=0, dim=8, x=P, ldx=8, ent=P, lde=8, bias=P, cand=P, ldc=10, label=P, ldl=10, g=P, ldg=10,
            parts=P):
        return lib.mgcn_cand_bce_fwd(batch, k, n, row0, dim, x, ldx, ent, lde, bias, cand, ldc, label, ldl, 1.0, 0.0, 0.1, g, ldg, parts, N)

    def bwd_x(batch=4, k=10, n=100, row0=0, dim=8, g=P, ldg=10, cand=P, ldc=10, ent=P, lde=8, dx=P, ldx=8):
        return lib.mgcn_cand_bce_bwd_x(batch, k, n, row0, dim, g, ldg, cand, ldc, ent, lde, dx, ldx, N)

    def bwd_ent(batch=4, k=10, n=100, row0=0, dim=8, g=P, ldg=10, cand=P, ldc=10, perm=P, n_live=40, x=P, ldx=8, d_ent=P, lde=8,
                d_bias=P):
        return lib.mgcn_cand_bce_bwd_ent(batch, k, n, row0, dim, g, ldg, cand, ldc, perm, n_live, x, ldx, d_ent, lde, d_bias, N)

    def labels(batch=4, k=10, qkey=P, nkeys=3, keys=P, ptr=P, tails=P, row0=0, n=100, cand=P, ldc=10, label=P, ldl=10):
        return lib.mgcn_cand_labels(batch, k, qkey, nkeys, keys, ptr, tails, row0, n, cand, ldc, label, ldl, N)

    big = (1 << 31) - 64
    cases = [
        (fwd, 'cand_bce_fwd', [dict(x=N), dict(ent=N), dict(bias=N), dict(cand=N), dict(label=N), dict(g=N), dict(parts=N),
                               dict(ldc=9), dict(ldl=9), dict(ldg=9), dict(ldx=7), dict(lde=7), dict(row0=-1), dict(batch=-1),
                               dict(k=-1), dict(n=-1), dict(dim=0), dict(n=big), dict(batch=big),
                               dict(k=big, ldc=1 << 31, ldl=1 << 31, ldg=1 << 31)]),
        (bwd_x, 'cand_bce_bwd_x', [dict(g=N), dict(cand=N), dict(ent=N), dict(dx=N), dict(ldg=9), dict(ldc=9), dict(lde=7),
                                   dict(ldx=7), dict(row0=-1), dict(batch=-1), dict(k=-1), dict(n=-1), dict(dim=0), dict(n=big)]),
        (bwd_ent, 'cand_bce_bwd_ent', [dict(g=N), dict(cand=N), dict(perm=N), dict(x=N), dict(ldg=9), dict(ldc=9), dict(ldx=7),
                                       dict(lde=7), dict(n_live=-1), dict(n_live=41), dict(row0=-1), dict(dim=0), dict(k=big, ldg=1 << 31, ldc=1 << 31)]),
        (labels, 'cand_labels', [dict(qkey=N), dict(ptr=N), dict(cand=N), dict(label=N), dict(keys=N), dict(tails=N), dict(ldc=9),
                                 dict(ldl=9), dict(row0=-1), dict(batch=-1), dict(k=-1), dict(n=-1), dict(nkeys=-1), dict(n=big)]),
    ]
    for fn, name, kws in cases:
        for kw in kws:
            rc = fn(**kw)
            msg = lib.mgcn_last_error().decode()
            assert rc == 1 and msg.startswith(name), (name, kw, rc, msg)
        for kw in (dict(batch=0), dict(k=0), dict(n=0)):
            if fn is bwd_ent and 'n' not in kw:
                kw = dict(kw, n_live=0)               # (an empty list has no live prefix)
            assert fn(**kw) == 0, (name, kw)
    assert bwd_ent(n_live=0) == 0 and bwd_ent(d_ent=N, d_bias=N) == 0      # nothing to write
    assert bwd_ent(d_ent=N, x=N, ldx=0, lde=0, n_live=0) == 0              # d_bias alone: x and its strides are not looked at
    assert labels(nkeys=0, keys=N, tails=N, batch=0) == 0


def test_python_surface_needs_a_gpu(pkg):
    nat = pkg._native
    x, ent, bias = torch.zeros(2, 8), torch.zeros(5, 8), torch.zeros(5)
    cand = torch.zeros((2, 3), dtype=torch.int64)
    label = torch.zeros((2, 3), dtype=torch.uint8)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.cand_bce_fwd(x, ent, bias, cand, label, 1.0, 0.0)
    with pytest.raises(nat.NativeError, match='cand'):
        nat.cand_bce_fwd(x, ent, bias, cand[:1], label, 1.0, 0.0)
    with pytest.raises(nat.NativeError, match='label'):
        nat.cand_bce_fwd(x, ent, bias, cand, label[:, :2], 1.0, 0.0)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.cand_bce_bwd_x(torch.zeros(2, 3), cand, ent)
    with pytest.raises(nat.NativeError, match='ent'):
        nat.cand_bce_bwd_x(torch.zeros(2, 3), cand, bias)                # a 1-d table
    with pytest.raises(nat.NativeError, match='x must be'):
        nat.cand_bce_bwd_ent(torch.zeros(2, 3), cand, bias, torch.zeros(6, dtype=torch.int64), 0, 5)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.cand_bce_bwd_ent(torch.zeros(2, 3), cand, x, torch.zeros(6, dtype=torch.int64), 0, 5)
