"""The weighted candidate draw (include/mgcn_hip.h (17)) without a GPU: mgcn_alias_build_host word for word against
the Python-integer restatement tests/cand_alias_ref.py and the properties of the distribution it realises, mgcn_cand_draw_alias_host
(the same inline function the kernel calls) against the restatement, the equal-weights table against mgcn_cand_draw_host, corrupt
tables, the frequencies, the refusals (every check precedes the first HIP call) and sampling.NegativeSampler."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

from . import cand_alias_ref as A
from . import cand_draw_ref as R
from .conftest import ROOT

EINVAL = 1


@pytest.fixture(scope='module')
def tables():
    """name -> (weights, reference table as Python ints): built once, shared, never changed."""
    return {name: (w, A.build(w)) for name, w in A.WEIGHT_GRID}


# ---------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('name', [n for n, _ in A.WEIGHT_GRID])
def test_table_equals_the_restatement_and_realises_the_weights(pkg, tables, name):
    w, want = tables[name]
    N, W = len(w), sum(w)
    got = pkg._native.alias_build_host(torch.tensor(w, dtype=torch.int64))
    assert got.dtype == torch.int64 and got.tolist() == [A.signed(t) for t in want]
    assert all(0 <= (t >> 32) < N for t in want)
    cnt, deg = A.counts(want), A.indegree(want)
    assert sum(cnt) == N * A.TWO32
    worst = 0.0
    for n in range(N):
        if w[n] == 0:
            assert cnt[n] == 0, n
        err = abs(cnt[n] * W - w[n] * N * A.TWO32)
        assert err <= (1 + deg[n]) * W, (n, err, deg[n])
        worst = max(worst, err / float((1 + deg[n]) * W))
    print('ALIAS %s: N = %d, largest |cnt W - w N 2^32| / ((1 + indeg) W) = %.3f' % (name, N, worst))
    s = pkg.NegativeSampler.from_weights(torch.tensor(w, dtype=torch.int64))
    assert s.table.tolist() == got.tolist() and s.counts().tolist() == cnt
    want_logq = torch.tensor([math.log(max(c, 1) / float(A.TWO32)) for c in cnt], dtype=torch.float64).to(torch.float32)
    assert s.logq.dtype == torch.float32 and torch.equal(s.logq, want_logq) and bool(torch.isfinite(s.logq).all())


def test_equal_weights_give_the_identity_table(pkg, tables):
    w, want = tables['equal']
    assert want == [n << 32 | 0xffffffff for n in range(len(w))]
    for s in (pkg.NegativeSampler.from_weights(torch.tensor(w)), pkg.NegativeSampler.uniform(len(w))):
        assert s.table.tolist() == want
        assert bool((s.logq == 0).all()) and not bool(torch.signbit(s.logq).any())          # all +0.0
        assert s.counts().tolist() == [A.TWO32] * len(w)
    # the extremes of the grid, by hand: N = 1 is its own alias; (1, 2^32 - 1): m = (2, 2^33 - 2), W = 2^32
    assert tables['one'][1] == [0xffffffff]
    assert tables['two_extreme'][1] == [1 << 32 | 2, 1 << 32 | 0xffffffff]
    assert A.counts(tables['single_nonzero'][1]) == [0, 0, 6 * A.TWO32, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- the draw
def _weights_for(N):
    return {1: [3], 7: list(range(1, 8)), 4097: A.zipf_weights(4097), 40943: A.zipf_weights(40943)}[N]


@pytest.mark.parametrize('row0', A.GRID_ROW0)
@pytest.mark.parametrize('N', [1, 7, 4097, 40943])
def test_host_draw_equals_reference_on_the_grid(pkg, N, row0):
    """One reference block per (N, row0) at the largest (B, K): every smaller block is its corner. Written through padded windows
    (ldc > K), whose columns beyond K keep their poison."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    k = R.key(1234, 5)
    table = A.build(_weights_for(N))
    tt = A.table_tensor(table)
    Bm, Km = max(A.GRID_B), max(A.GRID_K)
    q = R.grid_queries(Bm)
    want_c, want_l = A.draw(q, keys, ptr, tails, N, Km, k, table, row0)
    uni_c, _ = R.draw(q, keys, ptr, tails, N, Km, k, row0)
    assert torch.equal(want_c[:, 0], uni_c[:, 0])                      # column 0 is (15)'s
    assert int(want_c[:, 1:].min()) >= 0 and int(want_c[:, 1:].max()) < N
    if N > 1:
        assert not torch.equal(want_c, uni_c)                          # the table does change the negatives
    for B in A.GRID_B:
        for K in A.GRID_K:
            cbuf = torch.full((B, K + 3), -77, dtype=torch.int64)
            lbuf = torch.full((B, K + 5), 77, dtype=torch.uint8)
            cand, label = nat.cand_draw_host(q[:B], keys, ptr, tails, N, K, k, row0=row0, table=tt, out=(cbuf[:, :K], lbuf[:, :K]))
            assert torch.equal(cand, want_c[:B, :K]) and torch.equal(label, want_l[:B, :K]), (B, K, N, row0)
            assert bool((cbuf[:, K:] == -77).all()) and bool((lbuf[:, K:] == 77).all())
            only, none = nat.cand_draw_host(q[:B], keys, ptr, tails, N, K, k, row0=row0, labels=False, table=tt)
            assert none is None and torch.equal(only, cand)


def test_k_equal_one_never_reads_the_table(pkg):
    """K = 1 holds the known tail only: a table of poison words changes nothing (and nothing of it is followed)."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    q, k = R.grid_queries(5), R.key(2, 2)
    poison = torch.full((7,), -1, dtype=torch.int64)
    a = nat.cand_draw_host(q, keys, ptr, tails, 7, 1, k, table=poison)
    b = nat.cand_draw_host(q, keys, ptr, tails, 7, 1, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('N', [1, 2, 7, 4097])
def test_equal_weights_draw_is_the_uniform_draw(pkg, N):
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    q = R.grid_queries(67)
    s = pkg.NegativeSampler.uniform(N)
    assert torch.equal(s.table, nat.alias_build_host(torch.full((N,), 11, dtype=torch.int64)))
    for row0 in A.GRID_ROW0:
        got = nat.cand_draw_host(q, keys, ptr, tails, N, 65, R.key(9, 4), row0=row0, table=s.table)
        want = nat.cand_draw_host(q, keys, ptr, tails, N, 65, R.key(9, 4), row0=row0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_corrupt_tables_give_dead_positions(pkg):
    """thr = 0 everywhere, so every negative takes its slot's alias: an alias of N, of -1 (the word -1 << 32) or of 2^31 is
    written as -1 at exactly the positions the restatement says, the good aliases are written as they are."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    N, q, k = 7, R.grid_queries(67), R.key(5, 6)
    table = [3 << 32, N << 32, A.M64 & (-1 << 32), (2 ** 31) << 32, 0 << 32, 6 << 32, (N + 1) << 32 | 0x80000000]
    want_c, want_l = A.draw(q, keys, ptr, tails, N, 65, k, table)
    got_c, got_l = nat.cand_draw_host(q, keys, ptr, tails, N, 65, k, table=A.table_tensor(table))
    assert torch.equal(got_c, want_c) and torch.equal(got_l, want_l)
    neg = got_c[:, 1:]
    assert set(neg.reshape(-1).tolist()) == {-1, 0, 3, 6}      # slot 6 returns itself below its threshold, else -1
    assert int((neg == -1).sum()) > 0 and int(got_l[:, 1:][neg == -1].sum()) == 0


def test_frequencies_follow_the_table(pkg):
    """N = 8, weights 1..8, 2^20 negatives under (seed 1234, step 5): fixed inputs, so deterministic. Every entity's count lies
    within 6 binomial standard deviations of 2^20 Q(n), Q the table's exact distribution."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    w = list(range(1, 9))
    s = pkg.NegativeSampler.from_weights(torch.tensor(w))
    cnt = A.counts(A.build(w))
    assert s.counts().tolist() == cnt
    B, K = 256, 4097                                           # 256 x 4096 negatives
    cand, _ = nat.cand_draw_host(R.grid_queries(B), keys, ptr, tails, 8, K, R.key(1234, 5), labels=False, table=s.table)
    got = torch.bincount(cand[:, 1:].reshape(-1), minlength=8).tolist()
    n = B * (K - 1)
    assert n == 2 ** 20 and sum(got) == n and len(got) == 8
    worst = 0.0
    for e in range(8):
        p = cnt[e] / float(8 * A.TWO32)
        assert abs(p - w[e] / 36.0) < 1e-8
        sigma = math.sqrt(n * p * (1.0 - p))
        worst = max(worst, abs(got[e] - n * p) / sigma)
    print('ALIAS frequencies %s: largest deviation %.2f sigma' % (got, worst))
    assert worst <= 6.0


# ---------------------------------------------------------------------------------------------- refusals
def test_exports_and_header(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    lib = pkg._native.lib()
    for n in ('mgcn_alias_build_host', 'mgcn_cand_draw_alias', 'mgcn_cand_draw_alias_dev', 'mgcn_cand_draw_alias_host'):
        assert n in pkg._native.EXPORTS and re.search(r'\bint %s\(' % n, header) and hasattr(lib, n), n
    assert '(17) Weighted candidate lists' in header
    assert lib.mgcn_abi_version() == 4 and pkg._native.ABI_VERSION == 4


def test_argument_validation_without_a_gpu(pkg):
    """Every refusal comes before the first HIP call: MGCN_EINVAL on a machine with no GPU, and the outputs keep their poison."""
    lib = pkg._native.lib()
    keys, ptr, tails = R.grid_index()
    q = R.grid_queries(4)
    table = pkg.NegativeSampler.uniform(7).table
    pad = torch.zeros(9, dtype=torch.int64)
    cbuf = torch.full((4, 8), -77, dtype=torch.int64)
    lbuf = torch.full((4, 8), 77, dtype=torch.uint8)
    word = torch.zeros(2, dtype=torch.int64)
    good = dict(batch=4, n_cand=8, N=7, q=q.data_ptr(), nk=4, keys=keys.data_ptr(), ptr=ptr.data_ptr(), tails=tails.data_ptr(), nt=9,
                t=table.data_ptr(), c=cbuf.data_ptr(), ldc=8, l=lbuf.data_ptr(), ldl=8)
    bad = [dict(t=None), dict(t=pad.data_ptr() + 4), dict(N=2 ** 31), dict(N=2 ** 40),
           dict(q=None), dict(ptr=None), dict(c=None), dict(keys=None), dict(tails=None), dict(batch=-1), dict(n_cand=0), dict(N=0),
           dict(ldc=7), dict(ldl=7), dict(nk=-1), dict(nt=-1), dict(batch=2 ** 31), dict(ldc=2 ** 59)]

    def call(name, **over):
        a = dict(good, **over)
        head = [a['batch'], a['n_cand'], a['N'], a['q'], a['nk'], a['keys'], a['ptr'], a['tails'], a['nt'], a['t']]
        tail = [0, a['c'], a['ldc'], a['l'], a['ldl']]
        if name == 'mgcn_cand_draw_alias_host':
            return lib.mgcn_cand_draw_alias_host(*(head + [1] + tail))
        if name == 'mgcn_cand_draw_alias':
            return lib.mgcn_cand_draw_alias(*(head + [1] + tail + [None]))
        return lib.mgcn_cand_draw_alias_dev(*(head + [a.get('w', word.data_ptr()), 0x2000] + tail + [None]))

    for name in ('mgcn_cand_draw_alias', 'mgcn_cand_draw_alias_dev', 'mgcn_cand_draw_alias_host'):
        for over in bad:
            assert call(name, **over) == EINVAL, (name, over)
            assert lib.mgcn_last_error().decode().startswith(name + ':'), (name, over)
        assert call(name, batch=0) == 0                          # nothing to do, no launch
        assert bool((cbuf == -77).all()) and bool((lbuf == 77).all()), name
    assert lib.mgcn_cand_draw_alias_dev(0, 8, 7, good['q'], 4, good['keys'], good['ptr'], good['tails'], 9, good['t'], None, 0x2000, 0,
                                        good['c'], 8, good['l'], 8, None) == EINVAL          # the word is checked first, at batch 0 too
    assert call('mgcn_cand_draw_alias_host', N=2 ** 31 - 1, batch=0) == 0                   # the largest table
    assert call('mgcn_cand_draw_alias_host') == 0 and bool((cbuf != -77).all())
    # the builder: nothing written on a refusal
    out = torch.full((3,), -77, dtype=torch.int64)
    w = torch.tensor([1, 2, 3])
    for ws, n, wp, op in (([1, 2, 3], 3, None, out.data_ptr()), ([1, 2, 3], 3, w.data_ptr(), None), ([1, 2, 3], 0, 1, 1), ([1, 2, 3], 2 ** 31, 1, 1),
                          ([1, -1, 3], 3, 0, 0), ([1, 2 ** 32, 3], 3, 0, 0), ([0, 0, 0], 3, 0, 0)):
        ww = torch.tensor(ws)
        assert lib.mgcn_alias_build_host(n, ww.data_ptr() if wp == 0 else wp, out.data_ptr() if op == 0 else op) == EINVAL, (ws, n)
        assert lib.mgcn_last_error().decode().startswith('mgcn_alias_build_host:')
        assert bool((out == -77).all())
    nat = pkg._native
    with pytest.raises(nat.NativeError):
        nat.cand_draw(q, keys, ptr, tails, 7, 8, 1, table=table)             # CPU tensors: the device entry point has no CPU fallback
    with pytest.raises(nat.NativeError):
        nat.cand_draw_host(q, keys, ptr, tails, 7, 8, 1, table=table[:6])
    with pytest.raises(nat.NativeError):
        nat.cand_draw_host(q, keys, ptr, tails, 7, 8, 1, table=table.to(torch.int32))
    with pytest.raises(nat.NativeError):
        nat.alias_build_host(torch.zeros(4, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- NegativeSampler
def test_sampler_round_trips_through_state_dict(pkg):
    s = pkg.NegativeSampler.from_weights(torch.tensor(A.zipf_weights(33)))
    sd = s.state_dict()
    assert set(sd) == {'table'} and sd['table'].dtype == torch.int64 and sd['table'].data_ptr() != s.table.data_ptr()
    t = pkg.NegativeSampler.uniform(33)
    at = (t.table.data_ptr(), t.logq.data_ptr())
    assert t.load_state_dict(sd) is t
    assert torch.equal(t.table, s.table) and torch.equal(t.logq, s.logq) and (t.table.data_ptr(), t.logq.data_ptr()) == at
    u = pkg.NegativeSampler.uniform(5).load_state_dict(sd)                  # another length: the tensors are replaced
    assert torch.equal(u.table, s.table) and torch.equal(u.logq, s.logq)
    assert s.to('cpu') is s and s.num_entities == 33
    bad = s.table.clone()
    bad[3] = 33 << 32
    with pytest.raises(pkg._native.NativeError):
        pkg.NegativeSampler(bad)
    with pytest.raises(pkg._native.NativeError):
        pkg.NegativeSampler.uniform(0)


def test_from_degrees_on_a_toy_index(pkg):
    """weights = floor((deg + shift)^power 2^16) in float64; deg defaults to how often the entity is a known tail."""
    keys, ptr, tails = R.grid_index()
    index = types.SimpleNamespace(keys=keys, ptr=ptr, tails=tails)
    deg = [1, 1, 1, 1, 1, 2, 2]                                             # bincount of grid_index()'s tails over 7 entities
    assert torch.bincount(tails.long(), minlength=7).tolist() == deg
    for power, shift in ((0.75, 1.0), (1.0, 0.0), (0.5, 2.5)):
        w = [min(int(math.floor(math.pow(d + shift, power) * 65536.0)), 2 ** 32 - 1) for d in deg]
        want = pkg.NegativeSampler.from_weights(torch.tensor(w))
        a = pkg.NegativeSampler.from_degrees(torch.tensor(deg), power=power, shift=shift)
        b = pkg.NegativeSampler.from_degrees(index=index, num_entities=7, power=power, shift=shift)
        assert torch.equal(a.table, want.table) and torch.equal(b.table, want.table)
    big = pkg.NegativeSampler.from_degrees(torch.tensor([2.0 ** 40, 1.0]), power=1.0, shift=0.0)      # clamped below 2^32
    assert torch.equal(big.table, pkg.NegativeSampler.from_weights(torch.tensor([2 ** 32 - 1, 65536])).table)
    with pytest.raises(pkg._native.NativeError):
        pkg.NegativeSampler.from_degrees()
