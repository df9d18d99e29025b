"""The counter-drawn candidate lists (include/mgcn_hip.h (15)) without a GPU: the definition's known answers,
mgcn_cand_draw_host (the same inline function the kernel calls) against the Python-integer restatement tests/cand_draw_ref.py,
slices, labels, padding, uniformity, and the argument validation of both entry points (every check precedes the first HIP
call)."""
import os
import re

import pytest
import torch

from . import cand_draw_ref as R
from . import cand_train_ref as T
from .conftest import ROOT

EINVAL = 1


def test_known_answers(pkg):
    """Recomputed here from dropout_ref's SplitMix64 and Philox, then pinned."""
    nat = pkg._native
    k = R.key(1234, 5)
    assert k == 0x3240e6b5af382cbd and nat.CAND_DRAW_SITE == R.SITE == 0x2000
    assert nat.dropout_key(1234, 5, nat.CAND_DRAW_SITE) == k
    assert R.values(k, 1, 4)[0] == [0xaf4614d3074fb72c, 0x64e215625067babc, 0x92a96b36e04e39f3, 0x3ba5c0f92d757254]
    # (r N) >> 64 of those values at N = 7, through the library: columns 1 .. 3 of a query without a key
    keys, ptr, tails = R.grid_index()
    cand, label = nat.cand_draw_host(torch.tensor([99]), keys, ptr, tails, 7, 4, k)
    assert cand.tolist() == [[-1, 2, 4, 1]] and label.tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize('row0', R.GRID_ROW0)
@pytest.mark.parametrize('N', R.GRID_N)
def test_host_draw_equals_reference_on_the_grid(pkg, N, row0):
    """One reference block per (N, row0) at the largest (B, K): position (b, j) depends on nothing else, so every smaller block is
    its corner. Queries below, between and above the keys and the query of the empty run give -1 / label 0 at column 0."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    k = R.key(1234, 5)
    Bm, Km = max(R.GRID_B), max(R.GRID_K)
    q = R.grid_queries(Bm)
    want_c, want_l = R.draw(q, keys, ptr, tails, N, Km, k, row0)
    for b, key in enumerate(q.tolist()):
        if key in (5, 25, 99, 30):
            assert int(want_c[b, 0]) == -1 and int(want_l[b, 0]) == 0
        else:
            assert int(want_c[b, 0]) >= 0 and int(want_l[b, 0]) == int(int(want_c[b, 0]) < N)
    if N == 2 ** 40:
        assert int(want_c.max()) >= 2 ** 32
    assert int(want_c[:, 1:].min()) >= 0 and int(want_c[:, 1:].max()) < N
    for B in R.GRID_B:
        for K in R.GRID_K:
            cand, label = nat.cand_draw_host(q[:B], keys, ptr, tails, N, K, k, row0=row0)
            assert torch.equal(cand, want_c[:B, :K]) and torch.equal(label, want_l[:B, :K]), (B, K, N, row0)
            only, none = nat.cand_draw_host(q[:B], keys, ptr, tails, N, K, k, row0=row0, labels=False)
            assert none is None and torch.equal(only, cand)


def test_malformed_runs_give_minus_one(pkg):
    nat = pkg._native
    k = R.key(7, 0)
    q = torch.tensor([10, 20, 30, 40])
    for (keys, ptr, tails), good in zip(R.malformed_index(), ((0,), (3,))):
        cand, label = nat.cand_draw_host(q, keys, ptr, tails, 7, 5, k)
        want_c, want_l = R.draw(q, keys, ptr, tails, 7, 5, k)
        assert torch.equal(cand, want_c) and torch.equal(label, want_l)
        for b in range(4):
            assert (int(cand[b, 0]) != -1) == (b in good), (b, cand[b].tolist())
            if b not in good:
                assert int(label[b].sum()) == 0               # no run: nothing is a known tail
    # an empty index: every column 0 is -1, the negatives are drawn all the same
    none = torch.zeros(0, dtype=torch.int64)
    cand, label = nat.cand_draw_host(q, none, torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 7, 5, k)
    assert cand[:, 0].tolist() == [-1] * 4 and torch.equal(cand[:, 1:], want_c[:, 1:]) and int(label.sum()) == 0


def test_slices_equal_the_whole(pkg):
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    k, q = R.key(3, 9), R.grid_queries(8)
    for base in (0, 2 ** 32 - 2):
        whole = nat.cand_draw_host(q, keys, ptr, tails, 40943, 9, k, row0=base)
        a = nat.cand_draw_host(q[:3], keys, ptr, tails, 40943, 9, k, row0=base)
        b = nat.cand_draw_host(q[3:], keys, ptr, tails, 40943, 9, k, row0=base + 3)
        for i in (0, 1):
            assert torch.equal(torch.cat([a[i], b[i]]), whole[i])
    other = nat.cand_draw_host(q, keys, ptr, tails, 40943, 9, R.key(3, 10), row0=base)[0]          # another step: other lists
    assert float((other[:, 1:] != whole[0][:, 1:]).float().mean()) > 0.9


@pytest.mark.parametrize('N', [7, 40943])
def test_labels_equal_the_loop_labels_of_the_drawn_list(pkg, N):
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    q = R.grid_queries(67)
    cand, label = nat.cand_draw_host(q, keys, ptr, tails, N, 65, R.key(11, 2))
    assert torch.equal(label, T.loop_labels(q, keys, ptr, tails, cand, row0=0, n_local=N))
    live = cand[:, 0] != -1
    assert bool((label[:, 0] == live.to(torch.uint8)).all())           # column 0 is hot wherever it is not -1
    if N == 7:
        assert int(label[:, 1:].sum()) > 0                              # negatives that happen to be known tails are hot


def test_padded_rows_keep_their_poison(pkg):
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    q, k = R.grid_queries(5), R.key(1, 1)
    cbuf = torch.full((5, 12), -77, dtype=torch.int64)
    lbuf = torch.full((5, 16), 77, dtype=torch.uint8)
    cand, label = nat.cand_draw_host(q, keys, ptr, tails, 7, 9, k, out=(cbuf[:, :9], lbuf[:, :9]))
    want = nat.cand_draw_host(q, keys, ptr, tails, 7, 9, k)
    assert torch.equal(cbuf[:, :9], want[0]) and torch.equal(lbuf[:, :9], want[1])
    assert bool((cbuf[:, 9:] == -77).all()) and bool((lbuf[:, 9:] == 77).all())
    assert cand.data_ptr() == cbuf.data_ptr() and label.data_ptr() == lbuf.data_ptr()


def test_negatives_are_uniform(pkg):
    """B = 64, K = 4097, N = 7, (seed 1234, step 5): fixed inputs, so deterministic. Every id's count over the 262 144 negatives
    lies within 4 standard deviations (sigma = sqrt(n (1/7) (6/7)) = 179) of n / 7 = 37 449."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    cand, _ = nat.cand_draw_host(R.grid_queries(64), keys, ptr, tails, 7, 4097, R.key(1234, 5), labels=False)
    counts = torch.bincount(cand[:, 1:].reshape(-1), minlength=7).tolist()
    assert sum(counts) == 262144 and len(counts) == 7
    worst = max(abs(c - 37449) for c in counts)
    print('UNIFORM counts %s: largest deviation %.2f sigma' % (counts, worst / 179.0))
    assert worst <= 4 * 179


def test_exports_and_header(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    lib = pkg._native.lib()
    for n in ('mgcn_cand_draw', 'mgcn_cand_draw_host'):
        assert n in pkg._native.EXPORTS and re.search(r'\bint %s\(' % n, header) and hasattr(lib, n), n
    assert '(15) Counter-drawn candidate lists' in header
    assert lib.mgcn_abi_version() == 4 and pkg._native.ABI_VERSION == 4
    import __graft_entry__ as entry
    assert 'dropout.hip' in entry.SOURCES and len(entry.SOURCES) == 14


def test_argument_validation_without_a_gpu(pkg):
    """Every refusal of both entry points comes before the first HIP call: MGCN_EINVAL on a machine with no GPU, and the
    outputs keep their poison."""
    lib = pkg._native.lib()
    keys, ptr, tails = R.grid_index()
    q = R.grid_queries(4)
    cbuf = torch.full((4, 8), -77, dtype=torch.int64)
    lbuf = torch.full((4, 8), 77, dtype=torch.uint8)
    Q, KY, P, TL, C, L = q.data_ptr(), keys.data_ptr(), ptr.data_ptr(), tails.data_ptr(), cbuf.data_ptr(), lbuf.data_ptr()
    good = dict(batch=4, n_cand=8, N=7, q=Q, nk=4, keys=KY, ptr=P, tails=TL, nt=9, c=C, ldc=8, l=L, ldl=8)
    bad = [dict(q=None), dict(ptr=None), dict(c=None), dict(keys=None), dict(tails=None),
           dict(batch=-1), dict(n_cand=0), dict(n_cand=-3), dict(N=0), dict(N=-1), dict(N=2 ** 40 + 1),
           dict(ldc=7), dict(ldl=7), dict(nk=-1), dict(nt=-1), dict(batch=2 ** 31), dict(n_cand=2 ** 31, ldc=2 ** 31, ldl=2 ** 31),
           dict(ldc=2 ** 59)]

    def call(fn, host, **over):
        a = dict(good, **over)
        args = [a['batch'], a['n_cand'], a['N'], a['q'], a['nk'], a['keys'], a['ptr'], a['tails'], a['nt'], 1, 0, a['c'], a['ldc'],
                a['l'], a['ldl']]
        return fn(*(args if host else args + [None]))

    for fn, host, name in ((lib.mgcn_cand_draw, False, 'mgcn_cand_draw:'), (lib.mgcn_cand_draw_host, True, 'mgcn_cand_draw_host:')):
        for over in bad:
            assert call(fn, host, **over) == EINVAL, (name, over)
            assert lib.mgcn_last_error().decode().startswith(name), (name, over)
        assert call(fn, host, batch=0) == 0                       # nothing to do, no launch
        assert bool((cbuf == -77).all()) and bool((lbuf == 77).all()), name
    # without labels the label's leading dimension is not looked at
    assert call(lib.mgcn_cand_draw_host, True, l=None, ldl=0) == 0
    assert bool((cbuf != -77).all()) and bool((lbuf == 77).all())
    # 2^40 entities is the largest table
    assert call(lib.mgcn_cand_draw_host, True, N=2 ** 40) == 0
    # the Python wrappers refuse tensors on the wrong device and blocks of the wrong shape
    nat = pkg._native
    with pytest.raises(nat.NativeError):
        nat.cand_draw(q, keys, ptr, tails, 7, 8, 1)               # CPU tensors: the device entry point has no CPU fallback
    with pytest.raises(nat.NativeError):
        nat.cand_draw_host(q, keys, ptr, tails, 7, 8, 1, out=torch.zeros((4, 7), dtype=torch.int64))
    with pytest.raises(nat.NativeError):
        nat.cand_draw_host(q, keys, ptr[:-1], tails, 7, 8, 1)
