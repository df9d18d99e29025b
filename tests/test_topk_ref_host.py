"""tests/topk_ref.py checked without a GPU: the reference against torch's stable sort, the order on every boundary of
the f32 bit patterns, the torch stand-ins of test_topk_host.py against the reference, and that the grids really take the
paths their labels claim (a grid that never crosses a window edge or never walks the id bytes would test nothing)."""
import numpy as np
import pytest
import torch

from . import topk_ref as R
from .test_topk_host import TorchTopkKernels, _problem


def test_topk_ref_equals_torch_stable_sort_with_heavy_ties():
    g = torch.Generator().manual_seed(3)
    for n, k, levels in [(1, 1, 2), (50, 10, 3), (777, 100, 5), (5000, 1024, 40), (300, 1024, 7)]:
        score = (torch.randint(0, levels, (4, n), generator=g).float() - levels // 2) / 7.0     # finite, heavy ties
        filtered = torch.rand(4, n, generator=g) < 0.3
        for f in (None, filtered):
            s = score if f is None else torch.where(f, torch.full_like(score, float('-inf')), score)
            vals, idx = torch.sort(s, dim=1, descending=True, stable=True)
            live = torch.full((4,), n) - (0 if f is None else f.sum(1))
            want_s = torch.full((4, k), float('-inf'))
            want_i = torch.full((4, k), -1, dtype=torch.int64)
            m = min(k, n)
            want_s[:, :m], want_i[:, :m] = vals[:, :m], idx[:, :m] + 9
            dead = torch.arange(k)[None, :] >= live[:, None]
            want_s[dead], want_i[dead] = float('-inf'), -1
            got_s, got_i = R.topk_ref(score, torch.arange(n) + 9, k, f)
            assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s), (n, k, f is None)
            R.compare(got_s, got_i, want_s, want_i)
    # padding ids are dropped whatever their score; the lists need not be sorted
    s = torch.tensor([[1.0, 9.0, 3.0, 3.0, float('-inf'), 2.0]])
    i = torch.tensor([[4, -1, 8, 2, 6, -5]])
    got_s, got_i = R.topk_ref(s, i, 5)
    assert got_i.tolist() == [[2, 8, 4, 6, -1]] and got_s.tolist() == [[3.0, 3.0, 1.0, float('-inf'), float('-inf')]]


def test_order_key_is_monotone_on_every_boundary():
    """The boundary patterns in the order the header states, written out by hand: each step must not descend, and must
    ascend exactly when the two patterns are different scores (only -0 / +0 are equal)."""
    ladder = [0xffffffff, 0xfffffffe, 0xffc00001, 0xffc00000, 0xffbfffff, 0xff800001,      # NaNs, sign set: below -inf
              0xff800000,                                                                  # -inf
              0xff7fffff, 0xff7ffffe, 0xff000000, 0xbf800000, 0x81000000, 0x80800001, 0x80800000,   # -FLT_MAX .. -FLT_MIN
              0x807fffff, 0x807ffffe, 0x80000002, 0x80000001,                              # negative denormals
              0x80000000, 0x00000000,                                                      # -0 == +0
              0x00000001, 0x00000002, 0x007ffffe, 0x007fffff,                              # denormals
              0x00800000, 0x00800001, 0x01000000, 0x3f000000, 0x3f800000, 0x7f000000, 0x7f7ffffe, 0x7f7fffff,
              0x7f800000,                                                                  # +inf
              0x7f800001, 0x7fbfffff, 0x7fc00000, 0x7fc00001, 0x7ffffffe, 0x7fffffff]      # NaNs, sign clear: above +inf
    key = R.order_key(np.array(ladder, dtype=np.uint32))
    for j in range(len(ladder) - 1):
        zeros = ladder[j] == 0x80000000 and ladder[j + 1] == 0
        assert (key[j] == key[j + 1]) if zeros else (key[j] < key[j + 1]), (hex(ladder[j]), hex(ladder[j + 1]))
    assert set(R.BOUNDARY_BITS) >= {b for b in ladder if b not in (0xffbfffff, 0x7fbfffff)}     # the pool holds the ladder
    # on finite values and infinities it is the f32 comparison
    fin = np.array([b for b in R.BOUNDARY_BITS if not R.is_nan_bits(b)], dtype=np.uint32)
    v, kf = fin.view(np.float32).astype(np.float64), R.order_key(fin)
    assert ((v[:, None] < v[None, :]) == (kf[:, None] < kf[None, :])).all()
    assert ((v[:, None] == v[None, :]) == (kf[:, None] == kf[None, :])).all()
    # a sweep of +-300 patterns around each boundary, and the select's 32-bit key gives the same order everywhere
    sweep = np.unique(np.concatenate([(np.int64(b) + np.arange(-300, 301)) % 2 ** 32 for b in R.BOUNDARY_BITS])).astype(np.uint32)
    ks, k32 = R.order_key(sweep), R.radix_key32(sweep).astype(np.int64)
    o = np.argsort(ks, kind='stable')
    assert (np.diff(k32[o]) >= 0).all()
    assert ((np.diff(ks[o]) == 0) == (np.diff(k32[o]) == 0)).all()
    mag = sweep[o].astype(np.int64) & 0x7fffffff
    assert ((np.diff(ks[o]) == 0) <= ((mag[1:] == 0) & (mag[:-1] == 0))).all()          # only the zeros share a rank


def test_torch_stand_ins_of_the_gloo_rehearsal_agree_with_topk_ref():
    for world in (2, 3):
        x, ent, bias, sub, rel, known = _problem(world=world)
        g = torch.Generator().manual_seed(world)
        N = ent.size(0)
        for r in range(world):
            score = TorchTopkKernels.score(x[r], ent, bias)
            mask = torch.rand(score.shape, generator=g) < 0.4
            mask[1] = True
            mask[1, :5] = False                                # fewer than k left
            for k in (10, 40):
                lists = []
                for m in (None, mask):
                    got = TorchTopkKernels.score_topk(x[r], ent, bias, k, mask=m, ent_row0=100)
                    R.compare(*got, *R.topk_ref(score, torch.arange(N) + 100, k, m), label='stand-in score_topk')
                    lists.append(got)
                cat_s, cat_i = torch.cat([l[0] for l in lists], 1), torch.cat([l[1] for l in lists], 1)
                cat_i[:, k:][cat_i[:, k:] >= 0] += 1000       # distinct ids across the two lists
                R.compare(*TorchTopkKernels.topk_merge(cat_s, cat_i, k), *R.topk_ref(cat_s, cat_i, k), label='stand-in topk_merge')


@pytest.fixture(scope='module')
def merge_cases():
    return R.merge_grid()


@pytest.fixture(scope='module')
def merge_traces(merge_cases):
    return {c.label: [R.merge_trace(c.bits[b], c.ids[b], c.k) for b in range(c.bits.shape[0])] for c in merge_cases}


def test_merge_grid_is_inside_the_contract(merge_cases):
    for c in merge_cases:
        assert c.bits.shape == c.ids.shape == (c.bits.shape[0], c.k * c.lists) and 1 <= c.bits.shape[0] <= 3, c.label
        assert 1 <= c.k <= R.KMAX and c.ids.max() <= R.ID_MAX, c.label
        for row in c.ids:
            live = row[row >= 0]
            assert len(np.unique(live)) == len(live), c.label      # distinct ids: duplicates are outside the contract
    ids = np.concatenate([c.ids.reshape(-1) for c in merge_cases])
    assert (ids == 0).any() and (ids == R.ID_MAX).any() and (ids < -1).any()
    bits = np.concatenate([c.bits.reshape(-1)[c.ids.reshape(-1) >= 0] for c in merge_cases])
    assert set(R.POOL.tolist()) <= set(bits.tolist())                # every boundary pattern is some live candidate's score


def test_merge_grid_reaches_every_radix_pass_and_digit(merge_traces):
    """Vacuity: some case stops after each of passes 1..8; the threshold digits cover 0 and 255 (lanes 63 and 0 of the
    scan) in the FIRST pass, i.e. of the score's top byte, and all four positions within a lane."""
    passes, first, digits = set(), set(), set()
    for rows in merge_traces.values():
        for windows in rows:
            for w in windows:
                if w.passes:
                    passes.add(w.passes)
                    first.add(w.digits[0])
                    digits.update(w.digits)
    assert passes == set(range(1, 9)), passes
    assert {0, 255} <= first, sorted(first)
    assert {(255 - d) % 4 for d in digits} == {0, 1, 2, 3}
    assert {(255 - d) // 4 for d in digits} >= {0, 63}


def test_merge_grid_crosses_every_window_edge(merge_cases, merge_traces):
    k_of = {c.label: c.k for c in merge_cases}
    after = {'<': 0, '==': 0, '>': 0}         # candidates held after a window that another window follows
    for label, rows in merge_traces.items():
        for windows in rows:
            for w in windows[:-1]:
                after['<' if w.filled < k_of[label] else '==' if w.filled == k_of[label] else '>'] += 1
    assert all(after.values()), after
    empty_first = [label for label, rows in merge_traces.items() if all(len(w) > 1 and w[0].filled == 0 and w[-1].filled > 0 for w in rows)]
    assert len(empty_first) >= 5 and all('first window all padding' in l for l in empty_first), empty_first    # an empty window, then candidates
    assert all(l in empty_first for l in merge_traces if 'first window all padding' in l)
    totals = {(c.k, c.k * c.lists) for c in merge_cases}
    for k in (1, 1024):                       # around the first window's fit and the second's
        for edge in (R.CAP, R.CAP + (R.CAP - k)):
            near = sorted(t for kk, t in totals if kk == k and abs(t - edge) <= k)
            assert any(t < edge for t in near) and edge in near and any(t > edge for t in near), (k, edge, near)
    assert {(7, 8190), (7, 8197), (1000, 9000)} <= totals
    windows_of = {(c.k, c.k * c.lists): len(merge_traces[c.label][0]) for c in merge_cases if 'dense' in c.label}
    assert windows_of[(1, 8192)] == 1 and windows_of[(1, 8193)] == 2 and windows_of[(1, 16383)] == 2 and windows_of[(1, 16384)] == 3
    assert windows_of[(1024, 8192)] == 1 and windows_of[(1024, 9216)] == 2 and windows_of[(1024, 15360)] == 2 and windows_of[(1024, 16384)] == 3
    assert {c.k for c in merge_cases} >= set(R.MERGE_KS) == {1, 2, 3, 7, 64, 65, 511, 512, 513, 1000, 1023, 1024}


def _cpu_scores(op):
    """A CPU stand-in for score_fwd (float64 sigmoid rounded to f32): good enough to show what the grids are built to do."""
    z = op['x'].astype(np.float64) @ op['ent'].astype(np.float64).T + op['bias'].astype(np.float64)
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def test_selection_grids_are_inside_the_contract_and_the_depth_grid_reaches_every_pass():
    labels, ks = set(), set()
    for N in R.SELECT_NS:
        for c in R.select_grid(N):
            assert c.N == N and 1 <= c.B <= 3 and c.O in (3, 4) and 1 <= c.k <= R.KMAX and c.row0 + N <= R.ID_MAX, c.label
            assert c.label not in labels
            labels.add(c.label)
            ks.add(c.k)
    assert ks >= set(R.SELECT_KS)
    for N in R.CHUNK_NS:
        for c in R.chunk_grid(N):
            assert c.B == 2 and c.O == 4 and c.k in (10, 1024) and c.label not in labels
            labels.add(c.label)
    passes = set()
    for c in R.depth_grid():
        op = R.select_operands(c)
        for p, _ in R.segment_traces(_cpu_scores(op), np.arange(c.N) + c.row0, c.k):
            passes.add(p)
    assert passes >= set(range(1, 9)), passes
    # the counted masks leave what their label says
    c = [c for c in R.select_grid(8193) if c.mask == 'exact:seg:1' and c.k == 65][0]
    f = R.select_operands(c)['filtered']
    assert (~f[:, R.SEG:2 * R.SEG]).sum(1).tolist() == [64, 65, 66]
    c = [c for c in R.select_grid(8193) if c.mask == 'exact:row' and c.k == 1024][0]
    assert (~R.select_operands(c)['filtered']).sum(1).tolist() == [1023, 1024, 1025]
    # the packed mask: bit n & 31 of word n >> 5, everything past N set
    f = np.zeros((1, 70), dtype=bool)
    f[0, [0, 31, 33, 69]] = True
    w = R.pack_mask(f, spare=2).view(np.uint32)
    assert w.shape == (1, 5) and w[0].tolist() == [0x80000001, 0x00000002, 0xffffffe0, 0xffffffff, 0xffffffff]
