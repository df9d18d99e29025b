"""topk.hip (section (7) of mgcn_hip.h) at its internal boundaries on a real MI355X: the whole score range, crafted merge
inputs, the merge's window fits, segment and chunk edges, k around the bitonic pad sizes, and ties that walk every byte
of the select. Expected is always tests/topk_ref.topk_ref of exact inputs (for score_topk: of the block score_fwd itself
returned), so every comparison is exact. Every call writes into outputs wider than needed, pre-filled with a sentinel
(NaN scores, id -77), and everything outside [B, k] must come back untouched. Batches are 1 to 3 rows."""
import ctypes

import numpy as np
import pytest
import torch

from . import topk_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT_ID = -77
SEEN_PASSES = set()        # radix depths of the SELECT fills, from the scores score_fwd returned (asserted by the last test)


class Guarded(object):
    """(scores, ids) [B, k] views inside sentinel-filled buffers. strided: rows `k + 11` / `k + 5` apart at column
    offsets 3 / 2 (so ldo != ldi, both > k); otherwise contiguous [B, k] with 32 elements of slack on either side."""

    def __init__(self, B, k, strided):
        if strided:
            self.buf_s = torch.full((B, k + 11), float('nan'), device=DEV)
            self.buf_i = torch.full((B, k + 5), SENT_ID, dtype=torch.int64, device=DEV)
            self.s, self.i = self.buf_s[:, 3:3 + k], self.buf_i[:, 2:2 + k]
        else:
            self.buf_s = torch.full((B * k + 64,), float('nan'), device=DEV)
            self.buf_i = torch.full((B * k + 64,), SENT_ID, dtype=torch.int64, device=DEV)
            self.s, self.i = self.buf_s[32:32 + B * k].view(B, k), self.buf_i[32:32 + B * k].view(B, k)
        self.out = (self.s, self.i)

    def check_untouched(self, label):
        got_s, got_i = self.s.clone(), self.i.clone()
        self.s.fill_(float('nan'))
        self.i.fill_(SENT_ID)
        assert bool(torch.isnan(self.buf_s).all()), '%s: score written outside [B, k]' % label
        assert bool((self.buf_i == SENT_ID).all()), '%s: id written outside [B, k]' % label
        self.s.copy_(got_s)
        self.i.copy_(got_i)


# ---------------------------------------------------------------------------------------------------------------------
# merge, direct, crafted inputs
MERGE_CASES = R.merge_grid()


@pytest.mark.parametrize('case', MERGE_CASES, ids=[c.label for c in MERGE_CASES])
def test_merge_crafted(pkg, case):
    nat = pkg._native
    B, k = case.bits.shape[0], case.k
    s, i = R.floats_of(case.bits).to(DEV), torch.from_numpy(case.ids).to(DEV)
    assert torch.equal(s.cpu().view(torch.int32), R.floats_of(case.bits).view(torch.int32))     # the upload kept every bit
    want = R.topk_ref(case.bits, case.ids, k)
    g = Guarded(B, k, strided=False)
    got_s, got_i = nat.topk_merge(s, i, k, out=g.out)
    assert got_s.data_ptr() == g.s.data_ptr() and got_i.data_ptr() == g.i.data_ptr()
    R.compare(got_s, got_i, *want, label=case.label)
    g.check_untouched(case.label)
    gb = R.bits_of(got_s)
    assert not (gb == 0x80000000).any(), '%s: a returned zero is +0' % case.label
    # two calls give the same bits (NaNs included: compared as integers)
    again_s, again_i = nat.topk_merge(s, i, k)
    assert torch.equal(again_i, got_i) and torch.equal(again_s.view(torch.int32), got_s.view(torch.int32)), case.label
    # the same candidates in another arrangement: the order is total, so the output is the same
    perm = torch.from_numpy(np.random.default_rng(len(case.label)).permutation(s.size(1))).to(DEV)
    perm_s, perm_i = nat.topk_merge(s[:, perm].contiguous(), i[:, perm].contiguous(), k)
    R.compare(perm_s, perm_i, *want, label=case.label + ' (permuted)')
    assert torch.equal(perm_i, got_i)


def test_merge_ld_in_slack_columns_are_ignored(pkg):
    """Through the C ABI with ld_in > lists * k: the slack columns hold candidates that would win, and are not read."""
    nat = pkg._native
    rng = np.random.default_rng(5)
    B, k, lists, slack = 3, 65, 5, 37
    L, ld = lists * k, lists * k + slack
    bits = np.full((B, ld), 0x7f800000, dtype=np.uint32)                      # slack: +inf under valid, distinct ids
    ids = np.tile(np.arange(ld, dtype=np.int64) + 10 ** 6, (B, 1))
    for b in range(B):
        bits[b, :L] = rng.choice(R.POOL_NO_NEG_NAN, size=L)
        ids[b, :L] = R.distinct_ids(rng, L, hi=10 ** 6, must=(0,))
        ids[b, :L][rng.random(L) < 0.3] = -1
    s, i = R.floats_of(bits).to(DEV), torch.from_numpy(ids).to(DEV)
    g = Guarded(B, k, strided=False)
    rc = nat.lib().mgcn_topk_merge(B, lists, s.data_ptr(), i.data_ptr(), ld, k, g.s.data_ptr(), g.i.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, nat.lib().mgcn_last_error().decode()
    torch.cuda.synchronize()
    R.compare(g.s, g.i, *R.topk_ref(bits[:, :L], ids[:, :L], k), label='ld_in = lists k + 37')
    assert bool((g.i < 10 ** 6).all())
    g.check_untouched('ld_in')


def test_out_argument_is_checked(pkg):
    nat = pkg._native
    s = torch.zeros((2, 6), device=DEV)
    i = torch.arange(12, device=DEV).view(2, 6)
    wide_s, wide_i = torch.zeros((2, 9), device=DEV), torch.zeros((2, 9), dtype=torch.int64, device=DEV)
    with pytest.raises(nat.NativeError, match='contiguous'):
        nat.topk_merge(s, i, 3, out=(wide_s[:, :3], wide_i[:, :3]))                # the merge's ABI has no output stride
    with pytest.raises(nat.NativeError, match=r'must be \(2, 3\)'):
        nat.topk_merge(s, i, 3, out=(wide_s, wide_i))
    x, ent, bias = torch.zeros((2, 4), device=DEV), torch.zeros((5, 4), device=DEV), torch.zeros(5, device=DEV)
    with pytest.raises(nat.NativeError, match=r'must be \(2, 3\)'):
        nat.score_topk(x, ent, bias, 3, out=(wide_s[:, :4], wide_i[:, :4]))
    with pytest.raises(nat.NativeError, match='dtype'):
        nat.score_topk(x, ent, bias, 3, out=(wide_s[:, :3], wide_s[:, 3:6]))
    got_s, got_i = nat.score_topk(x, ent, bias, 3, out=(wide_s[:, :3], wide_i[:, 6:]))
    assert got_i.tolist() == [[0, 1, 2]] * 2 and got_s.tolist() == [[0.5] * 3] * 2 and wide_i[:, :6].eq(0).all()


# ---------------------------------------------------------------------------------------------------------------------
# selection through score_topk
def run_select(pkg, case):
    """One case against topk_ref of score_fwd's own block; returns the failure text or None."""
    nat = pkg._native
    op = R.select_operands(case)
    x, ent, bias = (torch.from_numpy(op[n]).to(DEV) for n in ('x', 'ent', 'bias'))
    f = op['filtered']
    mask = torch.from_numpy(R.pack_mask(f, case.spare)).to(DEV) if f is not None else None
    g = Guarded(case.B, case.k, strided=True)
    nat.score_topk(x, ent, bias, case.k, mask=mask, ent_row0=case.row0, out=g.out)
    score = nat.score_fwd(x, ent, bias).cpu()
    ids = np.arange(case.N, dtype=np.int64) + case.row0
    try:
        R.compare(g.s, g.i, *R.topk_ref(score, ids, case.k, f), label=case.label)
        g.check_untouched(case.label)
    except AssertionError as e:
        return str(e)
    SEEN_PASSES.update(p for p, _ in R.segment_traces(score, ids, case.k, f))
    return None


def run_all(pkg, cases):
    fails = [msg for msg in (run_select(pkg, c) for c in cases) if msg]
    assert not fails, '%d of %d cases fail:\n%s' % (len(fails), len(cases), '\n'.join(fails))


@pytest.mark.parametrize('N', R.SELECT_NS)
def test_select_segment_edges(pkg, N):
    """Every k around the pad sizes (and k = N where N <= 1024) at this N, on both arithmetic paths, unmasked and
    masked; masks that leave k - 1 / k / k + 1 columns in a segment and in the row; whole segments, bit 31 of every
    word and everything but the last column filtered; spare mask words; every ent_row0."""
    run_all(pkg, R.select_grid(N))


@pytest.mark.parametrize('N', R.CHUNK_NS)
def test_select_chunk_edges(pkg, N):
    """B = 2, O = 4 around the 2^18-row chunk: a last chunk of one row, mask0 != 0, ties planted across the chunk
    boundary, k = 10 and 1024 (at 2 * 2^18 + 4097 rows the running-list merge takes 66 560 entries: many windows)."""
    cases = R.chunk_grid(N)
    run_all(pkg, cases)
    if N > R.CHUNK:            # the planted ties at 1.0 are the top of every unmasked row, ids across the chunk boundary
        c = [c for c in cases if c.mask == 'none' and c.k == 10][0]
        op = R.select_operands(c)
        s, i = pkg._native.score_topk(*(torch.from_numpy(op[n]).to(DEV) for n in ('x', 'ent', 'bias')), 10, ent_row0=7)
        first = R.CHUNK - 3 + 7
        assert i[:, :min(6, N - R.CHUNK + 3)].tolist() == [list(range(first, min(first + 6, N + 7)))] * 2
        assert bool((s[:, :min(6, N - R.CHUNK + 3)] == 1.0).all())


def test_select_reaches_every_radix_pass(pkg):
    """Selections built to stop after each of the eight passes, each checked like every other case; then, over all the
    selection cases this module ran, passes 1 to 8 were each reached with the scores the GPU really produced."""
    run_all(pkg, R.depth_grid())
    assert SEEN_PASSES >= set(range(1, 9)), sorted(SEEN_PASSES)
