"""What csrc/topk.hip is held to: the order of section (7) of include/mgcn_hip.h as a total order on f32 bit patterns,
the top-k it defines, a host model of the radix select (used ONLY to show which path a case takes, never as an expected
value), and the case grids that put scores, candidate counts, ids and k on the kernels' internal boundaries. numpy and
torch-CPU only.

The order. A candidate ranks by (score descending, id ascending). Scores compare as f32 VALUES, so -0 == +0; the header
extends that to a total order: a NaN with the sign bit clear ranks above +inf, a NaN with the sign bit set below -inf,
NaNs among themselves by bit pattern (IEEE totalOrder with the two zeros merged). order_key computes it in integers from
the sign and the magnitude; it shares no code and no formula with the kernel's key.

Every expected value in the GPU tests is topk_ref of exact inputs: for the merge the crafted lists themselves, for
score_topk the block mgcn_score_fwd returned for the same operands (the header promises those bits). Nothing is rounded,
so there is no tolerance: ids are compared exactly and scores bit for bit (zeros by value, NaNs as NaNs)."""
import collections
import zlib

import numpy as np
import torch

SEG = 4096            # topk.hip TK_SEG: score columns per SELECT workgroup
CAP = 8192            # TK_CAP: candidates a workgroup holds in LDS
KMAX = 1024           # TK_KMAX
CHUNK = 2 ** 18       # TK_CHUNK: entity rows scored per pass
THREADS = 512         # TK_THREADS

NEG_INF_BITS = 0xff800000
ID_MAX = 2 ** 31 - 1


# ----------------------------------------------------------------------------------------------------------------
# the order and the reference
def bits_of(score):
    """f32 tensor / array (or uint32 bit patterns) -> np.uint32 bit patterns; no float arithmetic touches a value."""
    if isinstance(score, torch.Tensor):
        assert score.dtype == torch.float32
        return score.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)
    a = np.ascontiguousarray(score)
    if a.dtype == np.uint32:
        return a
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def floats_of(bits):
    """np.uint32 bit patterns -> torch f32 tensor with exactly those bits."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def order_key(score_bits):
    """int64 rank of f32 bit patterns: a > b as the header orders scores  <=>  order_key(a) > order_key(b).
    Sign and magnitude: +x -> mag, -x -> -mag, so +0 and -0 are both 0, infinities sit at +-0x7f800000 and NaNs beyond
    them on their sign's side, ordered by pattern."""
    b = np.asarray(score_bits, dtype=np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    return np.where((b >> 31) == 0, mag, -mag)


def _ids2d(ids, shape):
    i = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    return np.broadcast_to(i.astype(np.int64), shape)


def topk_ref(score, ids, k, filtered=None):
    """(scores [B, k] f32, ids [B, k] int64), torch-CPU, from the header's words: drop the filtered entries and the
    padding (id < 0), sort by (order_key descending, id ascending), first k, pad with (-inf, -1)."""
    bits = bits_of(score)
    B, n = bits.shape
    ids = _ids2d(ids, (B, n))
    live = ids >= 0
    if filtered is not None:
        f = filtered.detach().cpu().numpy() if isinstance(filtered, torch.Tensor) else np.asarray(filtered)
        live = live & ~f.astype(bool)
    out_b = np.full((B, k), NEG_INF_BITS, dtype=np.uint32)
    out_i = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        sb, si = bits[b][live[b]], ids[b][live[b]]
        o = np.lexsort((si, -order_key(sb)))[:k]
        out_b[b, :o.size], out_i[b, :o.size] = sb[o], si[o]
    return floats_of(out_b), torch.from_numpy(out_i)


def compare(got_s, got_i, want_s, want_i, label=''):
    """Ids exactly; scores bit for bit, except zeros (by value) and NaNs (both NaN). Raises AssertionError."""
    gi, wi = _ids2d(got_i, tuple(got_i.shape)), _ids2d(want_i, tuple(want_i.shape))
    gb, wb = bits_of(got_s), bits_of(want_s)
    assert gi.shape == wi.shape and gb.shape == wb.shape == gi.shape, (label, gi.shape, wi.shape, gb.shape, wb.shape)
    bad = np.argwhere(gi != wi)
    if bad.size:
        r, c = bad[0]
        raise AssertionError('%s: %d ids differ, first at [%d, %d]: got %d (score %#010x), want %d (score %#010x)'
                             % (label, len(bad), r, c, gi[r, c], gb[r, c], wi[r, c], wb[r, c]))
    mag_g, mag_w = gb & 0x7fffffff, wb & 0x7fffffff
    same = (gb == wb) | ((mag_g == 0) & (mag_w == 0)) | ((mag_g > 0x7f800000) & (mag_w > 0x7f800000))
    bad = np.argwhere(~same)
    if bad.size:
        r, c = bad[0]
        raise AssertionError('%s: %d scores differ, first at [%d, %d] (id %d): got %#010x, want %#010x'
                             % (label, len(bad), r, c, gi[r, c], gb[r, c], wb[r, c]))


# ----------------------------------------------------------------------------------------------------------------
# host model of the select: which passes a set of candidates takes (coverage only)
def radix_key32(score_bits):
    """An order-preserving unsigned 32-bit key as the header describes the select's: -0 folded onto +0, then the usual
    flip (sign set: all bits inverted; sign clear: sign bit set). Same order as order_key (the host test checks it)."""
    u = np.asarray(score_bits, dtype=np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order_words(score_bits, ids):
    """The 64-bit words the select walks: key above, inverted id below (a lower id is a larger word)."""
    return (radix_key32(score_bits).astype(np.uint64) << np.uint64(32)) | (~np.asarray(ids, dtype=np.int64).astype(np.uint32)).astype(np.uint64)


def trace_words(words, k):
    """(passes, threshold digits) of a radix select of the k largest of len(words) > k distinct words: 8-bit digits,
    best first, stop when the threshold digit's bin holds exactly what is still needed."""
    assert len(words) > k
    need, live, digits = k, words, []
    for shift in range(56, -1, -8):
        d = ((live >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        hist = np.bincount(d, minlength=256)
        cum = np.cumsum(hist[::-1])                      # cum[i]: words whose digit is >= 255 - i
        i = int(np.searchsorted(cum, need))
        digit = 255 - i
        need -= int(cum[i] - hist[digit])
        digits.append(digit)
        if hist[digit] == need:
            return len(digits), digits
        live = live[d == digit]
    raise AssertionError('the words are not distinct')


def radix_trace(score, ids, k, filtered=None):
    """Per row: (passes, [threshold digit of each pass]) of selecting the k best of the row's candidates in one fill;
    (0, []) when the row has no more than k candidates (no select runs)."""
    bits = bits_of(score)
    ids = _ids2d(ids, bits.shape)
    live = ids >= 0
    if filtered is not None:
        f = filtered.detach().cpu().numpy() if isinstance(filtered, torch.Tensor) else np.asarray(filtered)
        live = live & ~f.astype(bool)
    out = []
    for b in range(bits.shape[0]):
        w = order_words(bits[b][live[b]], ids[b][live[b]])
        out.append(trace_words(w, k) if len(w) > k else (0, []))
    return out


Window = collections.namedtuple('Window', 'filled passes digits')   # filled: candidates held after the window's fill


def merge_trace(score_row, ids_row, k):
    """The merge of one row in windows, as topk.hip's header describes it: the next min(CAP - held, rest) entries are
    appended after the candidates held (padding dropped); more than k held -> a select keeps the k best."""
    bits, ids = bits_of(score_row).reshape(-1), np.asarray(ids_row, dtype=np.int64).reshape(-1)
    held, pos, out = np.empty(0, dtype=np.uint64), 0, []
    while True:
        take = min(CAP - len(held), len(ids) - pos)
        sl = slice(pos, pos + take)
        ok = ids[sl] >= 0
        held = np.concatenate([held, order_words(bits[sl][ok], ids[sl][ok])])
        pos += take
        if len(held) > k:
            passes, digits = trace_words(held, k)
            out.append(Window(len(held), passes, digits))
            held = np.sort(held)[::-1][:k]
        else:
            out.append(Window(len(held), 0, []))
        if pos >= len(ids):
            return out


def segment_traces(score, ids, k, filtered=None):
    """radix_trace of every (row, chunk, segment) of a score_topk call: the SELECT workgroups' fills."""
    bits = bits_of(score)
    ids = _ids2d(ids, bits.shape)
    out = []
    for c0 in range(0, bits.shape[1], CHUNK):
        for s0 in range(c0, min(c0 + CHUNK, bits.shape[1]), SEG):
            s1 = min(s0 + SEG, c0 + CHUNK, bits.shape[1])
            f = None if filtered is None else filtered[:, s0:s1]
            out += radix_trace(bits[:, s0:s1], ids[:, s0:s1], k, f)
    return out


# ----------------------------------------------------------------------------------------------------------------
# bit patterns on every boundary of the order
def _around(b):
    return [(b + d) & 0xffffffff for d in (-1, 0, 1)]


BOUNDARY_BITS = sorted(set(sum((_around(b) for b in (
    0x00000000, 0x80000000,               # +0, -0 (and their neighbours: the denormal minima, -NaN 0xffffffff, +NaN 0x7fffffff)
    0x00000001, 0x80000001,               # +- denormal min
    0x007fffff, 0x807fffff,               # +- denormal max
    0x00800000, 0x80800000,               # +- FLT_MIN
    0x7f7fffff, 0xff7fffff,               # +- FLT_MAX
    0x7f800000, 0xff800000,               # +- inf
    0x7fc00000, 0xffc00000,               # +- quiet NaN
    0x7fffffff, 0xffffffff,               # the last NaN of each sign
    0x3f800000, 0xbf800000, 0x3f000000,   # +-1, 0.5
    0x01000000, 0x81000000, 0x7f000000, 0xff000000,   # top-byte boundaries of the key
)), [])))


def is_nan_bits(b):
    return (np.asarray(b, dtype=np.uint32) & 0x7fffffff) > 0x7f800000


POOL = np.array(BOUNDARY_BITS, dtype=np.uint32)
POOL_NO_NEG_NAN = POOL[~(is_nan_bits(POOL) & (POOL >> 31 == 1))]


def _rng(label):
    return np.random.default_rng(zlib.crc32(label.encode()))


def distinct_ids(rng, n, lo=0, hi=2 ** 31, must=()):
    """n distinct ids of [lo, hi) in random order, the ids in `must` among them."""
    must = [m for m in must][:n]
    v = np.unique(np.concatenate([rng.integers(lo, hi, size=n + n // 8 + 16, dtype=np.int64),
                                  np.array(must, dtype=np.int64)]))
    v = np.setdiff1d(v, np.array(must, dtype=np.int64))
    rng.shuffle(v)
    assert len(v) >= n - len(must)
    v = np.concatenate([np.array(must, dtype=np.int64), v[:n - len(must)]])
    rng.shuffle(v)
    return v


# ----------------------------------------------------------------------------------------------------------------
# the merge grid: crafted (score bits, ids) rows, [B, lists * k]
MergeCase = collections.namedtuple('MergeCase', 'label k lists bits ids')

PAD_IDS = np.array([-1, -7, -2 ** 31, -2 ** 63], dtype=np.int64)
PAD_SCORE_BITS = np.array([0xff800000, 0x7f800000, 0x3f800000, 0x7fc00000, 0x00000000], dtype=np.uint32)   # live-looking scores under a padding id

SCORE_MODES = ('bits', 'pool', 'ties', 'ulp', 'unit')


def _scores(rng, mode, n):
    if mode == 'bits':                    # any pattern: every top byte, both signs, the odd NaN
        return rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    if mode == 'pool':                    # the boundaries, NaNs of both signs included: heavy ties on each
        return rng.choice(POOL, size=n)
    if mode == 'ties':                    # five values: blocks of equal scores, k cuts through one
        return rng.choice(np.array([0x3f800000, 0x3f000000, 0x80000000, 0x00000000, 0xbf800000, 0xff800000], dtype=np.uint32), size=n)
    if mode == 'ulp':                     # adjacent floats: scores that differ in the last mantissa byte only
        return (np.uint32(0x3f000000) + rng.integers(0, 256, size=n).astype(np.uint32)).astype(np.uint32)
    if mode == 'unit':                    # [0, 1): what a sigmoid feeds the kernel
        return rng.random(n, dtype=np.float32).view(np.uint32)
    raise ValueError(mode)


def _pad(rng, bits, ids, where):
    """Turn the entries `where` into padding: a negative id under a score that would win if it counted."""
    n = int(where.sum())
    ids[where] = rng.choice(PAD_IDS, size=n)
    bits[where] = rng.choice(PAD_SCORE_BITS, size=n)


def _merge_case(label, k, lists, pad, modes=('bits', 'pool', 'ties'), first=None):
    """pad: 'dense' | 'interleaved' | 'all' | 'head' (the first window all padding, candidates after it) |
    'few' (the first window leaves `first[b]` candidates, more follow)."""
    rng = _rng(label)
    L, B = lists * k, len(modes)
    bits = np.empty((B, L), dtype=np.uint32)
    ids = np.empty((B, L), dtype=np.int64)
    for b, mode in enumerate(modes):
        bits[b] = _scores(rng, mode, L)
        ids[b] = distinct_ids(rng, L, must=(0, ID_MAX))
        where = np.zeros(L, dtype=bool)
        if pad == 'interleaved':
            where = rng.random(L) < 0.5
        elif pad == 'all':
            where[:] = True
        elif pad == 'head':
            assert L > CAP
            where[:CAP] = True
        elif pad == 'few':
            assert L > CAP
            where[:CAP] = True
            where[rng.permutation(CAP)[:first[b]]] = False
        else:
            assert pad == 'dense'
        _pad(rng, bits[b], ids[b], where)
    return MergeCase(label, k, lists, bits, ids)


def _placed(label, k, lists, rows):
    """rows: per row a list of (score bits, id) candidates, at most lists * k; the rest of the row is padding and the
    whole row is shuffled (unsorted lists, padding anywhere)."""
    rng = _rng(label)
    L = lists * k
    bits = np.empty((len(rows), L), dtype=np.uint32)
    ids = np.empty((len(rows), L), dtype=np.int64)
    for b, row in enumerate(rows):
        assert len(row) <= L and len({i for _, i in row}) == len(row)
        where = np.ones(L, dtype=bool)
        _pad(rng, bits[b], ids[b], where)
        p = rng.permutation(L)[:len(row)]
        bits[b, p] = np.array([s for s, _ in row], dtype=np.uint32)
        ids[b, p] = np.array([i for _, i in row], dtype=np.int64)
    return MergeCase(label, k, lists, bits, ids)


F = lambda v: int(np.float32(v).view(np.uint32))      # bit pattern of a float value

WINDOW_SETS = [(1, 8191), (1, 8192), (1, 8193), (1, 16382), (1, 16383), (1, 16384),      # total = CAP - 1, CAP, CAP + 1; CAP + (CAP - 1) exactly and +- 1
               (1024, 1), (1024, 7), (1024, 8), (1024, 9), (1024, 14), (1024, 15), (1024, 16),   # 8 fills the first window, 15 the second exactly
               (7, 1170), (7, 1171),                                         # 8190 / 8197: a window edge that is no multiple of k
               (1000, 9)]                                                    # 9000: second window of 808
SMALL_KS = (2, 3, 64, 65, 511, 512, 513, 1023)                               # around the bitonic pad P = 2^ceil(log2 k)
MERGE_KS = tuple(sorted({k for k, _ in WINDOW_SETS} | set(SMALL_KS)))


def tie_rows(M, k, a=5, b=6):
    """Three rows whose threshold falls in a block of a + b equal scores with consecutive ids M - a .. M + b - 1:
    the row needs a - 1, a and a + 1 of the block (after k - that many better candidates). Needing exactly the a ids
    below M lets the select stop at the id byte that M changes; one more or fewer walks every id byte."""
    rows = []
    for t in (a - 1, a, a + 1):
        better = [(F(2.0), (M * 3 + 17 * j + 1) % ID_MAX) for j in range(k - t)]
        block = [(F(1.0), M - a + j) for j in range(a + b)]
        worse = [(F(0.5), (M * 5 + 13 * j + 2) % ID_MAX) for j in range(3)]
        rows.append(better + block + worse)
    return rows


def merge_grid():
    cases = []
    for k, lists in WINDOW_SETS:
        L = k * lists
        tag = 'k%d x %d = %d' % (k, lists, L)
        where = ('one window' if L <= CAP else '%d windows' % len(merge_trace(np.zeros(L, np.float32), np.zeros(L, np.int64) - 1, k)))
        cases.append(_merge_case('%s, dense, %s' % (tag, where), k, lists, 'dense'))
        cases.append(_merge_case('%s, padding interleaved' % tag, k, lists, 'interleaved', modes=('unit', 'pool', 'ulp')))
        if L > CAP:
            cases.append(_merge_case('%s, first window all padding' % tag, k, lists, 'head', modes=('pool', 'bits', 'ties')))
            cases.append(_merge_case('%s, first window leaves k - 1 / k / k + 1' % tag, k, lists, 'few',
                                     modes=('bits', 'unit', 'pool'), first=(k - 1, k, k + 1)))
    for k in SMALL_KS:
        for lists, pad in ((1, 'dense'), (2, 'interleaved'), (5, 'dense'), (3, 'all' if k in (3, 512) else 'interleaved')):
            cases.append(_merge_case('k%d x %d, %s' % (k, lists, pad), k, lists, pad,
                                     modes=('ulp', 'pool', 'ties') if lists == 5 else ('bits', 'pool', 'unit')))
    # ties at the threshold with the tied ids across a multiple of 256, 65 536 and 2^24
    for M in (256, 65536, 2 ** 24, 2 ** 24 * 77 + 65536 * 3):
        cases.append(_placed('ties across id %d, need 4 / 5 / 6 of the 5 below' % M, 7, 3, tie_rows(M, 7)))
    cases.append(_placed('ties across id 2^24 at k = 512', 512, 2, tie_rows(2 ** 24, 512, a=100, b=300)))
    # one ulp apart, k through the run; every id distinct and large
    run = [(0x3f7fff00 + j, ID_MAX - 3 * j) for j in range(40)]
    cases.append(_placed('scores one ulp apart', 7, 8, [run, run[::-1], run[5:]]))
    # (-inf, valid id) beats padding and keeps its id; a NaN with the sign bit set ranks below it and still above padding
    ninf = [(0xff800000, i) for i in (ID_MAX, 0, 77, 2 ** 24)]
    cases.append(_placed('(-inf, id) next to (-inf, -1)', 7, 3,
                         [ninf, ninf + [(0xffc00000, 5), (0xffffffff, 6), (0xfffffffe, 3)], ninf[:1]]))
    # the two zeros are one score: ids decide
    zeros = [(0x80000000, 5), (0x00000000, 9), (0x80000000, ID_MAX), (0x00000000, 0), (0x80000001, 1), (0x80000000, 2)]
    cases.append(_placed('-0 and +0 tie, ids decide', 3, 2, [zeros, zeros[:4], zeros[::-1][:5]]))
    # the threshold in the lowest and the highest top byte of the key (scan lanes 63 and 0)
    low = [(F(3.0), 11), (F(1.0), 12), (F(0.5), 13), (0x00000001, 14), (0x80000001, 15), (F(-2.0), 16), (0xff7fffff, 17), (0xff800000, 18)]
    high = [(0x7f800000, 21), (0x7f7fffff, 22), (0x7f000000, 23), (0x7fc00000, 24), (F(1.0), 25)]
    cases.append(_placed('threshold in top byte 0 / 255', 7, 2, [low, low + [(0xffc00000, 19)], low[1:]]))
    cases.append(_placed('threshold in top byte 255', 2, 4, [high, high[1:], high[::-1]]))
    # NaNs of one sign, distinct payloads: ordered by pattern (0xffffffff below 0xfffffffe)
    nans = [(0xffffffff, 1), (0xfffffffe, 2), (0xff800001, 3), (0x7f800001, 4), (0x7fffffff, 5), (0x7ffffffe, 6), (0xff800000, 7)]
    cases.append(_placed('NaN payloads in pattern order', 3, 3, [nans, nans[:3], nans[::-1][:6]]))
    cases.append(_placed('NaN payloads in pattern order, k = 6', 6, 2, [nans, nans[:2] + nans[6:], nans[:3]]))
    labels = [c.label for c in cases]
    assert len(set(labels)) == len(labels)
    return cases


# ----------------------------------------------------------------------------------------------------------------
# the selection grid: operands of score_topk whose scores can be steered
SelectCase = collections.namedtuple('SelectCase', 'label N k O row0 B profile plant mask spare')

SELECT_NS = (1, 2, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 3 * SEG + 5)
SELECT_KS = (1, 2, 3, 7, 64, 65, 511, 512, 513, 1000, 1023, 1024)
CHUNK_NS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + SEG + 1)
ROW0S = lambda N: (0, 7, 2 ** 24 - 100, ID_MAX - N)

HIGH_SAT = (20.0, 30.0, 17.5)                                   # sigmoid rounds to exactly 1.0f
LOW_SAT = (-110.0, -95.0, -88.5, -88.0, -87.5, -87.0, -50.0)    # underflow to +0, the denormal range, a tiny normal


def select_operands(case):
    """-> dict(x [B, O], ent [N, O], bias [N], filtered bool [B, N] or None), numpy f32. Row 0 of x is zero, row b > 0 is
    one-hot at b - 1, so score[0] ~ sigmoid(bias) and score[b] ~ sigmoid(ent[:, b - 1] + bias). bias mixes a cluster of
    adjacent floats around 0.5 (steps of 1e-7), a wide spread and both saturations ('mixed'; 'wide' leaves the high
    saturation out); each `plant` = (first column, count) puts `count` columns at exactly 1.0f in every row. Profiles
    'plant', 'steps' and 'pair' keep everything else in the cluster, so what they place decides the threshold."""
    rng = _rng(case.label)
    N, O, B = case.N, case.O, case.B
    x = np.zeros((B, O), dtype=np.float32)
    for b in range(1, B):
        x[b, b - 1] = 1.0
    kind = rng.choice(3, size=N, p=(0.5, 0.3, 0.2))
    cluster = (1e-7 * rng.integers(-3000, 3001, size=N)).astype(np.float32)
    wide = (6.0 * rng.standard_normal(N)).astype(np.float32)
    sat = rng.choice(np.array(LOW_SAT + (HIGH_SAT if case.profile == 'mixed' else ()), dtype=np.float32), size=N)
    bias = np.where(kind == 0, cluster, np.where(kind == 1, wide, sat)).astype(np.float32)
    if case.profile in ('plant', 'steps', 'pair'):
        bias = cluster
    elif case.profile == 'wide':          # chunk cases: nothing saturates high, so the planted ties are the top
        bias = np.where(kind == 2, sat, np.where(kind == 0, cluster, np.clip(wide, -12.0, 12.0))).astype(np.float32)
    ent = (0.5 * rng.standard_normal((N, O))).astype(np.float32)
    ent[:, 0] = (3.0 * rng.standard_normal(N)).astype(np.float32) if case.profile == 'mixed' else cluster[::-1]
    if O > 1:
        ent[:, 1] = (1e-7 * rng.integers(-3000, 3001, size=N)).astype(np.float32)
    if case.profile == 'plant' and N > 7:     # one column just above the cluster: a unique best of the unplanted columns
        bias[7], ent[7] = 3001e-7, 0.0
    if case.profile == 'steps':               # 0.5 + j 2^-10: apart in the third key byte, far above the cluster
        bias[20:23], ent[20:23] = 4.0 * 2.0 ** -10 * np.arange(1, 4, dtype=np.float32), 0.0
    if case.profile == 'pair':                # far apart: different top key bytes
        bias[:], ent[:] = np.where(np.arange(N) % 2 == 0, 5.0, -5.0), 0.0
    for c0, cnt in case.plant:
        c0, c1 = max(c0, 0), min(c0 + cnt, N)
        bias[c0:c1] = 30.0
        ent[c0:c1] = 0.0
    return dict(x=x, ent=ent, bias=bias, filtered=select_mask(case, rng))


def select_mask(case, rng):
    """Dense bool [B, N], True = filtered. 'exact:seg:S' / 'exact:row' leave k - 1, k and k + 1 live columns (rows 0,
    1, 2) in segment S (50 % elsewhere) / in the whole row."""
    N, B, k, m = case.N, case.B, case.k, case.mask
    if m == 'none':
        return None
    f = np.zeros((B, N), dtype=bool)
    if m == 'random':
        f = rng.random((B, N)) < 0.3
    elif m == 'segments':                 # whole segments: every even one; row 1 the odd ones
        seg = np.arange(N) // SEG
        for b in range(B):
            f[b] = seg % 2 == b % 2
    elif m == 'bit31':
        f[:, 31::32] = True
    elif m == 'last':
        f[:, :N - 1] = True
    elif m.startswith('exact'):
        for b in range(B):
            want = max(k - 1 + b, 0)
            if m == 'exact:row':
                cols = np.arange(N)
                f[b] = True
            else:
                s = int(m.split(':')[2])
                cols = np.arange(s * SEG, min((s + 1) * SEG, N))
                f[b] = rng.random(N) < 0.5
                f[b, cols] = True
            assert len(cols) >= want, (case.label, len(cols), want)
            f[b, rng.permutation(cols)[:want]] = False
    else:
        raise ValueError(m)
    return f


def pack_mask(filtered, spare=0):
    """bool [B, N] -> int32 words [B, ceil(N / 32) + spare], bit (n & 31) of word n >> 5. The bits past N and the spare
    words are all SET: they name no entity and must not be read as one."""
    B, N = filtered.shape
    words = (N + 31) // 32 + spare
    full = np.ones((B, words * 32), dtype=bool)
    full[:, :N] = filtered
    w = np.packbits(full.reshape(B, words, 32), axis=2, bitorder='little')
    return np.ascontiguousarray(w).view('<u4').reshape(B, words).view(np.int32)


def _sel(label, N, k, O=4, row0=0, B=3, profile='mixed', plant=(), mask='none', spare=0):
    return SelectCase('N%d k%d O%d row0 %d %s: %s' % (N, k, O, row0, mask, label), N, k, O, row0, B, profile, tuple(plant), mask, spare)


def select_ks(N):
    return tuple(sorted(set(SELECT_KS) | ({N} if N <= KMAX else set())))


def select_grid(N):
    """The cases of one N: every k unmasked on the split path (O = 4) and randomly masked on the exact path (O = 3, with
    two spare mask words), the counted and the structural masks, every ent_row0."""
    segs = (N + SEG - 1) // SEG
    path = 'one segment, direct' if segs == 1 else '%d segments + merge of %d lists' % (segs, segs)
    out = []
    for j, k in enumerate(select_ks(N)):
        out.append(_sel(path, N, k, O=4, row0=ROW0S(N)[j % 4]))
        out.append(_sel(path + ', masked', N, k, O=3, row0=ROW0S(N)[(j + 1) % 4], mask='random', spare=2 * (j % 2)))
    for k in (1, 3, 64, 65, 512, 1024):
        if k + 1 <= N:
            out.append(_sel('count k - 1 / k / k + 1 in the row', N, k, mask='exact:row', O=3 + k % 2))
        for s in sorted({0, max(segs - 2, 0)}):   # (the last segment may hold a single column)
            if k + 1 <= min(SEG, N - s * SEG):
                out.append(_sel('count k - 1 / k / k + 1 in segment %d' % s, N, k, mask='exact:seg:%d' % s, spare=2, row0=7))
    for k in (1, 65, 1024):
        for m in ('segments', 'bit31', 'last'):
            out.append(_sel('structural mask', N, k, mask=m, row0=ROW0S(N)[2], O=3 if m == 'last' else 4))
    return out


def chunk_grid(N):
    """B = 2, O = 4: chunks of 2^18 rows, ties planted across the chunk boundary, with and without a mask."""
    chunks = (N + CHUNK - 1) // CHUNK
    tail = N - (chunks - 1) * CHUNK
    out = []
    for k in (10, 1024):
        lists = (CHUNK // SEG) + 1 if chunks > 1 else (N + SEG - 1) // SEG
        path = '%d chunks, last of %d rows; merges of up to %d entries' % (chunks, tail, lists * k)
        for mask in ('none', 'random'):
            out.append(_sel(path, N, k, O=4, row0=7, B=2, profile='wide', plant=((CHUNK - 3, 6),), mask=mask))
    return out


def depth_grid():
    """Selections built to stop after each of the eight radix passes (what score_fwd returns decides; the GPU test
    asserts the depth from the scores it got). One segment (direct) and two segments (through the merge)."""
    out = []
    for N in (513, SEG + 1):
        pl = lambda c0, n: ((c0, n),)
        out += [
            _sel('3 at 1.0 over a cluster at 0.5, k = 3: second key byte decides', N, 3, profile='plant', plant=pl(40, 3)),
            _sel('cluster of adjacent floats, k = 1 / 2: last key byte', N, 1, profile='plant'),
            _sel('cluster of adjacent floats, k = 1 / 2: last key byte', N, 2, profile='plant', O=3),
            _sel('three steps of 2^-10 above the cluster, k = 2: third key byte', N, 2, profile='steps'),
            _sel('ties across id 2^24, need exactly the 5 below: top id byte', N, 5, row0=2 ** 24 - 100, profile='plant', plant=pl(95, 11)),
            _sel('ties across id 2^24, need 4 of the 5 below: all id bytes', N, 4, row0=2 ** 24 - 100, profile='plant', plant=pl(95, 11)),
            _sel('ties across id 3 * 65536, need exactly the 5 below: second id byte', N, 5, row0=3 * 65536 - 100, profile='plant', plant=pl(95, 11)),
            _sel('ties across id 256, need exactly the 5 below: third id byte', N, 5, profile='plant', plant=pl(251, 11)),
            _sel('ties across id 256, need 6: last id byte', N, 6, profile='plant', plant=pl(251, 11)),
        ]
    out.append(_sel('two columns far apart, k = 1: top key byte decides', 2, 1, B=1, profile='pair'))
    return out
