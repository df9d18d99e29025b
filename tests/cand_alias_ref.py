"""Reference of the weighted candidate draw (include/mgcn_hip.h (17)), written from the definition in Python
integers: Vose's alias table on m[n] = w[n] N against W in the pairing order DESIGN states, the distribution the table realises,
and the draw (cand_draw_ref.values plus the slot / coin / table rule). A plain module: nothing here is ported from the C++, which
tests/test_cand_alias_host.py and tests/test_gpu_cand_alias.py hold against it. No numpy arithmetic on the 64-bit paths."""
from collections import deque

import torch

from . import cand_draw_ref as R

TWO32 = 1 << 32
FULL = TWO32 - 1
M64 = (1 << 64) - 1


def build(w):
    """The table as a list of Python ints in [0, 2^63): alias << 32 | thr. The smalls wait in a FIFO that starts as their
    ascending ids, the larges are taken in ascending id; the head small is filled by the current large, which loses W - m; a large
    that drops below W joins the back of the FIFO, one that lands on W is finished; either way the next large takes over."""
    w = [int(v) for v in w]
    N, W = len(w), sum(w)
    assert N >= 1 and W >= 1 and all(0 <= v < TWO32 for v in w)
    m = [v * N for v in w]
    table = [None] * N
    small = deque(n for n in range(N) if m[n] < W)
    large = deque(n for n in range(N) if m[n] > W)
    for n in range(N):
        if m[n] == W:
            table[n] = n << 32 | FULL
    while small:
        s, L = small.popleft(), large[0]
        table[s] = L << 32 | (m[s] * TWO32) // W
        m[L] -= W - m[s]
        if m[L] <= W:
            large.popleft()
            if m[L] == W:
                table[L] = L << 32 | FULL
            else:
                small.append(L)
    assert not large and all(t is not None for t in table)
    return table


def signed(word):
    """The int64 that holds a 64-bit word."""
    word &= M64
    return word - (1 << 64) if word >> 63 else word


def table_tensor(table):
    return torch.tensor([signed(t) for t in table], dtype=torch.int64)


def counts(table):
    """cnt[n] = thr[n] + the sum of (2^32 - thr[m]) over every m whose alias is n, m == n included. Python ints."""
    cnt = [(t & M64) & FULL for t in table]
    for t in table:
        cnt[(t & M64) >> 32] += TWO32 - ((t & M64) & FULL)
    return cnt


def indegree(table):
    """The number of OTHER slots whose alias is n."""
    deg = [0] * len(table)
    for m, t in enumerate(table):
        if (t & M64) >> 32 != m:
            deg[(t & M64) >> 32] += 1
    return deg


def negative(r, N, table):
    """The id of a negative from its 64-bit value: slot = high half of r N, u = upper 32 bits of the low half, one table word."""
    p = r * N
    slot, u = p >> 64, (p & M64) >> 32
    t = int(table[slot]) & M64
    if u < (t & FULL):
        return slot
    alias = t >> 32
    return alias if alias < N else -1


def draw(qkey, keys, ptr, tails, num_entities, K, k, table, row0=0):
    """cand_draw_ref.draw with the negatives through `table` (a list of ints, signed or not)."""
    N = int(num_entities)
    cand, label = R.draw(qkey, keys, ptr, tails, N, K, k, row0)       # column 0 and its label are (15)'s
    keys_l, ptr_l, tails_l = keys.tolist(), ptr.tolist(), tails.tolist()
    at = {v: i for i, v in enumerate(keys_l)}
    r = R.values(k, qkey.numel(), K, row0)
    for b, q in enumerate(qkey.tolist()):
        i = at.get(q)
        known = set()
        if i is not None and 0 <= ptr_l[i] < ptr_l[i + 1] <= len(tails_l):
            known = set(tails_l[ptr_l[i]:ptr_l[i + 1]])
        for j in range(1, K):
            v = negative(r[b][j], N, table)
            cand[b, j] = v
            label[b, j] = int(0 <= v < N and v in known)
    return cand, label


def zipf_weights(n, a=1.1, scale=1 << 20):
    """Integer weights floor(scale / rank^a), rank 1 first, at least 1: fixed, no RNG."""
    return [max(1, int(scale / float(i + 1) ** a)) for i in range(n)]


# The weight grid of the table tests: (name, weights).
WEIGHT_GRID = (
    ('one', [5]),
    ('two_extreme', [1, TWO32 - 1]),
    ('five_one_zero', [3, 0, 7, 1, 9]),
    ('equal', [6] * 9),
    ('single_nonzero', [0, 0, 4, 0, 0, 0]),
    ('zipf_4097', zipf_weights(4097)),
)

# The (B, K) grid of test_cand_draw_host.py, extended: K = 1 (the table is never read), K = 2, odd K.
GRID_K, GRID_B = (1, 2, 3, 7, 64, 65), R.GRID_B
GRID_ROW0 = (0, 3, 2 ** 32 + 5)
