"""Reference of the counter-drawn candidate lists (include/mgcn_hip.h (15)), written from the definition in Python
integers and numpy: SplitMix64 key with the site id 0x2000, Philox4x32-10 words with counter (row_lo, row_hi, j >> 1, 0), the
64-bit value of a position from two words, the id as the high half of a 128-bit product. A plain module: nothing here is ported
from csrc/dropout.hip, which tests/test_cand_draw_host.py and tests/test_gpu_cand_draw.py hold against it."""
import numpy as np
import torch

from . import dropout_ref as D

SITE = 0x2000


def key(seed, step):
    return D.key(seed, step, SITE)


def values(k, B, K, row0=0):
    """r of every list position of a [B, K] block whose first row is the global batch row `row0`: a list of B lists of K Python
    ints below 2^64."""
    npair = (K + 1) // 2
    row = [(int(row0) + b) & D.M64 for b in range(B)]
    r_lo = np.array([v & 0xffffffff for v in row], dtype=np.uint64).reshape(B, 1)
    r_hi = np.array([v >> 32 for v in row], dtype=np.uint64).reshape(B, 1)
    jp = np.arange(npair, dtype=np.uint64).reshape(1, npair)
    w = [np.broadcast_to(o, (B, npair)).tolist() for o in
         D.philox4x32_10(r_lo, r_hi, jp, np.zeros((1, 1), dtype=np.uint64), k & 0xffffffff, k >> 32)]
    out = []
    for b in range(B):
        line = []
        for j in range(K):
            a, c = (w[0], w[1]) if j % 2 == 0 else (w[2], w[3])
            line.append(int(a[b][j // 2]) | (int(c[b][j // 2]) << 32))
        out.append(line)
    return out


# The grid both test files walk. The index has runs of length 1, 3, 0 and 5 (tails ascending within a run); the queries cycle over
# its four keys and over a key below the smallest, between two and above the largest.
GRID_K, GRID_B, GRID_N, GRID_ROW0 = (1, 2, 3, 64, 65), (1, 5, 67), (1, 7, 40943, 2 ** 40), (0, 3, 2 ** 32 + 1)


def grid_index():
    """(keys, ptr, tails) on the CPU."""
    return (torch.tensor([10, 20, 30, 40]), torch.tensor([0, 1, 4, 4, 9]), torch.tensor([5, 0, 3, 6, 1, 2, 4, 5, 6], dtype=torch.int32))


def grid_queries(B):
    return torch.tensor([(20, 10, 40, 5, 30, 25, 99)[b % 7] for b in range(B)])


def malformed_index():
    """Key 10: a good run; 20: a run that leaves [0, n_tails]; 30: a reversed run; 40: a run that starts below 0."""
    return (torch.tensor([10, 20, 30, 40]), torch.tensor([0, 2, 50, 4, 3]), torch.tensor([1, 4, 2, 3], dtype=torch.int32)), \
        (torch.tensor([10, 20, 30, 40]), torch.tensor([-1, 2, 2, 2, 4]), torch.tensor([1, 4, 2, 3], dtype=torch.int32))


def draw(qkey, keys, ptr, tails, num_entities, K, k, row0=0):
    """(cand [B, K] int64, label [B, K] uint8) on the CPU. Column 0: one tail of the query's run, -1 without a usable run (key
    absent; run empty, reversed or outside [0, len(tails)]); columns >= 1: (r N) >> 64. label: the id is an entity and a member of
    the run."""
    keys_l, ptr_l, tails_l = keys.tolist(), ptr.tolist(), tails.tolist()
    at = {v: i for i, v in enumerate(keys_l)}
    N, B = int(num_entities), qkey.numel()
    r = values(k, B, K, row0)
    cand = torch.empty((B, K), dtype=torch.int64)
    label = torch.zeros((B, K), dtype=torch.uint8)
    for b, q in enumerate(qkey.tolist()):
        i = at.get(q)
        run = []
        if i is not None and 0 <= ptr_l[i] < ptr_l[i + 1] <= len(tails_l):
            run = tails_l[ptr_l[i]:ptr_l[i + 1]]
        known = set(run)
        for j in range(K):
            if j == 0:
                v = run[(r[b][0] * len(run)) >> 64] if run else -1
            else:
                v = (r[b][j] * N) >> 64
            cand[b, j] = v
            label[b, j] = int(0 <= v < N and v in known)
    return cand, label
