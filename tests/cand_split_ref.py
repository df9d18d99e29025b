"""References for the list backward with split runs (include/mgcn_hip.h (18)). A plain module:
tests/test_cand_split_ref_host.py checks it on the CPU, tests/test_gpu_cand_split.py holds the kernels to it.

  * emul_ent_split_f32   the order of mgcn_cand_bce_bwd_ent_split in numpy f32: a run is cut into pieces of S plan entries counted
                         from its own first entry, a piece is cand_train_ref.emul_ent_f32's loop, a row the sequential sum of
                         its pieces' partials from +0;
  * plan_runs, piece_heads, slot_of, window_first   the integer side: the runs of a sorted row sequence, their piece heads, the
                         workspace slot of a head and the per-window first entry, as the header states them;
  * split_lists, one_id_lists   hand-built lists whose runs have the lengths the kernels' paths turn on.
Liveness and rows are cand_train_ref's."""
import math

import numpy as np
import torch

from . import cand_train_ref as C


def plan_rows(cand, perm, n_live, n_local, row0=0):
    """The row of every entry of the plan's live prefix as the kernels recompute it: -1 for an entry outside [0, B K) or dead."""
    live, row = C.live_rows(cand, row0, n_local)
    live, row = live.numpy().reshape(-1), row.numpy().reshape(-1)
    total = live.size
    return [int(row[p]) if 0 <= p < total and live[p] else -1 for p in perm.cpu().tolist()[:n_live]]


def plan_runs(rows):
    """[(first entry, length, row)] of the maximal stretches of equal valid rows, in plan order."""
    runs, i = [], 0
    while i < len(rows):
        if rows[i] < 0:
            i += 1
            continue
        k = i
        while k < len(rows) and rows[k] == rows[i]:
            k += 1
        runs.append((i, k - i, rows[i]))
        i = k
    return runs


def emul_ent_split_f32(g, cand, x, perm, n_live, n_local, S, row0=0, d_ent=None, d_bias=None):
    """(d_ent, d_bias) f32 after mgcn_cand_bce_bwd_ent_split with run_split = S on the given plan. Rows no run names keep what
    d_ent / d_bias held."""
    g, x = g.cpu().numpy().astype(np.float32), x.cpu().numpy().astype(np.float32)
    B, K = g.shape
    gf = g.reshape(-1)
    d_ent = np.zeros((n_local, x.shape[1]), dtype=np.float32) if d_ent is None else d_ent.cpu().numpy().copy()
    d_bias = np.zeros(n_local, dtype=np.float32) if d_bias is None else d_bias.cpu().numpy().copy()
    plan = perm.cpu().tolist()[:n_live]
    for s, L, r in plan_runs(plan_rows(cand, perm, n_live, n_local, row0)):
        acc, sb = np.zeros(x.shape[1], dtype=np.float32), np.float32(0.0)
        for p0 in range(s, s + L, S):
            part, pb = np.zeros(x.shape[1], dtype=np.float32), np.float32(0.0)
            for k in range(p0, min(p0 + S, s + L)):
                part = part + gf[plan[k]] * x[plan[k] // K]
                pb = np.float32(pb + gf[plan[k]])
            acc, sb = acc + part, np.float32(sb + pb)
        d_ent[r], d_bias[r] = acc, sb
    return torch.from_numpy(d_ent), torch.from_numpy(d_bias)


# ---------------------------------------------------------------------------------------------------------------- slots
def piece_heads(rows, S):
    """[(entry i, is the run's first head, the run has several pieces)] for every piece head of the row sequence."""
    return [(i, i == s, L > S) for s, L, _ in plan_runs(rows) for i in range(s, s + L, S)]


def slot_of(i, first, S):
    """The workspace slot of head i of a run of several pieces."""
    return 2 * (i // S) + (1 if first else 0)


def window_first(rows, S):
    """{window w: the first entry of the run of several pieces that begins in [w S, (w + 1) S)}; raises if two begin in one."""
    out = {}
    for s, L, _ in plan_runs(rows):
        if L > S:
            assert s // S not in out
            out[s // S] = s
    return out


# ---------------------------------------------------------------------------------------------------------------- lists
IDS = {1: lambda S: 1, 2: lambda S: S, 5: lambda S: S - 1, 6: lambda S: S + 1, 8: lambda S: 2 * S, 9: lambda S: 2 * S + 1,
       10: lambda S: S + 1, 11: lambda S: 2 * S + 1}
N_SPLIT = 16                                           # the entity table of split_lists
SHARDS = ((0, 7), (7, 10), (10, 16))                   # a partition of it with a run of several pieces in every part


def run_lengths(S):
    """{id: how often split_lists(S) names it}: one row each of length 1, S - 1, S, S + 1, 2 S, 2 S + 1, and the neighbours 10,
    11 with S + 1 and 2 S + 1: two runs of several pieces back to back, so that one window holds a head of each."""
    return {o: f(S) for o, f in IDS.items()}


def split_lists(S, B=16, K=16):
    """cand [B, K] int64 naming the ids of run_lengths(S) exactly that often, ids 13 / 14 (another shard's under n_local <= 12)
    and -1 padding in the rest, the entries of every run spread over the queries (position p holds element 37 p mod B K)."""
    flat = [o for o, n in sorted(run_lengths(S).items()) for _ in range(n)]
    assert len(flat) <= B * K - 6 and math.gcd(37, B * K) == 1
    flat += [(-1, 13, 14)[t % 3] for t in range(B * K - len(flat))]
    return torch.tensor([flat[(37 * p) % (B * K)] for p in range(B * K)], dtype=torch.int64).reshape(B, K)


def one_id_lists(B, K, o):
    return torch.full((B, K), o, dtype=torch.int64)
