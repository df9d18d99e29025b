"""References for training on per-query candidate lists (include/mgcn_hip.h (14)). A plain module:
tests/test_cand_train_ref_host.py checks it against stock torch on the CPU, tests/test_gpu_cand_train.py holds the kernels
to it.

  * ref_list_bce        float64 loss and gradients of a list: the gathered logits fed to dense_ref.ref_bce;
  * emul_dx_f32         the chunked f32 sum of mgcn_cand_bce_bwd_x in numpy f32 (product and sum rounded separately);
  * emul_ent_f32        the plan-order f32 sums of mgcn_cand_bce_bwd_ent in numpy f32, following the plan it is given the way the
                        header says the kernel does (every entry re-checked, an unusable one skipped);
  * loop_plan, loop_labels   Python-loop builders of the plan and of the labels.
Liveness everywhere: 0 <= id - row0 < n_local on Python integers."""
import numpy as np
import torch

from . import dense_ref as R

CHUNK = 64


def live_rows(cand, row0, n_local):
    """(live [B, K] bool, row [B, K] int64 with 0 at dead positions) on the CPU, from Python integers."""
    c = cand.cpu()
    live = torch.zeros(c.shape, dtype=torch.bool)
    row = torch.zeros(c.shape, dtype=torch.int64)
    for b, ids in enumerate(c.tolist()):
        for j, v in enumerate(ids):
            if 0 <= v - row0 < n_local:
                live[b, j], row[b, j] = True, v - row0
    return live, row


def ref_list_bce(x, ent, bias, cand, label, hot, cold, inv_count, row0=0, saturate_f32=False):
    """Float64 reference of the candidate-list loss on CPU tensors: a dict with loss, g [B, K] (0 at dead positions), p, z, mag (the
    logit's sum of magnitudes), y, live, row and the three gradients dx [B, dim], d_ent [n, dim], d_bias [n] in float64."""
    x, ent, bias = x.cpu(), ent.cpu(), bias.cpu()
    n = ent.size(0)
    live, row = live_rows(cand, row0, n)
    rows = ent.double()[row]                                              # [B, K, dim]
    z = (rows * x.double()[:, None, :]).sum(2) + bias.double()[row]
    mag = (rows.abs() * x.double().abs()[:, None, :]).sum(2) + bias.double().abs()[row]
    y = torch.where(label.cpu().bool(), torch.tensor(float(hot), dtype=torch.float64), torch.tensor(float(cold), dtype=torch.float64))
    B, K = row.shape
    loss = 0.0
    g = torch.zeros((B, K), dtype=torch.float64)
    p = torch.zeros((B, K), dtype=torch.float64)
    if bool(live.any()):
        l, gl, pl = R.ref_bce(z[live], y[live], inv_count, saturate_f32=saturate_f32)
        loss, g[live], p[live] = float(l), gl, pl
    dx = (g[:, :, None] * rows).sum(1)
    d_ent = torch.zeros((n, ent.size(1)), dtype=torch.float64)
    d_bias = torch.zeros(n, dtype=torch.float64)
    flat_row, flat_g = row.reshape(-1), g.reshape(-1)
    d_ent.index_add_(0, flat_row, flat_g[:, None] * x.double().repeat_interleave(K, 0))
    d_bias.index_add_(0, flat_row, flat_g)
    return dict(loss=loss, g=g, p=p, z=z, mag=mag, y=y, live=live, row=row, dx=dx, d_ent=d_ent, d_bias=d_bias)


def emul_dx_f32(g, cand, ent, row0=0):
    """dx [B, dim] f32: per chunk of 64 list positions a sequential f32 sum from 0 over its live positions of the rounded product
    g[b, j] * ent[o_j, :], the chunk sums added to dx (from 0) in chunk order."""
    g, ent = g.cpu().numpy().astype(np.float32), ent.cpu().numpy().astype(np.float32)
    live, row = live_rows(cand, row0, ent.shape[0])
    live, row = live.numpy(), row.numpy()
    B, K = row.shape
    dx = np.zeros((B, ent.shape[1]), dtype=np.float32)
    for b in range(B):
        for c0 in range(0, K, CHUNK):
            s = np.zeros(ent.shape[1], dtype=np.float32)
            for j in range(c0, min(c0 + CHUNK, K)):
                if live[b, j]:
                    s = s + g[b, j] * ent[row[b, j]]
            dx[b] = dx[b] + s
    return torch.from_numpy(dx)


def emul_ent_f32(g, cand, x, perm, n_live, n_local, row0=0, d_ent=None, d_bias=None):
    """(d_ent, d_bias) f32 after mgcn_cand_bce_bwd_ent on the given plan: the row of every plan entry is recomputed from cand (-1 for
    an entry outside [0, B K) or a dead one), entry i owns a run iff its row is valid and differs from entry i - 1's, and walks
    it while the rows stay equal: sequential f32 sums from 0 in plan order. Rows no run names keep what d_ent / d_bias held."""
    g, x = g.cpu().numpy().astype(np.float32), x.cpu().numpy().astype(np.float32)
    live, row = live_rows(cand, row0, n_local)
    live, row = live.numpy().reshape(-1), row.numpy().reshape(-1)
    B, K = g.shape
    gf = g.reshape(-1)
    d_ent = np.zeros((n_local, x.shape[1]), dtype=np.float32) if d_ent is None else d_ent.cpu().numpy().copy()
    d_bias = np.zeros(n_local, dtype=np.float32) if d_bias is None else d_bias.cpu().numpy().copy()
    plan = perm.cpu().tolist()[:n_live]
    rows = [int(row[p]) if 0 <= p < B * K and live[p] else -1 for p in plan]
    i = 0
    while i < len(plan):
        r = rows[i]
        if r < 0 or (i > 0 and rows[i - 1] == r):
            i += 1
            continue
        acc, sb, k = np.zeros(x.shape[1], dtype=np.float32), np.float32(0.0), i
        while k < len(plan) and rows[k] == r:
            acc = acc + gf[plan[k]] * x[plan[k] // K]
            sb = np.float32(sb + gf[plan[k]])
            k += 1
        d_ent[r], d_bias[r] = acc, sb
        i = k
    return torch.from_numpy(d_ent), torch.from_numpy(d_bias)


def loop_plan(cand, n_local, row0=0):
    """(perm, n_live) by a Python loop: live flat positions sorted by (row, position), then the dead ones by position."""
    flat = cand.cpu().reshape(-1).tolist()
    live = sorted((v - row0, pos) for pos, v in enumerate(flat) if 0 <= v - row0 < n_local)
    dead = [pos for pos, v in enumerate(flat) if not 0 <= v - row0 < n_local]
    return torch.tensor([pos for _, pos in live] + dead, dtype=torch.int64), len(live)


def loop_labels(qkey, keys, ptr, tails, cand, row0, n_local):
    """label [B, K] uint8 by a Python loop over the index: 1 iff the id is a row of the shard and a known tail of the query."""
    keys_l, ptr_l, tails_l = keys.cpu().tolist(), ptr.cpu().tolist(), tails.cpu().tolist()
    at = {k: i for i, k in enumerate(keys_l)}
    out = torch.zeros(cand.shape, dtype=torch.uint8)
    for b, (k, ids) in enumerate(zip(qkey.cpu().tolist(), cand.cpu().tolist())):
        i = at.get(k)
        known = set(tails_l[ptr_l[i]:ptr_l[i + 1]]) if i is not None else set()
        for j, v in enumerate(ids):
            out[b, j] = int(0 <= v - row0 < n_local and v in known)
    return out


def gamma(n):
    """The standard bound of a sum of n rounded addends in f32, any order: |fl - exact| <= gamma_n sum |addends|,
    gamma_n = n u / (1 - n u): each addend meets one product rounding and at most n - 1 additions, (1 + u)^n - 1 <= gamma_n.
    This is the rigorous form of the first-order expression n 2^-24 sum |addends|; it is larger than that expression by the
    factor 1 / (1 - n u), at most 1.00014 for the n <= 2340 of these tests."""
    return n * R.U / (1.0 - n * R.U)


def lists(N, B, K, seed, dup=True):
    """Uniform ids in [0, N) with repeats inside a row (every row names its own first id again at its last position)."""
    cand = torch.randint(0, N, (B, K), generator=R.gen(seed))
    if dup and K > 1:
        cand[:, -1] = cand[:, 0]
    return cand
