"""References for the softmax cross-entropy over per-query candidate lists (include/mgcn_hip.h (16)). A plain module:
tests/test_cand_ce_ref_host.py checks it against stock torch on the CPU and measures the constant below,
tests/test_gpu_cand_ce.py holds the kernels to it.

  * ref_list_ce         float64 restatement of the header's loss section: logits, row statistics, targets, g, loss, gradients;
  * stats64, merge64    a part's statistic and the fold of statistics in float64 (the merge's algebra);
  * emul_lp_f32         numpy-f32 emulation of the unit-then-merge order: per chunk of 64 (m, s), the sequential merge, lp;
  * the bars            logit -> lp -> g -> loss, each derived from the one before; no constant is taken from a kernel.
Liveness everywhere: cand_train_ref.live_rows (0 <= id - row0 < n_local on Python integers)."""
import math

import numpy as np
import torch

from . import cand_train_ref as C
from . import dense_ref as R

CHUNK = C.CHUNK
NINF = float('-inf')

# The f32 exp / log / sum term of lp = (z - M) - log S, in units of u (1 + |lp|): the rounding of z - M and of the last
# subtraction are u |z - M| and u |lp|, the rounding of log S is u log S, and S itself (a sum of at most n positive rounded
# exponentials, rescaled once per chunk) is off by a few u RELATIVE, which log turns into a few u absolute: the 1. The numpy-f32
# emulation below (emul_lp_f32 on f32 logits against float64 on the same logits) reaches 2.40 of that unit on this module's grids
# (LSE_GRID: worst case K = 257 at logit scale 30; 2.37 at K = 64, scale 1); M + log S is held in the same unit, u (1 + log S),
# and counts in that figure. The constant is 4 x that;
# tests/test_cand_ce_ref_host.py recomputes the ratio and fails when the emulation comes within a factor 2 of the constant.
LSE_RATIO_MEASURED = 2.40
C_LSE = 4 * LSE_RATIO_MEASURED
# (K, logit scale): the list lengths of the device grid, logits of the size the structural grid has and of the range test
LSE_GRID = [(1, 1.0), (63, 1.0), (64, 1.0), (65, 1.0), (130, 1.0), (257, 1.0), (65, 30.0), (257, 30.0), (130, 100.0), (257, 100.0)]
F32_TINY = 2.0 ** -126      # below it an f32 result may be flushed to zero


def ref_list_ce(x, ent, bias, cand, label, eps, inv_batch, row0=0):
    """Float64 reference on CPU tensors: a dict with z, mag (the logit's sum of magnitudes), live, row, the row statistics M, S
    (float64 [B]; -inf / 0 without a live position), n_live, n_pos (int64 [B]), q, lp, p, g [B, K] (0 at dead positions and in rows
    without a positive), terms [B, K], loss (float) and the gradients dx [B, dim], d_ent [n, dim], d_bias [n]."""
    x, ent, bias = x.cpu(), ent.cpu(), bias.cpu()
    n = ent.size(0)
    live, row = C.live_rows(cand, row0, n)
    rows = ent.double()[row]                                              # [B, K, dim]
    z = (rows * x.double()[:, None, :]).sum(2) + bias.double()[row]
    mag = (rows.abs() * x.double().abs()[:, None, :]).sum(2) + bias.double().abs()[row]
    B, K = row.shape
    pos = label.cpu().bool() & live
    n_live, n_pos = live.sum(1), pos.sum(1)
    zl = torch.where(live, z, torch.full_like(z, NINF))
    M = zl.max(1).values if K else torch.full((B,), NINF, dtype=torch.float64)
    act = (n_pos > 0)[:, None] & live                                      # the positions that carry a term and a gradient
    safe_M = torch.where(torch.isfinite(M), M, torch.zeros_like(M))
    e = torch.where(live, torch.exp(z - safe_M[:, None]), torch.zeros_like(z))
    S = e.sum(1)
    lp = torch.where(act, (z - safe_M[:, None]) - torch.log(torch.where(S > 0, S, torch.ones_like(S)))[:, None], torch.zeros_like(z))
    p = torch.where(act, torch.exp(lp), torch.zeros_like(z))
    q = (1.0 - eps) * pos.double() / n_pos.clamp(min=1)[:, None].double() + eps / n_live.clamp(min=1)[:, None].double()
    q = torch.where(act, q, torch.zeros_like(q))
    g = (p - q) * inv_batch
    terms = -(q * lp) * inv_batch
    dx = (g[:, :, None] * rows).sum(1)
    d_ent = torch.zeros((n, ent.size(1)), dtype=torch.float64)
    d_bias = torch.zeros(n, dtype=torch.float64)
    flat_row, flat_g = row.reshape(-1), g.reshape(-1)
    d_ent.index_add_(0, flat_row, flat_g[:, None] * x.double().repeat_interleave(K, 0))
    d_bias.index_add_(0, flat_row, flat_g)
    return dict(z=z, mag=mag, live=live, row=row, M=M, S=S, n_live=n_live, n_pos=n_pos, q=q, lp=lp, p=p, g=g, terms=terms,
                loss=float(terms.sum()), act=act, dx=dx, d_ent=d_ent, d_bias=d_bias)


def stats64(z, live, pos):
    """(m, s, n_live, n_pos) of one part: float64 1-d z, bool live / pos. The empty statistic is (-inf, 0, 0, 0)."""
    if not bool(live.any()):
        return (NINF, 0.0, 0, 0)
    zl = z[live].double()
    m = float(zl.max())
    return (m, float(torch.exp(zl - m).sum()), int(live.sum()), int((pos & live).sum()))


def merge64(parts):
    """The fold of statistics in part order, in float64: M = max m_p, S = sum of s_p exp(m_p - M) over the parts with a live
    position, the counts add."""
    M = max([m for m, _, _, _ in parts] + [NINF])
    S = 0.0
    for m, s, _, _ in parts:
        if m != NINF:
            S = S + s * math.exp(m - M)
    return (M, S, sum(p[2] for p in parts), sum(p[3] for p in parts))


def emul_lp_f32(z32, live):
    """(M [B], S [B], lp [B, K]) in numpy f32 from f32 logits, in the kernels' unit-then-merge order: per chunk of 64 positions
    m = max and s = the sequential sum of exp(z - m) over its live positions; rows merged sequentially in chunk order, S from 0
    as S + s_p * exp(m_p - M) (chunks without a live position skipped); lp = (z - M) - log S. Every operation rounds to f32."""
    z32, live = np.asarray(z32, dtype=np.float32), np.asarray(live, dtype=bool)
    B, K = z32.shape
    Ms, Ss = np.full(B, -np.inf, dtype=np.float32), np.zeros(B, dtype=np.float32)
    lp = np.zeros((B, K), dtype=np.float32)
    for b in range(B):
        parts = []
        for c0 in range(0, K, CHUNK):
            idx = [j for j in range(c0, min(c0 + CHUNK, K)) if live[b, j]]
            if not idx:
                parts.append((np.float32(-np.inf), np.float32(0.0)))
                continue
            m = np.float32(max(z32[b, j] for j in idx))
            s = np.float32(0.0)
            for j in idx:
                s = np.float32(s + np.exp(np.float32(z32[b, j] - m)))
            parts.append((m, s))
        M = np.float32(max(m for m, _ in parts)) if parts else np.float32(-np.inf)
        S = np.float32(0.0)
        for m, s in parts:
            if m != -np.inf:
                S = np.float32(S + np.float32(s * np.exp(np.float32(m - M))))
        Ms[b], Ss[b] = M, S
        if S > 0:
            logS = np.float32(np.log(S))
            for j in range(K):
                if live[b, j]:
                    lp[b, j] = np.float32(np.float32(z32[b, j] - M) - logS)
    return Ms, Ss, lp


def lse_grid_logits(K, scale, seed):
    """(z32 [4, K] f32 tensor, live [4, K] bool) of the measured-ratio check: normal logits times `scale`, a tenth dead."""
    g = R.gen(seed)
    z = R.randn_scaled((4, K), g, scale)
    live = torch.rand((4, K), generator=g) >= 0.1
    live[:, 0] = True
    return z, live


def lse_ratio(z32, live):
    """max over live positions of |lp_f32 - lp_64| and over rows of |(M + log S)_f32 - (M + log S)_64|, in units of
    u (1 + |lp|) and u (1 + log S): both figures from the same f32 logits."""
    M32, S32, lp32 = emul_lp_f32(z32.numpy(), live.numpy())
    z = z32.double()
    zl = torch.where(live, z, torch.full_like(z, NINF))
    M = zl.max(1).values
    S = torch.where(live, torch.exp(z - M[:, None]), torch.zeros_like(z)).sum(1)
    lp = (z - M[:, None]) - torch.log(S)[:, None]
    r_lp = ((torch.from_numpy(lp32).double() - lp).abs() / (R.U * (1.0 + lp.abs())))[live].max()
    L32 = torch.from_numpy(M32).double() + torch.log(torch.from_numpy(S32).double())
    r_L = ((L32 - (M + torch.log(S))).abs() / (R.U * (1.0 + torch.log(S)))).max()
    return float(max(r_lp, r_L))


DEAD = (-1, None, 2 ** 62, -2 ** 62, 'N+5')            # None: N itself
EDGE_KINDS = ('no_positive', 'all_dead', 'all_live_positive', 'only_last_of_chunk', 'first_chunk_dead')


def plant(cand, label, b, kind, N):
    """Row b of (cand, label) turned into one of EDGE_KINDS (in place). Dead ids cycle through -1, N, +-2^62, N + 5."""
    K = cand.size(1)
    dead = torch.tensor([N if v is None else N + 5 if v == 'N+5' else v for v in DEAD], dtype=torch.int64)
    fill = dead[torch.arange(K) % len(dead)]
    if kind == 'no_positive':                       # live and dead positions, no label set
        label[b] = False
        cand[b, K // 2] = -1
    elif kind == 'all_dead':                        # labels set on dead positions must not count
        cand[b] = fill
        label[b] = True
    elif kind == 'all_live_positive':               # every live position is a positive; the dead ones carry a label too
        cand[b, 1::3] = fill[1::3]
        label[b] = True
    elif kind == 'only_last_of_chunk':              # the one live position is the last of the first chunk (or of a shorter list)
        keep = int(cand[b, 0]) % N
        cand[b] = fill
        cand[b, min(CHUNK, K) - 1] = keep
        label[b] = True
    elif kind == 'first_chunk_dead':                # nothing live in positions 0..63 (a list of one chunk: nothing live at all)
        cand[b, :CHUNK] = fill[:CHUNK]
        label[b, min(CHUNK, K - 1):] = True
    else:
        raise ValueError(kind)


def problem(B, K, N, dim, seed, scale=None, edges=True):
    """(x, ent, bias, cand, label) on the CPU: +-U[0.25, 1] operands (with `scale`: scaled so that the largest |logit| is `scale`),
    cand_train_ref.lists (duplicates inside a row) with a few dead ids, labels at 30 % and at column 0, and, with `edges`, the
    EDGE_KINDS planted in the LAST min(B - 1, 5) rows, rotated by the seed (B >= 6 has all five; row 0 is always a plain row)."""
    g = R.gen(seed)
    x, ent, bias = R.pm_uniform((B, dim), g), R.pm_uniform((N, dim), g), R.pm_uniform((N,), g)
    if scale is not None:
        s = (scale / float(R.ref_logits(x, ent, bias)[0].abs().max())) ** 0.5
        x, ent, bias = x * s, ent * s, bias * (s * s)
    cand = C.lists(N, B, K, seed + 1)
    label = torch.rand((B, K), generator=g) < 0.3
    label[:, 0] = True
    if B * K > 5:
        for i in range(len(DEAD)):
            v = DEAD[i]
            cand[i % B, (3 * i + 1) % K] = N if v is None else N + 5 if v == 'N+5' else v
    kinds = []
    if edges:
        for i in range(min(B - 1, len(EDGE_KINDS))):
            kind = EDGE_KINDS[(seed + i) % len(EDGE_KINDS)]
            plant(cand, label, B - 1 - i, kind, N)
            kinds.append(kind)
    return x, ent, bias, cand, label


def lse_worst():
    """(worst ratio, its (K, scale)) over LSE_GRID: the figure LSE_RATIO_MEASURED records."""
    worst, where = 0.0, None
    for K, scale in LSE_GRID:
        r = lse_ratio(*lse_grid_logits(K, scale, R.seed_of(61, K, int(scale))))
        if r > worst:
            worst, where = r, (K, scale)
    return worst, where


# ----------------------------------------------------------------------------------------------------------------
# The bars, each from the one before
def logit_bars(ref, dim):
    """(zbar [B, K], rowbar [B]): dense_ref.dot_bar of every logit, and the largest one among a row's live positions."""
    zbar = R.dot_bar(ref['mag'], dim)
    rowbar = torch.where(ref['live'], zbar, torch.zeros_like(zbar)).max(1).values if zbar.size(1) else torch.zeros(zbar.size(0), dtype=torch.float64)
    return zbar, rowbar


def lse_bar(ref, rowbar):
    """M + log S per row: log-sum-exp moves by at most the largest move of a logit, plus the f32 term."""
    logS = torch.log(torch.where(ref['S'] > 0, ref['S'], torch.ones_like(ref['S'])))
    return rowbar + C_LSE * R.U * (1.0 + logS)


def lp_bar(ref, rowbar):
    """lp = z - (M + log S): the row's largest logit bar twice over (own logit; M + log S), plus the f32 exp / log / sum term."""
    return 2.0 * rowbar[:, None] + C_LSE * R.U * (1.0 + ref['lp'].abs())


def g_bar(ref, rowbar, inv_batch):
    """g = (p - q) inv_batch: lp off by lp_bar seen through exp (p (e^bar - 1), rigorous for either sign), then the f32 exp (in
    C_LSE's term already), the three operations of q, the subtraction and the product: 4 u (p + q); a p below the normal range
    may be flushed."""
    return inv_batch * (ref['p'] * torch.expm1(lp_bar(ref, rowbar)) + 4.0 * R.U * (ref['p'] + ref['q']) + F32_TINY)


def loss_bar(ref, rowbar, inv_batch, n_partials):
    """The sum of the term bars (-(q lp): q's three roundings and the product, 4 u q |lp|; lp's own bar times q) plus the sums:
    a unit's 64 terms meet at most 8 additions, the partials one torch sum: gamma(8 + n_partials + 1) of the terms' magnitudes."""
    tb = ref['q'] * lp_bar(ref, rowbar) + 4.0 * R.U * ref['q'] * ref['lp'].abs()
    mags = (ref['q'] * ref['lp']).abs().sum()
    return inv_batch * float(tb.sum() + C.gamma(8 + n_partials + 1) * mags)


def grad_bars(ref, x, ent, rowbar, inv_batch, row0=0):
    """(dx, d_ent, d_bias) bars: g's bar carried through the sums' magnitudes, plus the f32 sums themselves (cand_train_ref.gamma
    of the number of addends: K for dx, the longest run for a row of d_ent / d_bias)."""
    x, ent = x.cpu().double(), ent.cpu().double()
    gb = torch.where(ref['live'], g_bar(ref, rowbar, inv_batch), torch.zeros_like(ref['g']))
    rows = ent[ref['row']].abs()                                        # [B, K, dim]
    B, K = ref['g'].shape
    dx = (gb[:, :, None] * rows).sum(1) + C.gamma(K + 2) * (ref['g'].abs()[:, :, None] * rows).sum(1)
    n = ent.size(0)
    flat_row = ref['row'].reshape(-1)
    runs = int(torch.bincount(flat_row[ref['live'].reshape(-1)], minlength=1).max()) if bool(ref['live'].any()) else 1
    xa = x.abs().repeat_interleave(K, 0)
    de = torch.zeros((n, ent.size(1)), dtype=torch.float64).index_add_(
        0, flat_row, (gb.reshape(-1) + C.gamma(runs + 2) * ref['g'].abs().reshape(-1))[:, None] * xa)
    db = torch.zeros(n, dtype=torch.float64).index_add_(0, flat_row, gb.reshape(-1) + C.gamma(runs + 2) * ref['g'].abs().reshape(-1))
    return dx, de, db
