"""References for the softmax cross-entropy over the full entity table (include/mgcn_hip.h (20)). A plain module:
tests/test_table_ce_ref_host.py checks it against stock torch on the CPU and measures the constant below,
tests/test_gpu_table_ce.py holds the kernels to it.

  * ref_table_ce        float64 restatement of the header's loss section on the WHOLE table, returned for the shard
                        [row0, row0 + n_local): logits, GLOBAL row statistics, targets, g, loss, gradients; `convention` swaps in
                        one of the WRONG conventions the host test shows to leave the bars;
  * shard_stats64       the shards' statistics (cand_ce_ref.stats64), to be folded by cand_ce_ref.merge64;
  * emul_lp_f32         numpy-f32 emulation of the kernels' order: per tile of 32 entities m = max, s = the sequential sum of
                        exp(z - m) in row order; the tiles merged sequentially (two levels beyond 64 tiles); lp = (z - M) - log S;
  * the bars            logit -> lp -> g -> loss -> gradients, each derived from the one before. The logit bar is dense_ref's for
                        the exact-f32 family; no constant is taken from a kernel."""
import math

import numpy as np
import torch

from . import cand_ce_ref as L
from . import cand_train_ref as C
from . import dense_ref as R

TILE = 32
F32_TINY = L.F32_TINY

# The f32 exp / log / sum term of lp = (z - M) - log S in units of u (1 + |lp|), and of M + log S in units of u (1 + log S), as
# cand_ce_ref.C_LSE, for parts of 32 rows folded sequentially (in two levels beyond 64 tiles): the numpy-f32 emulation below on f32
# logits against float64 on the same logits reaches 3.06 of that unit on LSE_GRID (worst case n = 31 at logit scale 30, one part;
# 2.50 at n = 2100, scale 100, the two-level fold of 66 tiles; 1.68 at n = 2100, scale 1). The constant is 4 x that;
# tests/test_table_ce_ref_host.py recomputes the ratio and fails when the emulation comes within a factor 2 of the constant.
LSE_RATIO_MEASURED = 3.06
C_LSE = 4 * LSE_RATIO_MEASURED
# (n, logit scale): the table sizes of the device grid at the three logit scales of the list grid
LSE_GRID = [(n, s) for n in (1, 31, 32, 33, 64, 95, 257, 2100) for s in (1.0, 30.0, 100.0)]

CONVENTIONS = ('right', 'eps_over_n_pos', 'bce_smoothing', 'mass_not_shared', 'mean_over_BN', 'local_N', 'local_stats')


def ref_table_ce(x, ent, bias, y, eps, inv_batch, row0=0, n_local=None, convention='right'):
    """Float64 reference on CPU tensors. `ent` [N, dim] / `bias` [N] are the WHOLE table, y [B, N] bool the known tails; the
    result is the shard's: z, mag (the logit's sum of magnitudes), q, lp, p, g, terms [B, n_local], the GLOBAL row statistics M, S
    (float64 [B]), n_pos (int64 [B]), rowmag_max (the largest mag of a row over the whole table), loss (the shard's terms, float),
    dx [B, dim] (the shard's partial sum), d_ent [n_local, dim], d_bias [n_local]. A row without a positive has g = 0 and no term."""
    assert convention in CONVENTIONS
    x, ent, bias, y = x.cpu().double(), ent.cpu().double(), bias.cpu().double(), y.cpu().bool()
    N = ent.size(0)
    n_local = N - row0 if n_local is None else n_local
    sl = slice(row0, row0 + n_local)
    z_all = x @ ent.t() + bias
    mag_all = x.abs() @ ent.abs().t() + bias.abs()
    stat_src = z_all[:, sl] if convention == 'local_stats' else z_all
    B = x.size(0)
    if stat_src.size(1):
        M = stat_src.max(1).values
        S = torch.exp(stat_src - M[:, None]).sum(1)
    else:
        M, S = torch.full((B,), L.NINF, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    n_pos = y.sum(1)
    act = (n_pos > 0)[:, None].expand(B, n_local)
    z, yl = z_all[:, sl], y[:, sl].double()
    safe_M = torch.where(torch.isfinite(M), M, torch.zeros_like(M))
    lp = (z - safe_M[:, None]) - torch.log(torch.where(S > 0, S, torch.ones_like(S)))[:, None]
    share = n_pos.clamp(min=1)[:, None].double()
    count = float(n_local if convention == 'local_N' else N)
    if convention == 'eps_over_n_pos':
        q = (1.0 - eps) * yl / share + eps / share
    elif convention == 'bce_smoothing':
        q = (1.0 - eps) * yl + 1.0 / count
    elif convention == 'mass_not_shared':
        q = (1.0 - eps) * yl + eps / count
    else:
        q = (1.0 - eps) * yl / share + eps / count
    w = inv_batch / N if convention == 'mean_over_BN' else inv_batch
    lp, q = torch.where(act, lp, torch.zeros_like(lp)), torch.where(act, q, torch.zeros_like(q))
    p = torch.where(act, torch.exp(lp), torch.zeros_like(lp))
    g = (p - q) * w
    terms = -(q * lp) * w
    return dict(z=z, mag=mag_all[:, sl], rowmag_max=mag_all.max(1).values, M=M, S=S, n_pos=n_pos, act=act, q=q, lp=lp, p=p, g=g,
                terms=terms, loss=float(terms.sum()), dx=g @ ent[sl], d_ent=g.t() @ x, d_bias=g.sum(0))


def shard_stats64(x, ent, bias, y, bounds):
    """[[(m, s, n_live, n_pos) per shard] per row] for the shards [bounds[i], bounds[i + 1]) of the whole table, in float64."""
    z = x.cpu().double() @ ent.cpu().double().t() + bias.cpu().double()
    y = y.cpu().bool()
    live = torch.ones(z.size(1), dtype=torch.bool)
    return [[L.stats64(z[b, a:e], live[a:e], y[b, a:e]) for a, e in zip(bounds[:-1], bounds[1:])] for b in range(z.size(0))]


def fold_shape(n):
    """(tiles, G, P): _native.score_ce_fold_shape restated: one sequential fold up to 64 tiles, beyond G = ceil(sqrt(tiles))
    groups (group g: the tiles g, g + G, ...), folded first, then the groups in order."""
    tiles = (n + 31) // 32
    G = 1 if tiles <= 64 else math.isqrt(tiles - 1) + 1
    return tiles, G, (tiles + G - 1) // G


def _fold_f32(parts):
    """The sequential merge of (m, s) parts in numpy f32: one part is copied."""
    if len(parts) == 1:
        return parts[0]
    M = np.max(np.stack([m for m, _ in parts]), axis=0)
    S = np.zeros(M.shape, dtype=np.float32)
    for m, s in parts:
        f = np.where(m == M, np.float32(1.0), np.exp((m - M).astype(np.float32)).astype(np.float32)).astype(np.float32)
        S = (S + (s * f).astype(np.float32)).astype(np.float32)
    return M, S


def emul_lp_f32(z32):
    """(M [B], S [B], lp [B, n]) in numpy f32 from f32 logits z32 [B, n] (n >= 1), in the kernels' order: per tile of 32 entities
    m = max and s = the sequential sum from 0 of exp(z - m) in row order; the tiles merged sequentially, S from 0 as
    S + s_t * (1 if m_t == M else exp(m_t - M)), in tile order up to 64 tiles and in the two levels of fold_shape beyond;
    lp = (z - M) - log S. Every operation rounds to f32."""
    z32 = np.asarray(z32, dtype=np.float32)
    B, n = z32.shape
    parts = []
    for t0 in range(0, n, TILE):
        zt = z32[:, t0:t0 + TILE]
        m = zt.max(1)
        s = np.zeros(B, dtype=np.float32)
        for r in range(zt.shape[1]):
            s = (s + np.exp((zt[:, r] - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
        parts.append((m, s))
    _, G, _ = fold_shape(n)
    M, S = _fold_f32(parts) if G == 1 else _fold_f32([_fold_f32(parts[g::G]) for g in range(G)])
    lp = ((z32 - M[:, None]).astype(np.float32) - np.log(S).astype(np.float32)[:, None]).astype(np.float32)
    return M, S, lp


def lse_ratio(z32):
    """max over elements of |lp_f32 - lp_64| and over rows of |(M + log S)_f32 - (M + log S)_64|, in units of u (1 + |lp|) and
    u (1 + log S): both figures from the same f32 logits (a tensor [B, n])."""
    M32, S32, lp32 = emul_lp_f32(z32.numpy())
    z = z32.double()
    M = z.max(1).values
    S = torch.exp(z - M[:, None]).sum(1)
    lp = (z - M[:, None]) - torch.log(S)[:, None]
    r_lp = ((torch.from_numpy(lp32).double() - lp).abs() / (R.U * (1.0 + lp.abs()))).max()
    L32 = torch.from_numpy(M32).double() + torch.log(torch.from_numpy(S32).double())
    r_L = ((L32 - (M + torch.log(S))).abs() / (R.U * (1.0 + torch.log(S)))).max()
    return float(max(r_lp, r_L))


def lse_worst():
    """(worst ratio, its (n, scale)) over LSE_GRID, eight rows of normal logits times `scale` each: the figure
    LSE_RATIO_MEASURED records."""
    worst, where = 0.0, None
    for n, scale in LSE_GRID:
        r = lse_ratio(R.randn_scaled((8, n), R.gen(R.seed_of(67, n, int(scale))), scale))
        if r > worst:
            worst, where = r, (n, scale)
    return worst, where


def problem(B, N, dim, seed, scale=None):
    """(x, ent, bias, y) on the CPU: +-U[0.25, 1] operands (with `scale`: scaled so that the largest |logit| is `scale`) and known
    tails y [B, N] bool cycling through the row kinds: one positive, several (about 30 %), all N, none (row 3 of every four)."""
    g = R.gen(seed)
    x, ent, bias = R.pm_uniform((B, dim), g), R.pm_uniform((N, dim), g), R.pm_uniform((N,), g)
    if scale is not None:
        s = (scale / float(R.ref_logits(x, ent, bias)[0].abs().max())) ** 0.5
        x, ent, bias = x * s, ent * s, bias * (s * s)
    y = torch.zeros((B, N), dtype=torch.bool)
    several = torch.rand((B, N), generator=g) < 0.3
    one = torch.randint(0, N, (B,), generator=g)
    for b in range(B):
        kind = b % 4
        if kind == 0:
            y[b, one[b]] = True
        elif kind == 1:
            y[b] = several[b]
            y[b, one[b]] = True
        elif kind == 2:
            y[b] = True
    return x, ent, bias, y


def index_of(y):
    """(keys, ptr, tails) int64 / int64 / int32 CPU tensors of a filter index in which query b has the key b and the tails y[b]
    (rows without a tail have no key), for mgcn_filter_mask."""
    keys, ptr, tails = [], [0], []
    for b in range(y.size(0)):
        t = torch.nonzero(y[b]).reshape(-1).tolist()
        if t:
            keys.append(b)
            tails += t
            ptr.append(len(tails))
    return (torch.tensor(keys, dtype=torch.int64), torch.tensor(ptr, dtype=torch.int64), torch.tensor(tails, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------------
# The bars, each from the one before
def logit_bars(ref, dim):
    """(zbar [B, n_local], rowbar [B]): dense_ref.dot_bar of every logit of the shard, and of the row's largest magnitude over
    the WHOLE table (M and S are global: they move with any entity's logit)."""
    return R.dot_bar(ref['mag'], dim), R.dot_bar(ref['rowmag_max'], dim)


def lse_bar(ref, rowbar):
    """M + log S per row: log-sum-exp moves by at most the largest move of a logit, plus the f32 term."""
    return rowbar + C_LSE * R.U * (1.0 + torch.log(ref['S']))


def lp_bar(ref, rowbar):
    """lp = z - (M + log S): the row's largest logit bar twice over (own logit; M + log S), plus the f32 exp / log / sum term."""
    return 2.0 * rowbar[:, None] + C_LSE * R.U * (1.0 + ref['lp'].abs())


def g_bar(ref, rowbar, inv_batch):
    """cand_ce_ref.g_bar with this module's lp bar: p (e^bar - 1), the operations of q, the subtraction and the product
    (4 u (p + q)), a p below the normal range may be flushed."""
    return inv_batch * (ref['p'] * torch.expm1(lp_bar(ref, rowbar)) + 4.0 * R.U * (ref['p'] + ref['q']) + F32_TINY)


def loss_bar(ref, rowbar, inv_batch, n_partials):
    """The sum of the term bars (q's roundings and the product, 4 u q |lp|; lp's own bar times q) plus the sums: a term meets 8
    additions in its lane, 6 in the xor tree and 3 over the waves, the partials one torch sum: gamma(17 + n_partials + 1)."""
    tb = ref['q'] * lp_bar(ref, rowbar) + 4.0 * R.U * ref['q'] * ref['lp'].abs()
    mags = (ref['q'] * ref['lp']).abs().sum()
    return inv_batch * float(tb.sum() + C.gamma(17 + n_partials + 1) * mags)


def grad_bars(ref, x, ent_shard, rowbar, inv_batch):
    """(dx, d_ent, d_bias) bars: g's bar carried through the sums' magnitudes, plus the f32 sums themselves in any order
    (cand_train_ref.gamma of the number of addends: n_local for dx, B for a row of d_ent / d_bias)."""
    x, e = x.cpu().double().abs(), ent_shard.cpu().double().abs()
    gb, ga = g_bar(ref, rowbar, inv_batch), ref['g'].abs()
    B, n = ga.shape
    return ((gb + C.gamma(n + 2) * ga) @ e, (gb + C.gamma(B + 2) * ga).t() @ x, (gb + C.gamma(B + 2) * ga).sum(0))
