"""Float64 references, operand builders, shape grids and error bars for the dense / scoring / training kernels
(csrc/dense.hip, csrc/train_layer.hip). A plain module: tests/test_dense_ref_host.py checks the references against stock
torch and measures the constants below on the CPU; tests/test_gpu_dense_edges.py and tests/test_gpu_train_edges.py hold
the kernels to them.

Everything is torch and device-agnostic: the same function gives the float64 reference on the CPU (host test) and on
the GPU in double precision (device tests). Paragraph numbers (4), (4t), (5) ... are those of include/mgcn_hip.h.

The grids are built from the kernels' own tiling constants (k-blocks of 32 / slabs of 16, strips of 64 queries, row
tiles of 16 / 32, pick_nt's switches at 32 / 64 / 128 / 208 columns, 128-row statistic blocks, 256-column trips). Each
case carries a LABEL naming the path it is meant to take. The labels are test data written by hand from pick_nt,
split_scoring, launch and mgcn_matmul_f32 in csrc/dense.hip, not a second dispatcher; the host test only checks that no
label of its list has dropped out of the grids.

The training epilogue's bars (train_bars) serve both its unsplit form (4t) and its split stages (4s) at the ragged rank
boundaries of TRAIN_RAGGED_CASES: emul_train_split_f32 restates the stages' association in f32 and the host test shows that
it stays inside those bars, and that per-rank statistics do not."""
import functools
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24                      # unit roundoff of f32

# ----------------------------------------------------------------------------------------------------------------
# The bars. None of these constants is taken from a kernel: each is 4 x what a float32 emulation on the CPU shows
# against float64 on the grids' own inputs; tests/test_dense_ref_host.py recomputes every ratio and fails when the
# emulation comes within a factor 2 of its constant (i.e. when the measured figure written here went stale).
#
# Dot products on the exact-f32 MFMA (tile_kernel, small_matmul_kernel, matmul_tn): |got - ref64| <= c u mag with
# mag = sum_k |a_k||b_k| (+ |bias|). c = K + 2 holds rigorously for ANY summation order; a sequential f32 chain (product
# and sum rounded separately: pessimistic against an fma) on the grids' inputs reaches 2.50 (worst case of the
# grids: bn_tanh 97-100-18, K = 300), so c = min(K + 2, 10.0). The margin is for another association (four partial chains per k-block,
# split-K blocks), which can only shorten the chains.
DOT_RATIO_MEASURED = 2.50
C_DOT = 4 * DOT_RATIO_MEASURED
# f32 sigmoid (exp + division) of an f32 logit: torch-CPU f32 is 1.50 u off float64 on the grids' logits.
SIG_RATIO_MEASURED = 1.50
C_SIG = 4 * SIG_RATIO_MEASURED
# f32 tanh of an f32 argument: torch-CPU f32 is 0.534 u off on the grids' BN arguments.
TANH_RATIO_MEASURED = 0.534
C_TANH = 4 * TANH_RATIO_MEASURED
# The affine BN step t = (pre - mean) / sqrt(var + eps) * gamma + beta evaluated in f32 from the f32-rounded `pre`:
# error in units of u (S (|pre| + |mean|) + |t| + |beta|), S = |gamma| / sqrt(var + eps); torch-CPU f32 reaches 2.25.
EPI_RATIO_MEASURED = 2.25
C_EPI = 4 * EPI_RATIO_MEASURED
# Ill-conditioned training columns (mean 100, spread 1e-2): the bar on rstd is 4 x the relative error of a two-pass f32
# variance after a sequential f32 mean (emul_two_pass_rstd_f32) ON THE SAME z, computed per case by the test that uses it
# (ill_rstd_bar): 1.78e-5 at N = 129, 3.05e-4 at N = 5003 on the z of ill_conditioned_z().
# Column means of such a z: a dot product with ones, K = N, but of SAME-SIGN terms -- the roundings of a growing partial sum
# drift instead of cancelling, so the sequential f32 chain is measured on its own: 43.7 u mag at N = 5003 (the
# rigorous (N + 2) u mag caps it, and is the bar at N = 129).
COLSUM_RATIO_MEASURED = 43.7
C_COLSUM = 4 * COLSUM_RATIO_MEASURED


def colsum_bar(mag, n):
    """Column sums / means of n same-sign terms (mag = sum |z| / n for a mean)."""
    return min(n + 2.0, C_COLSUM) * U * mag


def ill_rstd_bar(z, eps):
    """Relative bar on rstd for the columns of the f32 tensor `z`: 4 x the worst relative error of the two-pass f32 CPU
    emulation on this very z against float64 statistics of it."""
    z = z.detach().cpu()
    rstd64 = 1.0 / torch.sqrt(z.double().var(0, unbiased=False) + eps)
    _, rstd32 = emul_two_pass_rstd_f32(z, eps)
    return 4.0 * float(((rstd32.double() - rstd64).abs() / rstd64).max())


def dot_bar(mag, k):
    """Exact-f32 dot products of length k."""
    return min(k + 2.0, C_DOT) * U * mag


def split_logit_bar(mag):
    """score_split_kernel, the header's contract (5) / (2)+(4): six bf16 products of exactly split operands."""
    return 4.0 * U * mag + 2e-7


def sigmoid_bar(p64, logit_bar):
    """A logit off by `logit_bar` seen through the sigmoid: slope p (1 - p), plus the f32 exp and division."""
    return p64 * (1.0 - p64) * logit_bar + C_SIG * U


def tanh_bar(y64, arg_bar):
    """An argument off by `arg_bar` seen through tanh: slope 1 - y^2, the second-order term (|tanh''| < 0.77), plus
    the f32 tanh itself."""
    return (1.0 - y64 * y64) * arg_bar + arg_bar * arg_bar + C_TANH * U


def derived_bar(cpu_err, floor, today=None):
    """Bars of the training epilogue: 4 x the error torch-CPU f32 shows against float64 on the same inputs, but not below
    `floor` (a few u of the result and of the terms of its last additions: with a handful of elements the CPU's own error
    can be zero by luck, and no f32 evaluation in another order is bound by that). Wherever torch-CPU f32 itself sits
    inside a quarter of the bar of test_training_layer_kernels_vs_torch_autograd (`today`) -- as it does at that test's
    shape -- the result is not looser than that bar; where f32 cannot meet it (two-row batches whose rows nearly
    coincide: z - mean cancels, torch-CPU f32 is 5.7e-6 off on y at N = 2, O = 300) it does not apply."""
    bar = max(4.0 * cpu_err, floor)
    if today is not None and 4.0 * cpu_err <= today:
        bar = min(bar, today)
    return bar


def bce_grad_bar(g64, p64, y, logit_bar, inv_count):
    """d loss / d logit: 4 u |G| for its own products, plus a logit off by `logit_bar` and an f32 sigmoid (C_SIG u) seen
    through G's slope. G = (p - y) pq / max(pq, 1e-12) * inv_count with pq = p (1 - p): where pq >= 1e-12 this is
    (p - y) inv_count and the slope is pq, the sigmoid's. Under the floor G = 1e12 (p - y) pq inv_count and
    |dG / dz| = 1e12 pq |(p - y)(1 - 2p) + pq| inv_count, up to |p - y| inv_count at pq = 1e-12 -- twelve orders above pq.
    (The plain p (1 - p) slope is wrong there: torch-CPU f32 itself breaks it at logits of -30, test_dense_ref_host.py.)"""
    y = y.double()
    pq = p64 * (1.0 - p64)
    slope = torch.where(pq >= 1e-12, pq, 1e12 * pq * (((p64 - y) * (1.0 - 2.0 * p64)).abs() + pq))
    return 4.0 * U * g64.abs() + inv_count * (slope * logit_bar + C_SIG * U)


# ----------------------------------------------------------------------------------------------------------------
# Inputs
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def pm_uniform(shape, g):
    """+-U[0.25, 1]: no element is ignorable. One dropped, duplicated or misplaced k moves a dot product by at least
    1/16, i.e. mag / (16 K) -- three orders above c u mag for every K of the grids."""
    mag = torch.rand(shape, generator=g, dtype=torch.float32) * 0.75 + 0.25
    sign = (torch.rand(shape, generator=g) < 0.5).float() * 2.0 - 1.0
    return mag * sign


def randn_scaled(shape, g, scale):
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


LAYOUTS = ('contiguous', 'window', 'offset1', 'oddstride')


def layout(t, kind):
    """The values of the 2-d f32 tensor `t` laid out as
    contiguous  a tensor of its own;
    window      columns [4, 4 + c) of a wider tensor whose row stride is a multiple of 4: aligned base, aligned rows --
                stays on the aligned path;
    offset1     columns [1, 1 + c) of such a tensor: the base is one float off 16 bytes;
    oddstride   columns [0, c) of a tensor whose row stride is not a multiple of 4
    (the last two must take the guarded path and give the same values)."""
    r, c = t.shape
    if kind == 'contiguous':
        return t.contiguous()
    if kind == 'window':
        wide = torch.full((r, (c + 3) // 4 * 4 + 8), float('nan'), dtype=t.dtype, device=t.device)
        v = wide[:, 4:4 + c]
    elif kind == 'offset1':
        wide = torch.full((r, (c + 3) // 4 * 4 + 8), float('nan'), dtype=t.dtype, device=t.device)
        v = wide[:, 1:1 + c]
    elif kind == 'oddstride':
        w = c + 5
        w += (w % 4 == 0)
        wide = torch.full((r, w), float('nan'), dtype=t.dtype, device=t.device)
        v = wide[:, :c]
    else:
        raise ValueError(kind)
    v.copy_(t)
    return v


GUARD_F32 = 0x7FC0DEAD              # a quiet NaN with a recognisable payload
GUARD_I32 = 0x5AFEC0DE
GUARD_I64 = 0x5AFEC0DE5AFEC0DE


class Guarded(object):
    """An output buffer [rows + 2, ld] (a vector of n: rows = 1, cols = n) filled with a guard pattern; `view` is the [rows, cols]
    part the kernel may write. check() asserts bit for bit that everything else still holds the pattern."""

    def __init__(self, rows, cols, ld, device, dtype=torch.float32, pattern=None):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.idtype = torch.int64 if dtype == torch.int64 else torch.int32
        self.pattern = pattern if pattern is not None else (GUARD_I64 if dtype == torch.int64 else
                                                            GUARD_F32 if dtype == torch.float32 else GUARD_I32)
        self.raw = torch.full((rows + 2, ld), self.pattern, dtype=self.idtype, device=device)
        self.buf = self.raw.view(dtype)
        self.view = self.buf[:rows, :cols]

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what=''):
        probe = self.raw.clone()
        probe[:self.rows, :self.cols] = self.pattern
        assert bool((probe == self.pattern).all()), '%s: wrote outside its [%d, %d] block (ld %d)' % (what, self.rows, self.cols, self.ld)

    def untouched(self):
        return bool((self.raw == self.pattern).all())


# ----------------------------------------------------------------------------------------------------------------
# References (float64)
def ref_logits(x, ent, bias):
    """(5): z[b, n] = x[b, :] . ent[n, :] + bias[n]; mag = sum_k |x||ent| + |bias|."""
    x, ent, bias = x.double(), ent.double(), bias.double()
    return x @ ent.t() + bias, x.abs() @ ent.abs().t() + bias.abs()


def ref_scores(x, ent, bias):
    z, mag = ref_logits(x, ent, bias)
    return torch.sigmoid(z), z, mag


def ref_matmul(a, b):
    """C = A B; mag = |A||B|."""
    a, b = a.double(), b.double()
    return a @ b, a.abs() @ b.abs()


def ref_matmul_tn(a, b):
    """C = A^T B for A [K, M], B [K, N]."""
    a, b = a.double(), b.double()
    return a.t() @ b, a.abs().t() @ b.abs()


def ref_dense_bn_tanh(a, w, bias, mean, var, gamma, beta, eps):
    """(4): tanh(BN_eval(A W / 3 + bias)). Returns (y, bar): the bar is the dot-product bar on A W carried through the
    affine step and the tanh (tanh_bar), plus the f32 evaluation of the affine step itself (C_EPI)."""
    k = a.shape[1]
    a, w = a.double(), w.double()
    mean, var, gamma, beta = mean.double(), var.double(), gamma.double(), beta.double()
    b = bias.double() if bias is not None else torch.zeros_like(mean)
    pre = (a @ w) / 3.0 + b
    mag = (a.abs() @ w.abs()) / 3.0 + b.abs()
    s = gamma.abs() / torch.sqrt(var + eps)
    t = (pre - mean) / torch.sqrt(var + eps) * gamma + beta
    y = torch.tanh(t)
    arg_bar = s * dot_bar(mag, k) + C_EPI * U * (s * (pre.abs() + mean.abs()) + t.abs() + beta.abs())
    return y, tanh_bar(y, arg_bar)


def ref_train_epilogue(u_in, u_out, u_loop, bias, gamma, beta, running_mean, running_var, momentum, eps, gy, dtype=torch.float64):
    """(4t) forward and backward through autograd of F.batch_norm(training=True) + tanh, in `dtype` (float64: the
    reference; float32 on the CPU: the emulation the bars are derived from). Returns a dict."""
    cv = lambda t: None if t is None else t.detach().to(dtype).clone()
    z = (cv(u_in) + cv(u_out) + cv(u_loop)) / 3.0
    if bias is not None:
        z = z + cv(bias)
    z = z.detach().requires_grad_(True)
    g, b = cv(gamma).requires_grad_(True), cv(beta).requires_grad_(True)
    rm, rv = cv(running_mean), cv(running_var)
    y = torch.tanh(F.batch_norm(z, rm, rv, g, b, True, momentum, eps))
    y.backward(cv(gy))
    zz = z.detach()
    mean = zz.mean(0)
    rstd = 1.0 / torch.sqrt(zz.var(0, unbiased=False) + eps)
    return dict(z=zz, y=y.detach(), mean=mean, rstd=rstd, rm=rm, rv=rv, gz=z.grad, gu=z.grad / 3.0, ggamma=g.grad, gbeta=b.grad)


def ref_bce(z64, y, inv_count, saturate_f32=False):
    """Mean BCE of sigmoid(z) against targets y, and d loss / d z, with torch's clamps (log at -100, the 1e-12 floor of
    BCELoss's backward) evaluated in float64 on the float64 logits: header paragraph of mgcn_score_bce_fwd.
    saturate_f32: where torch-CPU f32 sigmoid of the logit rounded to f32 is exactly 0 or 1, p takes that value (the
    behaviour the header promises there: torch's formulas are discontinuous at saturation -- a loss term jumps to 100 and
    the gradient to 0 -- so float64's unsaturated p is no reference for an f32 kernel on those entries)."""
    p = torch.sigmoid(z64)
    if saturate_f32:
        p32 = torch.sigmoid(z64.float().cpu()).to(z64.device)
        p = torch.where((p32 == 0) | (p32 == 1), p32.double(), p)
    y = y.double()
    loss = ((y - 1.0) * torch.clamp(torch.log1p(-p), min=-100.0) - y * torch.clamp(torch.log(p), min=-100.0)).sum() * inv_count
    pq = p * (1.0 - p)
    g = (p - y) / torch.clamp(pq, min=1e-12) * pq * inv_count
    return loss, g, p


def emul_bce_loss_f32(z64, y, inv_count):
    """torch-CPU f32: BCELoss's terms on sigmoid(f32(z)), each term in f32, summed in float64."""
    z = z64.float().cpu()
    terms = F.binary_cross_entropy(torch.sigmoid(z), y.float().cpu(), reduction='none')
    return float(terms.double().sum()) * inv_count


def bce_loss_bar(loss_ref, loss_cpu_f32):
    """Relative 1e-6 (the existing tests' bar), or 4 x what torch-CPU f32 itself misses the reference by, whichever is
    larger. The second term matters as soon as logits pass ~10: log1p(-p) of an f32 p within a few ulps of 1 is
    ill-conditioned (at z = 15, 1 - p is 5 ulps: half an ulp on p moves the term by 0.1 of 15), so NO f32 sigmoid + log
    meets 1e-6 there -- tests/test_dense_ref_host.py shows torch-CPU f32 missing it on the saturated-logit inputs."""
    return max(1e-6 * abs(loss_ref), 4.0 * abs(loss_cpu_f32 - loss_ref))


def ref_filter(qkey, keys, ptr, tails, ent_row0, n_local):
    """filter bits / label rows by a Python loop over the index: a [B, n_local] bool tensor (CPU)."""
    keys_l, ptr_l, tails_l = keys.tolist(), ptr.tolist(), tails.tolist()
    pos = {k: i for i, k in enumerate(keys_l)}
    hit = torch.zeros((len(qkey), n_local), dtype=torch.bool)
    for b, k in enumerate(qkey.tolist()):
        i = pos.get(k)
        if i is None:
            continue
        for t in tails_l[ptr_l[i]:ptr_l[i + 1]]:
            if ent_row0 <= t < ent_row0 + n_local:
                hit[b, t - ent_row0] = True
    return hit


def pack_bits(hit, words=None):
    """[B, n] bool -> [B, words] int32, bit (n & 31) of word n >> 5."""
    B, n = hit.shape
    w = (n + 31) // 32
    words = w if words is None else words
    bits = torch.zeros((B, w * 32), dtype=torch.int64, device=hit.device)
    bits[:, :n] = hit.long()
    m = (bits.view(B, w, 32) << torch.arange(32, device=hit.device)).sum(2)
    m = torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)
    out = torch.zeros((B, words), dtype=torch.int32, device=hit.device)
    out[:, :w] = m
    return out


def ill_conditioned_z(n, o, g):
    """Columns with mean 100 and spread 1e-2 (mean / spread = 1e4 > 1 / sqrt(u)): u_in = u_out = u_loop = z, bias NULL,
    so the kernel's (a + b + c) / 3 returns a z within one rounding of these values."""
    return (100.0 + 1e-2 * torch.randn((n, o), generator=g, dtype=torch.float64)).float()


# ----------------------------------------------------------------------------------------------------------------
# f32 emulations on the CPU (host test): where the constants above are measured
def emul_dot_f32(a, b):
    """A B by one sequential f32 chain per output, product and sum rounded separately (numpy f32 arithmetic)."""
    import numpy as np
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    return torch.from_numpy(acc)


def emul_two_pass_rstd_f32(z, eps):
    """Sequential f32 mean, then a sequential f32 sum of (z - mean)^2: (mean, rstd) as f32 tensors."""
    import numpy as np
    zz = z.numpy().astype(np.float32)
    s = np.zeros(zz.shape[1], dtype=np.float32)
    for r in range(zz.shape[0]):
        s = s + zz[r]
    mean = s / np.float32(zz.shape[0])
    q = np.zeros_like(s)
    for r in range(zz.shape[0]):
        d = zz[r] - mean
        q = q + d * d
    var = q / np.float32(zz.shape[0])
    return torch.from_numpy(mean), torch.from_numpy(np.float32(1.0) / np.sqrt(var + np.float32(eps)))


# ----------------------------------------------------------------------------------------------------------------
# Grids. Labels: see the module docstring.
SPLIT = 'split'
G_NT = 'tile/guarded/NT-operand'


def _fast_nt(nt, strips=''):
    return 'tile/fast/NT=%d%s/NT-operand' % (nt, strips)


# (batch, n_local, dim, label): every value of each axis at least twice against two different values of the others.
# dim: split = one half (4), two halves (8), k-block edges (28 32 36 60 64 68), 100, 200, the widest (348 352); aligned
# but past the split's LDS strip (356 384 512); guarded (6 35 198 353). batch: strip of 64 and its tails, pick_nt's
# classes. n_local: row tiles of 16, pairs of 32, 256.
SCORE_CASES = [
    (1, 1, 4, SPLIT), (3, 15, 4, SPLIT), (4, 16, 8, SPLIT), (15, 17, 8, SPLIT), (16, 31, 28, SPLIT), (17, 32, 28, SPLIT),
    (63, 33, 32, SPLIT), (64, 255, 32, SPLIT), (65, 257, 36, SPLIT), (128, 4099, 36, SPLIT), (209, 1, 60, SPLIT),
    (333, 15, 60, SPLIT), (1, 16, 64, SPLIT), (3, 17, 64, SPLIT), (4, 31, 68, SPLIT), (15, 32, 68, SPLIT),
    (16, 33, 100, SPLIT), (17, 255, 100, SPLIT), (63, 257, 200, SPLIT), (64, 4099, 200, SPLIT), (65, 1, 348, SPLIT),
    (128, 15, 348, SPLIT), (209, 16, 352, SPLIT), (333, 4099, 352, SPLIT),
    (1, 17, 356, _fast_nt(2)), (63, 31, 356, _fast_nt(4)), (65, 32, 384, _fast_nt(8)), (200, 33, 384, _fast_nt(13)),
    (209, 255, 512, _fast_nt(8, '/strips128')), (416, 257, 512, _fast_nt(13, '/strips208')),
    (3, 4099, 6, G_NT), (128, 1, 6, G_NT), (4, 15, 35, G_NT), (333, 16, 35, G_NT), (15, 17, 198, G_NT),
    (16, 31, 198, G_NT), (17, 32, 353, G_NT), (64, 33, 353, G_NT),
]
SCORE_EPILOGUES = ('SIGMOID', 'TARGET', 'RANK')
# layouts (b)-(d) of x and ent at three shapes: (batch, n_local, dim, label of the contiguous / window layouts)
SCORE_LAYOUT_CASES = [(17, 33, 36, SPLIT), (65, 257, 200, SPLIT), (63, 31, 384, _fast_nt(4))]
# an entity shard whose first global id is 37: (batch, n_local, dim, label)
SCORE_SHARD_CASES = [(65, 33, 68, SPLIT), (17, 255, 198, G_NT)]
# the distributions of the existing tests (randn * scale, tanh-ed entities): saturated sigmoids and small products
SCORE_RANDN_CASES = [(17, 257, 100, 0.05, SPLIT), (64, 255, 200, 0.5, SPLIT), (65, 33, 36, 4.0, SPLIT), (63, 257, 384, 4.0, _fast_nt(4)),
                     (15, 31, 198, 0.5, G_NT)]

SMALL = 'small_matmul'
G_NN = 'tile/guarded/NN'


def _dma(nt, strips=''):
    return 'tile/fast/NT=%d%s/NN/dma/NONE' % (nt, strips)


# (M, K, N, label): mgcn_matmul_f32 takes small_matmul_kernel for m <= 1024, n <= 4096, k <= 2048, else tile_kernel<NONE>:
# LDS-DMA when K % 4 == 0 and N % 4 == 0, else guarded.
MATMUL_CASES = [
    (1, 1, 1, SMALL), (31, 3, 4, SMALL), (32, 4, 32, SMALL), (33, 15, 36, SMALL), (1024, 16, 64, SMALL), (1, 17, 68, SMALL),
    (31, 100, 128, SMALL), (32, 2048, 132, SMALL), (1024, 2048, 4, SMALL), (1024, 100, 256, SMALL), (32, 4, 1028, SMALL),
    (33, 100, 1040, SMALL),
    (1025, 4, 32, _dma(2)), (1025, 16, 64, _dma(4)), (5003, 100, 128, _dma(8)), (5003, 16, 208, _dma(13)),
    (1025, 100, 212, _dma(8, '/strips128')), (5003, 4, 416, _dma(13, '/strips208')), (1025, 100, 416, _dma(13, '/strips208')),
    (1025, 16, 1028, _dma(13, '/strips208')), (1025, 4, 1040, _dma(13, '/strips208')), (33, 2052, 256, _dma(8, '/strips128')),
    (1, 2052, 208, _dma(13)), (33, 16, 4100, _dma(13, '/strips208')), (1024, 4, 4100, _dma(13, '/strips208')),
    (1025, 1, 1, G_NN), (5003, 3, 36, G_NN), (1025, 15, 132, G_NN), (1025, 17, 68, G_NN), (5003, 17, 212, G_NN),
]
# layouts of A and B at three shapes (the model passes column views whose base is offset by d floats, model.py:61)
MATMUL_LAYOUT_CASES = [(33, 100, 36, SMALL), (1025, 16, 64, _dma(4)), (1025, 100, 212, _dma(8, '/strips128'))]


def _bn(nt, strips=''):
    return 'tile/fast/NT=%d%s/NN/dma/BN_TANH' % (nt, strips)


G_BN = 'tile/guarded/NN/BN_TANH'
# (N, D, O, bias given, extra floats of lda, extra floats of ldo, label). K = 3 D: below one k-slab (D = 4, 5), slab
# tails (12, 20, 100, 172), not a multiple of 4 (D = 5); lda extra 6 breaks the alignment of A's rows (guarded); an ldo
# that is not a multiple of 4 takes the scalar store path of the staged epilogue.
BN_TANH_CASES = [
    (1, 4, 4, True, 0, 0, _bn(2)), (5003, 172, 4, False, 4, 4, _bn(2)), (33, 4, 32, False, 0, 3, _bn(2)), (97, 20, 32, True, 8, 0, _bn(2)),
    (97, 12, 36, True, 0, 0, _bn(4)), (1, 100, 36, False, 4, 1, _bn(4)), (5003, 12, 64, False, 0, 0, _bn(4)), (33, 12, 64, True, 0, 2, _bn(4)),
    (1, 20, 128, True, 0, 4, _bn(8)), (97, 172, 128, False, 0, 0, _bn(8)), (33, 20, 132, False, 0, 0, _bn(13)), (5003, 4, 132, True, 4, 1, _bn(13)),
    (97, 100, 200, True, 0, 0, _bn(13)), (5003, 100, 200, True, 0, 8, _bn(13)), (5003, 100, 208, False, 0, 0, _bn(13)), (1, 12, 208, True, 0, 3, _bn(13)),
    (1, 172, 212, True, 0, 0, _bn(8, '/strips128')), (33, 100, 212, False, 4, 2, _bn(8, '/strips128')),
    (33, 172, 256, False, 0, 0, _bn(8, '/strips128')), (97, 4, 256, True, 0, 5, _bn(8, '/strips128')),
    (97, 4, 416, True, 0, 0, _bn(13, '/strips208')), (33, 20, 416, False, 0, 4, _bn(13, '/strips208')),
    (5003, 5, 18, True, 0, 0, G_BN), (33, 5, 200, False, 3, 0, G_BN), (97, 100, 18, True, 0, 1, G_BN), (1, 5, 64, True, 0, 0, G_BN),
    (33, 100, 200, True, 6, 0, G_BN),
]

# (4t): (N, O, bias given, running statistics given, extra floats of ldu). N around the 128-row blocks, O around the
# 256-column trips of combine_sum_kernel / partial_kernel and the 256-column blocks of fold_kernel / stats_finish_kernel.
TRAIN_CASES = [
    (2, 1, True, True, 0), (2, 257, False, False, 3), (127, 3, False, True, 1), (127, 513, True, False, 0), (128, 200, True, True, 8),
    (128, 256, False, False, 0), (129, 257, True, True, 0), (129, 300, False, True, 4), (5003, 200, True, True, 0), (5003, 513, True, True, 7),
    (5003, 1, False, False, 0), (128, 3, True, False, 5), (2, 300, True, True, 0), (127, 256, True, True, 0),
]
TRAIN_ILL_CASES = [(129, 257), (5003, 300)]
# (4s) against (4t) bit for bit, two "ranks" whose first rows are multiples of 128: (N, cut, O)
TRAIN_SPLIT_CASES = [(1000, 384, 257), (5003, 2560, 513)]

# mgcn_matmul_tn_f32 (K, M, N): split-K edges (K < 4, K % 4, around one 256-row block, past the 256-block cap at 65 536),
# the wave / column-tile map (N around 128: have1), M around 16 and at 208.
MATMUL_TN_CASES = [
    (1, 1, 1), (1, 100, 200), (3, 15, 16), (3, 208, 127), (4, 16, 128), (4, 1, 256), (5, 17, 129), (5, 100, 1), (255, 15, 200),
    (255, 208, 256), (256, 16, 16), (256, 17, 127), (257, 100, 128), (257, 1, 129), (1023, 208, 200), (1023, 16, 256),
    (65537, 15, 1), (65537, 17, 128), (70001, 100, 129), (70001, 16, 16), (1023, 100, 127), (256, 208, 129),
]

# mgcn_score_bce_fwd (B, n_local, dim, label smoothing, label): tile_kernel<BCE, NT-operand, NT, fast> only (other shapes
# are refused). Smoothing 0 gives targets 1 / 0, 0.1 gives 0.9 + 1/N and 1/N (n_local = 1 stays unsmoothed: 0.9 + 1 is no target).
def _bce(nt, strips=''):
    return 'tile/fast/NT=%d%s/NT-operand/BCE' % (nt, strips)


BCE_CASES = [
    (4, 1, 4, 0.0, _bce(2)), (4, 4099, 36, 0.1, _bce(2)), (32, 31, 36, 0.0, _bce(2)), (32, 1000, 200, 0.1, _bce(2)),
    (36, 33, 4, 0.1, _bce(4)), (36, 1, 200, 0.0, _bce(4)), (64, 1000, 4, 0.0, _bce(4)), (64, 31, 200, 0.1, _bce(4)),
    (68, 33, 36, 0.0, _bce(8)), (68, 4099, 4, 0.1, _bce(8)), (128, 1, 36, 0.0, _bce(8)), (128, 1000, 200, 0.1, _bce(8)),
    (132, 31, 4, 0.1, _bce(13)), (132, 33, 200, 0.0, _bce(13)), (208, 4099, 36, 0.0, _bce(13)), (208, 1, 4, 0.0, _bce(13)),
    (212, 1000, 36, 0.1, _bce(8, '/strips128')), (212, 31, 200, 0.0, _bce(8, '/strips128')), (256, 33, 4, 0.0, _bce(8, '/strips128')),
    (256, 4099, 200, 0.1, _bce(8, '/strips128')), (416, 1000, 36, 0.0, _bce(13, '/strips208')), (416, 33, 200, 0.1, _bce(13, '/strips208')),
]


def all_labels():
    out = set()
    for case in SCORE_CASES + SCORE_LAYOUT_CASES + SCORE_SHARD_CASES:
        out.update('%s:%s' % (e, case[3]) for e in SCORE_EPILOGUES)
    out.update('%s:%s' % (e, c[4]) for c in SCORE_RANDN_CASES for e in SCORE_EPILOGUES)
    out.update(c[3] for c in MATMUL_CASES + MATMUL_LAYOUT_CASES)
    out.update(c[4] for c in BCE_CASES)
    out.update(c[6] for c in BN_TANH_CASES)
    return out


def case_id(case):
    return '-'.join(str(int(v)) if isinstance(v, bool) else str(v) for v in case).replace('/', '.').replace(' ', '')


def score_inputs(batch, n_local, dim, seed, scale=None):
    """(x, ent, bias) on the CPU: +-U[0.25, 1] for the structural grid; with `scale`, x = randn * scale, ent = tanh(randn)
    (the layer's output range), bias = randn * 0.1 as in the existing tests."""
    g = gen(seed)
    if scale is None:
        return pm_uniform((batch, dim), g), pm_uniform((n_local, dim), g), pm_uniform((n_local,), g)
    return randn_scaled((batch, dim), g, scale), torch.tanh(randn_scaled((n_local, dim), g, 1.0)), randn_scaled((n_local,), g, 0.1)


def seed_of(*nums):
    s = 17
    for v in nums:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def max_ratio(got, want, bar):
    """max |got - want| / bar (bar elementwise or scalar), as a float; inf when got is not finite."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    bar = torch.as_tensor(bar, dtype=torch.float64, device=got.device)
    return float(((got - want).abs() / bar).max())


# ----------------------------------------------------------------------------------------------------------------
# Seeded inputs of the other grids (CPU tensors; the device tests move them, the host test emulates on them)
def matmul_inputs(m, k, n):
    g = gen(seed_of(1, m, k, n))
    return pm_uniform((m, k), g), pm_uniform((k, n), g)


def matmul_tn_inputs(k, m, n):
    g = gen(seed_of(2, k, m, n))
    return pm_uniform((k, m), g), pm_uniform((k, n), g)


def bn_tanh_inputs(n, d, o, with_bias):
    """a [N, 3D], w [3D, O] (scaled so that the pre-activation stays of order 1), bias, BN mean / var / gamma / beta with
    var == 0 in every fifth column (eps alone under the root) and gamma of both signs."""
    g = gen(seed_of(3, n, d, o))
    a, w = pm_uniform((n, 3 * d), g), pm_uniform((3 * d, o), g) * (3.0 / math.sqrt(3.0 * d))
    bias = pm_uniform((o,), g) * 0.2 if with_bias else None
    mean, var = randn_scaled((o,), g, 0.3), torch.rand((o,), generator=g) + 0.5
    var[::5] = 0.0
    gamma, beta = pm_uniform((o,), g) * 1.5, randn_scaled((o,), g, 0.1)
    return a, w, bias, mean, var, gamma, beta


BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def train_inputs(n, o, with_bias, with_running):
    g = gen(seed_of(4, n, o))
    u = [randn_scaled((n, o), g, 0.5) for _ in range(3)]
    bias = randn_scaled((o,), g, 0.1) if with_bias else None
    gamma, beta = pm_uniform((o,), g) * 1.5, randn_scaled((o,), g, 0.1)
    rm = randn_scaled((o,), g, 0.05) if with_running else None
    rv = torch.rand((o,), generator=g) + 0.5 if with_running else None
    gy = randn_scaled((n, o), g, 1.0)
    return u, bias, gamma, beta, rm, rv, gy


# ----------------------------------------------------------------------------------------------------------------
# (4t) / (4s): the bars of the training epilogue, shared by the unsplit test and the split stages at ragged cuts. A partition
# changes the association of the sums, not what is computed: one float64 reference, one set of bars.
def train_bars(inputs, r64, cpu_err):
    """{name: bar} for z, mean, rstd, y, gz, gu, ggamma, gbeta (and rm, rv when running statistics are given), in the order
    the tests report them. inputs = train_inputs(...), r64 = ref_train_epilogue(...) in float64, cpu_err = {name: max |torch-CPU
    f32 autograd - r64|}. z: two adds, a division, an add, each within u / 2 of its result (elementwise). The others:
    derived_bar(cpu_err, floor, today) with floor = 8 u x the result and the largest term of its last additions and today =
    the bar of test_training_layer_kernels_vs_torch_autograd (None: none)."""
    u, bias, gamma, beta, rm, rv, gy = inputs
    zmag = sum(t.double().abs() for t in u) + (bias.double().abs() if bias is not None else 0.0)
    z64 = r64['z']
    zabs = float(z64.abs().max())
    rstd_max = float(r64['rstd'].max())
    S = float((gamma.double().abs() * r64['rstd']).max())                       # |d y / d z| <= |gamma| rstd
    gp = gy.double() * (1 - r64['y'] ** 2)
    gp_max = float(gp.abs().max())
    xh_max = float(((z64 - r64['mean']) * r64['rstd']).abs().max())
    table = {
        # name: (floor = 8 u x the result and the largest term of its last additions, today's bar or None)
        'mean': (8 * U * zabs, None),
        'rstd': (8 * U * rstd_max, None),
        'y': (8 * U, 2e-6),
        'gz': (8 * U * S * gp_max * (1 + xh_max * xh_max), 2e-5 * float(r64['gz'].abs().max())),
        'gu': (8 * U * S * gp_max * (1 + xh_max * xh_max) / 3, 2e-5 * float(r64['gu'].abs().max())),
        'ggamma': (8 * U * (float(r64['ggamma'].abs().max()) + gp_max * xh_max), 2e-5 * float(r64['ggamma'].abs().max())),
        'gbeta': (8 * U * (float(r64['gbeta'].abs().max()) + gp_max), 2e-5 * float(r64['gbeta'].abs().max())),
    }
    if rm is not None:
        table['rm'] = (8 * U * float(r64['rm'].abs().max()), 1e-7)
        table['rv'] = (8 * U * float(r64['rv'].abs().max()), 1e-5 * float(r64['rv'].abs().min()) + 1e-7)
    bars = {'z': 2 * U * zmag + 1e-45}
    for name, (floor, today) in table.items():
        bars[name] = derived_bar(cpu_err[name], floor, today)
    return bars


@functools.lru_cache(maxsize=3)
def train_reference(n, o, with_bias, with_running):
    """(inputs, r64, bars) of train_inputs(n, o, ...), on the CPU: computed once for all the partitions of one shape and shared
    (treat it as read-only)."""
    inputs = train_inputs(n, o, with_bias, with_running)
    u, bias, gamma, beta, rm, rv, gy = inputs
    r64 = ref_train_epilogue(*u, bias, gamma, beta, rm, rv, BN_MOMENTUM, BN_EPS, gy)
    r32 = ref_train_epilogue(*u, bias, gamma, beta, rm, rv, BN_MOMENTUM, BN_EPS, gy, dtype=torch.float32)
    cpu_err = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64 if r64[k] is not None}
    return inputs, r64, train_bars(inputs, r64, cpu_err)


def train_ratios(got, r64, bars):
    """{name: max |got - float64| / bar} over the names of `bars`."""
    return {name: max_ratio(got[name].cpu(), r64[name], bar) for name, bar in bars.items()}


RB = 128                            # rows per statistic block (csrc/train_layer.hip)


def rank_blocks(cuts):
    """[(first row, end row)] of the 128-row blocks of the ranks [cuts[r], cuts[r + 1]), each rank counting from ITS first
    row, in rank-then-block order: the order in which the stages fold them."""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.extend((r, min(r + RB, b)) for r in range(a, b, RB))
    return out


def _chain_fold_f32(terms, blocks):
    """Column sums of the f32 `terms` [N, O] the way the kernels form them: one sequential f32 chain per block, the blocks'
    sums added in the order given. (Short blocks are padded with +0 terms, which change no partial sum.)"""
    longest = max(b - a for a, b in blocks)
    pad = torch.zeros((len(blocks), longest, terms.shape[1]), dtype=torch.float32)
    for i, (a, b) in enumerate(blocks):
        pad[i, :b - a] = terms[a:b]
    s = torch.zeros((len(blocks), terms.shape[1]), dtype=torch.float32)
    for i in range(longest):
        s = s + pad[:, i]
    f = torch.zeros(terms.shape[1], dtype=torch.float32)
    for i in range(len(blocks)):
        f = f + s[i]
    return f


def emul_train_split_f32(inputs, cuts, wrong=None):
    """The five stages of (4s) restated in f32 on the CPU (torch f32 elementwise arithmetic: every operation rounded on its
    own) for ranks [cuts[r], cuts[r + 1]): per-rank 128-row blocks, a sequential chain inside a block, blocks folded in
    rank-then-block order, mean = sum x (1 / float(N)), var = sum / float(N), and rstd, the running statistics, y, gz, gu,
    ggamma, gbeta by the kernels' formulas. Not bit-exact to the device (an fma contracts differently): it shows what an f32
    evaluation in this association is off by. Returns the dict of ref_train_epilogue.
    wrong (the vacuity check of the host test; the statistics returned are those of the rank with the most rows, the hardest
    to tell from right):
      'own_mean'   every rank centres on the mean of its own rows,
      'own_count'  every rank divides the global sums by its own row count."""
    u, bias, gamma, beta, rm, rv, gy = inputs
    n, o = u[0].shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    three = f32(3.0)
    z = (u[0] + u[1] + u[2]) / three
    if bias is not None:
        z = z + bias
    ranks = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    assert cuts[0] == 0 and cuts[-1] == n and all(b >= a for a, b in zip(cuts[:-1], cuts[1:]))
    blocks = rank_blocks(cuts)
    big = max(ranks, key=lambda ab: ab[1] - ab[0])

    def stats(a, b):
        """(mean, count as the kernel's float(n)) that the rank [a, b) uses."""
        if wrong == 'own_mean':
            return _chain_fold_f32(z, rank_blocks([a, b])) * (f32(1.0) / f32(float(b - a))), n
        if wrong == 'own_count':
            return _chain_fold_f32(z, blocks) * (f32(1.0) / f32(float(b - a))), b - a
        return _chain_fold_f32(z, blocks) * (f32(1.0) / f32(float(n))), n

    mean_rows = torch.empty_like(z)                         # the mean each row is centred on (one value unless `wrong`)
    for a, b in ranks:
        mean_rows[a:b] = stats(a, b)[0]
    d = z - mean_rows
    q = _chain_fold_f32(d * d, blocks)
    mean, count = stats(*big)
    var = q / f32(float(count))
    rstd = f32(1.0) / torch.sqrt(var + f32(BN_EPS))
    rstd_rows = rstd
    if wrong == 'own_count':
        rstd_rows = torch.empty_like(z)
        for a, b in ranks:
            rstd_rows[a:b] = f32(1.0) / torch.sqrt(q / f32(float(b - a)) + f32(BN_EPS))
    new_rm = new_rv = None
    if rm is not None:
        unbiased = q / f32(float(count - 1)) if count > 1 else var
        keep, mom = f32(1.0) - f32(BN_MOMENTUM), f32(BN_MOMENTUM)
        new_rm, new_rv = keep * rm + mom * mean, keep * rv + mom * unbiased
    xhat = d * rstd_rows
    y = torch.tanh(xhat * gamma + beta)
    gp = gy * (f32(1.0) - y * y)
    gbeta, ggamma = _chain_fold_f32(gp, blocks), _chain_fold_f32(gp * xhat, blocks)
    inv_n = f32(1.0) / f32(float(n))
    gz = torch.empty_like(z)
    for a, b in ranks:
        inv = f32(1.0) / f32(float(b - a)) if wrong == 'own_count' else inv_n
        rs = rstd_rows[a:b] if rstd_rows.dim() == 2 else rstd_rows
        gz[a:b] = (gamma * rs) * (gp[a:b] - gbeta * inv - xhat[a:b] * (ggamma * inv))
    return dict(z=z, y=y, mean=mean, rstd=rstd, rm=new_rm, rv=new_rv, gz=gz, gu=gz / three, ggamma=ggamma, gbeta=gbeta)


def _each(n):
    return tuple(range(n + 1))      # one row per rank


EIGHT_RANKS_5003 = (0, 640, 1312, 1888, 2496, 3104, 3744, 4352, 5003)      # cuts at multiples of 32, as GraphCSR.balanced_bounds
# (4s) at the cuts training produces: (N, O, bias given, running statistics given, cuts). Cuts that are no multiples of 128:
# a short last block on one rank, a first block that starts mid-way on the next; ranks without rows first, in the middle and
# last; ranks of one row, of 127, 128 and 129; one row per rank up to N = 129 (beyond that the emulation itself nears the bar:
# 0.88 at N = 300 -- every one-row block is one more rounding of the fold).
TRAIN_RAGGED_CASES = [
    (2, 257, False, False, (0, 1, 2)), (2, 257, False, False, (0, 0, 2, 2)),
    (127, 3, False, True, (0, 1, 127)), (127, 3, False, True, (0, 32, 96, 96, 127)), (127, 3, False, True, _each(127)),
    (129, 257, True, True, (0, 1, 129)), (129, 257, True, True, (0, 128, 129)), (129, 257, True, True, (0, 32, 64, 129)),
    (129, 257, True, True, (0, 0, 129, 129)), (129, 257, True, True, _each(129)),
    (300, 200, True, True, (0, 96, 96, 224, 300)), (300, 200, True, True, (0, 127, 255, 300)), (300, 200, True, True, (0, 129, 300)),
    (1000, 200, True, True, (0, 160, 352, 352, 608, 1000)), (1000, 200, True, True, (0, 999, 1000)), (1000, 200, True, True, (0, 1, 1000)),
    (5003, 200, True, True, EIGHT_RANKS_5003), (5003, 200, True, True, (0, 5002, 5003)),
    (5003, 513, True, True, (0, 1696, 3296, 5003)),
]
# extra floats of ldu (the products as column windows of wider tensors, NaN in the spare columns) for some of them
TRAIN_RAGGED_LDU_EXTRA = {(300, 200, (0, 129, 300)): 5, (129, 257, (0, 32, 64, 129)): 3}
# worst |emul_train_split_f32 - float64| / bar over TRAIN_RAGGED_CASES (y at N = 300, cuts 0-127-255-300): a record that
# tests/test_dense_ref_host.py recomputes (stale beyond a factor 2), not the source of any bar.
TRAIN_RAGGED_EMUL_WORST_RATIO_MEASURED = 0.65
# ill-conditioned columns (ill_conditioned_z) on ragged cuts: (N, O, cuts)
TRAIN_RAGGED_ILL_CASES = [(129, 257, (0, 32, 96, 129)), (129, 257, (0, 1, 129)), (5003, 300, (0, 1696, 3296, 5003)),
                          (5003, 300, EIGHT_RANKS_5003)]
# zero-row ranks first and last at block-aligned cuts: bit-identical to (4t). (N, O, cuts)
TRAIN_SPLIT_EMPTY_ENDS = (1000, 257, (0, 0, 128, 1000, 1000))


def ragged_id(case):
    cuts = case[-1]
    tail = 'each1' if len(cuts) > 9 else 'cuts' + '_'.join(str(c) for c in cuts)
    return case_id(case[:-1]) + '-' + tail


def bce_inputs(batch, n_local, dim, logit_scale=None):
    """(x, ent, bias, hit [B, n] bool): +-U[0.25, 1] operands; with `logit_scale` the operands are scaled so that the
    largest |logit| is about that value (40: f32 p saturates at 1; 120: log's clamp at -100 and the 1e-12 floor)."""
    g = gen(seed_of(5, batch, n_local, dim))
    x, ent, bias = pm_uniform((batch, dim), g), pm_uniform((n_local, dim), g), pm_uniform((n_local,), g)
    hit = torch.rand((batch, n_local), generator=g) < 0.1
    if logit_scale is not None:
        z, _ = ref_logits(x, ent, bias)
        s = math.sqrt(logit_scale / float(z.abs().max()))
        x, ent, bias = x * s, ent * s, bias * (s * s)
    return x, ent, bias, hit
