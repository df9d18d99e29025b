"""Float64 reference, inputs, shape grid and error bar of the eval-mode ConvE query trunk (csrc/conve_trunk.hip, paragraph
(8) of include/mgcn_hip.h). A plain module like tests/dense_ref.py, whose constants and helpers it reuses:
tests/test_trunk_ref_host.py checks the reference against the oracle and re-measures the constants at the trunk's lengths
on the CPU; tests/test_gpu_trunk.py holds the kernel to the bar. GRID is the shapes in use; LIMIT_GRID the limits of the domain
both trunks take (kernels up to 1024 taps, one output position, F = 1 and F > 256), with what each geometry reaches beside it.

The trunk, for a query with rows s, r [O], O = k_w k_h (reference model.py:161-175 in eval mode):
  1. image [2 k_w, k_h], flat element 2 j = s[j], 2 j + 1 = r[j] (interleaved, not two stacked halves);
  2. bn0 (one channel, running statistics);
  3. valid ks x ks convolution to F channels of H x W, H = 2 k_w - ks + 1, W = k_h - ks + 1 (bias optional);
  4. bn1 per channel, relu;
  5. flatten to f H W + y W + x;
  6. fc [O, F H W] + bias;
  7. bn2 per output, relu;
  8. [B, O].

The bar (all in float64, u = 2^-24; C_DOT, C_EPI, dot_bar from dense_ref.py -- no new constant):
  conv stage, per activation before the relu: bar1 = (C_DOT + C_EPI) u m1,
      m1 = |s1| (sum |tap| (|s0| |x| + |t0|) + |conv bias| + |mean1|) + |beta1|,  s = gamma / sqrt(var + eps), t0 = beta0 - mean0 s0
      (a dot of ks^2 + 1 terms plus an affine step, in any folding); relu is 1-Lipschitz, so the activation h carries bar1;
  fc stage: bar_z = bar1 |W_fc|^T + D, D = dot_bar(sum |h64| |W| + |b_fc|, K) (the kernel's fc is exact-f32 MFMA);
  output: bar_y = |s2| bar_z + C_EPI u (|s2| (|z64| + |mean2|) + |bn2(z64)| + |beta2|); the last relu is 1-Lipschitz."""
import math

import torch

from . import dense_ref as R

U = R.U
BN_EPS = 1e-5

# (k_w, k_h, ks, F, conv bias): production (also toy_d100, syn_c); the goldens toy_small, syn_a, syn_b; O = 512; ks = 1;
# F H W = 90 (not a multiple of 32; H W = 30 is not a multiple of 4 either)
GRID = [
    (10, 20, 7, 200, False),
    (4, 8, 3, 8, False),
    (3, 8, 3, 6, True),
    (5, 8, 3, 8, False),
    (16, 32, 5, 32, True),
    (4, 8, 1, 5, True),
    (3, 7, 2, 3, False),
]
PRODUCTION = GRID[0]
BATCHES = (1, 63, 128, 333)

# The limits of the trunks' domain (O <= 512, 1 <= ks <= min(2 k_w, k_h), F >= 1), which GRID (ks in {1, 2, 3, 5, 7}, F <= 200,
# T + 1 = ks^2 + 1 <= 50, P = H W >= 30) never reaches. What each geometry is there for, training trunk (9) and eval trunk (8):
#   (4, 8, 8, 8, True)       P = 1 (H = W = 1, ks = k_h = 2 k_w): idx / P, idx % P and k / g.P degenerate, bn1 is a statistic
#                            over the batch alone, K = F = 8 so the fc product has KU = 1 and S = 1; T + 1 = 65, the first
#                            256-thread launch of tt_tap_kernel; eval: PQ = 1, plan_make returns nsplit = 0 -- the one-launch
#                            form with no workspace at every batch
#   (16, 32, 32, 3, False)   T = 1024: accumulator slots s >= 1 of acc[TT_SLOTS_T] hold taps and the conv-bias sum t == T lands
#                            in slot 4 of thread 0; O = 512, NCG = 3; K = 3, the non-vector fc path; P = 1
#   (16, 32, 17, 4, True)    T + 1 = 290: tap slots 0 and 1; P = 256; the generic convolution (KS = 0) with a large kernel
#   (10, 20, 9, 32, False)   the production image with ks = 9: T + 1 = 82, P = 144
#   (4, 8, 4, 300, True)     F > 256: a second block of tt_bn1_finish_kernel and tt_prep_kernel; an even generic ks; K = 7500
#   (4, 8, 3, 1, False)      F = 1: the eval trunk's two-filter software pipeline never iterates, only the tail step runs
#   (5, 8, 6, 7, True)       ks = 6; K = 105, odd
#   (2, 4, 3, 5, False)      eval trunk: P = 4, PQ = 1
#   (3, 5, 4, 3, True)       eval trunk: P = 6, PQ = 2, a second segment that is half zero-weight padding (two positions)
LIMIT_GRID = [
    (4, 8, 8, 8, True),
    (16, 32, 32, 3, False),
    (16, 32, 17, 4, True),
    (10, 20, 9, 32, False),
    (4, 8, 4, 300, True),
    (4, 8, 3, 1, False),
    (5, 8, 6, 7, True),
    (2, 4, 3, 5, False),
    (3, 5, 4, 3, True),
]
LIMIT_BATCHES = (1, 63, 333)


def launch_figures(case):
    """The launch arithmetic of csrc/conve_trunk.hip and csrc/conve_train.hip restated: T taps, P output positions, PQ position
    quads (segments of the eval trunk), K = F P, NCG column groups of 13 tiles of 16 outputs."""
    k_w, k_h, ks, f, _ = case
    h, w, k = sizes(case)
    return dict(T=ks * ks, P=h * w, PQ=(h * w + 3) // 4, K=k, NCG=((k_w * k_h + 15) // 16 + 12) // 13)


def geometry(case):
    """(k_w, k_h, ks, F, O) -- the argument order of the C ABI."""
    k_w, k_h, ks, f, _ = case
    return (k_w, k_h, ks, f, k_w * k_h)


def sizes(case):
    k_w, k_h, ks, f, _ = case
    h, w = 2 * k_w - ks + 1, k_h - ks + 1
    return h, w, f * h * w


def case_id(case):
    return '%dx%d-k%d-f%d%s' % (case[0], case[1], case[2], case[3], '-bias' if case[4] else '')


def hyper(case):
    """The reference's hyper-parameters of a grid case (what oracle.conve_trunk and the model's params read)."""
    k_w, k_h, ks, f, bias = case
    return dict(k_w=k_w, k_h=k_h, kernel_size=ks, num_filter=f, gcn_out_dim=k_w * k_h, bias=bias, feat_drop=0.3, hidden_drop=0.3)


def weights(case, seed=0):
    """A state dict with the reference's key names (f32, CPU): +-U[0.25, 1] weights scaled so that activations and outputs stay
    of order 1, BN statistics and affine pairs away from their defaults (gamma of both signs)."""
    k_w, k_h, ks, f, bias = case
    o = k_w * k_h
    _, _, k = sizes(case)
    g = R.gen(R.seed_of(8, k_w, k_h, ks, f, seed))
    sd = {'conv2.conv_e.weight': R.pm_uniform((f, 1, ks, ks), g) * (1.0 / ks),
          'conv2.fc.weight': R.pm_uniform((o, k), g) * (2.0 / math.sqrt(k)),
          'conv2.fc.bias': R.pm_uniform((o,), g) * 0.2}
    if bias:
        sd['conv2.conv_e.bias'] = R.pm_uniform((f,), g) * 0.2
    for name, n in (('bn0', 1), ('bn1', f), ('bn2', o)):
        sd['conv2.%s.running_mean' % name] = R.randn_scaled((n,), g, 0.3)
        sd['conv2.%s.running_var' % name] = torch.rand((n,), generator=g) + 0.5
        sd['conv2.%s.weight' % name] = R.pm_uniform((n,), g) * 1.5
        sd['conv2.%s.bias' % name] = R.randn_scaled((n,), g, 0.1)
    return sd


def queries(case, batch, seed=0):
    """(s, r) [B, O] f32: +-U[0.25, 1]."""
    o = case[0] * case[1]
    g = R.gen(R.seed_of(9, case[0], case[1], case[2], case[3], batch, seed))
    return R.pm_uniform((batch, o), g), R.pm_uniform((batch, o), g)


def _bn(sd, name, dtype, device):
    t = lambda k: sd['conv2.%s.%s' % (name, k)].to(device=device, dtype=dtype)
    scale = t('weight') / torch.sqrt(t('running_var') + BN_EPS)
    return t('running_mean'), scale, t('bias')


def _patches(case, s, r):
    """[B, H, W, ks, ks] windows of the interleaved image."""
    k_w, k_h, ks, _, _ = case
    img = torch.stack([s, r], dim=2).reshape(s.size(0), 2 * k_w, k_h)      # flat 2 j = s[j], 2 j + 1 = r[j]
    return img.unfold(1, ks, 1).unfold(2, ks, 1)


def ref_trunk(case, sd, s, r, want_conv=False):
    """(y, bar_y) [B, O] in float64 on s's device, from the eight steps; want_conv: also (pre-relu conv stage, m1)."""
    dev, f64 = s.device, torch.float64
    k_w, k_h, ks, f, bias = case
    pat = _patches(case, s.to(f64), r.to(f64))
    mean0, s0, beta0 = _bn(sd, 'bn0', f64, dev)
    mean1, s1, beta1 = _bn(sd, 'bn1', f64, dev)
    mean2, s2, beta2 = _bn(sd, 'bn2', f64, dev)
    w = sd['conv2.conv_e.weight'].to(device=dev, dtype=f64).reshape(f, ks, ks)
    cb = sd['conv2.conv_e.bias'].to(device=dev, dtype=f64) if bias else torch.zeros(f, dtype=f64, device=dev)
    fw, fb = sd['conv2.fc.weight'].to(device=dev, dtype=f64), sd['conv2.fc.bias'].to(device=dev, dtype=f64)
    t0 = beta0 - mean0 * s0
    x0 = (pat - mean0) * s0 + beta0                                                          # 2
    conv = torch.einsum('bhwyx,fyx->bfhw', x0, w) + cb[None, :, None, None]                  # 3
    pre = (conv - mean1[None, :, None, None]) * s1[None, :, None, None] + beta1[None, :, None, None]   # 4
    m1 = s1.abs()[None, :, None, None] * (torch.einsum('bhwyx,fyx->bfhw', s0.abs() * pat.abs() + t0.abs(), w.abs())
                                          + (cb.abs() + mean1.abs())[None, :, None, None]) + beta1.abs()[None, :, None, None]
    h = torch.relu(pre).reshape(s.size(0), -1)                                               # 5
    z = h @ fw.t() + fb                                                                      # 6
    t = (z - mean2) * s2 + beta2
    y = torch.relu(t)                                                                        # 7
    bar1 = ((R.C_DOT + R.C_EPI) * U * m1).reshape(s.size(0), -1)
    bar_z = bar1 @ fw.abs().t() + R.dot_bar(h.abs() @ fw.abs().t() + fb.abs(), h.size(1))
    bar_y = s2.abs() * bar_z + R.C_EPI * U * (s2.abs() * (z.abs() + mean2.abs()) + t.abs() + beta2.abs())
    if want_conv:
        return y, bar_y, pre, m1
    return y, bar_y


def ref_trunk_folded(case, sd, s, r):
    """The same in float64 from the folded form the pack kernel builds: scaled taps, one constant per filter, one
    scale / shift per output."""
    f64 = torch.float64
    k_w, k_h, ks, f, bias = case
    pat = _patches(case, s.to(f64), r.to(f64))
    mean0, s0, beta0 = _bn(sd, 'bn0', f64, s.device)
    mean1, s1, beta1 = _bn(sd, 'bn1', f64, s.device)
    mean2, s2, beta2 = _bn(sd, 'bn2', f64, s.device)
    w = sd['conv2.conv_e.weight'].to(f64).reshape(f, ks, ks)
    cb = sd['conv2.conv_e.bias'].to(f64) if bias else torch.zeros(f, dtype=f64)
    taps = w * s0 * s1[:, None, None]
    const = s1 * ((beta0 - mean0 * s0) * w.sum((1, 2)) + cb - mean1) + beta1
    scale, shift = s2, (sd['conv2.fc.bias'].to(f64) - mean2) * s2 + beta2
    h = torch.relu(torch.einsum('bhwyx,fyx->bfhw', pat, taps) + const[None, :, None, None]).reshape(s.size(0), -1)
    return torch.relu((h @ sd['conv2.fc.weight'].to(f64).t()) * scale + shift)
