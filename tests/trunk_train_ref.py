"""Float64 reference, inputs and error bars of the training-mode ConvE trunk (csrc/conve_train.hip, paragraph (9) of
include/mgcn_hip.h): bn0 -> convolution -> bn1 -> relu -> feature_drop -> fc with batch statistics, forward and backward,
from plain tensor operations and float64 autograd with the dropout mask given. A plain module like tests/trunk_ref.py, whose
grid, weights and queries it reuses: tests/test_trunk_train_ref_host.py checks it against the torch modules in float64 and
its bars against their vacuity caps on the CPU; tests/test_gpu_trunk_train.py holds the kernels to the bars.

The bar of a tensor is dense_ref.derived_bar(cpu_err, floor): 4 x the largest error the SAME computation shows in torch-CPU
f32 against float64 on the same inputs, floored at 8 u of the terms of the tensor's last additions -- for a reduced output
8 u max(mag), mag being the same sum over the absolute values of its terms. Nothing is taken from the kernels."""
import functools
import math

import torch

from . import dense_ref as R
from . import trunk_ref as T

U = R.U
BN_EPS = T.BN_EPS
BN_MOMENTUM = 0.1

REDUCED = ('z', 'd_fc_w', 'd_fc_b', 'd_g1', 'd_b1', 'd_conv_w', 'd_conv_b', 'd_g0', 'd_b0', 'ds', 'dr')
STATS = ('mu0', 'rstd0', 'mu1', 'rstd1', 'rm0', 'rv0', 'rm1', 'rv1')
# the three whose float64 value cancels analytically (bn1 removes a per-filter shift and scale)
CANCELLING = ('d_conv_b', 'd_b0', 'd_g0')
CAPPED = ('z', 'ds', 'dr', 'd_conv_w', 'd_g1', 'd_b1', 'd_fc_w', 'd_fc_b')


GRID_BATCHES = (1, 2, 15, 16, 17, 63)       # around the 16-row tiles and partial blocks; 63 = several blocks, the last one short
PRODUCTION_BATCHES = (128, 130)
SMALL = (4, 8, 3, 8, False)


def grid_cases():
    """(case, B, p) of the parity test: every geometry of trunk_ref.GRID at every batch, the NULL mask (p = 0) and p = 0.2
    alternating over the batches; the production geometry and the small case with the other mask as well; p = 1 once."""
    cases = []
    for case in T.GRID:
        batches = PRODUCTION_BATCHES if case == T.PRODUCTION else GRID_BATCHES
        cases += [(case, b, 0.0 if i % 2 else 0.2) for i, b in enumerate(batches)]
    return cases + [(T.PRODUCTION, 128, 0.0), (SMALL, 17, 0.0), (SMALL, 16, 0.2), (SMALL, 17, 1.0)]


LIMIT_B4096 = (3, 7, 2, 3, False)          # the small geometry with P > 1 (P = 30, K = 90) that takes the batch limit
# (case, B, p, seed). p alternates between the NULL mask and 0.2; seed is the first from 0 upward at which the inputs meet both
# conditions tests/test_trunk_train_ref_host.py asserts: the vacuity() caps, and margin() >= 4.
_LIMIT_CASES = [
    (T.LIMIT_GRID[0], 33, 0.0, 0),
    (T.LIMIT_GRID[1], 65, 0.2, 0),
    (T.LIMIT_GRID[2], 17, 0.0, 1),
    (T.LIMIT_GRID[3], 65, 0.2, 1),
    (T.LIMIT_GRID[4], 17, 0.0, 0),
    (T.LIMIT_GRID[5], 17, 0.2, 0),
    (T.LIMIT_GRID[6], 31, 0.0, 0),
    (T.LIMIT_GRID[7], 18, 0.2, 0),
    (T.LIMIT_GRID[8], 33, 0.0, 0),
    (SMALL, 64, 0.2, 0),
    (SMALL, 65, 0.0, 0),
    (SMALL, 257, 0.2, 0),
    (LIMIT_B4096, 4096, 0.0, 1),
    (LIMIT_B4096, 4095, 0.2, 2),
]
MANY_TAPS = _LIMIT_CASES[2]
MOST_TAPS = _LIMIT_CASES[1]
FULL_BATCH = _LIMIT_CASES[12]
# (case, B) of the module test at the production image with ks = 9: its inputs are trunk_ref's at seed 0, and B is one at which
# they keep margin() >= 4 (the activations do not depend on the masks the test draws on the device)
MODULE_KS9 = (T.LIMIT_GRID[3], 17)


def limit_cases():
    """(case, B, p, seed) at the limits of the training trunk's domain, which grid_cases() (T + 1 <= 50, F <= 200, P >= 30,
    B <= 130) never reaches. Every geometry of trunk_ref.LIMIT_GRID (the training trunk takes them all):
      4x8 ks 8 F 8 bias, B = 33     P = 1 (H = W = 1, ks = k_h = 2 k_w): idx / P, idx % P and k / g.P degenerate, bn1 is a
                                    statistic over the batch alone (hence B >= 16: B P >= 2 is the ABI's minimum, and with very
                                    few rows bn1 over the batch cancels everything), K = F = 8 so the fc product has KU = 1 and
                                    S = 1; T + 1 = 65: the first 256-thread launch of tt_tap_kernel
      16x32 ks 32 F 3, B = 65       T = 1024: accumulator slots s >= 1 of acc[TT_SLOTS_T] hold taps, and the conv-bias sum
                                    t == T lands in slot 4 of thread 0 -- the one shape TT_SLOTS_T = 5 exists for; O = 512,
                                    NCG = 3; K = 3, the non-vector fc path; P = 1; tt_gh_kernel's second 64-row block
      16x32 ks 17 F 4 bias, B = 17  T + 1 = 290: tap slots 0 and 1; P = 256; tt_conv_kernel<0>, the generic convolution, with
                                    a large kernel
      10x20 ks 9 F 32, B = 65       the production image with ks = 9: T + 1 = 82, P = 144
      4x8 ks 4 F 300 bias, B = 17   F > 256: the second block of tt_bn1_finish_kernel and tt_prep_kernel; an even generic ks;
                                    K = 7500
      4x8 ks 3 F 1, B = 17          F = 1
      5x8 ks 6 F 7 bias, B = 31     ks = 6; K = 105, odd
      2x4 ks 3 F 5, B = 18          P = 4
      3x5 ks 4 F 3 bias, B = 33     P = 6
    the small geometry 4x8 ks 3 F 8 at B = 64, 65, 257: tt_gh_kernel's 64-row blocks (r0 = blockIdx.y 64) full, crossed by one
    row, and five of them; and the batch limit at 3x7 ks 2 F 3 (P = 30): B = 4096 = TT_MAX_B fills gb[256] and gg[256] of
    tt_bn0_bwd_apply_kernel, one entry per thread, and B = 4095 leaves the last of the 256 blocks of 16 rows one short."""
    return list(_LIMIT_CASES)


def case_ids(cases):
    """pytest ids of (case, B, p[, seed]) tuples: those pytest itself forms from the three values, '-sN' added for a seed."""
    return ['%s-%d-%s%s' % (T.case_id(c[0]), c[1], c[2], '-s%d' % c[3] if len(c) > 3 else '') for c in cases]


def cancelling_of(case):
    """The tensors whose exact value is 0 for this geometry. With a 1 x 1 kernel c[b, f, :] = w[f] x0[b, :] + cb[f], and bn1
    removes the per-filter scale w[f] as it removes the shift cb[f]: d conv weight cancels like the other three (its
    float64 value is ~1e-14 of its terms), so its cap is the one of a cancelling tensor as well."""
    return CANCELLING + (('d_conv_w',) if case[2] == 1 else ())


def inputs(case, batch, p, seed=0):
    """(sd, s, r, keep, inv_keep, gz) on the CPU, f32: trunk_ref's weights and queries, a seeded keep-mask of rate 1 - p
    (None at p = 0, zeros with inv_keep = 0 at p = 1) and a seeded +-U[0.25, 1] gradient of z. `seed` picks another draw of
    all of them (0: the one every case of grid_cases() has always had)."""
    _, _, k = T.sizes(case)
    o = case[0] * case[1]
    sd = T.weights(case, seed)
    s, r = T.queries(case, batch, seed)
    g = R.gen(R.seed_of(12, batch, int(round(p * 1000)), *(T.geometry(case) + ((seed,) if seed else ()))))
    gz = R.pm_uniform((batch, o), g)
    if p <= 0:
        keep, inv_keep = None, 1.0
    elif p >= 1:
        keep, inv_keep = torch.zeros((batch, k), dtype=torch.bool), 0.0
    else:
        keep, inv_keep = torch.empty((batch, k)).bernoulli_(1.0 - p, generator=g).bool(), 1.0 / (1.0 - p)
    return sd, s, r, keep, inv_keep, gz


def _patches(x, ks):
    """[B, H, W, ks ks] windows of x [B, 2 k_w, k_h]."""
    b = x.size(0)
    pat = x.unfold(1, ks, 1).unfold(2, ks, 1)
    return pat.reshape(b, pat.size(1), pat.size(2), ks * ks)


def run(case, sd, s, r, keep, inv_keep, gz, dtype=torch.float64, with_mag=False, tail=None, extra=()):
    """Every output of the forward and the backward in `dtype` (a dict of detached tensors), and with `with_mag` the
    magnitudes of the reduced ones (same keys). `tail(z, dtype) -> (y, loss)`: backpropagate that loss instead of gz (the
    module test's hidden_drop -> bn2 -> relu), and return y as well. `extra`: intermediates to return with the outputs, 'a'
    (the activation before the relu, [B, F, H, W]) and 'gc' (the gradient of the convolution's output)."""
    k_w, k_h, ks, f, bias = case
    b = s.size(0)
    t = lambda k: sd['conv2.' + k].to(dtype)
    leaf = lambda v: v.clone().requires_grad_(True)
    s_, r_ = leaf(s.to(dtype)), leaf(r.to(dtype))
    w = leaf(t('conv_e.weight').reshape(f, ks * ks))
    cb = leaf(t('conv_e.bias')) if bias else None
    g0, b0, g1, b1 = leaf(t('bn0.weight')), leaf(t('bn0.bias')), leaf(t('bn1.weight')), leaf(t('bn1.bias'))
    fw, fb = leaf(t('fc.weight')), leaf(t('fc.bias'))

    img = torch.stack([s_, r_], dim=2).reshape(b, 2 * k_w, k_h)                 # flat 2 j = s[j], 2 j + 1 = r[j]
    n0 = img.numel()
    mu0 = img.sum() / n0
    var0 = ((img - mu0) ** 2).sum() / n0
    rstd0 = 1.0 / torch.sqrt(var0 + BN_EPS)
    xh = (img - mu0) * rstd0
    x0 = g0 * xh + b0
    x0.retain_grad()
    pat = _patches(x0, ks)
    c = torch.einsum('bhwt,ft->bfhw', pat, w)
    if bias:
        c = c + cb[None, :, None, None]
    c.retain_grad()
    n1 = b * c.size(2) * c.size(3)
    mu1 = c.sum((0, 2, 3)) / n1
    var1 = ((c - mu1[None, :, None, None]) ** 2).sum((0, 2, 3)) / n1
    rstd1 = 1.0 / torch.sqrt(var1 + BN_EPS)
    ch = (c - mu1[None, :, None, None]) * rstd1[None, :, None, None]
    a = g1[None, :, None, None] * ch + b1[None, :, None, None]
    a.retain_grad()
    h = torch.relu(a).reshape(b, -1)
    if keep is not None:
        h = h * keep.to(dtype) * inv_keep
    z = h @ fw.t() + fb
    y = None
    if tail is None:
        z.backward(gz.to(dtype))
    else:
        z.retain_grad()
        y, loss = tail(z, dtype)
        loss.backward()
        gz = z.grad

    m = BN_MOMENTUM
    out = {'z': z, 'mu0': mu0.reshape(1), 'rstd0': rstd0.reshape(1), 'mu1': mu1, 'rstd1': rstd1,
           'rm0': (1 - m) * t('bn0.running_mean') + m * mu0, 'rv0': (1 - m) * t('bn0.running_var') + m * var0 * n0 / (n0 - 1),
           'rm1': (1 - m) * t('bn1.running_mean') + m * mu1, 'rv1': (1 - m) * t('bn1.running_var') + m * var1 * n1 / (n1 - 1),
           'ds': s_.grad, 'dr': r_.grad, 'd_conv_w': w.grad.reshape(f, 1, ks, ks), 'd_g0': g0.grad, 'd_b0': b0.grad,
           'd_g1': g1.grad, 'd_b1': b1.grad, 'd_fc_w': fw.grad, 'd_fc_b': fb.grad}
    if bias:
        out['d_conv_b'] = cb.grad
    else:                                       # without a conv bias the kernel still forms sum gc when asked: same value
        out['d_conv_b'] = c.grad.sum((0, 2, 3))
    if y is not None:
        out['y'] = y
    for k, v in (('a', a), ('gc', c.grad)):
        if k in extra:
            out[k] = v
    out = {k: v.detach() for k, v in out.items()}
    if not with_mag:
        return out
    with torch.no_grad():
        ga, gc, gx0 = a.grad, c.grad, x0.grad
        scale0 = (g0 * rstd0).abs()
        mag = {'z': h.abs() @ fw.abs().t() + fb.abs(),
               'd_fc_b': gz.to(dtype).abs().sum(0), 'd_fc_w': gz.to(dtype).abs().t() @ h.abs(),
               'd_b1': ga.abs().sum((0, 2, 3)), 'd_g1': (ga * ch).abs().sum((0, 2, 3)),
               'd_conv_b': gc.abs().sum((0, 2, 3)),
               'd_conv_w': torch.einsum('bfhw,bhwt->ft', gc.abs(), pat.abs()).reshape(f, 1, ks, ks),
               'd_b0': gx0.abs().sum().reshape(1), 'd_g0': (gx0 * xh).abs().sum().reshape(1)}
    # mag of gx0: the correlation of |gc| with |w|, as the gradient of the convolution with absolute weights
    probe = torch.zeros_like(x0, requires_grad=True)
    (mag_gx0,) = torch.autograd.grad(torch.einsum('bhwt,ft->bfhw', _patches(probe, ks), w.detach().abs()), probe, gc.abs())
    with torch.no_grad():
        mag_gx = scale0 * (mag_gx0 + out['d_b0'].abs() / n0 + xh.abs() * out['d_g0'].abs() / n0)
        flat = mag_gx.reshape(b, -1)
        mag['ds'], mag['dr'] = flat[:, 0::2], flat[:, 1::2]
        mu1_mag = c.abs().sum((0, 2, 3)) / n1
        for k, v in (('mu0', img.abs().sum().reshape(1) / n0), ('rstd0', rstd0.abs().reshape(1)), ('mu1', mu1_mag),
                     ('rstd1', rstd1.abs())):
            mag[k] = v
        for k, stat in (('rm0', 'mu0'), ('rm1', 'mu1')):
            mag[k] = (1 - m) * t('bn%s.running_mean' % k[2]).abs() + m * mag[stat]
        mag['rv0'] = (1 - m) * t('bn0.running_var').abs() + m * var0 * n0 / (n0 - 1)
        mag['rv1'] = (1 - m) * t('bn1.running_var').abs() + m * var1 * n1 / (n1 - 1)
        if y is not None:
            mag['y'] = y.abs() + t('bn2.bias').abs()
    return out, {k: v.detach() for k, v in mag.items()}


class Reference(object):
    """ref[name] float64, mag[name], cpu_err[name] (torch-CPU f32 against float64) and bar[name] of one set of inputs."""

    def __init__(self, case, sd, s, r, keep, inv_keep, gz, tail=None):
        self.case = case
        self.ref, self.mag = run(case, sd, s, r, keep, inv_keep, gz, torch.float64, with_mag=True, tail=tail, extra=('a',))
        f32 = run(case, sd, s, r, keep, inv_keep, gz, torch.float32, tail=tail, extra=('a',))
        a64, a32 = self.ref.pop('a'), f32.pop('a').double()
        # the relu masks: smallest |a| in float64, largest |a32 - a64|, and how many masks torch-CPU f32 flips
        self.a_min, self.a_err = float(a64.abs().min()), float((a32 - a64).abs().max())
        self.a_flips = int(((a32 > 0) != (a64 > 0)).sum())
        self.cpu_err = {k: float((f32[k].double() - v).abs().max()) for k, v in self.ref.items()}
        self.floor = {k: 8 * U * float(self.mag[k].abs().max()) for k in self.ref}
        self.bar = {k: R.derived_bar(self.cpu_err[k], self.floor[k]) for k in self.ref}

    def ratio(self, name, got):
        """max |got - ref64| / bar; where the bar is 0 (p = 1: every term of the sum is 0) the value must be exactly the reference's."""
        if self.bar[name] == 0.0:
            return 0.0 if torch.equal(got.detach().cpu().double().reshape(self.ref[name].shape), self.ref[name]) else math.inf
        return R.max_ratio(got.detach().cpu().reshape(self.ref[name].shape), self.ref[name], self.bar[name])


@functools.lru_cache(maxsize=None)
def reference(case, batch, p, seed=0):
    """The reference of inputs(case, batch, p, seed), computed once per session and shared (treat it as read-only)."""
    return Reference(case, *inputs(case, batch, p, seed))


def margin(ref):
    """smallest float64 |a| / largest |a32 - a64| of the activations before the relu (inf where torch-CPU f32 is exact), or 0
    when torch-CPU f32 flips a mask. Below 4 -- the factor derived_bar gives a kernel over the CPU's f32 error -- an f32
    evaluation inside its bar may flip a relu mask, and the case is a coin toss."""
    if ref.a_flips:
        return 0.0
    return math.inf if ref.a_err == 0.0 else ref.a_min / ref.a_err


def vacuity(ref):
    """{name: bar / cap}: the cap is 1e-4 max |ref64| for the eight well-scaled tensors and 1e-4 max(mag) for the three
    analytically cancelling ones. A bar above its cap would pass a kernel that is wrong in the fourth digit."""
    out = {}
    cancelling = cancelling_of(ref.case)
    for k in CAPPED + CANCELLING:
        scale = ref.mag[k] if k in cancelling else ref.ref[k]
        out[k] = ref.bar[k] / (1e-4 * float(scale.abs().max()))
    return out
