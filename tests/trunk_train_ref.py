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


def cancelling_of(case):
    """The tensors whose exact value is 0 for this geometry. With a 1 x 1 kernel c[b, f, :] = w[f] x0[b, :] + cb[f], and bn1
    removes the per-filter scale w[f] as it removes the shift cb[f]: d conv weight cancels like the other three (its
    float64 value is ~1e-14 of its terms), so its cap is the one of a cancelling tensor as well."""
    return CANCELLING + (('d_conv_w',) if case[2] == 1 else ())


def inputs(case, batch, p):
    """(sd, s, r, keep, inv_keep, gz) on the CPU, f32: trunk_ref's weights and queries, a seeded keep-mask of rate 1 - p
    (None at p = 0, zeros with inv_keep = 0 at p = 1) and a seeded +-U[0.25, 1] gradient of z."""
    _, _, k = T.sizes(case)
    o = case[0] * case[1]
    sd = T.weights(case)
    s, r = T.queries(case, batch)
    g = R.gen(R.seed_of(12, batch, int(round(p * 1000)), *T.geometry(case)))
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


def run(case, sd, s, r, keep, inv_keep, gz, dtype=torch.float64, with_mag=False, tail=None):
    """Every output of the forward and the backward in `dtype` (a dict of detached tensors), and with `with_mag` the
    magnitudes of the reduced ones (same keys). `tail(z, dtype) -> (y, loss)`: backpropagate that loss instead of gz (the
    module test's hidden_drop -> bn2 -> relu), and return y as well."""
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
        self.ref, self.mag = run(case, sd, s, r, keep, inv_keep, gz, torch.float64, with_mag=True, tail=tail)
        f32 = run(case, sd, s, r, keep, inv_keep, gz, torch.float32, tail=tail)
        self.cpu_err = {k: float((f32[k].double() - v).abs().max()) for k, v in self.ref.items()}
        self.floor = {k: 8 * U * float(self.mag[k].abs().max()) for k in self.ref}
        self.bar = {k: R.derived_bar(self.cpu_err[k], self.floor[k]) for k in self.ref}

    def ratio(self, name, got):
        """max |got - ref64| / bar; where the bar is 0 (p = 1: every term of the sum is 0) the value must be exactly the reference's."""
        if self.bar[name] == 0.0:
            return 0.0 if torch.equal(got.detach().cpu().double().reshape(self.ref[name].shape), self.ref[name]) else math.inf
        return R.max_ratio(got.detach().cpu().reshape(self.ref[name].shape), self.ref[name], self.bar[name])


@functools.lru_cache(maxsize=None)
def reference(case, batch, p):
    """The reference of inputs(case, batch, p), computed once per session and shared (treat it as read-only)."""
    return Reference(case, *inputs(case, batch, p))


def vacuity(ref):
    """{name: bar / cap}: the cap is 1e-4 max |ref64| for the eight well-scaled tensors and 1e-4 max(mag) for the three
    analytically cancelling ones. A bar above its cap would pass a kernel that is wrong in the fourth digit."""
    out = {}
    cancelling = cancelling_of(ref.case)
    for k in CAPPED + CANCELLING:
        scale = ref.mag[k] if k in cancelling else ref.ref[k]
        out[k] = ref.bar[k] / (1e-4 * float(scale.abs().max()))
    return out
