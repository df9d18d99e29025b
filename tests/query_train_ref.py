"""Inputs, references and error bars of the training step's query path (csrc/query_train.hip, paragraph (11) of
include/mgcn_hip.h). A plain module like tests/trunk_train_ref.py: tests/test_query_train_ref_host.py checks it against torch
autograd and its bars against their vacuity caps on the CPU; tests/test_gpu_query_train.py holds the kernels to it.

The row-gradient scatter has an EXACT reference: the sequential f32 loop out[idx[b]] += d[b] in ascending b, in numpy. Its
addends carry mixed magnitudes, so that another order of the same addends gives other bits (checked on the CPU: the reversed
loop differs wherever a row has three or more addends).

The tail (hidden_drop -> bn2 -> relu with batch statistics) is held to float64 torch autograd. The bar of a tensor is
dense_ref.derived_bar(cpu_err, floor): 4 x the largest error the SAME computation shows in torch-CPU f32 against float64 on the
same inputs, floored at 8 u of the terms of the tensor's last additions -- for a batch sum 8 u max(mag), mag being the same sum
over the absolute values of its terms. Nothing is taken from the kernels."""
import functools
import math

import numpy as np
import torch

from . import dense_ref as R

U = R.U
BN_EPS = 1e-5
BN_MOMENTUM = 0.1

# ---------------------------------------------------------------------------------------------------------------- scatter
SCATTER_BATCHES = (1, 2, 3, 63, 64, 65, 257)
SCATTER_DIMS = (1, 3, 4, 200)
SCATTER_ROWS = (1, 5, 300)
PATTERNS = ('distinct', 'equal', 'alternate', 'ends', 'first_last', 'random')


def scatter_index(pattern, B, num_rows):
    """int64 [B] of the pattern, or None where the shape cannot hold it (more distinct indices than rows)."""
    g = R.gen(R.seed_of(21, B, num_rows, PATTERNS.index(pattern)))
    if pattern == 'distinct':
        return torch.randperm(num_rows, generator=g)[:B] if B <= num_rows else None
    if pattern == 'equal':
        return torch.full((B,), num_rows // 2, dtype=torch.int64)
    if pattern == 'alternate':
        return torch.tensor([(2 * num_rows) // 3 if b % 2 else num_rows // 3 for b in range(B)], dtype=torch.int64)
    if pattern == 'ends':                       # row 0 and row num_rows - 1, in a seeded order
        return (torch.rand(B, generator=g) < 0.5).long() * (num_rows - 1)
    if pattern == 'first_last':                 # one index at b = 0 and b = B - 1 only, every other one distinct
        if B < 3 or B - 1 > num_rows:
            return None
        perm = torch.randperm(num_rows, generator=g)[:B - 1]
        return torch.cat([perm, perm[:1]])
    if pattern == 'random':
        return torch.randint(0, num_rows, (B,), generator=g)
    raise ValueError(pattern)


def scatter_addends(B, dim):
    """f32 [B, dim]: +-U[0.25, 1] times a power of two from 2^-12 to 2^12, so that the order of a sum shows in its bits."""
    g = R.gen(R.seed_of(22, B, dim))
    scale = torch.pow(2.0, torch.randint(-12, 13, (B, dim), generator=g).float())
    return R.pm_uniform((B, dim), g) * scale


def scatter_loop(idx, d, num_rows, reverse=False):
    """The contract: out[:] = 0; for b in 0 .. B - 1: out[idx[b], :] += d[b, :], in f32 (numpy), as a torch tensor."""
    idx, d = idx.numpy(), d.numpy().astype(np.float32)
    out = np.zeros((num_rows, d.shape[1]), dtype=np.float32)
    order = range(len(idx) - 1, -1, -1) if reverse else range(len(idx))
    for b in order:
        out[idx[b], :] = out[idx[b], :] + d[b, :]
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------------- tail
TAIL_BATCHES = (2, 3, 15, 16, 17, 63, 130)      # around the 16 row lanes; 130 = several rounds, the last one short
TAIL_DIMS = (1, 32, 200)                        # one column, whole 16-column workgroups, a last workgroup of 8
TAIL_PS = (0.0, 0.3, 1.0)
OUTPUTS = ('x', 'mean', 'rstd', 'rm', 'rv', 'gz', 'd_gamma', 'd_beta')


def tail_inputs(B, O, p):
    """z, keep (bool or None), inv_keep, gamma, beta, running_mean, running_var, gx on the CPU in f32, seeded by (B, O, p)."""
    g = R.gen(R.seed_of(23, B, O, int(round(p * 1000))))
    z = R.pm_uniform((B, O), g)
    gamma, beta = R.pm_uniform((O,), g), R.pm_uniform((O,), g)
    rm, rv = R.randn_scaled((O,), g, 0.1), torch.rand((O,), generator=g) + 0.5
    gx = R.pm_uniform((B, O), g)
    if p <= 0:
        keep, inv_keep = None, 1.0
    elif p >= 1:
        keep, inv_keep = torch.zeros((B, O), dtype=torch.bool), 0.0
    else:
        keep, inv_keep = torch.empty((B, O)).bernoulli_(1.0 - p, generator=g).bool(), 1.0 / (1.0 - p)
    return z, keep, inv_keep, gamma, beta, rm, rv, gx


def tail_run(z, keep, inv_keep, gamma, beta, rm, rv, gx, dtype=torch.float64, with_mag=False):
    """Every output of the tail's forward and backward in `dtype` by plain tensor operations and autograd (a dict of detached
    tensors); with `with_mag` also the magnitudes behind the floors (same keys) and the smallest |pre-activation|."""
    B = z.size(0)
    leaf = lambda v: v.to(dtype).clone().requires_grad_(True)
    z_, g_, b_ = leaf(z), leaf(gamma), leaf(beta)
    u = z_ if keep is None else z_ * keep.to(dtype) * inv_keep
    mean = u.sum(0) / B
    var = ((u - mean) ** 2).sum(0) / B
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    uh = (u - mean) * rstd
    a = uh * g_ + b_
    a.retain_grad()
    x = torch.relu(a)
    x.backward(gx.to(dtype))
    m = BN_MOMENTUM
    unbiased = var * B / (B - 1)
    out = {'x': x, 'mean': mean, 'rstd': rstd, 'rm': (1 - m) * rm.to(dtype) + m * mean, 'rv': (1 - m) * rv.to(dtype) + m * unbiased,
           'gz': z_.grad, 'd_gamma': g_.grad, 'd_beta': b_.grad}
    out = {k: v.detach() for k, v in out.items()}
    if not with_mag:
        return out
    with torch.no_grad():
        ga = a.grad
        mag_db, mag_dg = ga.abs().sum(0), (ga * uh).abs().sum(0)
        mag_mean = u.abs().sum(0) / B
        mag_gu = (g_ * rstd).abs() * (ga.abs() + mag_db / B + uh.abs() * mag_dg / B)
        mag = {'x': (uh * g_).abs() + b_.abs(), 'mean': mag_mean, 'rstd': rstd.abs(),
               'rm': (1 - m) * rm.to(dtype).abs() + m * mag_mean, 'rv': (1 - m) * rv.to(dtype).abs() + m * unbiased,
               'gz': mag_gu if keep is None else mag_gu * keep.to(dtype) * inv_keep, 'd_gamma': mag_dg, 'd_beta': mag_db}
        margin = float(a.abs().min())
    return out, {k: v.detach() for k, v in mag.items()}, margin


class TailReference(object):
    """ref[name] float64, mag[name], cpu_err[name] (torch-CPU f32 against float64) and bar[name] of one set of inputs."""

    def __init__(self, *inputs):
        self.inputs = inputs
        self.ref, self.mag, self.margin = tail_run(*inputs, dtype=torch.float64, with_mag=True)
        f32 = tail_run(*inputs, dtype=torch.float32)
        self.cpu_err = {k: float((f32[k].double() - v).abs().max()) for k, v in self.ref.items()}
        self.floor = {k: 8 * U * float(self.mag[k].abs().max()) for k in self.ref}
        self.bar = {k: R.derived_bar(self.cpu_err[k], self.floor[k]) for k in self.ref}

    def ratio(self, name, got, cols=None):
        """max |got - ref64| / bar (`cols`: got holds these columns of the reference only); where the bar is 0 (p = 1: every
        term of the sum is 0) the value must be exactly the reference's."""
        ref = self.ref[name] if cols is None else self.ref[name][..., cols]
        got = got.detach().cpu().reshape(ref.shape)
        if self.bar[name] == 0.0:
            return 0.0 if torch.equal(got.double(), ref) else math.inf
        return R.max_ratio(got, ref, self.bar[name])


@functools.lru_cache(maxsize=None)
def tail_reference(B, O, p):
    """The reference of tail_inputs(B, O, p), computed once per session and shared (treat it as read-only)."""
    return TailReference(*tail_inputs(B, O, p))


def tail_vacuity(ref):
    """{name: bar / cap}, the cap being 1e-4 of the tensor's scale max |ref64|: a bar above it would pass a kernel that is wrong in
    the fourth digit. A tensor that is all zeros (the gradients at p = 1) has bar 0 and is left out. With B = 2 the normalised
    values of a column are +-1 / sqrt(1 + eps / var), so gz = gamma rstd (ga - mean(ga) - uh mean(ga uh)) cancels analytically
    up to the eps term: there its cap is 1e-4 of its terms, max(mag), as for trunk_train_ref's cancelling tensors."""
    out = {}
    B = ref.inputs[0].size(0)
    for k in OUTPUTS:
        scale = float((ref.mag[k] if (k == 'gz' and B == 2) else ref.ref[k]).abs().max())
        if scale > 0.0:
            out[k] = ref.bar[k] / (1e-4 * scale)
    return out
