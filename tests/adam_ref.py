"""Float64 reference, inputs and error bars of the clip-and-Adam kernels (csrc/optim.hip, include/mgcn_hip.h (10)).

Reference: clip_grad_norm_'s formulas and torch's single-tensor Adam (amsgrad = False, maximize = False) restated in float64
over lists of tensors and several steps; test_adam_ref_host.py pins it to torch itself run in float64.

Bars, by the rule of dense_ref.derived_bar: 4 x the error that torch-CPU f32 (clip_grad_norm_(foreach=False) +
Adam(foreach=False)) shows against float64 on the same inputs, per tensor and separately for p, m, v and the total norm, but
not below FLOOR_ULP units in the last place of the quantity: a tensor of a handful of elements can have a CPU error of zero
by luck, and an f32 evaluation with one rounding placed differently (a division, a square root) is not bound by that. The
floor is per ELEMENT, and the "quantity" is the largest magnitude that element went through on the way (dense_ref.derived_bar: "the result and the terms of
its last additions"): p = p0 - sum of updates and m = m + (1 - beta1)(g' - m) are rounded at the size of their terms, and
an element that three steps of lr happen to carry close to zero keeps the rounding of where it came from (a 1-element
tensor of the K + 1 list does exactly that; emulating torch's own order of operations in f32 shows it). Where the reference never leaves zero (an all-zero gradient
with zero moments) the bar is zero: the result must be exact. The coefficient is not returned by torch; its bar is the total's relative bar plus two roundings (one
addition, one division): coef (bar_total / total + 2 u), and exactly 1.0 where the norm is below max_norm.
"""
import math

import torch

from . import dense_ref as D

U = D.U
FLOOR_ULP = 4                        # 1 ulp = 2 u
HYPER = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8)
MAX_NORM = 1.0
STEPS = 3
MODES = ('active', 'inactive', 'none')      # norm far above max_norm, far below it (coef exactly 1), no clipping at all
GRAD_SCALE = {'active': 10.0, 'inactive': 1e-4, 'none': 1.0}


def grid_specs(chunk):
    """(numel, role) of the C-ABI grid's list. Roles: plain; zero = all-zero gradients (and zero moments: its update is exactly
    0 without weight decay); empty = no elements; nograd = no gradient (p, m, v must keep their bits); offset1 = all four bases
    one element into their buffers (4-byte aligned only)."""
    C = int(chunk)
    specs = [(n, 'plain') for n in (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)]
    return specs + [(6, 'zero'), (0, 'empty'), (9, 'nograd'), (C + 7, 'offset1')]


def mixed_specs(batch):
    """K + 9 tensors of 1 to 7 elements with every fifth without a gradient and every seventh empty: the norm batches by list
    index, the update by live tensors, so the two launch plans differ."""
    return [(0, 'empty') if i % 7 == 3 else (1 + i % 7, 'nograd' if i % 5 == 2 else 'plain') for i in range(int(batch) + 9)]


def many_specs(batch):
    """K + 1 tensors of 1 to 7 elements: crosses the launch-batch edge."""
    return [(1 + i % 7, 'plain') for i in range(int(batch) + 1)]


def inputs(specs, mode, seed, steps=STEPS):
    """(p0 [list of f32], grads [steps][list of f32 or None]): +-U[0.25, 1] values, parameters scaled by 0.1 (three steps at
    lr 0.01 move them by a third), gradients by GRAD_SCALE[mode]."""
    g = D.gen(D.seed_of(90, seed, MODES.index(mode)))
    p0 = [D.pm_uniform((n,), g) * 0.1 for n, _ in specs]
    grads = []
    for _ in range(steps):
        step = []
        for n, role in specs:
            x = D.pm_uniform((n,), g) * GRAD_SCALE[mode]
            step.append(None if role == 'nograd' else torch.zeros(n) if role == 'zero' else x)
        grads.append(step)
    return p0, grads


def clip_ref(grads, max_norm):
    """(total, coef) in float64: clip_grad_norm_'s formulas."""
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))
    return total, (1.0 if max_norm is None else min(max_norm / (total + 1e-6), 1.0))


def new_scale(p):
    """Per element, the largest magnitude p, m, v went through (the floors' "quantity"), started from the initial values."""
    return dict(p=[x.abs().double() for x in p], m=[torch.zeros_like(x, dtype=torch.float64) for x in p],
                v=[torch.zeros_like(x, dtype=torch.float64) for x in p])


def adam_ref(p, m, v, g, coef, t, lr, betas, eps, weight_decay, scale=None, i=None):
    """One update of one tensor, float64, in place: the issue's formulas. `scale`, `i`: keep new_scale's entry i up to date."""
    b1, b2 = betas
    gc = coef * g.double()
    if weight_decay != 0:
        gc = gc + weight_decay * p
    m += (gc - m) * (1 - b1)
    v.mul_(b2).add_((1 - b2) * gc * gc)
    step_size, bc2_sqrt = lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
    p -= step_size * m / (v.sqrt() / bc2_sqrt + eps)
    if scale is not None and p.numel():
        scale['p'][i] = torch.maximum(scale['p'][i], p.abs())
        scale['m'][i] = torch.maximum(torch.maximum(scale['m'][i], m.abs()), (1 - b1) * gc.abs())
        scale['v'][i] = torch.maximum(scale['v'][i], v.abs())


def reference(p0, grads, max_norm, weight_decay, hyper=HYPER):
    """dict(p, m, v: final float64 lists; totals, coefs: per step) of len(grads) steps from zero moments."""
    p = [x.double().clone() for x in p0]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    steps = [0] * len(p)
    totals, coefs, scale = [], [], new_scale(p)
    for gs in grads:
        total, coef = clip_ref(gs, max_norm)
        totals.append(total)
        coefs.append(coef)
        for i, g in enumerate(gs):
            if g is None:
                continue
            steps[i] += 1
            adam_ref(p[i], m[i], v[i], g, coef, steps[i], hyper['lr'], hyper['betas'], hyper['eps'], weight_decay, scale, i)
    return dict(p=p, m=m, v=v, totals=totals, coefs=coefs, scale=scale)


def torch_steps(p0, grads, max_norm, weight_decay, hyper=HYPER, dtype=torch.float32, optimizer=None):
    """The same steps by torch on the CPU in `dtype`: clip_grad_norm_(foreach=False) + Adam(foreach=False) (or `optimizer`, a
    callable params -> optimizer whose clip_and_step is then used if it has one). Same dict as `reference`."""
    params = [torch.nn.Parameter(x.to(dtype).clone()) for x in p0]
    opt = torch.optim.Adam(params, weight_decay=weight_decay, foreach=False, **hyper) if optimizer is None else optimizer(params)
    totals = []
    for gs in grads:
        for q, g in zip(params, gs):
            q.grad = None if g is None else g.to(dtype).clone()
        if hasattr(opt, 'clip_and_step'):
            total = opt.clip_and_step(max_norm)
        else:
            total = None if max_norm is None else torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
            opt.step()
        totals.append(None if total is None else float(total))
    zero = lambda q: torch.zeros_like(q.detach())
    return dict(p=[q.detach() for q in params], m=[opt.state[q]['exp_avg'] if q in opt.state else zero(q) for q in params],
                v=[opt.state[q]['exp_avg_sq'] if q in opt.state else zero(q) for q in params], totals=totals, opt=opt)


def tensor_bar(cpu, ref, scale):
    """Elementwise bar of one tensor of one quantity: max(4 x the CPU's worst error over the tensor, FLOOR_ULP ulp of `scale`,
    the largest magnitude each element went through); 0.0 where the reference never left zero and the CPU is exact."""
    if ref.numel() == 0:
        return torch.zeros_like(ref, dtype=torch.float64)
    err = float((cpu.double() - ref).abs().max())
    floor = FLOOR_ULP * 2 * U * torch.as_tensor(scale, dtype=torch.float64).expand_as(ref)
    return torch.clamp(floor, min=D.derived_bar(err, 0.0))


def bars(ref, cpu):
    """dict(p, m, v: per tensor, an elementwise bar; totals: per step; coefs: per step) and the measured CPU errors behind them ('cpu_err')."""
    out = {k: [tensor_bar(c, r, s) for c, r, s in zip(cpu[k], ref[k], ref['scale'][k])] for k in ('p', 'm', 'v')}
    out['cpu_err'] = {k: [float((c.double() - r).abs().max()) if r.numel() else 0.0 for c, r in zip(cpu[k], ref[k])] for k in ('p', 'm', 'v')}
    out['totals'], out['coefs'] = [], []
    for t_cpu, t_ref, c_ref in zip(cpu['totals'], ref['totals'], ref['coefs']):
        err = 0.0 if t_cpu is None else abs(t_cpu - t_ref)
        bt = D.derived_bar(err, FLOOR_ULP * 2 * U * t_ref)
        out['totals'].append(bt)
        out['coefs'].append(0.0 if c_ref == 1.0 else c_ref * (bt / t_ref + 2 * U))
    return out


def ratio(got, want, bar):
    """worst |got - want| / bar over a tensor (or scalar), bar a number or elementwise; a zero bar demands exactness there
    (0.0 or inf)."""
    got = torch.as_tensor(got).double().cpu()
    want = torch.as_tensor(want).double()
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64).expand_as(err)
    if bool(((bar == 0) & (err > 0)).any()):
        return math.inf
    return float(torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err)).max())


_cache = {}


def case(kind, chunk, batch, mode, weight_decay):
    """Specs, inputs, reference and bars of one grid case, computed once and shared (never modified by the tests)."""
    key = (kind, int(chunk), int(batch), mode, float(weight_decay))
    if key not in _cache:
        specs = {'grid': grid_specs(chunk), 'many': many_specs(batch), 'mixed': mixed_specs(batch)}[kind]
        p0, grads = inputs(specs, mode, ('grid', 'many', 'mixed').index(kind) + 1)
        max_norm = None if mode == 'none' else MAX_NORM
        ref = reference(p0, grads, max_norm, weight_decay)
        cpu = torch_steps(p0, grads, max_norm, weight_decay)
        _cache[key] = dict(specs=specs, p0=p0, grads=grads, max_norm=max_norm, ref=ref, cpu=cpu, bars=bars(ref, cpu))
    return _cache[key]
