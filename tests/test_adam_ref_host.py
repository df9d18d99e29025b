"""CPU-only tests of the clip-and-Adam optimizer: the float64 reference is torch's own arithmetic, the bars rest on measured
f32 errors, ClipAdam falls back to the torch pair off the GPU, its state interchanges with torch.optim.Adam, and the C ABI
carries and validates the new entry points."""
import os
import re

import pytest
import torch

from . import adam_ref as A
from .conftest import ROOT

EINVAL = 1
C, K = 8192, 64          # the values the header and the binding must agree on (checked below)


@pytest.mark.parametrize('mode', A.MODES)
@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_reference_is_torch_in_float64(mode, wd):
    """clip_grad_norm_ + torch.optim.Adam run in float64 on the CPU give the reference to ~1e-14 relative over 3 steps."""
    specs = A.grid_specs(64) + A.many_specs(8)
    p0, grads = A.inputs(specs, mode, 7)
    max_norm = None if mode == 'none' else A.MAX_NORM
    ref = A.reference(p0, grads, max_norm, wd)
    t64 = A.torch_steps(p0, grads, max_norm, wd, dtype=torch.float64)
    for k in ('p', 'm', 'v'):
        for a, b in zip(t64[k], ref[k]):
            if b.numel():
                assert float((a - b).abs().max()) <= 1e-14 * max(float(b.abs().max()), 1e-300) + 0.0, k
    if max_norm is not None:
        for a, b in zip(t64['totals'], ref['totals']):
            assert abs(a - b) <= 1e-14 * b
        assert (mode == 'inactive') == all(c == 1.0 for c in ref['coefs'])
        assert mode != 'active' or all(c < 0.05 for c in ref['coefs'])


@pytest.mark.parametrize('kind', ['grid', 'many', 'mixed'])
@pytest.mark.parametrize('mode', A.MODES)
def test_bars_rest_on_measured_f32_errors(kind, mode):
    """Prints the worst torch-CPU f32 error per quantity and the bar built on it; the bars stay far below the size of one
    update (a kernel that is wrong in the third digit of the step must fail) and the zero-gradient tensor's are zero."""
    c = A.case(kind, C, K, mode, 0.0)
    ref, bars = c['ref'], c['bars']
    for k in ('p', 'm', 'v'):
        worst = max(bars['cpu_err'][k])
        print('%s %s %s: cpu f32 err %.3g, largest bar %.3g' % (kind, mode, k, worst, max(float(b.max()) for b in bars[k] if b.numel())))
    for i, (n, role) in enumerate(c['specs']):
        if n == 0:
            continue
        if role in ('zero', 'nograd'):
            assert not bool(bars['m'][i].any()) and not bool(bars['v'][i].any())
            assert torch.equal(c['cpu']['p'][i], c['p0'][i]) and float(bars['p'][i].max()) <= A.FLOOR_ULP * 2 * A.U * 0.1
            continue
        assert float(bars['p'][i].max()) < 1e-4 * A.HYPER['lr'], (i, bars['p'][i])      # (the first step moves every element by lr)
        assert float(bars['m'][i].max()) < 1e-5 * float(ref['scale']['m'][i].max())      # (of the terms: m itself can cancel)
        assert float(bars['v'][i].max()) < 1e-5 * float(ref['scale']['v'][i].max())
    for bt, t in zip(bars['totals'], ref['totals']):
        assert bt <= 1e-5 * t


def cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (7,), (2, 2, 2))]


def test_clip_adam_on_cpu_is_the_torch_pair_bit_for_bit(pkg):
    ours, theirs = cpu_params(), cpu_params()
    opt = pkg.optim.ClipAdam(ours, lr=0.01, weight_decay=0.01)
    ref = torch.optim.Adam(theirs, lr=0.01, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        for a, b in zip(ours, theirs):
            a.grad = torch.randn(a.shape, generator=g) * 5
            b.grad = a.grad.clone()
        total = opt.clip_and_step(1.0)
        want = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        ref.step()
        assert torch.equal(total, want)
    for a, b in zip(ours, theirs):
        assert torch.equal(a, b)
        for k in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(opt.state[a][k], ref.state[b][k])
    assert opt._torch_step_count == 3 and opt._hip_step_count == 0
    for a in ours:
        a.grad = torch.ones_like(a)
    opt.step()                                             # the plain step falls back too
    assert opt._torch_step_count == 4 and opt._hip_step_count == 0
    assert opt.clip_and_step(None) is None and opt._torch_step_count == 5


def test_fallback_with_a_reducer(pkg):
    """The fallback that is handed a reducer cannot call clip_grad_norm_ (it has no place for one): it takes the per-parameter
    norms as clip_grad_norm_ does, squares them, lets the reducer at them, and clips with clip_grads_with_norm_. With a reducer
    that changes nothing the step is clip_grad_norm_'s to rounding of sqrt(x^2); a reducer that doubles one entry is seen."""
    ours, theirs = cpu_params(), cpu_params()
    opt = pkg.optim.ClipAdam(ours, lr=0.01)
    ref = torch.optim.Adam(theirs, lr=0.01)
    for a, b in zip(ours, theirs):
        a.grad = torch.full_like(a, 2.0)
        b.grad = a.grad.clone()
    seen = []

    def reducer(sq, params):
        seen.append((sq.clone(), list(params)))
    total = opt.clip_and_step(1.0, reduce_sq_norms=reducer)
    want = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    ref.step()
    assert len(seen) == 1 and seen[0][0].shape == (3,) and all(a is b for a, b in zip(seen[0][1], ours))
    assert torch.allclose(seen[0][0], torch.tensor([4.0 * p.numel() for p in ours]), rtol=1e-6, atol=0)
    assert abs(float(total) - float(want)) <= 4 * A.U * float(want) and opt._torch_step_count == 1
    for a, b in zip(ours, theirs):
        assert torch.allclose(a, b, rtol=0, atol=1e-7)
    for a in ours:
        a.grad = torch.full_like(a, 2.0)

    def doubling(sq, params):
        sq[0] *= 4.0
    total2 = opt.clip_and_step(1.0, reduce_sq_norms=doubling)
    assert abs(float(total2) - (4.0 * (4 * 15 + 7 + 8)) ** 0.5) < 1e-5


def test_state_dict_interchanges_with_torch_adam(pkg):
    ours, theirs = cpu_params(), cpu_params()
    opt = pkg.optim.ClipAdam(ours, lr=0.02)
    for a in ours:
        a.grad = torch.full_like(a, 0.5)
    opt.clip_and_step(1.0)
    sd = opt.state_dict()
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'} and sd['state'][0]['step'].device.type == 'cpu'
    ref = torch.optim.Adam(theirs, lr=0.5)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]['lr'] == 0.02 and torch.equal(ref.state[theirs[0]]['exp_avg'], opt.state[ours[0]]['exp_avg'])
    back = pkg.optim.ClipAdam(cpu_params(), lr=0.5)
    back.load_state_dict(ref.state_dict())
    assert float(back.state[back.param_groups[0]['params'][1]]['step']) == 1.0
    assert torch.equal(back.state[back.param_groups[0]['params'][2]]['exp_avg_sq'], opt.state[ours[2]]['exp_avg_sq'])


def test_header_and_binding_carry_the_optimizer(pkg):
    names = ('mgcn_adam_sq_norms_workspace', 'mgcn_adam_sq_norms', 'mgcn_adam_clip_coef', 'mgcn_adam_step')
    with open(os.path.join(ROOT, 'include', 'mgcn_hip.h')) as fh:
        header = fh.read()
    for n in names:
        assert n in pkg._native.EXPORTS and n + '(' in header
    assert '#define MGCN_ABI_VERSION 4' in header and pkg._native.ABI_VERSION == 4
    assert int(re.search(r'#define MGCN_ADAM_CHUNK (\d+)', header).group(1)) == pkg._native.ADAM_CHUNK == C
    assert int(re.search(r'#define MGCN_ADAM_BATCH (\d+)', header).group(1)) == pkg._native.ADAM_BATCH == K
    assert pkg.ClipAdam is pkg.optim.ClipAdam and issubclass(pkg.ClipAdam, torch.optim.Adam)


def test_optimizer_entry_points_refuse_bad_arguments_without_a_gpu(pkg):
    """All argument checks precede the first launch: MGCN_EINVAL on a machine with no GPU (the device pointers are made-up,
    16-byte aligned addresses that are never followed)."""
    import ctypes
    lib = pkg._native.lib()
    P = 0x10000
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    numel = i64(5, 0, C + 1)
    assert lib.mgcn_adam_sq_norms_workspace(3, numel) == 4 * (1 + 0 + 2)
    assert lib.mgcn_adam_sq_norms_workspace(0, None) == 0 and lib.mgcn_adam_sq_norms_workspace(-1, numel) == 0
    assert lib.mgcn_adam_sq_norms_workspace(3, i64(5, -1, 2)) == 0
    three = ptrs(P, None, P)

    def norms(n=3, g=three, numel=numel, sq=P, ws=P, nbytes=12):
        return lib.mgcn_adam_sq_norms(n, g, numel, sq, ws, nbytes, None)

    for kw in (dict(n=-1), dict(g=None), dict(numel=None), dict(numel=i64(5, -1, 2)), dict(sq=None), dict(ws=None), dict(ws=P + 2),
               dict(nbytes=11)):
        assert norms(**kw) == EINVAL, kw
        assert lib.mgcn_last_error()
    for args in ((-1, P, 1.0, P), (2, None, 1.0, P), (2, P, 1.0, None), (2, P, -1.0, P), (2, P, float('nan'), P)):
        assert lib.mgcn_adam_clip_coef(*args, None) == EINVAL, args

    def step(n=3, g=three, p=three, m=three, v=three, numel=numel, lr=0.01, bc2=0.5, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
        return lib.mgcn_adam_step(n, g, p, m, v, numel, None, lr, bc2, b1, b2, eps, wd, None)

    bad = [dict(n=-1), dict(g=None), dict(p=None), dict(m=None), dict(v=None), dict(numel=None), dict(numel=i64(5, 0, -3)),
           dict(p=ptrs(None, None, P)), dict(m=ptrs(P, None, None)), dict(v=ptrs(None, P, P)), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0),
           dict(b2=float('nan')), dict(eps=-1e-8), dict(lr=-0.01), dict(lr=float('nan')), dict(wd=-0.1), dict(bc2=0.0), dict(bc2=1.5)]
    for kw in bad:
        assert step(**kw) == EINVAL, kw
        assert lib.mgcn_last_error()
    assert step(n=0, g=None, p=None, m=None, v=None, numel=None) == 0          # an empty list: nothing to do, nothing launched
    assert step(g=ptrs(None, P, None)) == 0                                      # every tensor skipped (no gradient / no elements)
