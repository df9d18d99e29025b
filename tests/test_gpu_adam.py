"""The clip-and-Adam kernels (csrc/optim.hip) and optim.ClipAdam on a real MI355X: the C ABI over a grid of lengths, alignments
and launch-batch edges against the float64 reference of adam_ref.py, bit reproducibility, refusals, and ClipAdam driving the
goldens' model next to clip_grad_norm_ + torch.optim.Adam (one GPU, a layout switch, a checkpoint hand-over, StepLR with two
groups, the sharded step at one rank and at two ranks over gloo).

Model-level comparisons: the two optimizers run their own steps, so from the second step on they see slightly different
gradients. Each run is therefore held against float64 optimizer arithmetic ON ITS OWN RECORDED GRADIENTS (adam_ref's formulas):
the torch pair's distance to that is the measured f32 error, 4 x it (floored, adam_ref.tensor_bar) is the bar, and the HIP
run's distance to ITS float64 twin must stay inside the bar. Everything is compared in reference edge order.

Conditioning, one place only. In test_step_lr_and_two_groups the second group has weight_decay = 0.01, and there
g' = coef g + wd p can cancel. The golden model's conv1.loop_weight has such an element (flat index 315: p = -0.12934,
coef g = 0.0012934 at the first step), where |g'| comes down to a few eps and the update lr g' / (|g'| + eps) depends on the
last bit of coef g. Measured there with the per-tensor bar alone: HIP 9.0e-7 from its float64 twin, the torch pair 2.0e-7 from
its own (five times its error anywhere else in the tensor), bar 8.0e-7, ratio 1.126; every other tensor of that run sat at
0.01 - 0.63. No f32 evaluation resolves such an element: g' carries u (|coef g| + |wd p| + |g'|) of rounding from its two
products and its sum, and coef is itself an f32 result (a division and an addition, 2 u), together about 4 u |coef g| at a
cancellation -- what a relative change of coef by 4 u does -- and the torch pair's error there is one draw of that. So for
that test alone, and only at elements of a weight-decay group where the float64 twin's |g'| fell to NEAR_EPS x eps or below
at some step (26 elements in four tensors when measured; the test prints them), `_hold` adds the twin's own sensitivity to that perturbation: half the
distance between the twins run with coef (1 + 4 u) and coef (1 - 4 u). NEAR_EPS = 100: the update's slope
lr eps / (|g'| + eps)^2 times 4 u |coef g| (3e-10 at that element) stays under a tenth of the floor once |g'| > 100 eps.
At those elements the term is needed for m and v as well as p: the next step's g' = coef g + wd p takes p's error in through
the weight decay, so m moves by (1 - beta1) wd dp per step (measured with the term on p alone: m of conv1.loop_weight at
ratio 1.180, 1.7e-9 off where p is 9e-7 off and 0.1 x 0.01 x 9e-7 x 2 steps = 1.8e-9). Every other element and every other
model-level test are held to the plain bar for p, m and v."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from . import adam_ref as A
from . import dense_ref as D
from .test_gpu_train_sharded import _batches, _models, _np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HYP = A.HYPER
NEAR_EPS = 100.0


def _consts(pkg):
    return pkg._native.ADAM_CHUNK, pkg._native.ADAM_BATCH


def _i64(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*vals)


def _ptrs(vals):
    return (ctypes.c_void_p * max(len(vals), 1))(*vals)


class _Slot(object):
    """One tensor of the grid: p, m, v as windows of guarded buffers (at element `off` of the buffer), g a plain tensor."""

    def __init__(self, n, role, p0):
        self.n, self.role, self.off = n, role, 1 if role == 'offset1' else 0
        self.bufs = {k: D.Guarded(1, n + self.off, n + self.off + 8, DEV) for k in 'pmv'}
        for k in 'pmv':
            self.win(k).copy_(p0.to(DEV) if k == 'p' else torch.zeros(n, device=DEV))
        self.gbuf = torch.zeros(n + self.off + 4, device=DEV)

    def win(self, k):
        return self.bufs[k].buf[0, self.off:self.off + self.n]

    def grad(self):
        return self.gbuf[self.off:self.off + self.n]

    def ptr(self, k):
        t = self.grad() if k == 'g' else self.win(k)
        return t.data_ptr()

    def check(self):
        for k in 'pmv':
            self.bufs[k].check('%s of a %d-element %s tensor' % (k, self.n, self.role))
            if self.off:                                  # the element in front of an offset window still holds the guard
                assert int(self.bufs[k].raw[0, 0]) == self.bufs[k].pattern


def _run_abi(pkg, c, weight_decay, steps=A.STEPS, slots=None):
    """The case's steps through mgcn_adam_sq_norms / mgcn_adam_clip_coef / mgcn_adam_step. Returns (slots, per-step totals,
    per-step coefs, last sq tensor, last out tensor)."""
    lib = pkg._native.lib()
    specs = c['specs']
    slots = slots or [_Slot(n, role, p0) for (n, role), p0 in zip(specs, c['p0'])]
    n = len(slots)
    numel = _i64([s.n for s in slots])
    nbytes = lib.mgcn_adam_sq_norms_workspace(n, numel)
    ws = D.Guarded(1, max(nbytes // 4, 1), nbytes // 4 + 8, DEV)
    stream = torch.cuda.current_stream().cuda_stream
    totals, coefs, sq, out = [], [], None, None
    for k in range(steps):
        for s, g in zip(slots, c['grads'][k]):
            if g is not None:
                s.grad().copy_(g.to(DEV))
        before = [s.gbuf.clone() for s in slots]
        gp = _ptrs([None if g is None else s.ptr('g') for s, g in zip(slots, c['grads'][k])])
        coef_ptr = None
        if c['max_norm'] is not None:
            sq, out = D.Guarded(1, n, n + 8, DEV), D.Guarded(1, 2, 10, DEV)
            assert lib.mgcn_adam_sq_norms(n, gp, numel, sq.ptr(), ws.ptr(), nbytes, stream) == 0, lib.mgcn_last_error()
            assert lib.mgcn_adam_clip_coef(n, sq.ptr(), c['max_norm'], out.ptr(), stream) == 0, lib.mgcn_last_error()
            coef_ptr = out.ptr() + 4
        t = k + 1
        b1, b2 = HYP['betas']
        rc = lib.mgcn_adam_step(n, gp, _ptrs([s.ptr('p') for s in slots]), _ptrs([s.ptr('m') for s in slots]),
                                _ptrs([s.ptr('v') for s in slots]), numel, coef_ptr, HYP['lr'] / (1 - b1 ** t),
                                math.sqrt(1 - b2 ** t), b1, b2, HYP['eps'], weight_decay, stream)
        assert rc == 0, lib.mgcn_last_error()
        torch.cuda.synchronize()
        for s, b in zip(slots, before):
            assert torch.equal(s.gbuf.view(torch.int32), b.view(torch.int32)), 'a gradient was written'
        if out is not None:
            sq.check('sq')
            out.check('total, coef')
            ws.check('workspace')
            totals.append(float(out.view[0, 0]))
            coefs.append(float(out.view[0, 1]))
    return slots, totals, coefs, sq, out


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('mode', A.MODES)
@pytest.mark.parametrize('kind', ['grid', 'many', 'mixed'])
def test_abi_grid_vs_float64(pkg, kind, mode, wd):
    C, K = _consts(pkg)
    c = A.case(kind, C, K, mode, wd)
    slots, totals, coefs, _, _ = _run_abi(pkg, c, wd)
    ref, bars = c['ref'], c['bars']
    worst = {}
    for i, s in enumerate(slots):
        s.check()
        for k in 'pmv':
            worst[k] = max(worst.get(k, 0.0), A.ratio(s.win(k), ref[k][i], bars[k][i]))
        if s.role == 'nograd' or (s.role == 'zero' and wd == 0.0):
            assert torch.equal(s.win('p').cpu(), c['p0'][i]) and not bool(s.win('m').any()) and not bool(s.win('v').any()), s.role
    for k in range(len(totals)):
        worst['total'] = max(worst.get('total', 0.0), A.ratio(totals[k], ref['totals'][k], bars['totals'][k]))
        worst['coef'] = max(worst.get('coef', 0.0), A.ratio(coefs[k], ref['coefs'][k], bars['coefs'][k]))
        if mode == 'inactive':
            assert coefs[k] == 1.0
    for k, r in sorted(worst.items()):
        print('RATIO adam_abi %s/%s/wd%g/%s %.3f' % (kind, mode, wd, k, r))
    assert (mode == 'none') == (not totals)
    for k, r in worst.items():
        assert r <= 1.0, (k, r)


def test_same_inputs_same_bits(pkg):
    C, K = _consts(pkg)
    c = A.case('grid', C, K, 'active', 0.01)
    runs = []
    for _ in range(2):
        slots, _, _, sq, out = _run_abi(pkg, c, 0.01, steps=2)
        runs.append([s.win(k).clone() for s in slots for k in 'pmv'] + [sq.view.clone(), out.view.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_refusals_write_nothing(pkg):
    lib = pkg._native.lib()
    C, K = _consts(pkg)
    c = A.case('many', C, K, 'active', 0.0)
    slots = [_Slot(n, role, p0) for (n, role), p0 in zip(c['specs'], c['p0'])]
    for s, g in zip(slots, c['grads'][0]):
        s.grad().copy_(g.to(DEV))
    n, numel = len(slots), _i64([s.n for s in slots])
    arr = {k: _ptrs([s.ptr(k) for s in slots]) for k in 'gpmv'}
    keep = [s.win(k).clone() for s in slots for k in 'pmv']
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = lib.mgcn_adam_sq_norms_workspace(n, numel)
    sq, ws, out = D.Guarded(1, n, n + 8, DEV), D.Guarded(1, nbytes // 4, nbytes // 4 + 8, DEV), D.Guarded(1, 2, 10, DEV)
    assert lib.mgcn_adam_sq_norms(n, arr['g'], numel, sq.ptr(), ws.ptr(), nbytes - 1, stream) == 1
    assert lib.mgcn_adam_sq_norms(n, arr['g'], _i64([s.n for s in slots[:-1]] + [-1]), sq.ptr(), ws.ptr(), nbytes, stream) == 1
    assert lib.mgcn_adam_clip_coef(n, sq.ptr(), -1.0, out.ptr(), stream) == 1
    ok = dict(lr=0.01, bc2=0.5, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, numel=numel, m=arr['m'])
    for bad in (dict(b1=1.0), dict(b2=-0.5), dict(eps=-1.0), dict(lr=-0.01), dict(wd=-1.0), dict(bc2=0.0),
                dict(numel=_i64([s.n for s in slots[:-1]] + [-1])), dict(m=_ptrs([s.ptr('m') for s in slots[:-1]] + [None]))):
        a = dict(ok, **bad)
        rc = lib.mgcn_adam_step(n, arr['g'], arr['p'], a['m'], arr['v'], a['numel'], None, a['lr'], a['bc2'], a['b1'], a['b2'],
                                a['eps'], a['wd'], stream)
        assert rc == 1, bad
    torch.cuda.synchronize()
    assert sq.untouched() and ws.untouched() and out.untouched()
    for t, s in zip(keep, [s.win(k) for s in slots for k in 'pmv']):
        assert torch.equal(t.view(torch.int32), s.view(torch.int32))


# -- ClipAdam on the goldens' model -----------------------------------------------------------------------------------------
CLIP = 0.5


def _ref_order(model, name, t):
    """A parameter-shaped tensor of a per-edge table in reference edge order (others as they are), on the CPU."""
    tables = {n for n, _ in model._edge_tables()}
    if name in tables and model._slot_csr is not None and model._edge_shard is None:
        t = t.index_select(0, model._slot_csr.inv_perm.to(t.device))
    return t.detach().cpu().clone()


def _run(pkg, model, dl, make_opt, batches, clip=CLIP, before_step=None, after_step=None, lbl_smooth=0.1):
    """Steps of forward_loss + backward + (clip_and_step | clip_grad_norm_ + step) -- harness.train_device_labels' calls -- with
    everything the float64 twin needs recorded in reference order: p0, per-step gradients, hyperparameters and totals."""
    idx = dl.train_index().to(DEV)
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    opt = make_opt(model)
    model.attach_optimizer(opt)
    run = dict(names=names, grads=[], hyper=[], totals=[], losses=[], clip=clip, model=model)
    model.train()
    for k, q in enumerate(batches):
        if before_step is not None:
            opt = before_step(k, model, opt) or opt
        opt.zero_grad()
        loss = model.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=lbl_smooth)
        loss.backward()
        if k == 0:
            run['p0'] = [_ref_order(model, n, p) for n, p in zip(names, params)]
        run['grads'].append([None if p.grad is None else _ref_order(model, n, p.grad) for n, p in zip(names, params)])
        group_of = {id(p): g for g in opt.param_groups for p in g['params']}
        run['hyper'].append([(group_of[id(p)]['lr'], group_of[id(p)]['weight_decay'], group_of[id(p)]['betas'],
                              group_of[id(p)]['eps']) for p in params])
        if hasattr(opt, 'clip_and_step'):
            total = opt.clip_and_step(clip)
        else:
            total = torch.nn.utils.clip_grad_norm_(model.parameters(), clip) if clip is not None else None
            opt.step()
        run['totals'].append(None if total is None else float(total))
        run['losses'].append(float(loss))
        if after_step is not None:
            after_step(k, model, opt)
    run['opt'] = opt
    sd = model.optimizer_state_dict(opt)['state']
    order = [id(p) for g in opt.param_groups for p in g['params']]
    state = [sd.get(order.index(id(p)), {}) for p in params]
    run['p'] = [_ref_order(model, n, p) for n, p in zip(names, params)]
    run['m'] = [st['exp_avg'].cpu() if st else torch.zeros_like(x) for st, x in zip(state, run['p'])]
    run['v'] = [st['exp_avg_sq'].cpu() if st else torch.zeros_like(x) for st, x in zip(state, run['p'])]
    return run


def _f64(run, coef_factor=1.0):
    """The run's optimizer arithmetic in float64 on its own recorded gradients and hyperparameters (`coef_factor`: every
    step's clip coefficient times this, for the conditioning term)."""
    p = [x.double().clone() for x in run['p0']]
    m, v, t = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p], [0] * len(p)
    totals, coefs, scale = [], [], A.new_scale(p)
    near = [torch.zeros_like(x, dtype=torch.bool) for x in p]       # weight decay on and |g'| <= NEAR_EPS eps at some step
    for gs, hs in zip(run['grads'], run['hyper']):
        total, coef = A.clip_ref(gs, run['clip'])
        totals.append(total)
        coefs.append(coef)
        coef = coef * coef_factor
        for i, (g, (lr, wd, betas, eps)) in enumerate(zip(gs, hs)):
            if g is not None:
                t[i] += 1
                if wd != 0:
                    near[i] |= (coef * g.double() + wd * p[i]).abs() <= NEAR_EPS * eps
                A.adam_ref(p[i], m[i], v[i], g, coef, t[i], lr, betas, eps, wd, scale, i)
    return dict(p=p, m=m, v=v, totals=totals, coefs=coefs, scale=scale, near=near)


def _hold(tag, hip, ref, cancelling=False):
    """`hip` against its float64 twin within the bars that `ref` (the torch pair) earns against its own. `cancelling`: the
    module docstring's conditioning term, at the elements the twin marks `near`."""
    bars = A.bars(_f64(ref), ref)
    twin = _f64(hip)
    if cancelling:
        hi, lo = _f64(hip, 1.0 + 4 * A.U), _f64(hip, 1.0 - 4 * A.U)
        for i, near in enumerate(twin['near']):
            if bool(near.any()):
                print('%s: %d element(s) of %s with |g\'| <= %g eps' % (tag, int(near.sum()), hip['names'][i], NEAR_EPS))
                for k in ('p', 'm', 'v'):
                    bars[k][i] = bars[k][i] + torch.where(near, (hi[k][i] - lo[k][i]).abs() / 2, torch.zeros_like(bars[k][i]))
    worst = {}
    for k in ('p', 'm', 'v'):
        rs = [A.ratio(hip[k][i], twin[k][i], bars[k][i]) for i in range(len(hip['names']))]
        worst[k] = max(rs)
        bad = [(hip['names'][i], r) for i, r in enumerate(rs) if r > 1.0]
        print('RATIO clip_adam %s/%s %.3f' % (tag, k, worst[k]))
        assert not bad, (tag, k, bad)
    if hip['clip'] is not None:
        r = max(A.ratio(a, b, c) for a, b, c in zip(hip['totals'], twin['totals'], bars['totals']))
        print('RATIO clip_adam %s/total %.3f' % (tag, r))
        assert r <= 1.0, (tag, r)
    return bars


def _adam(lr=0.01, **kw):
    return lambda model: torch.optim.Adam(model.parameters(), lr=lr, **kw)


def _clip_adam(pkg, lr=0.01, **kw):
    return lambda model: pkg.optim.ClipAdam(model.parameters(), lr=lr, **kw)


@pytest.fixture
def deterministic():
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    yield
    torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize('layers', [1, 2])
def test_clip_adam_on_the_golden_model(pkg, deterministic, layers):
    ref_m, dl, params = _models(pkg, 'syn_b', layers)
    hip_m, dl_h, _ = _models(pkg, 'syn_b', layers)
    batches = _batches(dl, 3)
    ref = _run(pkg, ref_m, dl, _adam(), batches)
    hip = _run(pkg, hip_m, dl_h, _clip_adam(pkg), batches)
    assert hip['opt']._hip_step_count == 3 and hip['opt']._torch_step_count == 0
    assert hip['losses'][0] == ref['losses'][0]
    _hold('golden/layers%d' % layers, hip, ref)
    stamp = [p._version for p in hip_m.parameters() if p.grad is not None]
    hip['opt'].step()                                              # the plain step: HIP path too, versions move
    assert hip['opt']._hip_step_count == 4
    assert all(p._version > s for p, s in zip([p for p in hip_m.parameters() if p.grad is not None], stamp))


def test_harness_epoch_loss_with_clip_adam(pkg, deterministic):
    """harness.train_device_labels, two batches: the first loss is the same number; the second differs by what the parameters'
    difference after one step can do to it. That difference is at most bar + the torch pair's own error per element; to first
    order the loss moves by at most sum_i |dL/dp_i| |dp_i|, doubled here for the curvature and for taking the gradient at the
    torch pair's point; plus 4 ulp of the loss for its own f32 evaluation. The epoch's mean halves the second step's share."""
    models = [_models(pkg, 'syn_b') for _ in range(3)]
    queries = models[0][1].train_queries()
    Q = queries.size(0)
    bs = (Q + 1) // 2
    losses = []
    for (model, dl, params), make in zip(models[:2], (_adam(), _clip_adam(pkg))):
        params.clip_grad = CLIP
        opt = make(model)
        losses.append(pkg.harness.train_device_labels(model, queries, dl.train_index().to(DEV), dl.graph, opt, params, bs,
                                                      generator=torch.Generator().manual_seed(4)))
    assert opt._hip_step_count == 2 and opt._torch_step_count == 0
    model, dl, params = models[2]                                   # the torch pair again, by hand, for the bound
    order = torch.randperm(Q, generator=torch.Generator().manual_seed(4))
    b1, b2 = queries[order[:bs]].to(DEV), queries[order[bs:]].to(DEV)
    one = _run(pkg, model, dl, _adam(), [b1], lbl_smooth=params.lbl_smooth)
    bars = A.bars(_f64(one), one)
    opt = one['opt']
    opt.zero_grad()
    loss2 = model.forward_loss(b2[:, 0], b2[:, 1], dl.graph, dl.train_index().to(DEV), lbl_smooth=params.lbl_smooth)
    loss2.backward()
    names = one['names']
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    bound = sum(float(grads[n].abs().sum()) * 1.25 * float(bars['p'][i].max()) for i, n in enumerate(names) if n in grads)
    bound = (2.0 * bound + 8 * A.U * float(loss2)) / 2
    print('RATIO clip_adam harness/loss %.3f (|d| %.3g, bound %.3g)' % (abs(losses[0] - losses[1]) / bound,
                                                                        abs(losses[0] - losses[1]), bound))
    assert abs(losses[0] - losses[1]) <= bound


def test_layout_switch_between_steps(pkg, deterministic):
    """Step, model._use_reference_order(), step again (the forward lays the tables out in slot order once more): the moments
    must have followed their rows both ways, and no pointer of the first step may be reused."""
    def switch(k, model, opt):
        if k == 1:
            model._use_reference_order()
            assert model._slot_csr is None
    ref_m, dl, _ = _models(pkg, 'syn_b')
    hip_m, dl_h, _ = _models(pkg, 'syn_b')
    batches = _batches(dl, 2)
    ref = _run(pkg, ref_m, dl, _adam(), batches, before_step=switch)
    hip = _run(pkg, hip_m, dl_h, _clip_adam(pkg), batches, before_step=switch)
    assert hip['opt']._hip_step_count == 2
    _hold('layout_switch', hip, ref)                         # (m, v of _run come from optimizer_state_dict: reference order)
    i = hip['names'].index('edge_embeddings')
    assert float(hip['m'][i].abs().max()) > 0


@pytest.mark.parametrize('direction', ['hip_to_torch', 'torch_to_hip'])
def test_checkpoint_interchange(pkg, deterministic, direction):
    """Two steps with one optimizer, its optimizer_state_dict loaded into the other kind, one more step: held against float64
    like three steps of one kind (the float64 twin does not know which optimizer ran a step)."""
    first, second = (_clip_adam(pkg), _adam()) if direction == 'hip_to_torch' else (_adam(), _clip_adam(pkg))

    seen = []

    def hand_over(k, model, opt):
        if k == 2:
            seen.append(opt)
            new = second(model)
            model.load_optimizer_state_dict(new, model.optimizer_state_dict(opt))
            return new
    ref_m, dl, _ = _models(pkg, 'syn_b')
    mix_m, dl_m, _ = _models(pkg, 'syn_b')
    batches = _batches(dl, 3)
    ref = _run(pkg, ref_m, dl, _adam(), batches)
    mix = _run(pkg, mix_m, dl_m, first, batches, before_step=hand_over)
    assert isinstance(mix['opt'], pkg.optim.ClipAdam) == (direction == 'torch_to_hip')
    hip_opt, hip_steps = (seen[0], 2) if direction == 'hip_to_torch' else (mix['opt'], 1)
    assert hip_opt._hip_step_count == hip_steps and hip_opt._torch_step_count == 0
    assert all(float(st['step']) == 3.0 for st in mix['opt'].state.values())
    _hold('interchange/' + direction, mix, ref)


def test_step_lr_and_two_groups(pkg, deterministic):
    """Two groups with their own lr and weight_decay, StepLR halving both after every step: the kernels read the groups' values at
    every call (the float64 twin uses the values recorded at each step)."""
    def two_groups(cls):
        def make(model):
            tables = {id(p) for _, p in model._edge_tables()} | {id(model.entity_embedding)}
            a = [p for p in model.parameters() if id(p) in tables]
            b = [p for p in model.parameters() if id(p) not in tables]
            opt = cls([dict(params=a, lr=0.02, weight_decay=0.0), dict(params=b, lr=0.004, weight_decay=0.01)], lr=1.0)
            opt._sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
            return opt
        return make

    def tick(k, model, opt):
        opt._sched.step()
    ref_m, dl, _ = _models(pkg, 'syn_b')
    hip_m, dl_h, _ = _models(pkg, 'syn_b')
    batches = _batches(dl, 3)
    ref = _run(pkg, ref_m, dl, two_groups(torch.optim.Adam), batches, after_step=tick)
    hip = _run(pkg, hip_m, dl_h, two_groups(pkg.optim.ClipAdam), batches, after_step=tick)
    assert hip['opt']._hip_step_count == 3
    lrs = sorted({h[0] for step in hip['hyper'] for h in step})
    assert lrs == [0.001, 0.002, 0.004, 0.005, 0.01, 0.02]
    _hold('step_lr_two_groups', hip, ref, cancelling=True)


@pytest.mark.parametrize('case,layers,shard', [('syn_b', 1, True), ('syn_a', 2, False)])
def test_sharded_world1_is_the_one_gpu_step(pkg, deterministic, case, layers, shard):
    """train_step_sharded with a ClipAdam at one rank equals forward_loss + backward + clip_and_step bit for bit (3 steps)."""
    ref, dl, params = _models(pkg, case, layers)
    sm, dl_s, _ = _models(pkg, case, layers, shard=shard)
    idx = dl.train_index().to(DEV)
    opt_r, opt_s = pkg.optim.ClipAdam(ref.parameters(), lr=1e-3), pkg.optim.ClipAdam(sm.parameters(), lr=1e-3)
    for q in _batches(dl, 3):
        opt_r.zero_grad()
        loss_r = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
        loss_r.backward()
        opt_r.clip_and_step(0.5)
        loss_s = pkg.dist.train_step_sharded(sm, dl_s.graph, q[:, 0], q[:, 1], idx, opt_s, lbl_smooth=0.1, clip=0.5)
        assert torch.equal(loss_s, loss_r.detach())
    assert opt_r._hip_step_count == 3 and opt_s._hip_step_count == 3
    sd_r, sd_s = ref.state_dict(), sm.state_dict()
    names = {'edge_embeddings'} | {'edge_embeddings_extra.%d' % i for i in range(layers - 1)}
    for k, v in sd_r.items():
        if k in names and shard:                                 # the shard model's state holds slot order
            v = v.index_select(0, ref._slot_csr.perm)
        assert torch.equal(sd_s[k], v), k


# -- two processes on one GPU over gloo -------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    try:
        _worker_body(rank, world, port, q)
    except Exception:                                            # surface the failure in the parent instead of a timeout
        import traceback
        q.put((rank, {'error': traceback.format_exc()}))


def _worker_body(rank, world, port, q):
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    pkg = importlib.import_module('kgc-gcn_amd')
    torch.use_deterministic_algorithms(True, warn_only=True)
    out = {}
    for kind in ('hip', 'torch'):
        sm, dl, params = _models(pkg, 'syn_b', 1, 0.0, shard=True, world=world, rank=rank)
        idx = dl.train_index().to(DEV)
        opt = pkg.optim.ClipAdam(sm.parameters(), lr=0.01) if kind == 'hip' else torch.optim.Adam(sm.parameters(), lr=0.01)
        seen = {}
        named = list(sm.named_parameters())

        def snap():
            seen['grads'] = {n: _np(p.grad) for n, p in named if p.grad is not None}

        if kind == 'hip':
            inner = opt.clip_and_step

            def clip_and_step(max_norm, reduce_sq_norms=None):
                snap()
                seen['norm'] = inner(max_norm, reduce_sq_norms=reduce_sq_norms)
                return seen['norm']
            opt.clip_and_step = clip_and_step
        else:
            inner = pkg.dist.clip_grad_norm_sharded

            def clip_sharded(model, max_norm, group=None):
                snap()
                seen['norm'] = inner(model, max_norm, group)
                return seen['norm']
            pkg.dist.clip_grad_norm_sharded = clip_sharded
        p0 = {n: _np(p) for n, p in named}
        batch = _batches(dl, 1)[0]
        loss = pkg.dist.train_step_sharded(sm, dl.graph, batch[:, 0], batch[:, 1], idx, opt, clip=CLIP)
        if kind == 'torch':
            pkg.dist.clip_grad_norm_sharded = inner
        out[kind] = dict(p0=p0, grads=seen['grads'], norm=float(seen['norm']), loss=float(loss),
                         p={n: _np(p) for n, p in named}, tables=[n for n, _ in sm._edge_tables()],
                         hip_steps=getattr(opt, '_hip_step_count', None))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_clip_adam_vs_torch(pkg):
    """One sharded step over two processes with ClipAdam and one with torch.optim.Adam + clip_grad_norm_sharded, from the same
    state. The global norm in float64 comes from the recorded unclipped gradients (replicated ones once, both ranks' table
    shards); each run's norm and parameters are held against float64 on its own gradients, the bars earned by the torch run."""
    import torch.multiprocessing as mp
    world, port = 2, 33700 + (os.getpid() * 7) % 2000
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        assert 'error' not in got[r], got[r]['error']
    assert got[0]['hip']['hip_steps'] == 1 and got[1]['hip']['hip_steps'] == 1
    tables = set(got[0]['hip']['tables'])

    def norm64(kind):
        s = 0.0
        for r in range(world):
            for n, g in got[r][kind]['grads'].items():
                if n in tables or r == 0:
                    s += float((torch.from_numpy(g).double() ** 2).sum())
        return math.sqrt(s)

    def twin(kind, r, total):
        coef = min(CLIP / (total + 1e-6), 1.0)
        res = {}
        for n, g in got[r][kind]['grads'].items():
            p = torch.from_numpy(got[r][kind]['p0'][n]).double().clone()
            m, v = torch.zeros_like(p), torch.zeros_like(p)
            A.adam_ref(p, m, v, torch.from_numpy(g), coef, 1, 0.01, (0.9, 0.999), 1e-8, 0.0)
            res[n] = p
        return res

    n64 = {kind: norm64(kind) for kind in ('hip', 'torch')}
    for kind in ('hip', 'torch'):
        assert got[0][kind]['norm'] == got[1][kind]['norm'] and got[0][kind]['loss'] == got[1][kind]['loss']
    norm_bar = D.derived_bar(abs(got[0]['torch']['norm'] - n64['torch']), A.FLOOR_ULP * 2 * A.U * n64['torch'])
    r_norm = abs(got[0]['hip']['norm'] - n64['hip']) / norm_bar
    print('RATIO clip_adam two_ranks/total %.3f' % r_norm)
    assert r_norm <= 1.0
    assert abs(got[0]['hip']['norm'] - got[0]['torch']['norm']) <= norm_bar * 1.25 + abs(n64['hip'] - n64['torch'])
    worst = 0.0
    for r in range(world):
        tw_t, tw_h = twin('torch', r, n64['torch']), twin('hip', r, n64['hip'])
        for n in tw_t:
            bar = A.tensor_bar(torch.from_numpy(got[r]['torch']['p'][n]), tw_t[n],
                               torch.maximum(torch.from_numpy(got[r]['torch']['p0'][n]).double().abs(), tw_t[n].abs()))
            ratio = A.ratio(torch.from_numpy(got[r]['hip']['p'][n]), tw_h[n], bar)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (r, n, ratio)
    print('RATIO clip_adam two_ranks/p %.3f' % worst)
    for n, v in got[0]['hip']['p'].items():                       # replicated parameters: the same bits on both ranks
        if n not in tables:
            assert np.array_equal(v, got[1]['hip']['p'][n]), n
