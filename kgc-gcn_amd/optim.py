"""ClipAdam: global-norm gradient clipping and the Adam update of main.py:69-70 as one call on the HIP optimizer kernels
(csrc/optim.hip, include/mgcn_hip.h (10)). Opt-in: `opt = ClipAdam(model.parameters(), lr=...)` in place of main.py:217's
torch.optim.Adam; the callers (harness.train, harness.train_device_labels, dist.train_step_sharded) use `clip_and_step`
when the optimizer has one and keep the clip_grad_norm_ + step() pair otherwise.

The state is torch.optim.Adam's, key for key (`step` a CPU scalar tensor, `exp_avg`, `exp_avg_sq`), so state_dict() /
load_state_dict() interchange with torch.optim.Adam in both directions and MGCN.attach_optimizer / optimizer_state_dict /
load_optimizer_state_dict treat it like any Adam.

Gradient contract: after clip_and_step the CONTENTS of .grad are unspecified. clip_grad_norm_ rescales every gradient in
place; the HIP path never writes a gradient (the coefficient is applied where the update reads it) and leaves them unscaled.
Code that reads .grad after the step must not rely on either.
"""
import torch

from . import _native


class ClipAdam(torch.optim.Adam):
    """torch.optim.Adam whose step runs on the HIP kernels, plus `clip_and_step`. Counters: `_hip_step_count` calls took the
    kernels, `_torch_step_count` calls took torch's own sequence (the fallback for anything the kernels do not take: a
    parameter, gradient or moment that is not a contiguous f32 tensor on one GPU, a sparse gradient, amsgrad, maximize,
    capturable, differentiable, fused, decoupled_weight_decay, a tensor lr or beta). One such parameter sends the WHOLE call
    down torch's path, so a step is never half one and half the other.

    Hooks: step() runs the optimizer's registered step pre / post hooks on either path, as any torch optimizer's step does.
    clip_and_step() is not step(): on the HIP path it runs NO step hooks and no profiler record (it only sets `_opt_called`, what
    an lr scheduler's wrapper of step() records, so that schedulers do not warn); on the fallback it calls torch.optim.Adam.step,
    whose hooks run only if that class-level method has been wrapped (torch wraps a class's step when the first optimizer of
    exactly that class is built). Code that relies on step hooks should call step() after clipping on its own.

    The fallback of clip_and_step with a `reduce_sq_norms` cannot be clip_grad_norm_ verbatim (that function has no place for a
    reducer): it takes torch._foreach_norm per parameter, squares, hands the squares to the reducer, and clips with
    clip_grads_with_norm_ to sqrt(sum); without a reducer it is clip_grad_norm_ + Adam.step, bit for bit."""

    _hip_step_count = 0
    _torch_step_count = 0

    # -- which path ------------------------------------------------------------------------------
    def _hip_plan(self):
        """[(group, [parameters with a gradient])] when every group and parameter is one the kernels take, else None."""
        plan, device = [], None
        for group in self.param_groups:
            if group['amsgrad'] or group['maximize'] or group['capturable'] or group['differentiable'] or group.get('fused') or \
                    group.get('decoupled_weight_decay') or torch.is_tensor(group['lr']) or \
                    any(torch.is_tensor(b) for b in group['betas']):
                return None
            ps = []
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                st = self.state.get(p)
                tensors = [p, g] + ([st['exp_avg'], st['exp_avg_sq']] if st else [])
                if g.is_sparse or any(t.layout != torch.strided for t in tensors):
                    return None
                for t in tensors:
                    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                        return None
                    if device is None:
                        device = t.device
                    if t.device != device:
                        return None
                if st and 'max_exp_avg_sq' in st:
                    return None
                ps.append(p)
            plan.append((group, ps))
        return plan

    def _state_of(self, p):
        state = self.state[p]
        if len(state) == 0:                           # torch.optim.Adam._init_group, capturable and fused off
            state['step'] = torch.tensor(0.0, dtype=torch.get_default_dtype())
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif state['step'].is_cuda:                   # (a state dict of a fused / capturable Adam: torch's plain layout keeps
            state['step'] = state['step'].cpu()       # the step on the host, where reading it waits for nothing)
        return state

    @staticmethod
    def _step_hyper(group, step):
        """(step_size, bc2_sqrt) of `group` at step count `step`, in Python doubles as torch's single-tensor Adam forms them: the
        two scalars of kernel (3) that change from step to step. The eager update passes them by value; a captured step writes
        the same doubles, rounded to float, into the device buffer its launches read (hyper_values)."""
        beta1, beta2 = group['betas']
        step_size = group['lr'] / (1 - beta1 ** step)
        bc2_sqrt = (1 - beta2 ** step) ** 0.5
        return step_size, bc2_sqrt

    def _hip_update(self, plan, coef):
        """Kernel (3) over the plan: one call per (group, step count), hyperparameters read from the group now. Between
        begin_device_hyper and end_device_hyper the launches read (step_size, bc2_sqrt) from one row of the device buffer each."""
        touched = []
        dev = self._device_hyper
        for group, ps in plan:
            beta1, beta2 = group['betas']
            by_step = {}
            for p in ps:
                state = self._state_of(p)
                state['step'] += 1
                by_step.setdefault(float(state['step']), []).append((p, state))
            for step, items in by_step.items():
                step_size, bc2_sqrt = self._step_hyper(group, step)
                row = None
                if dev is not None:
                    buf, rows = dev
                    if len(rows) >= buf.size(0):
                        raise _native.NativeError('ClipAdam: the device hyper buffer has %d rows, the step needs more (one per group '
                                                  'and step count)' % buf.size(0))
                    row = buf[len(rows)]
                    rows.append((group, [s for _, s in items]))
                _native.adam_step([p.grad for p, _ in items], [p for p, _ in items], [s['exp_avg'] for _, s in items],
                                  [s['exp_avg_sq'] for _, s in items], coef, step_size, bc2_sqrt, beta1, beta2, group['eps'],
                                  group['weight_decay'], hyper_dev=row)
            touched += ps
        if touched:                                   # written through raw pointers: tell autograd and every (_version, ...) stamp
            torch.autograd.graph.increment_version(touched)
        self._hip_step_count += 1

    # -- a captured step (captured.CapturedTrainStep) ------------------------------------------------
    _device_hyper = None

    def begin_device_hyper(self, buf):
        """From now until end_device_hyper, clip_and_step / step launch the device form of kernel (3): call k (one per group and
        step count, in the order _hip_update issues them) reads (step_size, bc2_sqrt) from row k of `buf`, a contiguous f32
        [rows, 2] device tensor, when it RUNS. Meant for the one pass that is captured into a graph."""
        if buf.dim() != 2 or buf.size(1) != 2 or buf.dtype != torch.float32 or not buf.is_cuda or not buf.is_contiguous():
            raise _native.NativeError('ClipAdam.begin_device_hyper: a contiguous f32 [rows, 2] device tensor is required')
        self._device_hyper = (buf, [])

    def end_device_hyper(self):
        """Back to by-value scalars. Returns the rows the launches in between were bound to: [(group, [state, ...])]."""
        rows, self._device_hyper = ([] if self._device_hyper is None else self._device_hyper[1]), None
        return rows

    def hyper_values(self, rows):
        """[(step_size, bc2_sqrt)] that the NEXT step's launches of `rows` must find in the buffer: _step_hyper at each row's step
        count + 1, from the groups' hyperparameters as they are now (so a scheduler's lr takes effect)."""
        return [self._step_hyper(group, float(states[0]['step']) + 1) for group, states in rows]

    def advance_steps(self, rows):
        """What one replayed step leaves on the host: every row's state['step'] + 1 and the kernel-path counter, no launch."""
        for _, states in rows:
            for state in states:
                state['step'] += 1
        self._hip_step_count += 1
        self._opt_called = True

    # -- public ----------------------------------------------------------------------------------
    @torch.no_grad()
    def clip_and_step(self, max_norm, reduce_sq_norms=None):
        """Clip the gradients of ALL groups to the global norm `max_norm` (clip_grad_norm_'s formulas), then one Adam step.
        Returns the total norm as a 0-dim tensor on the parameters' device, without synchronising; `max_norm=None` skips the
        norm and the clipping and returns None. `reduce_sq_norms(sq, params)` may change the [n] device tensor `sq` of
        per-parameter sums of squares (n = parameters with a gradient, in group order) in place before the coefficient is
        formed, e.g. all-reduce the entries of parameters that are sharded over ranks."""
        self._opt_called = True                        # (what a scheduler's wrapper of step() records)
        plan = self._hip_plan()
        if plan is None:
            return self._torch_clip_and_step(max_norm, reduce_sq_norms)
        params = [p for _, ps in plan for p in ps]
        if not params:
            return None if max_norm is None else torch.tensor(0.0)
        total = coef = None
        if max_norm is not None:
            sq = _native.adam_sq_norms([p.grad for p in params])
            if reduce_sq_norms is not None:
                reduce_sq_norms(sq, params)
            out = _native.adam_clip_coef(sq, max_norm)
            total, coef = out[0], out[1:]
        self._hip_update(plan, coef)
        return total

    def _torch_clip_and_step(self, max_norm, reduce_sq_norms):
        params = [p for group in self.param_groups for p in group['params'] if p.grad is not None]
        total = None
        if max_norm is not None and reduce_sq_norms is None:
            total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        elif max_norm is not None and params:
            sq = torch.stack(list(torch._foreach_norm([p.grad for p in params], 2.0))) ** 2
            reduce_sq_norms(sq, params)
            total = sq.sum().sqrt()
            torch.nn.utils.clip_grads_with_norm_(params, max_norm, total)
        torch.optim.Adam.step(self)
        self._torch_step_count += 1
        return total

    def _torch_step_inside_hooks(self):
        fn = torch.optim.Adam.step                     # (wrapped with the step hooks once a plain Adam has been built: this
        if getattr(fn, 'hooked', False):               # call already runs inside ClipAdam.step's own wrapper)
            fn = fn.__wrapped__
        fn(self)

    def step(self, closure=None):
        """A plain Adam step (no clipping) on kernel (3); torch's own step for what the kernels do not take."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            plan = self._hip_plan()
            if plan is None:
                self._torch_step_inside_hooks()
                self._torch_step_count += 1
            else:
                self._hip_update(plan, None)
        return loss
