"""CapturedTrainStep: one training step of harness.train_device_labels (fused_loss=True) -- zero_grad, MGCN.forward_loss, backward,
ClipAdam.clip_and_step -- captured once into a hipGraph (torch.cuda.CUDAGraph) and replayed, so that a step costs the host a check of the
capture key, one small copy and one replay(), and never waits for the device.

What makes the step capturable: the clip coefficient is formed on the device (optim.ClipAdam), the targets and the loss are built
on the device (MGCN.forward_loss), the counter-based dropout has no generator, and the scalars that change from step to step are
read from device memory by the captured launches: Adam's (step_size, bc2_sqrt) per parameter group (mgcn_adam_step_dev) and the
dropout step word sm(sm(seed) ^ step) (mgcn_dropout_*_dev). Before every replay the wrapper writes the values the eager step would
have passed by value into a pinned buffer and enqueues ONE host-to-device copy ahead of the replay; nothing is computed on the
device that the host computes in the eager step, so the trajectory is the eager one bit for bit wherever the eager step is
reproducible (the HIP trunk and query path). A scheduler's lr, load_dropout_state, a changed seed and model.load_state_dict (an
in-place copy) take effect on the next replay without a new capture.

With params.edge_drop / params.edge_drop_queries on the step's record rewrite is captured too: the zero fill and the
flags kernel follow the batch, mgcn_edge_drop_records_dev reads the same step word, and both switches are part of the capture key.

CapturedCandidateStep, at the end of the module, is the same wrapper around the sampled-negative step: its lists are
drawn inside the graph by mgcn_cand_draw_dev from a second device word that travels in the same copy.

Out of scope: dist.train_step_sharded (its collectives would sit inside the capture), harness.train (its label rows are built on
the host) and torch-drawn dropout (a generator's state does not advance in a replay): the wrapper refuses a dropout site with
p > 0 unless params.dropout is 'counter'.

Counters. `captures`: graphs captured (1 + re-captures); `replays`: steps run from a graph; `eager_steps`: steps run without one
(the warm-up, other batch sizes, everything after a failed capture); `disabled`: a capture raised and the wrapper went eager for
good. model._query_rows_count, conv2._trunk_train_count and conv2._tail_train_count are advanced by Python code, which a replay does
not run: under this wrapper they count eager steps and CAPTURES, not replays.

After a replay every .grad is one of the graph's static tensors (contents unspecified, as after any clip_and_step); the graph's
private pool keeps the step's activations, gradients and workspaces alive for as long as the wrapper lives.
"""
import logging
import operator
import os
import types

import numpy as np
import torch

from . import _native
from .model import _counter_dropout_wanted, edge_drop_switches

_ENV_SWITCHES = ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN', 'MGCN_DROPOUT', 'MGCN_TRAIN_TORCH', 'MGCN_TRUNK', 'MGCN_EDGE_DROP', 'MGCN_EDGE_DROP_QUERIES')
_PARAM_SWITCHES = ('query_path_train', 'conve_trunk_train', 'dropout', 'conve_trunk', 'edge_drop', 'edge_drop_queries')
_RING = 8      # pinned staging slots: the host may run this many replays ahead of the device before it waits for a copy


class CapturedTrainStep(object):
    """step = CapturedTrainStep(model, graph, index, optimizer, lbl_smooth=0.0, clip=None, warmup=2, loss='bce'); loss = step(src, rel).

    `loss` is a 0-dim device tensor; no call waits for the device, and the next call overwrites it (clone it to keep it). The
    first `warmup` (>= 1) calls are ordinary eager steps on the real batches (they create the optimizer state whose addresses
    the graph holds); the next call captures and replays at once. The model must be in training mode. A call with another
    batch size than the captured one (an epoch's last batch) runs eagerly and does not re-capture. The wrapper re-captures
    when something the captured launches hold by value or by address changed: the graph's CSR, the address of a parameter, a
    buffer, an optimizer state tensor or an index tensor, the set of parameters that take a gradient, a dispatch switch or
    its environment variable, a dropout probability, a BatchNorm momentum or eps, betas / eps / weight_decay of a group,
    `lbl_smooth`, `clip` or `loss` (MGCN.forward_loss's 'bce' / 'softmax'; all plain attributes). optimizer.load_state_dict replaces the state tensors and so re-captures;
    model.load_state_dict copies in place and does not.

    Raises NativeError, before anything is captured, for: a model on the CPU, in eval mode (the step is a training step: call
    model.train() first) or holding a table shard; an optimizer without clip_and_step, without ClipAdam's device-hyper hooks, or
    whose _hip_plan() is None; a parameter group whose parameters disagree on the step count; a dropout site with p > 0 while
    params.dropout is not 'counter'; a batch the fused score + loss launch does not take.

    Host cost of a call: besides the copy and the replay, every call re-forms the capture key in Python (addresses of all
    parameters, buffers and optimizer state tensors, the switches): O(number of parameters), no device work, no wait. It is part
    of every wall time tools/bench_train_captured.py reports."""

    def __init__(self, model, graph, index, optimizer, lbl_smooth=0.0, clip=None, warmup=2, loss='bce'):
        self.model, self.graph, self.index, self.optimizer = model, graph, index, optimizer
        self.loss = loss
        self.lbl_smooth, self.clip, self.warmup = float(lbl_smooth), clip, max(1, int(warmup))
        self.captures = self.replays = self.eager_steps = 0
        self.disabled = False
        self._hit = None
        self._stage = None
        self._warmed = False

    # -- the step itself -------------------------------------------------------------------------
    def _body(self, src, rel):
        opt = self.optimizer
        opt.zero_grad(set_to_none=True)
        extra = {} if self.loss == 'bce' else {'loss': self.loss}           # the default is the call as it was
        loss = self.model.forward_loss(src, rel, self.graph, self.index, lbl_smooth=self.lbl_smooth, **extra)
        loss.backward()
        opt.clip_and_step(self.clip)
        return loss.detach()

    def _eager(self, src, rel):
        self.eager_steps += 1
        return self._body(src, rel)

    # -- what a capture depends on -----------------------------------------------------------------
    def _layers(self):
        m = self.model
        return [m.conv1] + list(m.conv1_extra)

    def _dropout_ps(self):
        m = self.model
        return tuple(float(layer.drop.p) for layer in self._layers()) + (
            float(m.params.gcn_drop), float(m.conv2.hidden_drop.p), float(m.conv2.feature_drop.p))

    def _refuse(self, src):
        """The reasons not to capture at all: raised (NativeError) before anything is captured."""
        m, opt = self.model, self.optimizer
        if self.loss not in ('bce', 'softmax'):
            raise _native.NativeError("%s: loss must be 'bce' or 'softmax', got %r" % (type(self).__name__, self.loss))
        if _native.is_ee16(m.edge_embeddings):
            raise _native.NativeError('CapturedTrainStep: this model holds its per-edge tables in bf16 (params.edge_table_dtype), '
                                      'which is inference-only')
        if not m.entity_embedding.is_cuda:
            raise _native.NativeError('CapturedTrainStep: the model is on the CPU; the training step runs on a GPU only')
        if m._edge_shard is not None:
            raise _native.NativeError('CapturedTrainStep: this model holds a shard of the per-edge tables; the sharded step '
                                      '(dist.train_step_sharded) has collectives, which cannot sit inside a capture')
        if not m.training:
            raise _native.NativeError('CapturedTrainStep: the model is in eval mode; call model.train() first')
        if not hasattr(opt, 'clip_and_step'):
            raise _native.NativeError('CapturedTrainStep: the optimizer has no clip_and_step (optim.ClipAdam is required: a captured '
                                      'Adam step reads its bias corrections from device memory)')
        if not all(hasattr(opt, name) for name in ('begin_device_hyper', 'end_device_hyper', 'hyper_values', 'advance_steps', '_hip_plan')):
            raise _native.NativeError('CapturedTrainStep: the optimizer has clip_and_step but not ClipAdam\'s device-hyper hooks '
                                      '(begin_device_hyper, end_device_hyper, hyper_values, advance_steps)')
        if opt._hip_plan() is None:
            raise _native.NativeError('CapturedTrainStep: ClipAdam would take torch\'s own step for this optimizer (amsgrad, maximize, '
                                      'capturable, a tensor lr, a parameter that is not contiguous f32 on one GPU, ...): only the HIP '
                                      'kernels\' step is captured')
        for gi, group in enumerate(opt.param_groups):
            steps = {float(opt.state[p]['step']) for p in group['params'] if opt.state.get(p)}
            if len(steps) > 1:
                raise _native.NativeError('CapturedTrainStep: the parameters of group %d disagree on the step count (%s); one '
                                          '(step_size, bc2_sqrt) pair per group is written per replay' % (gi, sorted(steps)))
        if any(p > 0 for p in self._dropout_ps()) and not _counter_dropout_wanted(m.params):
            raise _native.NativeError('CapturedTrainStep: a dropout site has p > 0 and params.dropout is not \'counter\': masks drawn '
                                      'from a torch generator would be frozen into the graph')
        self._refuse_batch(src)

    def _refuse_batch(self, src):
        """The batch the step's scoring launch does not take (here: the full-table score + loss launch)."""
        m = self.model
        B, O = int(src.numel()), int(m.params.gcn_out_dim)
        probe = torch.empty((B, O), dtype=torch.float32, device=m.entity_embedding.device)
        if B == 0 or not _native.score_bce_supported(probe, probe):
            raise _native.NativeError('CapturedTrainStep: the fused score + loss launch does not take a batch of %d x %d (both must '
                                      'be multiples of 4)' % (B, O))

    def _key(self):
        m, opt, g, ix = self.model, self.optimizer, self.graph, self.index
        # the layout switch every encode begins with (after a load_state_dict the tables are back in reference order): a replay
        # runs no Python of the step, so it happens here, in place, ahead of the replay
        csr, ent_identity, edge_identity = m._layout_for(g)
        key = [id(csr), ent_identity, edge_identity, g.edge_index.data_ptr(), g.edge_attr.data_ptr(), ix.keys.data_ptr(), ix.ptr.data_ptr(), ix.tails.data_ptr(),
               ix.num_rel_ids, self.lbl_smooth, self.clip, self.loss, self._dropout_ps(), int(getattr(m.params, 'gcn_layers', 1))]
        key += [os.environ.get(name) for name in _ENV_SWITCHES] + [getattr(m.params, name, None) for name in _PARAM_SWITCHES]
        key += [(p.data_ptr(), p.requires_grad) for p in m.parameters()] + [b.data_ptr() for b in m.buffers()]
        key += [(bn.momentum, bn.eps) for bn in m.modules() if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm)]
        for group in opt.param_groups:
            key.append((tuple(group['betas']), group['eps'], group['weight_decay'], len(group['params'])))
            for p in group['params']:
                st = opt.state.get(p)
                key.append((p.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()) if st else (p.data_ptr(),))
        return tuple(key)

    def _ready(self):
        """Whether the optimizer state the graph will hold exists: an eager step has run since it was (re)built."""
        opt = self.optimizer
        with_grad = [p for group in opt.param_groups for p in group['params'] if p.grad is not None]
        return bool(with_grad) and all(len(opt.state.get(p, ())) > 0 for p in with_grad)

    # -- staging of the step scalars ---------------------------------------------------------------
    _WORDS = 1     # 64-bit words at the head of the staging buffer: the dropout step word (a subclass may add its own after it)

    def _staging(self, device, rows):
        """The device buffer the captured launches read (8 bytes: the dropout step word; then `rows` float pairs: Adam's
        step_size and bc2_sqrt per group) and a ring of pinned host images of it."""
        st = self._stage
        if st is None or st.device != device or st.rows != rows:
            head = 8 * self._WORDS
            nbytes = head + 8 * rows
            dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
            st = types.SimpleNamespace(device=device, rows=rows, dev=dev, word=dev[:8].view(torch.int64), words=dev[:head].view(torch.int64),
                                       hyper=dev[head:].view(torch.float32).view(rows, 2), slots=[], next=0)
            st.hyper.fill_(1.0)
            for _ in range(_RING):
                host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
                image = host.numpy()
                st.slots.append(types.SimpleNamespace(host=host, word=image[:head].view(np.uint64), hyper=image[head:].view(np.float32),
                                                      event=torch.cuda.Event(), used=False))
            self._stage = st
        return st

    def _upload(self, st, hit):
        """The values the eager step would pass by value now, through one pinned image and one non-blocking copy on the
        current stream."""
        m = self.model
        slot = st.slots[st.next]
        st.next = (st.next + 1) % len(st.slots)
        if slot.used:
            slot.event.synchronize()                  # (its copy of _RING replays ago has long run: this returns at once)
        slot.word[0] = _native.dropout_step_key(m.dropout_seed, m.dropout_step)
        self._stage_words(slot)
        for k, (step_size, bc2_sqrt) in enumerate(self.optimizer.hyper_values(hit.rows)):
            slot.hyper[2 * k], slot.hyper[2 * k + 1] = step_size, bc2_sqrt     # doubles rounded to float, as the by-value call
        st.dev.copy_(slot.host, non_blocking=True)
        slot.event.record()
        slot.used = True

    def _stage_words(self, slot):
        """The words of a subclass (slot.word[1:]), written into the same pinned image: still one copy per replay."""

    def _warm_kernels(self, st):
        """One launch of the device-scalar entry points on scratch tensors, once per wrapper, outside the capture; leaves no
        trace. A precaution of the same kind as the warm-up pass of MGCN._encode_replay: the runtime resolves a kernel (and
        loads its code object) at its first launch, and the eager warm-up steps only ever launched the by-value forms, so
        without this the _dev forms would meet that lazy work inside the capture. The shapes cover the vector and the element
        path and both weight-decay variants; a form this list misses is merely first launched inside the capture."""
        if self._warmed:
            return
        self._warmed = True
        dev = st.device
        k0, k1 = _native.DeviceKey(st.word, 0), _native.DeviceKey(st.word, 1)
        for x in (torch.zeros((2, 8), device=dev), torch.zeros((2, 8), device=dev)[:, :7]):
            _native.dropout_apply(x, k0, 0, 0.5)
            _native.dropout_apply_pair(x, k0, x, k1, 0, 0.5)
            _native.dropout_mask(2, x.size(1), k0, 0, 0.5, out=torch.zeros((2, 8), dtype=torch.uint8, device=dev)[:, :x.size(1)])
        p_edge, by_queries = edge_drop_switches(self.model.params)
        if p_edge > 0 or by_queries:      # this step's records: the _dev rewrite and the flags, into scratch tensors
            csr = self.model._layout_for(self.graph)[0]
            state = csr.edge_drop_state()
            flags = _native.edge_flags_from_queries(torch.zeros(1, dtype=torch.int64, device=dev), state, csr.num_edges_half,
                                                    out=torch.zeros_like(state.forced))
            _native.edge_drop_records(csr, state, _native.DeviceKey(st.word, _native.EDGE_DROP_SITE), p_edge, flags)
        t = [torch.ones(4, device=dev) for _ in range(4)]
        for wd in (0.0, 0.01):
            _native.adam_step([t[0]], [t[1]], [t[2]], [t[3]], None, 0.0, 1.0, 0.9, 0.999, 1e-8, wd, hyper_dev=st.hyper[0])

    # -- capture and replay ------------------------------------------------------------------------
    def _capture(self, src, rel, key):
        m, opt = self.model, self.optimizer
        device = m.entity_embedding.device
        st = self._staging(device, len(opt.param_groups))
        B = int(src.numel())
        s_src = torch.empty(B, dtype=torch.int64, device=device)
        s_rel = torch.empty(B, dtype=torch.int64, device=device)
        self._warm_kernels(st)
        # capturing executes nothing on the device but runs the Python side effects: keep the host counters as they are
        saved_drop = m.dropout_step
        saved_steps = [(state, state['step'].clone()) for state in opt.state.values() if 'step' in state]
        saved_opt = (opt._hip_step_count, getattr(opt, '_opt_called', False))
        graph = torch.cuda.CUDAGraph()
        m._step_key_dev = st.word
        opt.begin_device_hyper(st.hyper)
        rows, err = [], None
        try:
            # thread_local: as MGCN._encode_replay (other threads of the process must not invalidate this capture)
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                loss = self._body(s_src, s_rel)
        except RuntimeError as e:
            err = e
        finally:
            m._step_key_dev = None
            m.conv2._drop_ctx = None
            rows = opt.end_device_hyper()
            advance = m.dropout_step - saved_drop
            m.dropout_step = saved_drop
            for state, step in saved_steps:
                state['step'].copy_(step)
            opt._hip_step_count, opt._opt_called = saved_opt
        if err is not None:                              # capture refused: the same launches, without a graph, from now on
            logging.warning('hipGraph capture of the training step failed (%s): running the step eagerly', err)
            torch.cuda.synchronize()
            self.disabled = True
            return None
        written = [p for p in m.parameters() if p.grad is not None]
        for bn in m.modules():
            if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
                written += [b for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked) if b is not None]
        self.captures += 1
        self._hit = types.SimpleNamespace(key=key, graph=graph, loss=loss, rows=rows, batch=B, src=s_src, rel=s_rel, written=written,
                                          dropout_advance=advance)
        return self._hit

    def _replay(self, hit, src, rel):
        m = self.model
        self._upload(self._stage, hit)
        hit.src.copy_(src.reshape(-1), non_blocking=True)
        hit.rel.copy_(rel.reshape(-1), non_blocking=True)
        hit.graph.replay()
        # the host mirrors of what the eager step advances, and the version stamps of everything the graph wrote
        m.dropout_step += hit.dropout_advance
        self.optimizer.advance_steps(hit.rows)
        torch.autograd.graph.increment_version(hit.written)
        self.replays += 1
        return hit.loss

    def __call__(self, src, rel):
        if self.disabled:
            return self._eager(src, rel)
        hit = self._hit
        if hit is not None and int(src.numel()) != hit.batch:
            return self._eager(src, rel)                # e.g. an epoch's last batch: no re-capture
        if hit is None:
            self._refuse(src)
        key = self._key()
        if hit is None or hit.key != key:
            if hit is not None:
                self._refuse(src)
            if self.eager_steps < self.warmup or not self._ready():
                return self._eager(src, rel)
            self._hit = None                             # (releases the old graph and its pool before the new capture)
            hit = self._capture(src, rel, key)
            if hit is None:
                return self._eager(src, rel)
        return self._replay(hit, src, rel)


class CapturedCandidateStep(CapturedTrainStep):
    """step = CapturedCandidateStep(model, graph, index, optimizer, num_neg, draw_seed, draw_step=0, loss='bce', lbl_smooth=0.0,
    clip=None, warmup=2, sampler=None, run_split=None); loss = step(src, rel).

    CapturedTrainStep for the sampled-negative step: one step of harness.train_sampled_negatives(draw_seed=...) --
    zero_grad, harness.draw_candidates(..., labels=True), MGCN.forward_loss_candidates(labels=..., loss=...), backward,
    ClipAdam.clip_and_step -- with everything the parent says about warm-up, other batch sizes, re-captures, counters and the
    fall-back to eager. `draw_seed` and `draw_step` are plain int attributes: every call, eager or replayed, draws the lists of
    (draw_seed, draw_step) and then adds one to draw_step; both may be set at any time (a run resumes from a checkpoint's
    draw_seed and step count) and act on the next call without a new capture. Eager calls pass the list key by value. The
    captured draw (mgcn_cand_draw_dev) reads a second device word, dropout_step_key(draw_seed, draw_step), which the wrapper
    writes next to the dropout step word and the Adam pairs in the same pinned image: a replay still costs ONE host-to-device copy
    of scalars. `num_neg`, `loss` and `run_split` (forward_loss_candidates', None or an int in [16, 65536]) are plain attributes
    held by value in the graph: changing one re-captures. `cand` and `labels` are the
    [B, 1 + num_neg] int64 / uint8 blocks of the last call (after a replay: the graph's static tensors, overwritten by the next replay).

    Raises NativeError, before anything is captured, for what the parent refuses (but the scoring stage takes any batch >= 1),
    for num_neg < 0, a loss other than 'bce' / 'softmax', a run_split that forward_loss_candidates refuses and an index that is not
    on the model's device."""

    _WORDS = 2     # the dropout step word, then the draw word

    def __init__(self, model, graph, index, optimizer, num_neg, draw_seed, draw_step=0, loss='bce', lbl_smooth=0.0, clip=None, warmup=2,
                 sampler=None, run_split=None):
        super().__init__(model, graph, index, optimizer, lbl_smooth=lbl_smooth, clip=clip, warmup=warmup)
        self.num_neg, self.draw_seed, self.draw_step, self.loss = num_neg, int(draw_seed), int(draw_step), loss
        self.sampler, self.run_split = sampler, run_split
        self.cand = self.labels = None

    def _body(self, src, rel):
        from .harness import draw_candidates
        m, opt = self.model, self.optimizer
        # while the parent captures, the model holds the dropout step word: the draw then reads ITS word, the one next to it
        word = self._stage.words[1:2] if m._step_key_dev is not None else None
        opt.zero_grad(set_to_none=True)
        cand, labels = draw_candidates(torch.stack((src.reshape(-1), rel.reshape(-1)), 1), self.index, m.entity_embedding.size(0), self.num_neg,
                                       self.draw_seed, self.draw_step, labels=True, step_key_dev=word, sampler=self.sampler)
        self.draw_step += 1
        logq = self.sampler.logq if self.sampler is not None and self.loss == 'softmax' else None
        loss = m.forward_loss_candidates(src, rel, cand, self.graph, labels=labels, lbl_smooth=self.lbl_smooth, loss=self.loss, logq=logq,
                                         run_split=self.run_split)
        loss.backward()
        opt.clip_and_step(self.clip)
        self.cand, self.labels = cand, labels
        return loss.detach()

    def _refuse(self, src):
        super()._refuse(src)
        try:
            bad = operator.index(self.num_neg) < 0
        except TypeError:
            bad = True
        if bad:
            raise _native.NativeError('CapturedCandidateStep: num_neg must be an int >= 0, got %r' % (self.num_neg,))
        if self.loss not in ('bce', 'softmax'):
            raise _native.NativeError("CapturedCandidateStep: loss must be 'bce' or 'softmax', got %r" % (self.loss,))
        _native.check_run_split('CapturedCandidateStep', self.run_split)
        dev = self.model.entity_embedding.device
        if any(t.device != dev for t in (self.index.keys, self.index.ptr, self.index.tails)):
            raise _native.NativeError('CapturedCandidateStep: the index is not on the model\'s device (%s)' % (dev,))
        sm = self.sampler
        if sm is not None and (sm.device != dev or sm.num_entities != self.model.entity_embedding.size(0)):
            raise _native.NativeError('CapturedCandidateStep: the sampler must hold the model\'s %d entities on its device (%s)'
                                      % (self.model.entity_embedding.size(0), dev))

    def _refuse_batch(self, src):
        if int(src.numel()) == 0:
            raise _native.NativeError('CapturedCandidateStep: an empty batch')

    def _key(self):
        ix = self.index       # (the parent's key holds the index tensors' addresses too: here the draw reads them as well)
        sm = self.sampler     # (its tensors are persistent: their addresses are what the graph holds)
        return super()._key() + (self.num_neg, self.loss, self.run_split, ix.keys.data_ptr(), ix.ptr.data_ptr(), ix.tails.data_ptr()) + \
            (() if sm is None else (sm.table.data_ptr(), sm.logq.data_ptr()))

    def _stage_words(self, slot):
        slot.word[1] = _native.dropout_step_key(self.draw_seed, self.draw_step)

    def _warm_kernels(self, st):
        if not self._warmed:                           # the _dev draw, once, on scratch tensors (see the parent's)
            one = torch.zeros(1, dtype=torch.int64, device=st.device)
            for labels in (True, False):
                _native.cand_draw(one, one, torch.zeros(2, dtype=torch.int64, device=st.device), torch.zeros(1, dtype=torch.int32, device=st.device),
                                  1, 2, _native.DeviceKey(st.words[1:2], _native.CAND_DRAW_SITE), labels=labels)
                _native.cand_draw(one, one, torch.zeros(2, dtype=torch.int64, device=st.device), torch.zeros(1, dtype=torch.int32, device=st.device),
                                  1, 2, _native.DeviceKey(st.words[1:2], _native.CAND_DRAW_SITE), labels=labels, table=one)
        super()._warm_kernels(st)

    def _capture(self, src, rel, key):
        saved = self.draw_step                         # capturing runs _body's Python, not its launches
        try:
            hit = super()._capture(src, rel, key)
        finally:
            self.draw_step = saved
        if hit is not None:
            hit.cand, hit.labels = self.cand, self.labels      # the graph's static list and label blocks
        return hit

    def _replay(self, hit, src, rel):
        loss = super()._replay(hit, src, rel)          # (its _upload staged the word of draw_step)
        self.draw_step += 1
        self.cand, self.labels = hit.cand, hit.labels
        return loss
