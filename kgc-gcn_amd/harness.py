"""The callers of the hot path: one training epoch, filtered-rank prediction and evaluation — what
main.py:49-135 does, against the same model / loader surface, so the two are interchangeable.

`predict` has two forms of the same computation:
  * fused=True  (default): model.rank_counts — the HIP score+filter+count kernel, no [B, N] score
    matrix, rank = 1 + gt + ties_lower (stable tie rule);
  * fused=False: the reference's sequence on torch GPU ops over model(...)'s scores (main.py:121-126),
    double argsort included — kept for A/B timing and as the literal drop-in behaviour.
Both agree exactly on rows without ties.
"""
import logging

import numpy as np
import torch
import torch.nn as nn

from .utils import RunningAverage


def train(model, data_iter, graph, optimizer, params):
    """One epoch (main.py:49-77). Returns the running loss."""
    model.train()
    loss_avg = RunningAverage()
    for triplets, labels in data_iter:
        optimizer.zero_grad()
        triplets = triplets.to(params.device)
        pred = model(triplets[:, 0], triplets[:, 1], graph)
        loss = model.loss(pred, labels.to(params.device))
        loss.backward()
        if hasattr(optimizer, 'clip_and_step'):          # optim.ClipAdam: norm, clipping and update on the HIP kernels
            optimizer.clip_and_step(params.clip_grad)
        else:
            nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=params.clip_grad)
            optimizer.step()
        loss_avg.update(loss.item())
    return loss_avg()


def train_device_labels(model, queries, index, graph, optimizer, params, batch_size, generator=None, fused_loss=True, captured=None,
                        loss='bce'):
    """One epoch like `train`, but the label rows never exist on the host: `queries` [Q, 2] int64
    (DataLoader.train_queries()), `index` = DataLoader.train_index() on the device; per step only B keys are indexed
    and mgcn_label_rows writes the smoothed [B, N] targets next to the scores. Shuffles like the reference's loader
    (data_loader.py:190) with `generator`. Same loss / clipping / optimizer calls as main.py:56-70.
    `captured`: a captured.CapturedTrainStep built for this model, graph, index and optimizer (or True: one is built with
    params.lbl_smooth / params.clip_grad and kept on the model for the following epochs). Every step is then one call of it (a
    replay of the captured step once it is warm), the per-step losses stay on the device, and the epoch reads them ONCE at its
    end into the same RunningAverage; needs fused_loss=True. None (the default): the loop below, unchanged.
    `loss`: 'bce' (the above) or 'softmax', MGCN.forward_loss's; 'softmax' needs fused_loss=True (there is no
    label-row form of it). captured=True builds its step with this `loss`; a step handed in keeps its own."""
    from . import _native
    from .model import refuse_table_loss
    refuse_table_loss('train_device_labels', loss)
    if loss == 'softmax' and not fused_loss:
        raise _native.NativeError("train_device_labels: loss='softmax' is the fused_loss=True step")
    model.train()
    loss_avg = RunningAverage()
    dev = params.device
    queries = queries.to(dev)
    order = torch.randperm(queries.size(0), generator=generator).to(dev)
    n_ent = model.entity_embedding.size(0)
    if captured is not None and captured is not False:
        if not fused_loss:
            raise _native.NativeError('train_device_labels: a captured step is the fused_loss=True step')
        step = captured
        if captured is True:
            step = _captured_step(model, graph, index, optimizer, params)
            step.loss = loss
        starts = range(0, queries.size(0), batch_size)
        losses = torch.empty(len(starts), dtype=torch.float32, device=dev)
        for k, i in enumerate(starts):
            q = queries.index_select(0, order[i:i + batch_size])
            losses[k].copy_(step(q[:, 0], q[:, 1]))     # (the step's loss tensor is overwritten by the next call)
        for v in losses.tolist():                        # the epoch's one host read
            loss_avg.update(v)
        return loss_avg()
    for i in range(0, queries.size(0), batch_size):
        q = queries.index_select(0, order[i:i + batch_size])
        optimizer.zero_grad()
        if fused_loss:                                   # scores, targets and loss in one launch
            if loss == 'bce':
                step_loss = model.forward_loss(q[:, 0], q[:, 1], graph, index, lbl_smooth=params.lbl_smooth)
            else:
                step_loss = model.forward_loss(q[:, 0], q[:, 1], graph, index, lbl_smooth=params.lbl_smooth, loss=loss)
        else:
            labels = _native.label_rows(index.query_keys(q[:, 0], q[:, 1]), index.keys, index.ptr, index.tails, n_ent,
                                        lbl_smooth=params.lbl_smooth)
            step_loss = model.loss(model(q[:, 0], q[:, 1], graph), labels)
        step_loss.backward()
        if hasattr(optimizer, 'clip_and_step'):          # optim.ClipAdam: norm, clipping and update on the HIP kernels
            optimizer.clip_and_step(params.clip_grad)
        else:
            nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=params.clip_grad)
            optimizer.step()
        loss_avg.update(step_loss.item())
    return loss_avg()


def sample_candidates(q, index, num_entities, num_neg, generator=None, check=True):
    """Candidate lists [B, 1 + num_neg] int64 for the queries q [B, >= 2] (src, rel): column 0 is ONE known tail of the query drawn
    uniformly from its run in `index` (a dist.FilterIndex on q's device; every query must have a key in it, as every training
    query has in DataLoader.train_index()), the other columns are uniform ids in [0, num_entities). A negative that happens to be
    a known tail is simply labelled hot by cand_labels. Integer torch ops on q's device (CPU tensors work); `generator` must live
    on that device. check=False skips the test that every query has a key (two reads back from the device): for callers that
    have made it for all their queries already, as train_sampled_negatives does once per epoch."""
    B, dev = q.size(0), q.device
    keys = index.query_keys(q[:, 0], q[:, 1])
    at = torch.searchsorted(index.keys, keys)
    if check and B:
        nk = index.keys.numel()
        if nk == 0 or bool((at >= nk).any()) or not torch.equal(index.keys[at.clamp(max=nk - 1)], keys):
            raise ValueError('sample_candidates: a query has no known tail in the index')
    lo, hi = index.ptr[at], index.ptr[at + 1]
    pick = lo + (torch.rand(B, generator=generator, device=dev, dtype=torch.float64) * (hi - lo).double()).long().clamp(max=hi - lo - 1)
    cand = torch.empty((B, 1 + int(num_neg)), dtype=torch.int64, device=dev)
    cand[:, 0] = index.tails[pick].long()
    if num_neg:
        cand[:, 1:] = torch.randint(0, int(num_entities), (B, int(num_neg)), generator=generator, device=dev, dtype=torch.int64)
    return cand


def draw_candidates(q, index, num_entities, num_neg, seed, step, labels=False, step_key_dev=None, sampler=None):
    """sample_candidates without a generator: the lists [B, 1 + num_neg] int64 of the queries q [B, >= 2] on the GPU
    are a pure function of (seed, step, batch row, list position) and of `index`, drawn by one HIP launch
    (_native.cand_draw under the key of (seed, step, CAND_DRAW_SITE)): every rank of a sharded step that passes the same q, seed
    and step holds the same block without an exchange, and a run resumes its stream from (seed, step count). Column 0 is one
    known tail of the query, or -1 for a query without one (a dead position: it contributes nothing and counts in the mean's
    divisor; no host read checks it); the other columns are uniform ids in [0, num_entities). labels=True: returns
    (cand, label [B, 1 + num_neg] uint8), the labels _native.cand_labels gives the drawn list against the whole table, from the
    same launch: what forward_loss_candidates(labels=...) and dist.train_step_sharded_candidates(labels=...) take.
    step_key_dev: a one-element int64 tensor on q's device that holds _native.dropout_step_key(seed, step) when the launch RUNS
    (captured.CapturedCandidateStep's second word); `seed` and `step` are then unused.
    sampler (None: uniform negatives, unchanged): a sampling.NegativeSampler on q's device: the negatives are drawn through its
    alias table instead (mgcn_cand_draw_alias), with every promise above kept. The list BCE trains on such lists
    as they are (the word2vec convention); the softmax wants sampler.logq (forward_loss_candidates(logq=...))."""
    from . import _native
    if sampler is not None and (sampler.num_entities != int(num_entities) or sampler.device != q.device):
        raise _native.NativeError('draw_candidates: the sampler holds %d entities on %s, the draw is over %d on %s'
                                  % (sampler.num_entities, sampler.device, int(num_entities), q.device))
    key = _native.dropout_key(seed, step, _native.CAND_DRAW_SITE) if step_key_dev is None else _native.DeviceKey(step_key_dev, _native.CAND_DRAW_SITE)
    cand, label = _native.cand_draw(index.query_keys(q[:, 0], q[:, 1]).contiguous(), index.keys, index.ptr, index.tails, int(num_entities),
                                    1 + int(num_neg), key, labels=labels, table=None if sampler is None else sampler.table)
    return (cand, label) if labels else cand


def check_query_keys(queries, index):
    """ValueError unless every query [Q, >= 2] (src, rel) has a key in `index`: the once-per-epoch check of the sampled-negative
    loops on drawn lists (two reads back from the device; sample_candidates' own test, without its draw)."""
    if queries.size(0) == 0:
        return
    keys = index.query_keys(queries[:, 0], queries[:, 1])
    at = torch.searchsorted(index.keys, keys)
    nk = index.keys.numel()
    if nk == 0 or bool((at >= nk).any()) or not torch.equal(index.keys[at.clamp(max=nk - 1)], keys):
        raise ValueError('check_query_keys: a query has no known tail in the index')


def train_sampled_negatives(model, queries, index, graph, optimizer, params, batch_size, num_neg, generator=None, draw_seed=None,
                            first_step=0, loss='bce', captured=None, sampler=None, run_split=None):
    """One epoch like train_device_labels' eager loop, on sampled negatives: per step the candidate lists of
    sample_candidates (one known tail + num_neg uniform ids per query) and MGCN.forward_loss_candidates over them, so that no
    step touches a [B, N] block. `generator`: a CPU generator (or None: the default one) shuffles as train_device_labels does and
    seeds a generator on params.device that draws the epoch's lists; a generator that lives on params.device draws the lists
    itself and the shuffle takes the default CPU generator. Same clipping / optimizer calls as main.py:56-70.
    draw_seed (None: everything above, unchanged): step i of the epoch takes the lists AND their labels of
    draw_candidates(..., draw_seed, first_step + i, labels=True) instead; `generator` then only shuffles, no generator is made on
    the device, and the lists do not depend on any RNG state. A caller that trains several epochs passes the steps done so far as
    first_step (a checkpoint stores draw_seed and that count).
    loss: 'bce' or 'softmax', handed to forward_loss_candidates (the softmax cross-entropy over each list).
    captured: a captured.CapturedCandidateStep built for this model, graph, index and optimizer (or True: one is built with
    params.lbl_smooth / params.clip_grad and kept on the model for the following epochs); needs draw_seed. Every step is then one
    call of it (a replay of the captured step once it is warm), its draw_seed / num_neg / loss are set from the arguments and its
    draw_step to first_step, the per-step losses stay on the device, and the epoch reads them ONCE at its end into the same
    RunningAverage. None (the default): the loop below, unchanged.
    sampler (None: uniform negatives, unchanged): a sampling.NegativeSampler on params.device; needs draw_seed (the generator
    route stays uniform and refuses a sampler). The negatives follow its table; loss='softmax' subtracts its logq from every
    candidate's logit, loss='bce' takes the weighted lists without a correction (the word2vec convention). A
    checkpoint stores sampler.state_dict() next to draw_seed and the step count.
    run_split (None: unchanged): handed to every forward_loss_candidates, or set on the captured step."""
    kind = loss             # (`loss` below is a step's result)
    if sampler is not None and draw_seed is None:
        from . import _native
        raise _native.NativeError('train_sampled_negatives: a sampler draws through the counter-based draw: give draw_seed')
    logq = sampler.logq if sampler is not None and kind == 'softmax' else None
    if captured is not None and captured is not False and draw_seed is None:
        from . import _native
        raise _native.NativeError('train_sampled_negatives: a captured step draws its lists from (draw_seed, step): give draw_seed')
    model.train()
    loss_avg = RunningAverage()
    dev = torch.device(params.device)
    queries = queries.to(dev)
    on_cpu = generator is None or generator.device.type == 'cpu'
    order = torch.randperm(queries.size(0), generator=generator if on_cpu else None).to(dev)
    if draw_seed is None and on_cpu and dev.type != 'cpu':
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator))
        generator = torch.Generator(device=dev)
        generator.manual_seed(seed)
    n_ent = model.entity_embedding.size(0)
    if draw_seed is None:
        sample_candidates(queries, index, n_ent, 0, generator=generator)      # every query has a key: checked once, not per step
    else:
        check_query_keys(queries, index)
    if captured is not None and captured is not False:
        step = _captured_cand_step(model, graph, index, optimizer, params) if captured is True else captured
        step.num_neg, step.loss, step.draw_seed, step.draw_step = int(num_neg), kind, int(draw_seed), int(first_step)
        step.sampler, step.run_split = sampler, run_split
        starts = range(0, queries.size(0), batch_size)
        losses = torch.empty(len(starts), dtype=torch.float32, device=dev)
        for k, i in enumerate(starts):
            q = queries.index_select(0, order[i:i + batch_size])
            losses[k].copy_(step(q[:, 0], q[:, 1]))     # (the step's loss tensor is overwritten by the next call)
        for v in losses.tolist():                        # the epoch's one host read
            loss_avg.update(v)
        return loss_avg()
    for k, i in enumerate(range(0, queries.size(0), batch_size)):
        q = queries.index_select(0, order[i:i + batch_size])
        if draw_seed is None:
            cand = sample_candidates(q, index, n_ent, num_neg, generator=generator, check=False)
            optimizer.zero_grad()
            loss = model.forward_loss_candidates(q[:, 0], q[:, 1], cand, graph, index=index, lbl_smooth=params.lbl_smooth, loss=kind,
                                                 run_split=run_split)
        else:
            cand, labels = draw_candidates(q, index, n_ent, num_neg, draw_seed, int(first_step) + k, labels=True, sampler=sampler)
            optimizer.zero_grad()
            loss = model.forward_loss_candidates(q[:, 0], q[:, 1], cand, graph, labels=labels, lbl_smooth=params.lbl_smooth, loss=kind,
                                                 logq=logq, run_split=run_split)
        loss.backward()
        if hasattr(optimizer, 'clip_and_step'):          # optim.ClipAdam: norm, clipping and update on the HIP kernels
            optimizer.clip_and_step(params.clip_grad)
        else:
            nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=params.clip_grad)
            optimizer.step()
        loss_avg.update(loss.item())
    return loss_avg()


def _captured_step(model, graph, index, optimizer, params):
    """The CapturedTrainStep of train_device_labels(captured=True): built once per (graph, index, optimizer) and kept on the model."""
    from .captured import CapturedTrainStep
    hit = getattr(model, '_captured_train_step', None)
    if hit is None or hit.graph is not graph or hit.index is not index or hit.optimizer is not optimizer:
        hit = CapturedTrainStep(model, graph, index, optimizer)
        object.__setattr__(model, '_captured_train_step', hit)
    hit.lbl_smooth, hit.clip = float(params.lbl_smooth), params.clip_grad
    return hit


def _captured_cand_step(model, graph, index, optimizer, params):
    """The CapturedCandidateStep of train_sampled_negatives(captured=True): built once per (graph, index, optimizer) and kept on
    the model; the epoch sets its num_neg, loss, draw_seed and draw_step."""
    from .captured import CapturedCandidateStep
    hit = getattr(model, '_captured_cand_train_step', None)
    if hit is None or hit.graph is not graph or hit.index is not index or hit.optimizer is not optimizer:
        hit = CapturedCandidateStep(model, graph, index, optimizer, 0, 0)
        object.__setattr__(model, '_captured_cand_train_step', hit)
    hit.lbl_smooth, hit.clip = float(params.lbl_smooth), params.clip_grad
    return hit


def ranks_from_scores(pred, label, obj):
    """main.py:122-126 on a materialised score block."""
    rows = torch.arange(pred.size(0), device=pred.device)
    target = pred[rows, obj]
    pred = torch.where(label.to(torch.uint8).bool(), torch.full_like(pred, -10000000.0), pred)
    pred[rows, obj] = target
    order = torch.argsort(torch.argsort(pred, dim=1, descending=True), dim=1, descending=False)
    return 1 + order[rows, obj]


def _accumulate(results, ranks):
    ranks = ranks.float()
    results['count'] = torch.numel(ranks) + results.get('count', 0.0)
    results['mr'] = torch.sum(ranks).item() + results.get('mr', 0.0)
    results['mrr'] = torch.sum(1.0 / ranks).item() + results.get('mrr', 0.0)
    hits = (ranks.view(-1, 1) <= torch.arange(1, 11, device=ranks.device, dtype=ranks.dtype)).sum(0).tolist()
    for k in range(10):
        results['hits@{}'.format(k + 1)] = hits[k] + results.get('hits@{}'.format(k + 1), 0.0)
    return results


def predict(model, data_iters, graph, data_type, device, mode='tail_batch', fused=True):
    """main.py:105-135: sums of rank, 1/rank and hits@1..10 over one side of a split."""
    model.eval()
    results = {}
    with torch.no_grad():
        for triplets, label in data_iters['{}_{}'.format(data_type, mode.split('_')[0])]:
            triplets, label = triplets.to(device), label.to(device)
            sub, rel, obj = triplets[:, 0], triplets[:, 1], triplets[:, 2]
            if fused:
                counts, _ = model.rank_counts(sub, rel, obj.contiguous(), label, graph)
                ranks = 1 + counts[:, 0] + counts[:, 1]
            else:
                ranks = ranks_from_scores(model(sub, rel, graph), label, obj)
            _accumulate(results, ranks)
    return results


def evaluate(model, data_iters, graph, params, data_type, mark='Val', hits=(1, 3, 10), fused=True):
    """main.py:80-102: tail + head sides averaged, rounded to 5 decimals."""
    tail = predict(model, data_iters, graph, data_type, params.device, mode='tail_batch', fused=fused)
    head = predict(model, data_iters, graph, data_type, params.device, mode='head_batch', fused=fused)
    count = float(tail['count'])
    results = {'mr': np.round((tail['mr'] + head['mr']) / (2 * count), 5),
               'mrr': np.round((tail['mrr'] + head['mrr']) / (2 * count), 5)}
    for k in hits:
        results['hits@{}'.format(k)] = np.round((tail['hits@{}'.format(k)] + head['hits@{}'.format(k)]) / (2 * count), 5)
    logging.info('- {} metrics: {}  '.format(mark, '; '.join('{}: {:05.3f}'.format(k, v) for k, v in results.items())))
    return results


def evaluate_candidates(model, queries, cand, graph, batch_size, hits=(1, 3, 10)):
    """Evaluation against per-query candidate lists (sampled negatives: the usual protocol once the table is too large to
    rank against whole): queries [Q, 3] int64 rows (src, rel, obj) and cand [Q, K] int64, both on the device. The rank of
    a query is 1 + gt + ties_lower of model.rank_candidates over its list (the target itself, padding and ids outside the
    table are never counted). Returns evaluate's keys for this one side: mr, mrr and hits@k over the Q queries, rounded to
    5 decimals."""
    results = {}
    for i in range(0, queries.size(0), int(batch_size)):
        q, c = queries[i:i + batch_size], cand[i:i + batch_size]
        counts, _ = model.rank_candidates(q[:, 0].contiguous(), q[:, 1].contiguous(), q[:, 2].contiguous(), c, graph)
        _accumulate(results, 1 + counts[:, 0] + counts[:, 1])
    count = float(results.get('count', 0.0))
    out = {'mr': np.round(results.get('mr', 0.0) / max(count, 1.0), 5), 'mrr': np.round(results.get('mrr', 0.0) / max(count, 1.0), 5)}
    for k in hits:
        out['hits@{}'.format(k)] = np.round(results.get('hits@{}'.format(k), 0.0) / max(count, 1.0), 5)
    return out
