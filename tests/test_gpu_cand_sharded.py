"""The sharded training step on candidate lists (dist.train_step_sharded_candidates) on a real MI355X: one
rank against the one-GPU forward_loss_candidates step bit for bit, one process playing three ranks on the scoring stage, two
processes over gloo (both on one GPU) that draw their own lists, the epoch against harness.train_sampled_negatives(draw_seed=...),
and the refusals."""
import os

import numpy as np
import pytest
import torch

from . import cand_train_ref as C
from . import dense_ref as R
from .test_gpu_train_sharded import _PORTS, _assemble, _batches, _loader, _models, _np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NEG, SEED = 8, 77          # K = 9


def _lists(pkg, q, idx, n_ent, step):
    return pkg.harness.draw_candidates(q, idx, n_ent, NEG, SEED, step, labels=True)


def _same_state(ref, sm, layers, shard):
    sd_r, sd_s = ref.state_dict(), sm.state_dict()
    names = {'edge_embeddings'} | {'edge_embeddings_extra.%d' % i for i in range(layers - 1)}
    for k, v in sd_r.items():
        if k in names and shard:                                 # the shard model's state holds slot order
            v = v.index_select(0, ref._slot_csr.perm)
        assert torch.equal(sd_s[k], v), k


@pytest.mark.parametrize('case,layers,shard', [('syn_b', 1, False), ('syn_a', 2, True)])
def test_world1_equals_one_gpu_step(pkg, case, layers, shard):
    """train_step_sharded_candidates with one rank and forward_loss_candidates + backward + clip_grad_norm_(0.5) + Adam, 3 steps
    each from the same state on drawn lists (K = 9, lbl_smooth 0.1, dropout 0): every loss, parameter and BN statistic is
    bit-identical. The labels come from the draw in one step and from the index in the others."""
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    try:
        ref, dl, params = _models(pkg, case, layers)
        sm, dl_s, _ = _models(pkg, case, layers, shard=shard)
        idx = dl.train_index().to(DEV)
        opt_r, opt_s = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.optim.Adam(sm.parameters(), lr=1e-3)
        for step, q in enumerate(_batches(dl, 3)):
            cand, labels = _lists(pkg, q, idx, dl.num_entity, step)
            assert tuple(cand.shape) == (q.size(0), 1 + NEG) and bool((cand[:, 0] >= 0).all())
            opt_r.zero_grad()
            loss_r = ref.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, index=idx, lbl_smooth=0.1)
            loss_r.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
            opt_r.step()
            loss_s = pkg.dist.train_step_sharded_candidates(sm, dl_s.graph, q[:, 0], q[:, 1], cand, idx, opt_s,
                                                            labels=labels if step == 1 else None, lbl_smooth=0.1, clip=0.5)
            assert torch.equal(loss_s, loss_r.detach()) and bool(torch.isfinite(loss_s))
    finally:
        torch.use_deterministic_algorithms(False)
    _same_state(ref, sm, layers, shard)


def test_world1_equals_one_gpu_step_at_counter_dropout(pkg, monkeypatch):
    """The same at dropout 0.3 with the counter-based dropout, the HIP trunk and query-path switches on and ClipAdam: with one
    rank the masks are the one-GPU step's, so the bits still agree."""
    monkeypatch.setenv('MGCN_DROPOUT', 'counter')
    monkeypatch.setenv('MGCN_TRUNK_TRAIN', 'hip')
    monkeypatch.setenv('MGCN_QUERY_TRAIN', 'hip')
    case, layers, shard = 'syn_a', 2, True
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        ref, dl, params = _models(pkg, case, layers, dropout=0.3)
        sm, dl_s, _ = _models(pkg, case, layers, dropout=0.3, shard=shard)
        for m in (ref, sm):
            for layer in [m.conv1] + list(m.conv1_extra):
                layer.drop.p = 0.3
        idx = dl.train_index().to(DEV)
        opt_r, opt_s = pkg.optim.ClipAdam(ref.parameters(), lr=1e-3), pkg.optim.ClipAdam(sm.parameters(), lr=1e-3)
        ref.train()
        for step, q in enumerate(_batches(dl, 3)):
            cand, labels = _lists(pkg, q, idx, dl.num_entity, step)
            opt_r.zero_grad()
            loss_r = ref.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, labels=labels, lbl_smooth=0.1)
            loss_r.backward()
            opt_r.clip_and_step(0.5)
            loss_s = pkg.dist.train_step_sharded_candidates(sm, dl_s.graph, q[:, 0], q[:, 1], cand, idx, opt_s, labels=labels,
                                                            lbl_smooth=0.1, clip=0.5)
            assert torch.equal(loss_s, loss_r.detach())
    finally:
        torch.use_deterministic_algorithms(False)
    assert ref.dropout_state() == sm.dropout_state() == {'dropout_seed': 0, 'dropout_step': 3}
    _same_state(ref, sm, layers, shard)


# -- one process playing three ranks on the scoring stage ----------------------------------------------------------------
def _score(pkg, x, ent, bias, cand, label, hot, cold, n0, n1):
    """(loss, g, dx, d_ent, d_bias) of _CandBCEFn on rows [n0, n1)."""
    xs = x.clone().requires_grad_(True)
    es, bs = ent[n0:n1].clone().requires_grad_(True), bias[n0:n1].clone().requires_grad_(True)
    loss = pkg.model._CandBCEFn.apply(xs, es, bs, cand, label, hot, cold, n0)
    g = loss.grad_fn.saved_tensors[3]
    loss.backward()
    return loss.detach(), g, xs.grad, es.grad, bs.grad


@pytest.mark.parametrize('dim', [36, 200])
def test_three_ranks_of_the_scoring_stage(pkg, dim):
    """Bounds [0, a, a, N] (an empty middle shard, a no multiple of 16), B = 5, K = 65; every query names row 7 and row a, one
    position is -1. g_r has the one-rank g's bits where r owns the id and 0 elsewhere; d_ent_r / d_bias_r are rows [n0, n1) of
    the one-rank gradients bit for bit; the ranks' losses and dx add up to the float64 reference within
    gamma(K + W) sum |addends| (the bound of tests/test_cand_train_ref_host.py for K addends, with the W additions of the
    reduction).
    The inputs are scaled so that the largest |logit| is 4. That bound counts roundings of a SUM; it has no room for the error
    of an f32 loss term itself, which grows with the logit (log1p(-p) of an f32 p near 1: dense_ref.bce_loss_bar). With the
    unscaled +-1 inputs the logits reach 18 at dim = 200, and torch's own CPU f32 BCE of the same logits misses the float64
    loss by 25.5 x this bound -- the very figure the one-rank launch and the three ranks' sum miss it by (0.000189 against
    7.41e-06), so it says nothing about the partition; at |logit| <= 4 the same CPU f32 BCE is within 0.004 x the bound."""
    nat = pkg._native
    B, K, N, a, W = 5, 65, 50, 21, 3
    gen = R.gen(R.seed_of(51, dim))
    x, ent, bias = R.pm_uniform((B, dim), gen), R.pm_uniform((N, dim), gen), R.pm_uniform((N,), gen)
    s = (4.0 / float(R.ref_logits(x, ent, bias)[0].abs().max())) ** 0.5
    x, ent, bias = x * s, ent * s, bias * (s * s)
    cand = C.lists(N, B, K, R.seed_of(52, dim))
    cand[:, 1], cand[:, 2], cand[0, 5] = 7, a, -1
    label = torch.rand((B, K), generator=gen) < 0.3
    hot, cold = nat.smoothed_targets(0.1, N)
    dx_, dent_, dbias_ = (t.to(DEV) for t in (x, ent, bias))
    dcand, dlabel = cand.to(DEV), label.to(DEV)
    loss1, g1, dx1, de1, db1 = _score(pkg, dx_, dent_, dbias_, dcand, dlabel, hot, cold, 0, N)
    plain = nat.cand_bce_fwd(dx_, dent_, dbias_, dcand, dlabel, hot, cold)
    assert torch.equal(g1, plain[1]) and torch.equal(loss1, plain[0])          # one rank: model._CandBCEFn's launch
    bounds = [0, a, a, N]
    loss_sum, dx_sum = torch.zeros((), device=DEV), torch.zeros_like(dx1)
    seen = torch.zeros((B, K), dtype=torch.int64)
    for r in range(W):
        n0, n1 = bounds[r], bounds[r + 1]
        live, _ = C.live_rows(cand, n0, n1 - n0)
        seen += live.long()
        if n1 == n0:                                   # the step scores nothing on an empty shard: (xt * 0).sum()
            assert not bool(live.any())
            continue
        loss_r, g_r, dx_r, de_r, db_r = _score(pkg, dx_, dent_, dbias_, dcand, dlabel, hot, cold, n0, n1)
        assert torch.equal(g_r, torch.where(live.to(DEV), g1, torch.zeros_like(g1))), r
        assert torch.equal(de_r, de1[n0:n1]) and torch.equal(db_r, db1[n0:n1]), r
        loss_sum, dx_sum = loss_sum + loss_r, dx_sum + dx_r
    whole, _ = C.live_rows(cand, 0, N)
    assert torch.equal(seen, whole.long()) and int((~whole).sum()) == 1          # every live position on exactly one rank
    inv = 1.0 / (B * K)
    ref = C.ref_list_bce(x, ent, bias, cand, label, hot, cold, inv)
    p, y, lv = ref['p'], ref['y'], ref['live']
    terms = torch.where(lv, (y - 1.0) * torch.log1p(-p) - y * torch.log(p), torch.zeros_like(p))      # dense_ref.ref_bce's terms
    assert abs(float(terms.sum()) * inv - ref['loss']) <= 1e-9 * abs(ref['loss'])      # the addends are the reference's own
    bar = C.gamma(K + W) * float(terms.abs().sum()) * inv
    err = abs(float(loss_sum.double()) - ref['loss'])
    print('RATIO shard_loss dim=%d %.4f' % (dim, err / bar))
    assert err <= bar, (err, bar)
    rows = ent.double()[ref['row']]
    mag = (ref['g'].abs()[:, :, None] * rows.abs()).sum(1)
    ratio = float(((dx_sum.cpu().double() - ref['dx']).abs() / (C.gamma(K + W) * mag)).max())
    print('RATIO shard_dx dim=%d %.4f' % (dim, ratio))
    assert ratio <= 1.0, ratio


# -- two processes on one GPU over gloo -------------------------------------------------------------------------------
JOBS = [('one_layer', 'syn_b', 1), ('two_layer', 'syn_b', 2)]


def _gloo_worker(rank, world, port, q):
    try:
        _gloo_worker_body(rank, world, port, q)
    except Exception:                                        # surface the failure in the parent instead of a timeout
        import traceback
        q.put((rank, {'error': traceback.format_exc()}))


def _gloo_worker_body(rank, world, port, q):
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    pkg = importlib.import_module('kgc-gcn_amd')
    out = {}
    whole, dl, _ = _models(pkg, 'syn_b')
    q0 = _batches(dl, 1)[0]
    idx = dl.train_index().to(DEV)
    c0 = pkg.harness.draw_candidates(q0, idx, dl.num_entity, NEG, SEED, 0)
    try:                                                     # whole tables at two ranks: refused before any collective
        pkg.dist.train_step_sharded_candidates(whole, dl.graph, q0[:, 0], q0[:, 1], c0, idx, torch.optim.Adam(whole.parameters()))
        out['whole_table_refused'] = False
    except pkg._native.NativeError as err:
        out['whole_table_refused'] = 'whole per-edge tables' in str(err)
    for step, (name, case, layers) in enumerate(JOBS):
        sm, dl, params = _models(pkg, case, layers, 0.0, shard=True, world=world, rank=rank)
        idx = dl.train_index().to(DEV)
        opt = torch.optim.Adam(sm.parameters(), lr=1e-3)
        b = _batches(dl, 1)[0]
        cand, labels = pkg.harness.draw_candidates(b, idx, dl.num_entity, NEG, SEED, step, labels=True)     # this rank's own draw
        loss = float(pkg.dist.train_step_sharded_candidates(sm, dl.graph, b[:, 0], b[:, 1], cand, idx, opt, labels=labels))
        csr, n0, n1 = sm._edge_shard
        counts, sub = csr.shard_slot_counts(n0, n1), csr.shard_ee_sub(n0, n1)
        slots = (torch.arange(sum(counts)) + torch.tensor(sub).repeat_interleave(torch.tensor(counts))).to(DEV)
        tables = {n: p for n, p in sm._edge_tables()}
        out[name] = dict(losses=[loss], cand=_np(cand), labels=_np(labels), rows=(n0, n1), ref_ids=_np(csr.perm.index_select(0, slots)),
                         grads={n: _np(p.grad) for n, p in sm.named_parameters() if p.grad is not None},
                         state={k: _np(v) for k, v in sm.state_dict().items() if k not in tables},
                         tables={n: _np(t) for n, t in tables.items()})
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_draw_the_same_lists_and_match_the_single_step(pkg):
    """Two processes over gloo, one step each of the 1-layer and the 2-layer syn_b, dropout 0: each rank draws its own lists from
    (seed, step) and both hold the parent's block; the loss is the one-process forward_loss_candidates step's to 1e-5, every
    gradient matches it with test_two_ranks_one_gpu_match_golden_and_single_step's tolerances (the table gradient reassembled
    from both shards), replicated gradients and state are bit-identical on the two ranks, the table rows after the step match
    to 1e-5, and a whole-table model is refused before any collective."""
    import torch.multiprocessing as mp
    _PORTS[0] += 1
    world, port = 2, 31700 + (os.getpid() * 7 + 50 * _PORTS[0]) % 2000
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, queue)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(queue.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        assert 'error' not in got[r], got[r]['error']
    assert got[0]['whole_table_refused'] and got[1]['whole_table_refused']
    for step, (name, case, layers) in enumerate(JOBS):
        ref, dl, params = _models(pkg, case, layers)
        idx = dl.train_index().to(DEV)
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
        b = _batches(dl, 1)[0]
        cand, labels = pkg.harness.draw_candidates(b, idx, dl.num_entity, NEG, SEED, step, labels=True)
        for r in (0, 1):
            assert np.array_equal(got[r][name]['cand'], _np(cand)) and np.array_equal(got[r][name]['labels'], _np(labels)), (name, r)
        n0, n1 = got[0][name]['rows']
        assert 0 < n1 < dl.num_entity and got[1][name]['rows'] == (n1, dl.num_entity)
        own = ((cand >= n0) & (cand < n1)).sum().item()
        assert 0 < own < cand.numel()                             # both ranks score some of the list
        opt.zero_grad()
        loss = ref.forward_loss_candidates(b[:, 0], b[:, 1], cand, dl.graph, labels=labels, lbl_smooth=0.0)
        loss.backward()
        want_grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}
        opt.step()
        inv = ref._slot_csr.inv_perm
        for n in want_grads:
            if n.startswith('edge_embeddings'):
                want_grads[n] = want_grads[n].index_select(0, inv)   # slot order -> reference order
        for r in (0, 1):
            assert abs(got[r][name]['losses'][0] - float(loss.detach())) < 1e-5, (name, r)
        tgrads = _assemble(got, name, 'grads')
        for n, want in want_grads.items():
            gr = tgrads[n] if n.startswith('edge_embeddings') else got[0][name]['grads'][n]
            if not n.startswith('edge_embeddings'):
                assert np.array_equal(got[0][name]['grads'][n], got[1][name]['grads'][n]), (name, n)
            ref_g = want.cpu()
            scale = float(ref_g.abs().max()) + 1e-12
            floor = 2e-6 if n.startswith('conv2.') else 1e-9
            np.testing.assert_allclose(gr, ref_g.numpy(), rtol=2e-3, atol=2e-5 * scale + floor, err_msg='%s %s' % (name, n))
        for k, v in got[0][name]['state'].items():           # replicated state: the same bits on both ranks
            assert np.array_equal(v, got[1][name]['state'][k]), (name, k)
        ref_sd = ref.state_dict()
        for tname, t in _assemble(got, name, 'tables').items():
            np.testing.assert_allclose(t, ref_sd[tname].cpu().numpy(), rtol=0, atol=1e-5, err_msg=tname)


# -- the epoch ---------------------------------------------------------------------------------------------------------
def test_world1_epoch_equals_harness_epoch_and_repeats(pkg):
    """One train_epoch_sharded_candidates at one rank and one harness.train_sampled_negatives(draw_seed=...) with identically
    seeded shuffles (dropout 0): the same mean loss and bit-identical parameters; a second run from the same seeds gives the
    same bits again."""
    models = [_models(pkg, 'syn_b') for _ in range(3)]
    (ref, dl, params), (sm, dl_s, _), (again, dl_a, _) = models
    queries = dl.train_queries()
    Q = queries.size(0)
    bs = next(b for b in range(16, 4, -1) if Q % b and (Q % b) % 4)
    idx = dl.train_index().to(DEV)
    params.clip_grad = 0.5
    opts = [torch.optim.Adam(m.parameters(), lr=1e-3) for m, _, _ in models]
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    try:
        want = pkg.harness.train_sampled_negatives(ref, queries, idx, dl.graph, opts[0], params, bs, NEG,
                                                   generator=torch.Generator().manual_seed(4), draw_seed=SEED, first_step=10)
        got = pkg.dist.train_epoch_sharded_candidates(sm, queries, idx, dl_s.graph, opts[1], params, bs, NEG, SEED, first_step=10,
                                                      generator=torch.Generator().manual_seed(4))
        twice = pkg.dist.train_epoch_sharded_candidates(again, queries, idx, dl_a.graph, opts[2], params, bs, NEG, SEED, first_step=10,
                                                        generator=torch.Generator().manual_seed(4))
    finally:
        torch.use_deterministic_algorithms(False)
    assert got == want == twice and np.isfinite(got)
    sd_r, sd_s, sd_a = ref.state_dict(), sm.state_dict(), again.state_dict()
    for k, v in sd_r.items():
        assert torch.equal(sd_s[k], v) and torch.equal(sd_a[k], v), k
    assert not torch.equal(sd_r['entity_embedding'], golden_state(pkg)['entity_embedding'].to(DEV))      # it did train


def golden_state(pkg):
    from .conftest import golden
    return golden('syn_b').state_dict()


# -- refusals ----------------------------------------------------------------------------------------------------------
def test_candidate_step_refusals(pkg):
    nat = pkg._native
    step = pkg.dist.train_step_sharded_candidates
    model, dl, params = _models(pkg, 'syn_b')
    idx = dl.train_index().to(DEV)
    q = _batches(dl, 1)[0]
    cand, labels = _lists(pkg, q, idx, dl.num_entity, 0)
    opt = torch.optim.Adam(model.parameters())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for bad in (cand[:-1], cand.int(), cand.reshape(-1), cand.float()):
        with pytest.raises(nat.NativeError, match='candidates must be int64'):
            step(model, dl.graph, q[:, 0], q[:, 1], bad, idx, opt)
    for bad in (labels[:, :-1], labels.float(), labels.long()):
        with pytest.raises(nat.NativeError, match='labels must be uint8 / bool'):
            step(model, dl.graph, q[:, 0], q[:, 1], cand, idx, opt, labels=bad)
    csr = dl.graph.csr(model.relation_embedding.size(0) + 1)
    other, _, _ = _models(pkg, 'syn_b', shard=True)
    other._edge_shard = (csr, 0, csr.num_nodes // 2)          # the shard of another range than this rank's (0, N)
    with pytest.raises(nat.NativeError, match='destinations'):
        step(other, dl.graph, q[:, 0], q[:, 1], cand, idx, torch.optim.Adam(other.parameters()))
    dl16, p16 = _loader(pkg, 'syn_b', edge_table_dtype='bf16')
    m16 = pkg.MGCN(dl16.num_entity, dl16.num_relation, dl16.num_edge, p16).to(DEV)
    assert m16.edge_embeddings.dtype == torch.bfloat16
    with pytest.raises(nat.NativeError, match='inference-only'):
        step(m16, dl16.graph, q[:, 0], q[:, 1], cand, idx, torch.optim.Adam(m16.parameters()))
    after = model.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())              # a refused step changed nothing
    assert bool(torch.isfinite(step(model, dl.graph, q[:, 0], q[:, 1], cand, idx, opt, labels=labels.bool())))      # bool labels pass
