"""The destination-partitioned training step (dist.train_step_sharded) on a real MI355X: the shard backward and the split BN
epilogue against the whole-graph entry points, one rank against the one-GPU step bit for bit, and two ranks over gloo (both
processes on one GPU) against the reference's golden step."""
import os
import types

import numpy as np
import pytest
import torch

from .conftest import GOLDEN, golden
from .test_train_sharded_host import random_graph

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _shapes():
    out = [(c, None) for c in ('syn_a', 'syn_b', 'syn_c')]
    return out + [('wn18rr', (40943, 11, 86835, 0.0)), ('fb15k237', (14541, 237, 272115, 1.1))]


def _csr(pkg, name, spec):
    if spec is None:
        g = golden(name)
        ei, et = g.t('dl_edge_index'), g.t('dl_edge_attr')[0]
        N, R = int(g['dl_num_entity']), int(g['dl_num_relation'])
        return pkg.GraphCSR(N, 2 * R + 1, ei, et, DEV, hub_threshold=3, hub_chunk=2) if name == 'syn_b' else \
            pkg.GraphCSR(N, 2 * R + 1, ei, et, DEV)
    N, R, E, zipf = spec
    ei, et = random_graph(N, R, E, zipf=zipf, seed=3)
    return pkg.GraphCSR(N, 2 * R + 1, ei, et, DEV)


@pytest.mark.parametrize('dim', [100, 200])
@pytest.mark.parametrize('name,spec', _shapes())
def test_shard_backward_vs_full_backward(pkg, name, spec, dim):
    """Every rank's gee rows are the whole backward's rows of its slots; the partial gx / grel of the ranks add up to the whole
    backward's (1e-5 relative); with one rank everything is bit-identical to mgcn_aggregate_bwd."""
    nat = pkg._native
    csr = _csr(pkg, name, spec)
    if name == 'fb15k237':
        assert csr.num_chunks > 0                                   # Zipf tails: hub chunks in play
    N, E2, T = csr.num_nodes, 2 * csr.num_edges_half, csr.num_rel_rows
    gen = torch.Generator().manual_seed(dim)
    x = torch.randn(N, dim, generator=gen).to(DEV)
    rel = torch.randn(T, dim, generator=gen).to(DEV)
    ee = torch.randn(E2, dim, generator=gen).to(DEV)
    g = torch.randn(N, 2 * dim, generator=gen).to(DEV)
    gx, gee, grel = nat.aggregate_bwd(csr, x, rel, ee, g)
    for world in (1, 2, 3, 8):
        b = csr.balanced_bounds(world)
        sx, srel = torch.zeros_like(gx), torch.zeros_like(grel)
        for r in range(world):
            n0, n1 = b[r], b[r + 1]
            px, pee, prel = nat.aggregate_bwd_shard(csr, x, rel, csr.edge_table_shard(ee, n0, n1), g[n0:n1], (n0, n1))
            assert torch.equal(pee, csr.edge_table_shard(gee, n0, n1)), (world, r)
            if world == 1:
                assert torch.equal(px, gx) and torch.equal(prel, grel)
            sx += px
            srel += prel
        for got, want, what in ((sx, gx, 'gx'), (srel, grel, 'grel')):
            err = float((got - want).abs().max())
            assert err <= 1e-5 * float(want.abs().max()), (world, what, err)


def test_bn_split_stages_equal_unsplit(pkg):
    """Cuts at multiples of 128 on identical z: mean, rstd, running statistics, y, gz, gu, ggamma and gbeta of the split stages
    (partials exchanged in rank order) equal the unsplit epilogue's bit for bit."""
    nat = pkg._native
    gen = torch.Generator().manual_seed(5)
    N, O = 1000, 200
    u = [torch.randn(N, O, generator=gen).to(DEV) for _ in range(3)]
    bias, gamma, beta = [torch.randn(O, generator=gen).to(DEV) for _ in range(3)]
    rm0, rv0 = torch.randn(O, generator=gen).to(DEV), torch.rand(O, generator=gen).to(DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    y, z, mean, rstd = nat.bn_tanh_train_fwd(*u, bias, gamma, beta, rm, rv, 0.1, 1e-5)
    gy = torch.randn(N, O, generator=gen).to(DEV)
    gz, gu, gg, gb = nat.bn_tanh_train_bwd(z, y, gy, mean, rstd, gamma)
    cuts = [0, 256, 640, 640, N]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    st1 = [nat.bn_train_stage_sum(*[t[a:b] for t in u], bias) for a, b in pieces]
    assert torch.equal(torch.cat([s[0] for s in st1]), z)
    parts = torch.cat([s[1] for s in st1])
    st2 = [nat.bn_train_stage_center(s[0], parts, N) for s in st1]
    parts2 = torch.cat([s[1] for s in st2])
    ys = []
    for s, c in zip(st1, st2):
        assert torch.equal(c[0], mean)
        m, v = rm0.clone(), rv0.clone()
        yy, rs = nat.bn_train_stage_finish(s[0], parts2, N, c[0], gamma, beta, m, v, 0.1, 1e-5)
        assert torch.equal(rs, rstd) and torch.equal(m, rm) and torch.equal(v, rv)
        ys.append(yy)
    assert torch.equal(torch.cat(ys), y)
    bw = [nat.bn_train_bwd_stage_sums(z[a:b], y[a:b], gy[a:b], mean, rstd) for a, b in pieces]
    allp = torch.cat(bw, dim=1)
    outs = [nat.bn_train_bwd_stage_apply(z[a:b], y[a:b], gy[a:b], mean, rstd, gamma, allp[0], allp[1], N) for a, b in pieces]
    assert torch.equal(torch.cat([o[0] for o in outs]), gz) and torch.equal(torch.cat([o[1] for o in outs]), gu)
    for o in outs:
        assert torch.equal(o[2], gg) and torch.equal(o[3], gb)


def _loader(pkg, case, **over):
    g = golden(case)
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**dict(g.hp, **over))
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    dl.graph.to(DEV)
    return dl, params


def _models(pkg, case, layers=1, dropout=0.0, shard=None, world=1, rank=0):
    """(whole-table model from the golden state, its data loader, params). With `shard`, a second model built with
    params.edge_table_rows and filled by dist.shard_model_tables for this rank's balanced range is returned instead."""
    over = dict(gcn_drop=dropout, hidden_drop=dropout, feat_drop=dropout, gcn_layers=layers)
    dl, params = _loader(pkg, case, **over)
    torch.manual_seed(0)                                   # extra layers: the same initial values in every process
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    missing = model.load_state_dict(golden(case).state_dict(), strict=False)
    assert not missing.unexpected_keys
    for layer in [model.conv1] + list(model.conv1_extra):
        layer.drop.p = dropout / 3
    model.to(DEV)
    if not shard:
        return model, dl, params
    csr = dl.graph.csr(model.relation_embedding.size(0) + 1)
    b = csr.balanced_bounds(world)
    ref = model.state_dict()
    names = ['edge_embeddings'] + ['edge_embeddings_extra.%d' % i for i in range(layers - 1)]
    sparams = types.SimpleNamespace(**vars(params))
    sparams.edge_table_rows = sum(csr.shard_slot_counts(b[rank], b[rank + 1]))
    torch.manual_seed(0)
    sm = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, sparams)
    sm.load_state_dict({k: v for k, v in ref.items() if k not in names}, strict=False)
    for layer in [sm.conv1] + list(sm.conv1_extra):
        layer.drop.p = dropout / 3
    sm.to(DEV)
    pkg.dist.shard_model_tables(sm, csr, b[rank], b[rank + 1], lambda li, ids: ref[names[li]].to(DEV).index_select(0, ids))
    return sm, dl, params


def _batches(dl, steps, B=8):
    q = dl.train_queries()
    g = torch.Generator().manual_seed(1)
    return [q[torch.randperm(q.size(0), generator=g)[:B]].to(DEV) for _ in range(steps)]


def _job_batches(name, case, dl, steps):
    """The golden step's own batch for the golden job (its loss and gradients are pinned), batches of 6 for the unfused scorer
    (B % 4 != 0), random batches of 8 otherwise."""
    if name == 'syn_b':
        return [golden(case).t('train_triple')[:, :2].to(DEV)]
    return _batches(dl, steps, B=6 if name == 'odd_batch' else 8)


@pytest.mark.parametrize('case,layers,shard', [('syn_b', 1, False), ('syn_b', 1, True), ('syn_a', 2, True), ('syn_c', 1, False)])
def test_world1_equals_one_gpu_step(pkg, case, layers, shard):
    """train_step_sharded with one rank and forward_loss + backward + clip_grad_norm_ + Adam, 3 steps each from the same state
    (dropout 0): every parameter and BN statistic is bit-identical afterwards, and so are the losses."""
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    try:
        ref, dl, params = _models(pkg, case, layers)
        sm, dl_s, _ = _models(pkg, case, layers, shard=shard)       # (its own loader: the shard belongs to that graph's CSR)
        idx = dl.train_index().to(DEV)
        opt_r, opt_s = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.optim.Adam(sm.parameters(), lr=1e-3)
        for q in _batches(dl, 3):
            opt_r.zero_grad()
            loss_r = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
            loss_r.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
            opt_r.step()
            loss_s = pkg.dist.train_step_sharded(sm, dl_s.graph, q[:, 0], q[:, 1], idx, opt_s, lbl_smooth=0.1, clip=0.5)
            assert torch.equal(loss_s, loss_r.detach())
    finally:
        torch.use_deterministic_algorithms(False)
    sd_r, sd_s = ref.state_dict(), sm.state_dict()
    names = {'edge_embeddings'} | {'edge_embeddings_extra.%d' % i for i in range(layers - 1)}
    for k, v in sd_r.items():
        if k in names:
            if shard:                                            # the shard model's state holds slot order
                v = v.index_select(0, ref._slot_csr.perm)
        assert torch.equal(sd_s[k], v), k


def test_world1_epoch_equals_harness_epoch(pkg):
    """One train_epoch_sharded at one rank and one harness.train_device_labels with identically seeded generators (dropout 0):
    the same order, the same mean loss and bit-identical parameters afterwards. The batch size leaves a last batch whose size
    is not a multiple of 4, so the unfused scorer (label rows + BCELoss) is compared too."""
    ref, dl, params = _models(pkg, 'syn_b')
    sm, dl_s, _ = _models(pkg, 'syn_b')
    queries = dl.train_queries()
    Q = queries.size(0)
    bs = next(b for b in range(16, 4, -1) if Q % b and (Q % b) % 4)
    idx = dl.train_index().to(DEV)
    params.clip_grad = 0.5
    opt_r, opt_s = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.optim.Adam(sm.parameters(), lr=1e-3)
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    try:
        want = pkg.harness.train_device_labels(ref, queries, idx, dl.graph, opt_r, params, bs,
                                               generator=torch.Generator().manual_seed(4))
        got = pkg.dist.train_epoch_sharded(sm, queries, idx, dl_s.graph, opt_s, params, bs,
                                           generator=torch.Generator().manual_seed(4))
    finally:
        torch.use_deterministic_algorithms(False)
    assert got == want
    sd_r, sd_s = ref.state_dict(), sm.state_dict()
    for k, v in sd_r.items():
        assert torch.equal(sd_s[k], v), k


def test_sharded_step_rejects_bad_models(pkg):
    nat = pkg._native
    model, dl, params = _models(pkg, 'syn_b')
    idx = dl.train_index().to(DEV)
    q = _batches(dl, 1)[0]
    opt = torch.optim.Adam(model.parameters())
    csr = dl.graph.csr(model.relation_embedding.size(0) + 1)
    N = csr.num_nodes
    other, _, _ = _models(pkg, 'syn_b', shard=True)
    other._edge_shard = (csr, 0, N // 2)                      # the shard of another range than this rank's (0, N)
    with pytest.raises(nat.NativeError, match='destinations'):
        pkg.dist.train_step_sharded(other, dl.graph, q[:, 0], q[:, 1], idx, torch.optim.Adam(other.parameters()))
    ids = dl.graph.edge_attr.clone()
    ids[1] = ids[1].flip(0)                                   # edge ids that are not the identity
    g2 = pkg.Graph(edge_index=dl.graph.edge_index, edge_attr=ids, entity=dl.graph.entity, num_nodes=N)
    with pytest.raises(nat.NativeError, match='identity'):
        pkg.dist.train_step_sharded(model, g2, q[:, 0], q[:, 1], idx, opt)


# -- two processes on one GPU over gloo -------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _gloo_worker(rank, world, port, jobs, q):
    try:
        _gloo_worker_body(rank, world, port, jobs, q)
    except Exception:                                        # surface the failure in the parent instead of a timeout
        import traceback
        q.put((rank, {'error': traceback.format_exc()}))


def _gloo_worker_body(rank, world, port, jobs, q):
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
    try:                                                     # whole tables at two ranks: refused before any collective
        pkg.dist.train_step_sharded(whole, dl.graph, q0[:, 0], q0[:, 1], dl.train_index().to(DEV), torch.optim.Adam(whole.parameters()))
        out['whole_table_refused'] = False
    except pkg._native.NativeError as err:
        out['whole_table_refused'] = 'whole per-edge tables' in str(err)
    for name, case, layers, dropout, steps in jobs:
        sm, dl, params = _models(pkg, case, layers, dropout, shard=True, world=world, rank=rank)
        idx = dl.train_index().to(DEV)
        opt = torch.optim.Adam(sm.parameters(), lr=1e-3)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(7)
        losses = [float(pkg.dist.train_step_sharded(sm, dl.graph, q[:, 0], q[:, 1], idx, opt, generator=gen))
                  for q in _job_batches(name, case, dl, steps)]
        csr, n0, n1 = sm._edge_shard
        counts, sub = csr.shard_slot_counts(n0, n1), csr.shard_ee_sub(n0, n1)
        slots = (torch.arange(sum(counts)) + torch.tensor(sub).repeat_interleave(torch.tensor(counts))).to(DEV)
        tables = {n: p for n, p in sm._edge_tables()}
        res = dict(losses=losses, ref_ids=_np(csr.perm.index_select(0, slots)),    # (numpy: pickled by value, not shared)
                   grads={n: _np(p.grad) for n, p in sm.named_parameters() if p.grad is not None},
                   state={k: _np(v) for k, v in sm.state_dict().items() if k not in tables})
        res['tables'] = {n: _np(t) for n, t in tables.items()}
        if name == 'syn_b':                                  # the trained shard model goes straight into the sharded evaluation
            filt = dl.filter_index().to(DEV)
            res['eval'] = pkg.dist.evaluate_sharded(sm, dl.graph, dl.eval_queries('test'), filt, shard_encoder=True)
        out[name] = res
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


_PORTS = [0]


def _run_two_ranks(jobs):
    import torch.multiprocessing as mp
    _PORTS[0] += 1
    world, port = 2, 31700 + (os.getpid() * 7 + 50 * _PORTS[0]) % 2000
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, jobs, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        assert 'error' not in got[r], got[r]['error']
    return got


def _assemble(got, name, key):
    """A per-edge table (or its gradient) in reference edge order from both ranks' shards."""
    parts = [(got[r][name]['ref_ids'], got[r][name][key]) for r in sorted(got)]
    n = sum(ids.size for ids, _ in parts)
    out = {}
    for tname in [k for k in parts[0][1] if k.startswith('edge_embeddings')]:
        t = np.empty((n,) + tuple(parts[0][1][tname].shape[1:]), dtype=np.float32)
        for ids, vals in parts:
            t[ids] = vals[tname]
        out[tname] = t
    return out


def test_two_ranks_one_gpu_match_golden_and_single_step(pkg):
    """Two processes over gloo, one step each of syn_b, syn_c and a 2-layer syn_b, dropout 0, lbl_smooth 0: the loss is the
    golden's (syn_b), every gradient matches the golden / the one-GPU step with test_train_step_gradients_vs_golden's
    tolerances (the table gradient reassembled from both shards), replicated parameters are bit-identical on both ranks after
    Adam, the table rows after the step match the one-GPU step's to 1e-5 — also for a batch the fused scorer does not take —,
    and the trained shard model evaluates through evaluate_sharded(shard_encoder=True) exactly as the same trained state,
    reassembled into one whole-table model, evaluates in one process."""
    jobs = [('syn_b', 'syn_b', 1, 0.0, 1), ('syn_c', 'syn_c', 1, 0.0, 1), ('two_layer', 'syn_b', 2, 0.0, 1),
            ('odd_batch', 'syn_b', 1, 0.0, 1)]
    got = _run_two_ranks(jobs)
    for name, case, layers, _, _ in jobs:
        g = golden(case)
        ref, dl, params = _models(pkg, case, layers)
        idx = dl.train_index().to(DEV)
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
        q = _job_batches(name, case, dl, 1)[0]
        opt.zero_grad()
        loss = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.0)
        loss.backward()
        want_grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
        opt.step()
        inv = ref._slot_csr.inv_perm
        for n in want_grads:
            if n.startswith('edge_embeddings'):
                want_grads[n] = want_grads[n].index_select(0, inv)   # slot order -> reference order
        for r in (0, 1):
            assert abs(got[r][name]['losses'][0] - float(loss.detach())) < 1e-5, (name, r)
        if name == 'syn_b':
            assert abs(got[0][name]['losses'][0] - float(g['train_loss'])) < 1e-5
        tgrads = _assemble(got, name, 'grads')
        for n, want in want_grads.items():
            gr = tgrads[n] if n.startswith('edge_embeddings') else got[0][name]['grads'][n]
            if not n.startswith('edge_embeddings'):
                assert np.array_equal(got[0][name]['grads'][n], got[1][name]['grads'][n]), (name, n)
            ref_g = g.grads()[n] if (name == 'syn_b' and n in g.grads()) else want.cpu()
            scale = float(ref_g.abs().max()) + 1e-12
            floor = 2e-6 if n.startswith('conv2.') else 1e-9
            np.testing.assert_allclose(gr, ref_g.numpy(), rtol=2e-3, atol=2e-5 * scale + floor, err_msg='%s %s' % (name, n))
        for k, v in got[0][name]['state'].items():           # replicated state: the same bits on both ranks
            assert np.array_equal(v, got[1][name]['state'][k]), (name, k)
        ref_sd = ref.state_dict()
        for tname, t in _assemble(got, name, 'tables').items():
            np.testing.assert_allclose(t, ref_sd[tname].cpu().numpy(), rtol=0, atol=1e-5, err_msg=tname)
    assert got[0]['whole_table_refused'] and got[1]['whole_table_refused']
    e0, e1 = got[0]['syn_b']['eval'], got[1]['syn_b']['eval']
    assert e0 == e1 and e0['count'] > 0
    trained, dl, _ = _models(pkg, 'syn_b')                   # the ranks' trained state as one whole-table model
    sd = {k: torch.from_numpy(v) for k, v in got[0]['syn_b']['state'].items()}
    sd.update({k: torch.from_numpy(v) for k, v in _assemble(got, 'syn_b', 'tables').items()})
    trained.load_state_dict(sd)
    want = pkg.dist.evaluate_sharded(trained, dl.graph, dl.eval_queries('test'), dl.filter_index().to(DEV))
    assert e0['count'] == want['count']
    for k in ('mr', 'mrr', 'hits@1', 'hits@3', 'hits@10'):
        assert abs(e0[k] - want[k]) < 1e-12, (k, e0[k], want[k])


def test_two_ranks_dropout_three_steps(pkg):
    """Dropout on (trunk masks from an identically seeded generator, layer masks per rank), 3 steps over two processes:
    replicated parameters and BN statistics stay bit-identical on both ranks and the loss is finite."""
    got = _run_two_ranks([('drop', 'syn_b', 2, 0.3, 3)])
    for r in (0, 1):
        assert all(np.isfinite(v) for v in got[r]['drop']['losses'])
    assert got[0]['drop']['losses'] == got[1]['drop']['losses']
    for k, v in got[0]['drop']['state'].items():
        assert np.array_equal(v, got[1]['drop']['state'][k]), k
