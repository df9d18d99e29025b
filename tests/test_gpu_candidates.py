"""Candidate-list scoring (section (13) of mgcn_hip.h) on a real MI355X. "Expected" is always an entry point that existed
before it: _native.score_fwd's block gathered at the candidates, score_target, MGCN.forward, rank_counts, predict_topk.
Everything is compared with torch.equal; there is no tolerance anywhere."""
import os
import types

import numpy as np
import pytest
import torch

from . import dense_ref as R
from .conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NINF = float('-inf')

# (N, B, K, dim). dim: 32 / 200 / 352 the six-product split (one k-block, a partial last block, the largest), 356 aligned just
# above the split's limit (exact-f32 chain, vector loads), 50 / 7 not a multiple of 4 (exact-f32 chain, guarded loads).
# K around the 16-row tile and across the 64-position workgroup; B = 130: more queries than a strip of the full kernels.
GRID = [
    (37, 1, 1, 32), (1000, 5, 15, 32), (37, 64, 16, 32), (1000, 130, 17, 32), (37, 1, 100, 32), (1000, 1, 16, 32),
    (1000, 5, 1, 200), (37, 64, 15, 200), (1000, 130, 16, 200), (37, 1, 17, 200), (1000, 5, 100, 200), (37, 130, 100, 200),
    (1000, 64, 100, 200),
    (37, 64, 1, 352), (1000, 130, 15, 352), (37, 1, 16, 352), (1000, 5, 17, 352), (37, 64, 100, 352), (37, 130, 16, 352),
    (1000, 130, 1, 356), (37, 1, 15, 356), (1000, 5, 16, 356), (37, 64, 17, 356), (1000, 130, 100, 356), (1000, 64, 1, 356),
    (37, 1, 1, 50), (1000, 5, 15, 50), (37, 64, 16, 50), (1000, 130, 17, 50), (37, 1, 100, 50), (37, 5, 17, 50),
    (1000, 1, 100, 50),
    (1000, 5, 1, 7), (37, 64, 15, 7), (1000, 130, 16, 7), (37, 1, 17, 7), (1000, 5, 100, 7), (37, 130, 15, 7),
]


def operands(N, B, dim, tag=0):
    x, ent, bias = R.score_inputs(B, N, dim, R.seed_of(13, tag, N, B, dim))
    return x.to(DEV), ent.to(DEV), bias.to(DEV)


def lists(N, B, K, seed):
    """Uniform ids with repeats; the last row is arange(K) % N (with one query: on its even positions)."""
    g = R.gen(seed)
    cand = torch.randint(0, N, (B, K), generator=g)
    ramp = torch.arange(K) % N
    if B > 1:
        cand[-1] = ramp
    else:
        cand[0, ::2] = ramp[::2]
    return cand.to(DEV)


@pytest.mark.parametrize('N,B,K,dim', GRID, ids=['%d-%d-%d-%d' % c for c in GRID])
def test_abi_grid_equals_score_fwd_gather(pkg, N, B, K, dim):
    nat = pkg._native
    x, ent, bias = operands(N, B, dim)
    cand = lists(N, B, K, R.seed_of(14, N, B, K, dim))
    got = nat.score_candidates(x, ent, bias, cand)
    want = nat.score_fwd(x, ent, bias).gather(1, cand)
    assert got.shape == (B, K) and got.dtype == torch.float32
    assert torch.equal(got, want)


@pytest.mark.parametrize('dim', [200, 356])
def test_entity_column_window_keeps_the_bits(pkg, dim):
    """ent as big[:, 4:4 + dim]: lde > dim, rows still 16-byte aligned: the same family, the same bits."""
    nat = pkg._native
    N, B, K = 1000, 5, 33
    x, ent, bias = operands(N, B, dim, tag=1)
    cand = lists(N, B, K, R.seed_of(15, dim))
    win = R.layout(ent, 'window')
    assert win.stride(0) > dim and win.data_ptr() % 16 == 0
    got = nat.score_candidates(x, win, bias, cand)
    assert torch.equal(got, nat.score_candidates(x, ent, bias, cand))
    assert torch.equal(got, nat.score_fwd(x, win, bias).gather(1, cand))


@pytest.mark.parametrize('dim', [200, 356, 50])
def test_unaligned_views_equal_score_fwd_on_the_same_views(pkg, dim):
    """ent as big[:, 1:1 + dim] and x one float off 16 bytes: the guarded family of score_fwd, on either operand alone too."""
    nat = pkg._native
    N, B, K = 1000, 5, 33
    x, ent, bias = operands(N, B, dim, tag=2)
    cand = lists(N, B, K, R.seed_of(16, dim))
    xo, eo = R.layout(x, 'offset1'), R.layout(ent, 'offset1')
    assert xo.data_ptr() % 16 == 4 and eo.data_ptr() % 16 == 4
    for xv, ev in ((xo, eo), (x, eo), (xo, ent)):
        assert torch.equal(nat.score_candidates(xv, ev, bias, cand), nat.score_fwd(xv, ev, bias).gather(1, cand))


@pytest.mark.parametrize('dim', [200, 50])
def test_strided_lists_and_output_leave_other_columns_alone(pkg, dim):
    nat = pkg._native
    N, B, K = 1000, 5, 33
    x, ent, bias = operands(N, B, dim, tag=3)
    cand = lists(N, B, K, R.seed_of(17, dim))
    wide = torch.full((B, K + 5), 2 ** 40, dtype=torch.int64, device=DEV)      # ids that would be skipped, were they read
    cv = wide[:, 3:3 + K]
    cv.copy_(cand)
    block = torch.full((B + 1, K + 7), 123.0, device=DEV)
    ov = block[:B, 2:2 + K]
    assert cv.stride(0) > K and ov.stride(0) > K
    res = nat.score_candidates(x, ent, bias, cv, out=ov)
    assert res.data_ptr() == ov.data_ptr()
    assert torch.equal(ov, nat.score_fwd(x, ent, bias).gather(1, cand))
    probe = block.clone()
    probe[:B, 2:2 + K] = 123.0
    assert bool((probe == 123.0).all())


@pytest.mark.parametrize('dim', [200, 356, 50])
def test_ids_outside_the_shard_are_not_read_and_not_written(pkg, dim):
    """-1, N, N + 5, -7, 2^62 and -2^62 at fixed positions: those elements keep the pre-filled value, every other element is
    the gather. The kernel compares id - row0 against n_local before it forms any address (a guarantee that is checked
    here, not a fault that is looked for)."""
    nat = pkg._native
    N, B, K = 1000, 6, 40
    x, ent, bias = operands(N, B, dim, tag=4)
    cand = lists(N, B, K, R.seed_of(18, dim))
    bad = [(0, 0, -1), (0, 15, N), (1, 16, N + 5), (2, 17, -7), (3, 39, 2 ** 62), (4, 1, -2 ** 62), (5, 0, -1), (5, 1, -1),
           (5, 38, N), (5, 39, 2 ** 63 - 1), (2, 3, -2 ** 63)]
    inside = torch.ones((B, K), dtype=torch.bool, device=DEV)
    for b, j, v in bad:
        cand[b, j] = v
        inside[b, j] = False
    out = torch.full((B, K), 7.5, device=DEV)
    nat.score_candidates(x, ent, bias, cand, out=out)
    want = nat.score_fwd(x, ent, bias).gather(1, cand.clamp(0, N - 1))
    assert bool((out[~inside] == 7.5).all())
    assert torch.equal(out[inside], want[inside])
    fresh = nat.score_candidates(x, ent, bias, cand)                             # out=None: a -inf block
    assert bool((fresh[~inside] == NINF).all()) and torch.equal(fresh[inside], want[inside])
    # a shard in the middle of the id range: ids below row0 are foreign as well
    row0 = 400
    got = nat.score_candidates(x, ent[row0:700], bias[row0:700], cand, ent_row0=row0)
    mine = inside & (cand >= row0) & (cand < 700)
    assert bool((got[~mine] == NINF).all()) and torch.equal(got[mine], want[mine]) and bool(mine.any())


@pytest.mark.parametrize('cuts', [(0, 333, 1000), (0, 100, 777, 1000)])
@pytest.mark.parametrize('dim', [200, 50])
def test_shards_fill_one_block_and_the_mask_gives_minus_inf(pkg, cuts, dim):
    nat = pkg._native
    N, B, K = 1000, 9, 50
    x, ent, bias = operands(N, B, dim, tag=5)
    cand = lists(N, B, K, R.seed_of(19, dim))
    cand[0, 7], cand[1, 8] = -1, N + 5
    whole = nat.score_candidates(x, ent, bias, cand)
    inside = (cand >= 0) & (cand < N)
    assert torch.equal(whole[inside], nat.score_fwd(x, ent, bias).gather(1, cand.clamp(0, N - 1))[inside])
    hit = torch.rand((B, N), generator=R.gen(R.seed_of(20, dim))) < 0.3
    hit[2] = True                                                                # a query with every entity filtered
    hit = hit.to(DEV)
    masked = nat.score_candidates(x, ent, bias, cand, mask=R.pack_bits(hit))
    filtered = hit.gather(1, cand.clamp(0, N - 1)) & inside
    assert bool(filtered.any()) and bool((masked[filtered] == NINF).all())
    assert torch.equal(masked[~filtered], whole[~filtered])
    block = torch.full((B, K), NINF, device=DEV)
    block_m = block.clone()
    for n0, n1 in zip(cuts[:-1], cuts[1:]):
        nat.score_candidates(x, ent[n0:n1], bias[n0:n1], cand, ent_row0=n0, out=block)
        nat.score_candidates(x, ent[n0:n1], bias[n0:n1], cand, ent_row0=n0, out=block_m, mask=R.pack_bits(hit[:, n0:n1]))
    assert torch.equal(block, whole)
    assert torch.equal(block_m, masked)


# ------------------------------------------------------------------------------------------------ the model
def _golden_model(pkg, case, **over):
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
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    missing = model.load_state_dict(g.state_dict(), strict=False)
    assert not missing.unexpected_keys
    trip = g.t('dl_q_test_tail_triple').to(DEV)
    return model.to(DEV).eval(), dl.graph, dl.num_entity, dl.filter_index().to(DEV), trip


def _random_model(pkg, oracle, **over):
    """A seeded graph of 300 entities, 5 relations, 1500 triples; one layer 32 -> 200."""
    N, Rn, E = 300, 5, 1500
    tri = oracle.synthetic_triples(N, Rn, E, seed=3, zipf=0.0)
    ei, ea = oracle.build_edge_list(tri, Rn)
    graph = pkg.Graph(edge_index=torch.from_numpy(ei), edge_attr=torch.from_numpy(ea))
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    base = dict(gcn_in_dim=32, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20, num_filter=8,
                kernel_size=7, bias=False, lbl_smooth=0.1, gcn_layers=1, device=torch.device(DEV))
    base.update(over)
    torch.manual_seed(4)
    model = pkg.MGCN(N, Rn, E, types.SimpleNamespace(**base))
    with torch.no_grad():
        model.entity_embedding.mul_(10.0)
        model.edge_embeddings.mul_(30.0)
    tri = torch.from_numpy(np.asarray(tri, dtype=np.int64))
    known = {}
    for s, r, o in tri.tolist():
        known.setdefault((s, r), set()).add(o)
        known.setdefault((o, r + Rn), set()).add(s)
    filt = pkg.dist.FilterIndex.from_known(known, 2 * Rn).to(DEV)
    graph.to(DEV)
    return model.to(DEV).eval(), graph, N, filt, tri[:24].to(DEV)


_MODELS = {}


def _case(pkg, oracle, name, bf16=False):
    key = (name, bf16)
    if key not in _MODELS:
        over = dict(edge_table_dtype='bf16') if bf16 else {}
        _MODELS[key] = _random_model(pkg, oracle, **over) if name == 'random300' else _golden_model(pkg, name, **over)
    return _MODELS[key]


def _model_lists(N, B, K=20, seed=21):
    cand = torch.randint(0, N, (B, K), generator=R.gen(seed))
    cand[0, 3], cand[0, 4], cand[B - 1, 0] = -1, N, N + 7
    cand[B - 1, 5] = cand[B - 1, 6]
    return cand.to(DEV)


CASES = ['toy_small', 'syn_a', 'random300']


@pytest.mark.parametrize('case', CASES)
def test_model_surface_equals_forward_rank_counts_and_topk(pkg, oracle, case, monkeypatch):
    monkeypatch.delenv('MGCN_EE', raising=False)
    model, graph, N, filt, trip = _case(pkg, oracle, case)
    src, rel, obj = trip[:, 0].contiguous(), trip[:, 1].contiguous(), trip[:, 2].contiguous()
    B = src.numel()
    with torch.no_grad():
        score = model(src, rel, graph)
    cand = _model_lists(N, B)
    inside = (cand >= 0) & (cand < N)
    want = torch.where(inside, score.gather(1, cand.clamp(0, N - 1)), torch.full_like(cand, NINF, dtype=torch.float32))
    model.train()
    got = model.score_candidates(src, rel, cand, graph)
    assert model.training                                                        # the mode is restored
    model.eval()
    assert torch.equal(got, want) and not got.requires_grad
    # with the filter: the known tails of (src, rel) read -inf, everything else is unchanged
    known = pkg._native.filter_mask(filt.query_keys(src, rel), filt.keys, filt.ptr, filt.tails, N)
    col = cand.clamp(0, N - 1)
    bit = ((known.long().gather(1, col >> 5) >> (col & 31)) & 1).bool() & inside
    got_f = model.score_candidates(src, rel, cand, graph, filter_index=filt)
    assert torch.equal(got_f, torch.where(bit, torch.full_like(want, NINF), want))
    # triples: the target of rank_counts
    counts, target = model.rank_counts(src, rel, obj, None, graph, filter_index=filt)
    assert torch.equal(model.score_triples(src, rel, obj, graph), target)
    assert torch.equal(target, score.gather(1, obj.view(-1, 1)).view(-1))
    # re-scoring predict_topk's ids (rows end in -1 padding where k > the entities left)
    for k, f in ((min(N + 3, 1024), None), (10, filt)):
        ids, s = model.predict_topk(src, rel, graph, k=k, filter_index=f)
        assert torch.equal(model.score_candidates(src, rel, ids, graph), s)
        if k > N:
            assert bool((ids[:, N:] == -1).all())
    # every entity as the list: rank_counts
    every = torch.arange(N, device=DEV).expand(B, N).contiguous()
    c2, t2 = model.rank_candidates(src, rel, obj, every, graph, filter_index=filt)
    assert c2.dtype == torch.int64 and torch.equal(c2, counts) and torch.equal(t2, target)
    pkg._native.check_fused_status(DEV)


@pytest.mark.parametrize('case', CASES)
def test_bf16_table_model_equals_its_own_forward(pkg, oracle, case, monkeypatch):
    monkeypatch.delenv('MGCN_EE', raising=False)
    model, graph, N, filt, trip = _case(pkg, oracle, case, bf16=True)
    assert model.edge_embeddings.dtype == torch.bfloat16
    src, rel, obj = trip[:, 0].contiguous(), trip[:, 1].contiguous(), trip[:, 2].contiguous()
    cand = _model_lists(N, src.numel(), seed=22)
    inside = (cand >= 0) & (cand < N)
    with torch.no_grad():
        score = model(src, rel, graph)
    got = model.score_candidates(src, rel, cand, graph)
    assert torch.equal(got[inside], score.gather(1, cand.clamp(0, N - 1))[inside]) and bool((got[~inside] == NINF).all())
    assert torch.equal(model.score_triples(src, rel, obj, graph), score.gather(1, obj.view(-1, 1)).view(-1))
    pkg._native.check_fused_status(DEV)


@pytest.mark.parametrize('case', ['toy_small', 'syn_a'])
def test_evaluate_candidates_equals_predict_over_the_whole_table(pkg, oracle, case, monkeypatch):
    """cand = every entity, no filter: the sums harness.predict forms from rank_counts (an all-zero label block filters
    nothing), normalised as evaluate normalises one side."""
    monkeypatch.delenv('MGCN_EE', raising=False)
    model, graph, N, filt, trip = _case(pkg, oracle, case)
    Q = trip.size(0)
    every = torch.arange(N, device=DEV).expand(Q, N).contiguous()
    got = pkg.harness.evaluate_candidates(model, trip, every, graph, batch_size=3)
    iters = {'test_tail': [(trip[i:i + 3].cpu(), torch.zeros(trip[i:i + 3].size(0), N)) for i in range(0, Q, 3)]}
    sums = pkg.harness.predict(model, iters, graph, 'test', torch.device(DEV), mode='tail_batch')
    assert sums['count'] == Q
    want = {'mr': np.round(sums['mr'] / Q, 5), 'mrr': np.round(sums['mrr'] / Q, 5)}
    for k in (1, 3, 10):
        want['hits@%d' % k] = np.round(sums['hits@%d' % k] / Q, 5)
    assert got == want
