"""The bf16 per-edge table on a real MI355X (`-m gpu`; DESIGN §4.9, include/mgcn_hip.h (2e)). There is no tolerance anywhere:
a launch given the bf16 table T must give, bit for bit, what the same launch of the project's own f32 path gives from the f32
table T.float() — the yardstick is the parent's kernels, reached through the unchanged f32 entry points. Every comparison is
torch.equal.

The graphs have 300 nodes and are built with tests/live_graphs.py; each one holds a destination without slots, leaf
destinations (dead slots: the live view is non-trivial), one hub of 33 slots and one of 129 (one and three chunks at threshold
32, chunk 64) — asserted from the graph's own arrays. The one graph WITHOUT a dead slot has every node on its source ring, so
it keeps the hubs and has no empty destination."""
import types

import numpy as np
import pytest
import torch

from .live_graphs import edge_list, random_halves

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, R = 300, 3
B33, B129 = 100, 200                # the two hub destinations
GEN4 = 0x400                        # `tune` bits 10-11 = 1: the reserved value

_cache = {}


def _halves(share, seed):
    """random_halves with a 33-slot destination, then a second destination brought to 129 slots per half; the halves are made
    equally long with copies of an edge that enters neither."""
    halves = [list(h) for h in random_halves(N, R, share, seed, big=(B33, 33))]
    rng = np.random.default_rng(seed + 100)
    for h in halves:
        srcs = sorted({int(e[0]) for e in h})
        h.append((B129, srcs[0], 0))                                      # B129 is a source of this half: its slots are live
        have = sum(1 for e in h if int(e[1]) == B129)
        h += [(srcs[int(rng.integers(0, len(srcs)))], B129, int(rng.integers(0, 2 * R))) for _ in range(129 - have)]
    E = max(len(h) for h in halves)
    for h in halves:
        pad = next(e for e in h if int(e[1]) not in (B33, B129))
        h += [pad] * (E - len(h))
    return halves


def _graph(pkg, share=0.5, seed=0, hubs=True):
    key = (share, seed, hubs)
    if key not in _cache:
        ei, et = edge_list(*_halves(share, seed))
        thr = dict(hub_threshold=32, hub_chunk=64) if hubs else dict(hub_threshold=0)
        _cache[key] = (pkg.GraphCSR(N, 2 * R + 1, ei, et, torch.device(DEV), **thr), ei, et)
    return _cache[key]


def _check_graph(pkg, share=0.5, seed=0):
    """What the module docstring promises, from the arrays of the graph with hubs (the one without has the same edges)."""
    csr = _graph(pkg, share, seed, True)[0]
    hub, chunks = csr.hubinfo.cpu(), csr.chunks.cpu()
    rp = csr.rowptr.cpu()
    for h in range(2):
        counts = {}
        for n in (B33, B129):
            first, cnt = int(hub[h, n, 0]), int(hub[h, n, 1])
            assert cnt > 0 and int(rp[h, n + 1] - rp[h, n]) == 0           # a hub's own run is empty
            counts[n] = (int(chunks[first + cnt - 1, 1]) - int(chunks[first, 0]), cnt)
        assert counts[B33] == (33, 1) and counts[B129] == (129, 3), counts
        empty = (rp[h, 1:] == rp[h, :-1]) & (hub[h, :, 1] == 0)
        assert share == 0 or bool(empty.any())     # a destination without slots (share = 0: every node is on the source ring)
    if share > 0:
        assert csr.live_rowptr is not None and csr.num_dead_slots > 20     # leaf destinations: their slots are dead
    else:
        assert csr.live_rowptr is None and csr.num_dead_slots == 0
    return csr


def _tables(E2, D, seed=7):
    """(unrounded f32, rounded f32 = the yardstick's table, bf16) [2E, D]."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(E2, D, generator=g) * 0.5
    t16 = raw.to(torch.bfloat16)
    return raw.to(DEV), t16.float().to(DEV), t16.to(DEV)


# ------------------------------------------------------------------------------------------------ unfused aggregate_fwd
class _Agg(object):
    def __init__(self, pkg, csr, D, seed=1):
        g = torch.Generator().manual_seed(seed)
        self.x = (torch.randn(N, D, generator=g) * 0.4).to(DEV)
        self.rel = (torch.randn(2 * R + 1, D, generator=g) * 0.5).to(DEV)
        self.loop_edge = (torch.randn(D, generator=g) * 0.5).to(DEV)
        self.nat, self.csr, self.D = pkg._native, csr, D

    def launch(self, ee, slot_order=True, rng=None, ee_sub=(0, 0, 0)):
        n0, n1 = rng or (0, N)
        out = torch.full((n1 - n0, 3 * self.D), float('nan'), device=DEV)
        self.nat.aggregate_fwd(self.csr, self.x, self.rel, ee, slot_order, self.loop_edge, out, node_range=rng, ee_sub=ee_sub,
                               out_row0=n0)
        return out


@pytest.mark.parametrize('slot_order', [True, False])
@pytest.mark.parametrize('D', [4, 100, 132, 6])
def test_aggregate_fwd(pkg, D, slot_order):
    """D = 4, 100, 132: 8-byte loads of the bf16 row (one, one and two column chunks per lane); D = 6: the element-wise path."""
    csr = _check_graph(pkg)
    raw, t32, t16 = _tables(2 * csr.num_edges_half, D)
    a = _Agg(pkg, csr, D)
    want = a.launch(t32, slot_order)
    assert torch.isfinite(want).all() and float(want.abs().mean()) > 1e-3
    assert not torch.equal(want, a.launch(raw, slot_order))                # the rounding is visible: the table matters
    assert torch.equal(a.launch(t16, slot_order), want)
    plain = _Agg(pkg, _graph(pkg, hubs=False)[0], D)                        # the same edges without the hub pre-pass
    assert torch.equal(plain.launch(t16, slot_order), plain.launch(t32, slot_order))


@pytest.mark.parametrize('D', [100, 6])
def test_aggregate_fwd_table_view_with_a_two_byte_aligned_base(pkg, D):
    csr = _check_graph(pkg)
    E2 = 2 * csr.num_edges_half
    raw, t32, t16 = _tables(E2, D)
    buf = torch.zeros(E2 * D + 1, dtype=torch.bfloat16, device=DEV)
    view = buf[1:].view(E2, D)
    view.copy_(t16)
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    buf32 = torch.zeros(E2 * D + 1, dtype=torch.float32, device=DEV)       # the f32 launch on its own element-wise path
    view32 = buf32[1:].view(E2, D)
    view32.copy_(t32)
    assert view32.data_ptr() % 16 == 4
    a = _Agg(pkg, csr, D)
    want = a.launch(view32)
    assert torch.equal(want, a.launch(t32))
    assert torch.equal(a.launch(view), want)


def test_aggregate_fwd_three_ranks_with_table_shards(pkg):
    D = 100
    csr = _check_graph(pkg)
    raw, t32, t16 = _tables(2 * csr.num_edges_half, D)
    a = _Agg(pkg, csr, D)
    whole = a.launch(t16)
    assert torch.equal(whole, a.launch(t32))
    b = csr.balanced_bounds(3)
    assert b[0] == 0 and b[-1] == N and all(b[i] < b[i + 1] for i in range(3))
    assert any(b[i] <= B33 < b[i + 1] and not b[i] <= B129 < b[i + 1] for i in range(3))        # the hubs sit on two ranks
    for r in range(3):
        n0, n1 = b[r], b[r + 1]
        shard = csr.edge_table_shard(t16, n0, n1)
        sub = csr.shard_ee_sub(n0, n1)
        assert shard.dtype == torch.bfloat16 and (r == 0 or sub[0] > 0)
        assert torch.equal(a.launch(shard, rng=(n0, n1), ee_sub=sub), whole[n0:n1])


# ------------------------------------------------------------------------------------------------ fused layer
class _Layer(object):
    """One layer's operands: seeded, with non-trivial BN statistics (as tests/test_gpu_live_slots.py)."""

    def __init__(self, pkg, csr, D, O, seed=1):
        torch.manual_seed(seed)
        self.conv = pkg.MGCNConv(D, O, 2 * R, bias=True).to(DEV).eval()
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            self.conv.ent_bn.running_mean.copy_(torch.randn(O, generator=g) * 0.05)
            self.conv.ent_bn.running_var.copy_(torch.rand(O, generator=g) * 0.5 + 0.05)
            self.conv.bias.copy_(torch.randn(O, generator=g) * 0.1)
        self.x = (torch.randn(N, D, generator=g) * 0.4).to(DEV)
        self.rel = (torch.randn(2 * R, D, generator=g) * 0.5).to(DEV)
        self.raw, self.t32, self.t16 = _tables(2 * csr.num_edges_half, D)
        self.pkg, self.csr, self.D, self.O = pkg, csr, D, O

    def launch(self, ee, live=None, tune=0, rng=None, balance=False, shard=False, wpack=None):
        nat, conv, bn, csr = self.pkg._native, self.conv, self.conv.ent_bn, self.csr
        n0, n1 = rng or (0, N)
        out = torch.full((n1 - n0, self.O), float('nan'), device=DEV)
        with torch.no_grad():
            nat.layer_fwd_fused(csr, self.x, self.rel, conv.loop_rel.reshape(-1), csr.edge_table_shard(ee, n0, n1) if shard else ee,
                                True, conv.loop_edge.reshape(-1), conv.derived_weights()[1] if wpack is None else wpack, self.O,
                                conv.bias, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out, node_range=rng,
                                ee_sub=csr.shard_ee_sub(n0, n1) if shard else (0, 0, 0), tune=tune, balance=balance, live=live)
        return out


@pytest.mark.parametrize('hubs', [True, False])
@pytest.mark.parametrize('live', [True, False])
@pytest.mark.parametrize('D,O', [(100, 200), (132, 8), (4, 8)])
def test_fused_generation2(pkg, D, O, live, hubs):
    """Launched without row bounds, so the 300 rows stay on the lockstep kernel: 13 and 2 column tiles, one and two 128-column
    stages, the relation table in LDS."""
    _check_graph(pkg)
    csr = _graph(pkg, hubs=hubs)[0]
    assert pkg._native.lib().mgcn_fused_kernel_generation(D, O, N, 0) == 2 and (csr.num_chunks > 0) == hubs
    lay = _Layer(pkg, csr, D, O)
    want = lay.launch(lay.t32, live)
    assert torch.isfinite(want).all() and float(want.abs().mean()) > 0.02
    assert not torch.equal(want, lay.launch(lay.raw, live))
    assert torch.equal(lay.launch(lay.t16, live), want)
    pkg._native.check_fused_status(DEV)


def test_fused_generation2_graph_without_a_dead_slot(pkg):
    csr = _check_graph(pkg, share=0.0, seed=3)
    lay = _Layer(pkg, csr, 100, 200)
    want = lay.launch(lay.t32)
    assert torch.isfinite(want).all() and torch.equal(lay.launch(lay.t16), want)
    with pytest.raises(pkg._native.NativeError):
        lay.launch(lay.t16, live=True)                                     # no view to walk
    pkg._native.check_fused_status(DEV)


@pytest.mark.parametrize('live', [True, False])
@pytest.mark.parametrize('D,O,bounds', [(260, 8, False), (100, 212, False), (100, 200, True)])
def test_fused_generation3(pkg, D, O, bounds, live):
    """The elastic kernel by shape (D > 256: more than one column pass; O > 208) and by dispatch (the lockstep shape with
    work-balanced row bounds)."""
    nat = pkg._native
    csr = _check_graph(pkg)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    if bounds:
        assert csr.workgroup_bounds(0, N, cus) is not None
    assert nat.lib().mgcn_fused_kernel_generation(D, O, N, int(bounds)) == 3
    lay = _Layer(pkg, csr, D, O)
    want = lay.launch(lay.t32, live, balance=bounds)
    assert torch.isfinite(want).all() and not torch.equal(want, lay.launch(lay.raw, live, balance=bounds))
    assert torch.equal(lay.launch(lay.t16, live, balance=bounds), want)
    if bounds:                                                             # generations 2 and 3 give the same rows, bf16 table too
        assert torch.equal(lay.launch(lay.t16, live, balance=False), want)
    nat.check_fused_status(DEV)


@pytest.mark.parametrize('live', [True, False])
def test_fused_generation3_destination_range_with_shard_offsets(pkg, live):
    D, O, n0, n1 = 100, 212, 71, 237                                       # both hubs inside, no multiple of 16
    csr = _check_graph(pkg)
    lay = _Layer(pkg, csr, D, O)
    full = lay.launch(lay.t16, live)
    assert torch.equal(full, lay.launch(lay.t32, live))
    sub = csr.shard_ee_sub(n0, n1)
    assert min(sub) > 0
    want = lay.launch(lay.t32, live, rng=(n0, n1), shard=True)
    assert torch.equal(want, full[n0:n1])
    assert torch.equal(lay.launch(lay.t16, live, rng=(n0, n1), shard=True), want)
    rows = pkg.dist.encode_layer_rows(lay.conv, csr, lay.x, lay.rel, csr.edge_table_shard(lay.t16, n0, n1), n0, n1, sub)
    assert torch.equal(rows, want)
    pkg._native.check_fused_status(DEV)


# ------------------------------------------------------------------------------------------------ the model
def _params(**kw):
    base = dict(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20, num_filter=8,
                kernel_size=7, bias=False, lbl_smooth=0.1, gcn_layers=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _model_graph(pkg):
    csr, ei, et = _graph(pkg)
    E = ei.size(1) // 2
    graph = pkg.Graph(edge_index=ei.clone(), edge_attr=torch.stack((et, torch.arange(2 * E))))
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    graph.to(DEV)
    return graph, E


def _model(pkg, E, seed, **kw):
    torch.manual_seed(seed)
    model = pkg.MGCN(N, R, E, _params(**kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for layer in [model.conv1] + list(model.conv1_extra):
            layer.ent_bn.running_mean.copy_(torch.randn(200, generator=g) * 0.05)
            layer.ent_bn.running_var.copy_(torch.rand(200, generator=g) * 0.5 + 0.05)
    return model


def test_two_layer_model_equals_its_f32_twin(pkg, monkeypatch):
    """encode (captured, then replayed), forward, rank_counts and predict_topk of the bf16 model against an f32 model whose
    tables hold the widened values; again after load_state_dict of another (f32) checkpoint: no stale cache, no stale capture."""
    monkeypatch.delenv('MGCN_EE', raising=False)
    nat = pkg._native
    graph, E = _model_graph(pkg)
    m16 = _model(pkg, E, 0, edge_table_dtype='bf16')
    twin = _model(pkg, E, 5)
    twin.load_state_dict(m16.state_dict())                                 # bf16 -> f32: the widened values
    other = {k: v.clone() for k, v in _model(pkg, E, 9).state_dict().items()}   # an f32 checkpoint of another model
    m16.to(DEV).eval()
    twin.to(DEV).eval()
    for t in [m16.edge_embeddings] + list(m16.edge_embeddings_extra):
        assert t.dtype == torch.bfloat16 and t.is_cuda and not t.requires_grad
    g = torch.Generator().manual_seed(2)
    B = 8
    src, rel = torch.randint(0, N, (B,), generator=g).to(DEV), torch.randint(0, 2 * R, (B,), generator=g).to(DEV)
    obj = torch.randint(0, N, (B,), generator=g).to(DEV)
    label = (torch.rand(B, N, generator=g) < 0.05).float().to(DEV)

    def compare():
        with torch.no_grad():
            for _ in range(2):                                             # capture, then replay
                e16, r16 = m16.encode(graph)
                e32, r32 = twin.encode(graph)
                assert torch.isfinite(e32).all() and torch.equal(e16, e32) and torch.equal(r16, r32)
            assert m16._hip_graph is not None and m16._slot_csr is not None
            s32 = twin(src, rel, graph)
            assert torch.equal(m16(src, rel, graph), s32)
            c16, t16 = m16.rank_counts(src, rel, obj, label, graph)
            c32, t32 = twin.rank_counts(src, rel, obj, label, graph)
            assert torch.equal(c16, c32) and torch.equal(t16, t32)
            i16, p16 = m16.predict_topk(src, rel, graph, k=10)
            i32, p32 = twin.predict_topk(src, rel, graph, k=10)
            assert torch.equal(i16, i32) and torch.equal(p16, p32)
        return e32.clone()

    first = compare()
    m16.load_state_dict(other)                                             # rounds the tables as it copies
    twin.load_state_dict(other)
    twin.load_state_dict({k: v for k, v in m16.state_dict().items() if 'edge_embeddings' in k}, strict=False)
    assert torch.equal(twin.edge_embeddings.data.cpu(), other['edge_embeddings'].to(torch.bfloat16).float())
    assert not torch.equal(compare(), first)
    nat.check_fused_status(DEV)


def test_refusals(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_EE', raising=False)
    nat = pkg._native
    csr = _check_graph(pkg)
    lay = _Layer(pkg, csr, 100, 200)
    g = torch.zeros(N, 200, device=DEV)
    rel_full = torch.cat([lay.rel, lay.conv.loop_rel.detach()], dim=0)
    with pytest.raises(nat.NativeError, match='inference-only'):
        nat.aggregate_bwd(csr, lay.x, rel_full, lay.t16, g)
    with pytest.raises(nat.NativeError, match='inference-only'):
        nat.aggregate_bwd_shard(csr, lay.x, rel_full, csr.edge_table_shard(lay.t16, 0, 64), g[:64], (0, 64))
    # the reserved `tune` value is refused for either table, and nothing packs for the generation it once forced
    with pytest.raises(nat.NativeError):
        nat.pack_weights(lay.conv.derived_weights()[0], generation=4)
    with pytest.raises(nat.NativeError):
        lay.launch(lay.t32, tune=GEN4)
    with pytest.raises(nat.NativeError):
        lay.launch(lay.t16, tune=GEN4)
    assert torch.equal(lay.launch(lay.t16), lay.launch(lay.t32))           # the refused launch left the hub buffers usable
    graph, E = _model_graph(pkg)
    m16 = _model(pkg, E, 0, edge_table_dtype='bf16').to(DEV)
    m16.train()
    with pytest.raises(nat.NativeError, match='inference-only'):
        m16.encode(graph)
    nat.check_fused_status(DEV)


def test_f32_default_path_is_the_old_entry_points(pkg, monkeypatch):
    """The model built without the switch: f32 tables with gradients, and its eval encode equals, bit for bit, the layers
    launched by hand through mgcn_layer_fwd_fused / _live on those tables."""
    monkeypatch.delenv('MGCN_EE', raising=False)
    nat = pkg._native
    graph, E = _model_graph(pkg)
    model = _model(pkg, E, 0).to(DEV).eval()
    tables = [model.edge_embeddings] + list(model.edge_embeddings_extra)
    assert all(t.dtype == torch.float32 and t.requires_grad for t in tables)
    called = []
    lib = nat.lib()
    for name in ('mgcn_layer_fwd_fused_ee16', 'mgcn_layer_fwd_fused_live_ee16', 'mgcn_aggregate_fwd_ee16'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: called.append(_n) or 1)
    with torch.no_grad():
        ent, rel = model.encode(graph)
        csr = graph.csr(2 * R + 1)
        x, r = model.entity_embedding.detach(), model.relation_embedding.detach()
        for layer, table in zip([model.conv1] + list(model.conv1_extra), tables):
            bn = layer.ent_bn
            out = torch.empty((N, 200), device=DEV)
            r_out = torch.empty((2 * R, 200), device=DEV)
            nat.layer_fwd_fused(csr, x.contiguous(), r.contiguous(), layer.loop_rel.reshape(-1), table.detach(), True,
                                layer.loop_edge.reshape(-1), layer.derived_weights()[1], 200, layer.bias, bn.running_mean,
                                bn.running_var, bn.weight, bn.bias, bn.eps, out, rels_weight=layer.rels_weight.detach().contiguous(),
                                rel_out=r_out)
            x, r = out, r_out
    assert not called and torch.isfinite(ent).all()
    assert torch.equal(ent, x) and torch.equal(rel, r)
    nat.check_fused_status(DEV)
