"""The fused layer on the graph's live view (`-m gpu`): mgcn_layer_fwd_fused_live walks only the slots whose norm is not
exactly zero (include/mgcn_hip.h (1v), (2b) "Live view"). The yardstick is the unchanged canonical entry point of the same
library (`live=False`); every comparison is torch.equal. Every graph asserts from its own arrays that it has dead slots
(except where the case IS "no dead slot": then no view exists and the launch is the canonical one).

Two cases the shapes force: a graph of ONE node cannot have a dead slot (its only destination is the source of every edge),
so N = 1 checks that no view is built and covers the one-row launch as a one-destination range of the 161-node graph; and
generation 2 takes 64-row tiles for every launch of at most one tile per CU, so its 80-row tiles at O = 200 (the kernel
instance the WN18RR benchmark runs) need 16 385 .. 20 480 rows: one case at N = 20 000."""
import types

import numpy as np
import pytest
import torch

from .live_graphs import edge_list, random_halves

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GEN2, GEN3 = 0x800, 0xc00          # `tune` bits 10-11: force the lockstep / the elastic kernel

_graphs = {}


def _graph(pkg, N, R=3, share=0.5, seed=0, hub_threshold=0, hub_chunk=4, **kw):
    key = (N, R, share, seed, hub_threshold, hub_chunk, tuple(sorted(kw.items())))
    if key not in _graphs:
        ei, et = edge_list(*random_halves(N, R, share, seed, **kw))
        csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, torch.device(DEV), hub_threshold=hub_threshold, hub_chunk=hub_chunk)
        _graphs[key] = (csr, ei, et)
    return _graphs[key]


def _dead_share(csr):
    rp = csr.rowptr.cpu()
    total = int(rp[1, -1] - rp[0, 0])
    return csr.num_dead_slots / max(total, 1)


class _Layer(object):
    """One layer's operands for a graph: seeded, with non-trivial BN statistics."""

    def __init__(self, pkg, csr, D, O, seed=1):
        R2, E2 = csr.num_rel_rows - 1, 2 * csr.num_edges_half
        torch.manual_seed(seed)
        self.conv = pkg.MGCNConv(D, O, R2, bias=True).to(DEV).eval()
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            self.conv.ent_bn.running_mean.copy_(torch.randn(O, generator=g) * 0.05)
            self.conv.ent_bn.running_var.copy_(torch.rand(O, generator=g) * 0.5 + 0.05)
            self.conv.bias.copy_(torch.randn(O, generator=g) * 0.1)
        self.x = (torch.randn(csr.num_nodes, D, generator=g) * 0.4).to(DEV)
        self.rel = (torch.randn(R2, D, generator=g) * 0.5).to(DEV)
        self.table = (torch.randn(max(E2, 1), D, generator=g) * 0.5)[:E2].to(DEV)       # slot order
        self.pkg, self.csr, self.O = pkg, csr, O
        self.packed = {}

    def wpack(self, gen):
        """Packed weights for a forced generation (0: the shape's own; generations 2 and 3 share one packing for O > 128)."""
        if gen not in self.packed:
            wcat, wp = self.conv.derived_weights()
            self.packed[gen] = wp if gen == 0 else self.pkg._native.pack_weights(wcat, generation=gen)
        return self.packed[gen]

    def launch(self, live, tune=0, rng=None, table=None, x=None, balance=True):
        nat, conv, bn, csr = self.pkg._native, self.conv, self.conv.ent_bn, self.csr
        n0, n1 = rng or (0, csr.num_nodes)
        out = torch.full((n1 - n0, self.O), float('nan'), device=DEV)
        ee = self.table if table is None else table
        sharded = rng is not None and table is None
        with torch.no_grad():
            nat.layer_fwd_fused(csr, self.x if x is None else x, self.rel, conv.loop_rel.reshape(-1),
                                csr.edge_table_shard(ee, n0, n1) if sharded else ee, True, conv.loop_edge.reshape(-1),
                                self.wpack(nat.tune_generation(tune)), self.O, conv.bias, bn.running_mean, bn.running_var,
                                bn.weight, bn.bias, bn.eps, out, node_range=rng,
                                ee_sub=csr.shard_ee_sub(n0, n1) if sharded else (0, 0, 0), tune=tune, balance=balance, live=live)
        return out


def _big_and_block(N):
    """One destination of 40 live slots (a record chunk is 32) flanked by dead runs; from 64 rows on, whole tiles of dead
    destinations: rows 64 .. 159 cover the second 64-row tile and the second 80-row tile of a 161-node graph."""
    kw = dict(big=(N // 3, 40))
    if N >= 161:
        kw['dead_block'] = (64, 160)
    return kw


@pytest.mark.parametrize('D', [100, 200])
@pytest.mark.parametrize('N', [79, 80, 81, 161])
def test_live_walk_equals_the_canonical_walk(pkg, N, D):
    """About half the slots dead, hub_threshold = 0: both generations on the live view against themselves on the canonical
    layout, and generation 2 against generation 3 on the live view. 200 -> 200 walks every record twice (two column passes)."""
    O = 200
    csr, _, _ = _graph(pkg, N, **_big_and_block(N))
    assert csr.live_rowptr is not None and 0.25 < _dead_share(csr) < 0.85 and csr.num_chunks == 0
    rp, lrp = csr.rowptr.cpu(), csr.live_rowptr.cpu()
    b = N // 3
    for h in range(2):
        assert int(lrp[h, b + 1] - lrp[h, b]) >= 40                                    # longer than one record chunk, live
        for n in (b - 1, b + 1):
            assert int(rp[h, n + 1] - rp[h, n]) > 0 and int(lrp[h, n + 1] - lrp[h, n]) == 0   # flanked by dead runs
        if N >= 161:
            assert int(lrp[h, 160] - lrp[h, 64]) == 0 and bool((rp[h, 65:161] > rp[h, 64:160]).all())   # tiles of dead runs only
    lay = _Layer(pkg, csr, D, O)
    want = lay.launch(False, GEN2)
    assert torch.isfinite(want).all() and float(want.abs().mean()) > 0.05
    got2, got3 = lay.launch(True, GEN2), lay.launch(True, GEN3)
    assert torch.equal(got2, want)
    assert torch.equal(lay.launch(False, GEN3), want)
    assert torch.equal(got3, want) and torch.equal(got2, got3)
    assert torch.equal(lay.launch(None), want)                                          # the default launch takes the view
    pkg._native.check_fused_status(DEV)


@pytest.mark.parametrize('O', [32, 64, 128])
def test_narrow_outputs(pkg, O):
    """The other column-tile variants of generation 2 (2, 4 and 8 column tiles, 80-row tiles: 161 rows = two tiles and one
    of a single row). (The elastic kernel does not take these shapes: it reads another packing for O <= 128.)"""
    csr, _, _ = _graph(pkg, 161, **_big_and_block(161))
    assert csr.num_dead_slots > 0
    lay = _Layer(pkg, csr, 100, O)
    assert pkg._native.lib().mgcn_fused_kernel_generation(100, O, 161, 0) == 2
    want = lay.launch(False)
    assert torch.isfinite(want).all() and torch.equal(lay.launch(True), want)
    pkg._native.check_fused_status(DEV)


def test_single_node_and_single_row(pkg):
    nat = pkg._native
    ei, et = edge_list([(0, 0, 0), (0, 0, 1)], [(0, 0, 1), (0, 0, 0)])
    one = pkg.GraphCSR(1, 3, ei, et, torch.device(DEV), hub_threshold=0)
    assert one.live_rowptr is None and one.num_dead_slots == 0                          # N = 1: no slot can be dead
    lay = _Layer(pkg, one, 100, 200)
    assert torch.equal(lay.launch(None), lay.launch(False))
    with pytest.raises(nat.NativeError):
        lay.launch(True)
    csr, _, _ = _graph(pkg, 161, **_big_and_block(161))
    lay = _Layer(pkg, csr, 200, 200)
    want = lay.launch(False)
    b = 161 // 3
    for n in (b, b - 1, 160, 0):                                                        # the long live run, a dead run, the ends
        for tune in (GEN2, GEN3):
            assert torch.equal(lay.launch(True, tune, rng=(n, n + 1)), want[n:n + 1])
    nat.check_fused_status(DEV)


@pytest.mark.parametrize('share', [0.0, 1.0])
def test_dead_share_none_and_all(pkg, share):
    csr, _, _ = _graph(pkg, 161, share=share, seed=3)
    lay = _Layer(pkg, csr, 200, 200)
    if share == 0.0:
        assert csr.live_rowptr is None and csr.num_dead_slots == 0                      # nothing to leave out: no view is built
        assert torch.equal(lay.launch(None, GEN2), lay.launch(False, GEN2))
        return
    assert _dead_share(csr) == 1.0 and int(csr.live_rowptr.abs().sum()) == 0            # every run of the view is empty
    want = lay.launch(False, GEN2)
    assert torch.equal(lay.launch(True, GEN2), want) and torch.equal(lay.launch(True, GEN3), want)
    pkg._native.check_fused_status(DEV)


def test_relation_table_too_large_for_lds(pkg):
    """42 relation rows x 200 columns do not fit beside the stage images: the kernel instances that read the relation rows
    from memory (the FB15k-237 step's)."""
    csr, _, _ = _graph(pkg, 161, R=21, **_big_and_block(161))
    assert csr.num_dead_slots > 0 and (csr.num_rel_rows - 1) * 200 * 4 > 32 * 1024
    lay = _Layer(pkg, csr, 200, 200)
    want = lay.launch(False, GEN2)
    assert torch.equal(lay.launch(True, GEN2), want) and torch.equal(lay.launch(True, GEN3), want)
    pkg._native.check_fused_status(DEV)


def test_generation2_eighty_row_tiles(pkg):
    """20 000 rows: the lockstep kernel takes 80-row tiles at O = 200 (250 tiles on 256 CUs, against 313 of 64 rows)."""
    N = 20000
    csr, _, _ = _graph(pkg, N, share=0.3, seed=5, max_in=3)
    assert 0.1 < _dead_share(csr) < 0.6
    lay = _Layer(pkg, csr, 200, 200)
    want = lay.launch(False, GEN2)
    assert torch.isfinite(want).all()
    assert torch.equal(lay.launch(True, GEN2), want) and torch.equal(lay.launch(True, GEN3), want)
    pkg._native.check_fused_status(DEV)


def test_generation3_range_hubs_and_table_shard(pkg):
    """The elastic kernel through a destination range that is no multiple of 16 (nodes 7 .. 131 of 161), with hubs
    (hub_threshold = 4, hub_chunk = 4), one of them a hub whose slots are all dead, with the whole table and with the
    range's table shard (non-zero ee_sub: the view's row word is an absolute slot index) through dist.encode_layer_rows."""
    N, n0, n1 = 161, 7, 131
    csr, _, _ = _graph(pkg, N, hub_threshold=4, hub_chunk=4, seed=2, big=(N // 3, 40), dead_hub=(90, 9))
    hub, nrm = csr.hubinfo.cpu(), csr.norms().cpu()
    chunks = csr.chunks.cpu()
    assert csr.num_chunks > 8 and csr.num_dead_slots > 0
    for h in range(2):
        first, cnt = int(hub[h, 90, 0]), int(hub[h, 90, 1])
        assert cnt == 3 and bool((nrm[int(chunks[first, 0]):int(chunks[first + cnt - 1, 1])] == 0).all())   # a hub of dead slots
        assert int(hub[h, N // 3, 1]) == 10                                                                # ... and a live one
    lay = _Layer(pkg, csr, 200, 200)
    full = lay.launch(False, GEN2)
    assert torch.equal(lay.launch(True, GEN3), full) and torch.equal(lay.launch(True, GEN2), full)
    want = lay.launch(False, GEN3, rng=(n0, n1), table=lay.table)
    assert torch.equal(want, full[n0:n1])
    assert torch.equal(lay.launch(True, GEN3, rng=(n0, n1), table=lay.table), want)        # the range, whole table
    sub = csr.shard_ee_sub(n0, n1)
    assert sub[0] > 0 and sub[1] > 0
    assert torch.equal(lay.launch(True, GEN3, rng=(n0, n1)), want)                          # the range's table shard
    assert torch.equal(lay.launch(True, GEN2, rng=(n0, n1)), want)
    rows = pkg.dist.encode_layer_rows(lay.conv, csr, lay.x, lay.rel, csr.edge_table_shard(lay.table, n0, n1), n0, n1, sub)
    assert torch.equal(rows, want)                                                          # one rank's launch (the default: live)
    pkg._native.check_fused_status(DEV)


def test_encoder_replay_equals_itself_without_the_view(pkg, monkeypatch):
    """MGCN.encode in eval mode, two layers, N = 161, replayed from a captured graph: with the view and with
    MGCN_LIVE_SLOTS=0 (the switch is read at import: its module flag is flipped here, on a fresh model)."""
    N, R, D, O = 161, 3, 100, 200
    csr, ei, et = _graph(pkg, N, **_big_and_block(N))
    E = ei.size(1) // 2
    params = types.SimpleNamespace(gcn_in_dim=D, gcn_out_dim=O, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20,
                                   num_filter=8, kernel_size=7, bias=False, lbl_smooth=0.1, gcn_layers=2, cache_encoder=False)

    def encode(live):
        monkeypatch.setattr(pkg._native, 'LIVE_SLOTS', live)
        graph = pkg.Graph(edge_index=ei.clone(), edge_attr=torch.stack((et, torch.arange(2 * E))))
        graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
        graph.to(DEV)
        torch.manual_seed(0)
        model = pkg.MGCN(N, R, E, params)
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for layer in [model.conv1] + list(model.conv1_extra):
                layer.ent_bn.running_mean.copy_(torch.randn(O, generator=g) * 0.05)
                layer.ent_bn.running_var.copy_(torch.rand(O, generator=g) * 0.5 + 0.05)
        model.to(DEV).eval()
        with torch.no_grad():
            model.encode(graph)                                                             # capture
            ent, rel = model.encode(graph)                                                  # replay
        assert model._hip_graph is not None and graph.csr(2 * R + 1).num_dead_slots > 0
        return ent.clone(), rel.clone()
    ent1, rel1 = encode(True)
    ent0, rel0 = encode(False)
    assert torch.isfinite(ent1).all() and torch.equal(ent1, ent0) and torch.equal(rel1, rel0)
    pkg._native.check_fused_status(DEV)


def test_non_finite_rows_that_only_dead_slots_read(pkg):
    """The one place where the two launches differ, pinned: inf in a per-edge row that only a dead slot reads does not reach
    the live launch's output (the canonical launch gives NaN there: inf * 0); inf in a live slot's row still makes that
    destination's row non-finite and leaves every other row bit-identical."""
    N = 161
    csr, _, _ = _graph(pkg, N, **_big_and_block(N))
    lay = _Layer(pkg, csr, 200, 200)
    clean = lay.launch(True, GEN2)
    rp, lrec = csr.rowptr.cpu(), csr.live_rec.cpu()
    nrm = csr.norms().cpu()
    dead_dst = N // 3 - 1                                                                   # a dead run of the in-half
    dead_slot = int(rp[0, dead_dst])
    assert float(nrm[dead_slot]) == 0.0 and dead_slot not in set(lrec[:, 3].tolist())
    t = lay.table.clone()
    t[dead_slot, 5] = float('inf')
    for tune in (GEN2, GEN3):
        assert torch.equal(lay.launch(True, tune, table=t), clean)
        canon = lay.launch(False, tune, table=t)
        assert not torch.isfinite(canon[dead_dst]).all()
        keep = torch.ones(N, dtype=torch.bool, device=DEV)
        keep[dead_dst] = False
        assert torch.equal(canon[keep], clean[keep])
    live_dst = N // 3
    live_slot = int(rp[0, live_dst]) + 33                                                   # in the run's second record chunk
    assert float(nrm[live_slot]) != 0.0 and live_slot < int(rp[0, live_dst + 1])
    t = lay.table.clone()
    t[live_slot, 130] = float('inf')
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[live_dst] = False
    for tune in (GEN2, GEN3):
        got = lay.launch(True, tune, table=t)
        assert not torch.isfinite(got[live_dst]).all() and torch.equal(got[keep], clean[keep])
    pkg._native.check_fused_status(DEV)
