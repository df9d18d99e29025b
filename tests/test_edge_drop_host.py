"""CPU-only tests of the per-step record rewrite (include/mgcn_hip.h (19)): the host twin against the restatement
of tests/edge_drop_ref.py byte for byte, a kept slot's norm against the feeder run on the kept edge list alone, the edge cases of
the definition, the flags' restatement, the Python surface that needs no GPU, and the refusals."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from . import edge_drop_ref as er
from .conftest import ROOT

GRAPHS = er.graphs()
NODE = {'degree': 5, 'hub': 0, 'type': 3}      # the node that loses every edge in the 'node' cases
NEW = ('mgcn_edge_drop_table_host', 'mgcn_edge_drop_records', 'mgcn_edge_drop_records_dev', 'mgcn_edge_drop_records_host',
       'mgcn_edge_flags_from_queries')

_built = {}


def layout(pkg, name):
    if name not in _built:
        N, R, ei, et, thr, chunk = GRAPHS[name]
        host = pkg._native.csr_build_host(N, 2 * R + 1, ei, et, hub_threshold=thr, hub_chunk=chunk)
        longest = pkg._native.max_run_host(host['rowptr'], host['hubinfo'], host['chunks'], host['num_chunks'])
        _built[name] = (host, pkg._native.edge_drop_table_host(longest + 1), longest)
    return _built[name]


def test_exports_and_header(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    handle = ctypes.CDLL(pkg._native.LIB_PATH)
    for n in NEW:
        assert n in pkg._native.EXPORTS and re.search(r'\bint %s\(' % n, header) and hasattr(handle, n), n
    assert pkg._native.ABI_VERSION == 4 and pkg._native.EDGE_DROP_SITE == 0x3000 == er.SITE


def test_graphs_cover_the_cases(pkg):
    for name, (N, R, ei, et, thr, chunk) in GRAPHS.items():
        assert (ei.size(1) // 2) % 64 != 0 and 12 <= N <= 64, name
    N, R, ei, et, _, _ = GRAPHS['degree']
    E = ei.size(1) // 2
    trip = list(zip(ei[0, :E].tolist(), et[:E].tolist(), ei[1, :E].tolist()))
    assert any(s == o for s, _, o in trip) and len(set(trip)) < len(trip)        # self edges, duplicate triples
    host, _, longest = layout(pkg, 'hub')
    assert host['num_chunks'] > 0 and longest == 2 * (16 * 16 + 1) - 1          # the longest hub segment (257 chunks, the last ragged)
    assert bool((host['hubinfo'][0, :, 1] > 0).any()) and bool((host['hubinfo'][1, :, 1] > 0).any())


def test_table_is_the_feeders_expression(pkg):
    t = pkg._native.edge_drop_table_host(600).numpy()
    d = np.arange(1, 600, dtype=np.float32)
    assert t[0] == 0.0 and not np.signbit(t[0])
    assert np.array_equal(t[1:].view(np.int32), (np.float32(1.0) / np.sqrt(d)).astype(np.float32).view(np.int32))
    for bad in (0, -1, 1 << 31):
        assert pkg._native.lib().mgcn_edge_drop_table_host(bad, torch.empty(1).data_ptr()) == 1
    assert pkg._native.lib().mgcn_edge_drop_table_host(4, None) == 1


@pytest.mark.parametrize('case', er.DROP_CASES, ids=[c[0] for c in er.DROP_CASES])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_host_twin_equals_restatement(pkg, name, case):
    _, p, kind = case
    N, R, ei, et, _, _ = GRAPHS[name]
    E = ei.size(1) // 2
    host, table, _ = layout(pkg, name)
    forced = er.forced_of(kind, ei, NODE[name])
    key = pkg._native.dropout_key(er.SEED, er.STEP, er.SITE)
    got, cinv = pkg._native.edge_drop_records_host(host, table, key, p, None if forced is None else torch.from_numpy(forced))
    kept = er.kept_edges(er.SEED, er.STEP, p, E, forced)
    norms = er.edge_norms(N, ei, kept, table.numpy())
    want = er.records(host, norms)
    assert np.array_equal(got.numpy(), want)                       # byte for byte: the norm column holds f32 bits
    f = got[:, 2].contiguous().view(torch.float32)
    assert bool(torch.isfinite(f).all()) and bool((f >= 0).all()) and not bool(torch.signbit(f).any())
    assert bool(torch.isfinite(cinv).all())
    dropped = ~kept[host['perm'].numpy() % E]
    assert bool((got[:, 2].numpy()[dropped] == 0).all())            # +0.0f, all 32 bits
    if p >= 1:
        assert bool((got[:, 2] == 0).all())
    if p == 0.0 and kind is None:
        assert kept.all() and torch.equal(got, host['rec'])         # what the wrapper returns without a launch
    if kind == 'node':                                              # a node that lost all its edges: norm 0, degree entries 0
        n = NODE[name]
        touch = (host['rec'][:, 0] == n) | ((host['slot_dst'] & 0x7fffffff) == n)
        assert int(touch.sum()) > 0 and bool((got[touch, 2] == 0).all()) and bool((cinv[:, n] == 0).all())
    # the keep bits are byte u of the [E, 1] mask of (12)
    if 0 < p < 1 and kind is None:
        assert np.array_equal(pkg._native.dropout_mask_host(E, 1, key, 0, p).numpy()[:, 0].astype(bool), kept)


@pytest.mark.parametrize('case', [c for c in er.DROP_CASES if c[1] < 1], ids=[c[0] for c in er.DROP_CASES if c[1] < 1])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_kept_norms_are_the_feeders_on_the_kept_list(pkg, name, case):
    _, p, kind = case
    N, R, ei, et, _, _ = GRAPHS[name]
    E = ei.size(1) // 2
    host, table, _ = layout(pkg, name)
    forced = er.forced_of(kind, ei, NODE[name])
    key = pkg._native.dropout_key(er.SEED, er.STEP, er.SITE)
    got, _ = pkg._native.edge_drop_records_host(host, table, key, p, None if forced is None else torch.from_numpy(forced))
    kept = er.kept_edges(er.SEED, er.STEP, p, E, forced)
    assert 0 < int(kept.sum())
    ei_k, et_k, ids = er.kept_list(ei, et, kept)
    sub = pkg._native.csr_build_host(N, 2 * R + 1, ei_k, et_k, hub_threshold=0)
    by_eid = np.zeros(2 * E, dtype=np.int32)
    by_eid[ids.numpy()[sub['rec'][:, 3].numpy()]] = sub['rec'][:, 2].numpy()
    mine = np.zeros(2 * E, dtype=np.int32)
    mine[got[:, 3].numpy()] = got[:, 2].numpy()
    assert np.array_equal(mine[ids.numpy()], by_eid[ids.numpy()])   # bit for bit, every kept edge
    # and against the float64 norms of the kept sub-graph they stay inside what aggregate_ref's bar budgets for the norm: its
    # TERM_ROUNDINGS minus the three product roundings of a term (kept degrees such as (7, 7) reach 2.5003 u, past the 2.5 u the
    # canonical graphs show, inside the 3 u of the budget)
    n64 = torch.cat(er.norm64_kept(N, ei, kept)).numpy()
    f = mine.view(np.float32).astype(np.float64)
    assert np.all(np.abs(f - n64) <= (er.ar.TERM_ROUNDINGS - 3) * er.ar.U * n64)
    assert np.all(f[~np.concatenate((kept, kept))] == 0)


def test_hub_partly_dropped(pkg):
    N, R, ei, et, _, _ = GRAPHS['hub']
    E = ei.size(1) // 2
    host, table, _ = layout(pkg, 'hub')
    kept = er.kept_edges(er.SEED, er.STEP, 0.5, E)
    ch, partly = host['chunks'][:host['num_chunks']].numpy(), 0
    eid = host['rec'][:, 3].numpy()
    for b, e, _, _ in ch:
        k = kept[eid[b:e] % E]
        partly += int(k.any() and not k.all())
    assert partly > 0      # the 'p05' case above walks chunks with kept and dropped slots side by side


def test_flags_restatement(pkg):
    for name, (N, R, ei, et, _, _) in GRAPHS.items():
        E = ei.size(1) // 2
        csr = pkg.graph.GraphCSR(N, 2 * R + 1, ei, et, torch.device('cpu'), hub_threshold=GRAPHS[name][4] or None, hub_chunk=GRAPHS[name][5])
        st = csr.edge_drop_state()
        assert st is csr.edge_drop_state() and st.table.numel() == st.max_run + 1
        ek = st.ekeys.tolist()
        assert ek == sorted(er.edge_keys(ei, et, R)) and st.eund.dtype == torch.int32 and st.ekeys.dtype == torch.int64
        for label, qs in er.query_cases(ei, et, R, N).items():
            want = er.flags(ei, et, R, qs)
            assert np.array_equal(er.flags_by_bisect(ek, st.eund.tolist(), E, qs), want), (name, label)
            if label in ('none', 'below_above', 'empty'):
                assert not want.any()
            if label == 'inverse':
                assert want.any()
    # by hand: edges 0: (0, r0, 1), 1: (1, r0, 2), 2: (0, r1, 2); R = 2, keys s * 4 + r
    ei = torch.tensor([[0, 1, 0, 1, 2, 2], [1, 2, 2, 0, 1, 0]])
    et = torch.tensor([0, 0, 1, 2, 2, 3])
    assert er.flags(ei, et, 2, [0 * 4 + 0]).tolist() == [1, 0, 0]            # (0, r0, ?)
    assert er.flags(ei, et, 2, [2 * 4 + 2]).tolist() == [0, 1, 0]            # (2, r0 + R, ?): the inverse of edge 1
    assert er.flags(ei, et, 2, [2 * 4 + 3, 0 * 4 + 1]).tolist() == [0, 0, 1]  # edge 2 from both ends
    assert er.flags(ei, et, 2, [1 * 4 + 1, 99, -1]).tolist() == [0, 0, 0]


def test_with_records_shares_everything_but_rec(pkg):
    N, R, ei, et, thr, chunk = GRAPHS['hub']
    csr = pkg.graph.GraphCSR(N, 2 * R + 1, ei, et, torch.device('cpu'), hub_threshold=thr, hub_chunk=chunk)
    rec = csr.rec.clone()
    view = csr.with_records(rec)
    assert view.rec is rec and view.live_rowptr is None and view.live_rec is None and csr.rec is not rec
    for k in ('rowptr', 'perm', 'hubinfo', 'chunks', 'slot_dst', 'mirror', 'typeptr', 'typeslots'):
        assert getattr(view, k) is getattr(csr, k), k
    assert view._shard_cache is csr._shard_cache and view._hub_partials is csr._hub_partials
    assert view.num_chunks == csr.num_chunks and view.chunk_range(0, N) == csr.chunk_range(0, N)
    for bad in (rec[:-1], rec.to(torch.int64), rec.t()):
        with pytest.raises(pkg._native.NativeError):
            csr.with_records(bad)


def test_refusals(pkg):
    nat = pkg._native
    N, R, ei, et, _, _ = GRAPHS['type']
    E = ei.size(1) // 2
    dev = torch.device('cpu')
    # a list whose second half is not the first reversed, and a graph without the backward index
    skew = ei.clone()
    skew[1, E] = (skew[1, E] + 1) % N
    for csr in (pkg.graph.GraphCSR(N, 2 * R + 1, skew, et, dev), pkg.graph.GraphCSR(N, 2 * R + 1, ei, et, dev, with_backward=False)):
        with pytest.raises(pkg._native.NativeError):
            csr.edge_drop_state()
        with pytest.raises(pkg._native.NativeError):
            nat.edge_drop_records(csr, None, 1, 0.5)
    host, table, longest = layout(pkg, 'type')
    with pytest.raises(pkg._native.NativeError, match='table'):            # T shorter than the longest run
        nat.edge_drop_records_host(host, table[:longest].contiguous(), 1, 0.5)
    with pytest.raises(pkg._native.NativeError):
        nat.edge_drop_records_host(host, table, 1, 0.5, torch.zeros(E + 1, dtype=torch.uint8))
    # the device entries refuse before any launch: null pointers, sizes outside int32 slots, the table, a misaligned step word
    lib = nat.lib()
    buf = torch.zeros(64, dtype=torch.int32)
    ptr = buf.data_ptr()
    assert ptr % 16 == 0
    ok = [N, E, ptr, ptr, ptr, None, None, 0, ptr, longest + 1, longest, None, 1, 7, ptr, ptr + 16, None]
    def call(i, v):
        a = list(ok)
        a[i] = v
        return lib.mgcn_edge_drop_records(*a)
    for i in (2, 3, 4, 8, 14, 15):
        assert call(i, None) == 1, i
    assert call(0, 1 << 31) == 1 and call(1, 1 << 30) == 1 and call(0, -1) == 1
    assert call(9, longest) == 1                                     # table_len <= max_run
    assert call(15, ptr) == 1 and call(15, ptr + 4) == 1             # rec_out == rec, misaligned records
    assert call(7, 3) == 1                                           # chunks without hubinfo / chunks
    dev_ok = ok[:12] + [ptr, nat.EDGE_DROP_SITE] + ok[13:]
    for word in (None, ptr + 4):
        a = list(dev_ok)
        a[12] = word
        assert lib.mgcn_edge_drop_records_dev(*a) == 1
    assert b'step_key' in lib.mgcn_last_error()
    assert lib.mgcn_edge_flags_from_queries(-1, ptr, E, ptr, ptr, ptr, None) == 1
    assert lib.mgcn_edge_flags_from_queries(1, None, E, ptr, ptr, ptr, None) == 1
    assert lib.mgcn_edge_flags_from_queries(1, ptr, E, ptr, ptr, None, None) == 1
    assert lib.mgcn_edge_flags_from_queries(1, ptr, 1 << 30, ptr, ptr, ptr, None) == 1


def test_switches(pkg, monkeypatch):
    sw = pkg.model.edge_drop_switches
    monkeypatch.delenv('MGCN_EDGE_DROP', raising=False)
    monkeypatch.delenv('MGCN_EDGE_DROP_QUERIES', raising=False)
    assert sw(types.SimpleNamespace()) == (0.0, False)
    assert sw(types.SimpleNamespace(edge_drop=0.2, edge_drop_queries=True)) == (0.2, True)
    monkeypatch.setenv('MGCN_EDGE_DROP', '0.4')
    monkeypatch.setenv('MGCN_EDGE_DROP_QUERIES', '0')
    assert sw(types.SimpleNamespace(edge_drop=0.2, edge_drop_queries=True)) == (0.4, False)
    monkeypatch.setenv('MGCN_EDGE_DROP_QUERIES', '1')
    assert sw(types.SimpleNamespace()) == (0.4, True)
