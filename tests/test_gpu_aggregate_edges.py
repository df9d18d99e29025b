"""csrc/aggregate.hip held to float64 at every geometry and edge (`-m gpu`): the forward aggregation, the hub pre-pass with
its two-level fold, the three gradient paths (fused and separate kernels) and the destination-range variants, each
instantiated for VEC in {4, 1} x CPL in {1, 2, 4, 8}. References, graphs, grids and the bar come from
tests/aggregate_ref.py (checked on the CPU by tests/test_aggregate_ref_host.py): every element is compared with a float64
sum built from the edge list alone, against (n + 6) u mag of ITS terms; elements without terms must be exactly 0.0.
Every output is a window of a NaN-filled buffer whose guard rows / columns must still be NaN afterwards. Every check prints
`RATIO what worst-error / bar` (pytest -s) before it asserts."""
import pytest
import torch

from . import aggregate_ref as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD_ROWS = 2
NAN = float('nan')

_ids = lambda cases: [A.case_id(c) for c in cases]
_graphs = {}


def _graph(pkg, key, thr=0, chunk=64):
    """(N, R, edge_index, edge_type on the device, GraphCSR), built once per module."""
    k = (key, thr, chunk)
    if k not in _graphs:
        name, arg = key
        if name == 'degree':
            gr = A.degree_profile(arg)
        elif name == 'hub':
            gr = A.hub_profile(thr, chunk)
        elif name == 'type':
            gr = A.type_profile(small=arg)
        elif name == 'switch':
            gr = A.switch_pair()[arg]
        else:
            gr = A.long_type()
        N, R, ei, et = gr
        csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, DEV, hub_threshold=thr, hub_chunk=chunk)
        assert (csr.num_chunks > 0) == (thr > 0)
        _graphs[k] = (N, R, ei.to(DEV), et.to(DEV), csr)
    return _graphs[k]


def _inputs(label, G, D):
    N, R, ei, et, csr = G
    return A.Inputs(*(t.to(DEV) for t in A.make_inputs(label, N, 2 * R + 1, ei.size(1), D)))


def _report(what, got, ref):
    ratio, bad_zero, _ = A.worst_ratio(got, ref)
    print('RATIO %s %.4f (elements without terms that are not 0.0: %d)' % (what, ratio, bad_zero))
    A.check(got, ref, what)


# ----------------------------------------------------------------------------------------------------------------
# operand layouts
def _pad_view(t, left, right, fill=NAN):
    """`t` as a column window of a wider NaN-filled buffer: a read outside the window poisons the result."""
    buf = torch.full((t.size(0), left + t.size(1) + right), fill, dtype=t.dtype, device=t.device)
    view = buf[:, left:left + t.size(1)]
    view.copy_(t)
    return view


def _place_x(x, layout, strided=False):
    if layout == A.XCOL:
        return _pad_view(x, 1, 7)                  # base pointer one float off, row stride D + 8
    if layout == A.XSTRIDE:
        return _pad_view(x, 0, 1)                  # row stride D + 1
    return _pad_view(x, 0, 4) if strided else x.contiguous()


def _place_g(g, layout):
    return _pad_view(g, 0, 2) if layout == A.GLD else _pad_view(g, 0, 8)      # ldg = 2D + 2 / an aligned ldg > 2D


def _is_aligned(*ts):
    return all(t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.size(0) < 2 or t.stride(0) % 4 == 0) for t in ts if t is not None)


class Window(object):
    """rows x cols window of a NaN-filled buffer with guard rows above and below and guard columns on both sides."""

    def __init__(self, rows, cols, left=4, right=4):
        self.raw = torch.full((rows + 2 * GUARD_ROWS, left + cols + right), NAN, dtype=torch.float32, device=DEV)
        self.view = self.raw[GUARD_ROWS:GUARD_ROWS + rows, left:left + cols]
        self.box = (GUARD_ROWS, GUARD_ROWS + rows, left, left + cols)

    def check(self, what, written_cols=None):
        r0, r1, c0, c1 = self.box
        if written_cols is not None:
            c1 = c0 + written_cols
        outside = torch.ones_like(self.raw, dtype=torch.bool)
        outside[r0:r1, c0:c1] = False
        assert bool(torch.isnan(self.raw[outside]).all()), '%s: a guard row / column was written' % what
        assert bool(torch.isfinite(self.raw[r0:r1, c0:c1]).all()), '%s: an element inside the window was not written' % what

    def untouched(self):
        return bool(torch.isnan(self.raw).all())


def _out_window(rows, D, layout):
    # 3D columns; a misaligned column window starts 3 floats in and has an odd row stride
    return Window(rows, 3 * D, 3, 2) if layout == A.OUTWIN else Window(rows, 3 * D, 4, 4 + (-3 * D) % 4)


def _bwd_windows(csr, D, rows_gee=None):
    """(gx, gee, grel) as contiguous row windows of NaN buffers."""
    E2 = 2 * csr.num_edges_half if rows_gee is None else rows_gee
    return [Window(r, D, 0, 0) for r in (csr.num_nodes, E2, csr.num_rel_rows)]


def _hub_counters_zero(csr, D):
    bufs = [(k, v[0]) for k, v in csr.__dict__.get('_hub_partials', {}).items() if k[0] == D]
    assert bufs or csr.num_chunks == 0
    torch.cuda.synchronize()
    for (d, c0, c1, _), buf in bufs:
        counters = buf[(c1 - c0) * D:].view(torch.int32)
        assert counters.numel() == 2 * (c1 - c0) and int(counters.abs().max()) == 0, 'hub arrival counters left non-zero'


# ----------------------------------------------------------------------------------------------------------------
# forward
def _forward_variants(inp, csr):
    """(name, ee operand, slot order?, ee of the reference, loop_edge?, loop_rel separate?)"""
    ee_slot = inp.ee.index_select(0, csr.perm).contiguous()
    return [('slot-order/mode3', ee_slot, True, inp.ee, True, False),
            ('edge-id-order/mode3/loop_rel-apart', inp.ee, False, inp.ee, True, True),
            ('no-table/mode2', None, True, None, False, False)]


def _launch_forward(pkg, G, inp, case, variant, node_range=None, full=None):
    """One guarded forward launch, checked against float64; returns the window's values. `node_range`: those rows only, from
    the range's own table shard, with out_row0 = the range's first node."""
    N, R, ei, et, csr = G
    nat = pkg._native
    D = case.d
    name, ee, slot_order, ee_ref, with_loop_edge, loop_rel_apart = variant
    n0, n1 = (0, N) if node_range is None else node_range
    x = _place_x(inp.x, case.layout)
    loop_rel = inp.rel[-1].clone() if loop_rel_apart else None
    rel = inp.rel[:-1] if loop_rel_apart else inp.rel
    win = _out_window(n1 - n0, D, case.layout)
    cols = (3 if with_loop_edge else 2) * D
    out = win.view[:, :cols]
    if case.layout == A.PLAIN and D % 4 == 0:
        assert _is_aligned(x, rel, ee, inp.loop_edge, out, loop_rel)
    kw = {}
    if node_range is not None:
        kw = dict(node_range=(n0, n1), out_row0=n0)
        if ee is not None:
            assert slot_order
            ee, kw['ee_sub'] = csr.edge_table_shard(ee, n0, n1), csr.shard_ee_sub(n0, n1)
    what = 'fwd %s %s [%d, %d)' % (A.case_id(case), name, n0, n1)
    nat.aggregate_fwd(csr, x, rel, ee, slot_order, inp.loop_edge if with_loop_edge else None, out, loop_rel=loop_rel, **kw)
    torch.cuda.synchronize()
    win.check(what, cols)
    got = out.clone()
    _hub_counters_zero(csr, D)
    out.fill_(NAN)
    nat.aggregate_fwd(csr, x, rel, ee, slot_order, inp.loop_edge if with_loop_edge else None, out, loop_rel=loop_rel, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, got), '%s: two launches differ' % what
    _hub_counters_zero(csr, D)
    ref = A.ref_forward(N, ei, et, inp.x, inp.rel, ee_ref)
    _report(what, got[:, :2 * D], A.slice_ref(ref, slice(n0, n1)))
    if with_loop_edge:
        A.check_loop(got[:, 2 * D:], A.ref_loop(inp.x, inp.rel, inp.loop_edge)[n0:n1], what)
    if full is not None:
        assert torch.equal(got, full[n0:n1]), '%s: the range differs from the full launch' % what
    return got


def _degree_graph(pkg, gs, hubs):
    """degree_profile(gs) with hubs off, or with every run above 5 slots cut into chunks of 2 gs + 1 slots: a full record
    window plus one slot in the pre-pass walks (rolling prefetch), and 4 gs + 1 = a chunk of 2 gs + 1 and one of 2 gs."""
    return _graph(pkg, ('degree', gs), thr=5, chunk=2 * gs + 1) if hubs else _graph(pkg, ('degree', gs))


@pytest.mark.parametrize('case', A.FAMILY_CASES['fwd'], ids=_ids(A.FAMILY_CASES['fwd']))
@pytest.mark.parametrize('hubs', [False, True], ids=['hubs-off', 'runs-as-hub-chunks'])
def test_forward_degree_profile(pkg, case, hubs):
    """agg_fwd_kernel at every width of the grid: run lengths on the batch and record-window edges of THAT width's lane
    group, hubs off; per-edge table in slot order / edge-id order / absent, two or three modes, the self-loop row apart.
    Then the same runs as hub chunks of a window and one slot (agg_hub_kernel's walk)."""
    vec, cpl, gs = A.case_geometry(case)
    G = _degree_graph(pkg, gs, hubs)
    inp = _inputs('fwd-%s-%s' % (A.case_id(case), hubs), G, case.d)
    for variant in _forward_variants(inp, G[4]):
        _launch_forward(pkg, G, inp, case, variant)


@pytest.mark.parametrize('case', A.FAMILY_CASES['hub_prepass'], ids=_ids(A.FAMILY_CASES['hub_prepass']))
def test_forward_hub_profile(pkg, case):
    """agg_hub_kernel and its in-launch fold: chunk counts 1, 2, 15, 16, 17, 32, 33 and 257 (17 spans), hubs on the first and
    the last node; the arrival counters are zero after every launch."""
    G = _graph(pkg, ('hub', None), thr=1, chunk=2)
    assert G[4].num_chunks > 257
    inp = _inputs('hub-' + A.case_id(case), G, case.d)
    for variant in _forward_variants(inp, G[4]):
        _launch_forward(pkg, G, inp, case, variant)


def _ranges(csr, N, extra):
    b = csr.balanced_bounds(3, align=1)
    return [(b[i], b[i + 1]) for i in range(3)] + extra


@pytest.mark.parametrize('case', A.FAMILY_CASES['hub_prepass'], ids=_ids(A.FAMILY_CASES['hub_prepass']))
def test_forward_destination_ranges(pkg, case):
    """node_range + out_row0 + the range's own table shard: three balanced ranges and hand-picked ones (empty, one node, a
    range that starts / ends on a hub, the last node alone = the 257-chunk hub), each against float64 directly and bit for
    bit against the full launch."""
    G = _graph(pkg, ('hub', None), thr=1, chunk=2)
    N, csr = G[0], G[4]
    inp = _inputs('range-' + A.case_id(case), G, case.d)
    slot_variant, _, noee_variant = _forward_variants(inp, csr)
    full = _launch_forward(pkg, G, inp, case, slot_variant)
    full_noee = _launch_forward(pkg, G, inp, case, noee_variant)
    for rng in _ranges(csr, N, [(9, 9), (20, 21), (0, 3), (3, 7), (6, N - 1), (N - 1, N)]):
        _launch_forward(pkg, G, inp, case, slot_variant, node_range=rng, full=full)
    _launch_forward(pkg, G, inp, case, noee_variant, node_range=(5, N), full=full_noee)
    # ... and ordinary runs only (hubs off)
    G = _graph(pkg, ('degree', A.case_geometry(case)[2]))
    inp = _inputs('range-degree-' + A.case_id(case), G, case.d)
    slot_variant = _forward_variants(inp, G[4])[0]
    full = _launch_forward(pkg, G, inp, case, slot_variant)
    for rng in _ranges(G[4], G[0], [(0, 1), (9, 10), (G[0] - 1, G[0])]):
        _launch_forward(pkg, G, inp, case, slot_variant, node_range=rng, full=full)


@pytest.mark.parametrize('case', A.SWITCH_CASES, ids=_ids(A.SWITCH_CASES))
@pytest.mark.parametrize('side', [0, 1], ids=['E=4N-1', 'E=4N'])
def test_forward_at_the_short_run_switch(pkg, case, side):
    """E < 4N picks agg_fwd_kernel<4,1,2> over <4,1,4>: the same node set one edge below and exactly at the switch."""
    G = _graph(pkg, ('switch', side))
    assert (G[4].num_edges_half < 4 * G[0]) == (side == 0)
    inp = _inputs('switch%d-%s' % (side, A.case_id(case)), G, case.d)
    for variant in _forward_variants(inp, G[4]):
        _launch_forward(pkg, G, inp, case, variant)


# ----------------------------------------------------------------------------------------------------------------
# backward
def _check_backward(pkg, G, case, tag):
    """Every `want_*` combination that picks a kernel, each against float64 through guarded outputs; the fused pass and the
    separate kernels give the same bits."""
    N, R, ei, et, csr = G
    nat = pkg._native
    D = case.d
    inp = _inputs('%s-%s' % (tag, A.case_id(case)), G, D)
    x = _place_x(inp.x, case.layout, strided=True)
    g = _place_g(inp.g, case.layout)
    ee = inp.ee.index_select(0, csr.perm).contiguous()                      # slot order
    if case.layout == A.PLAIN and D % 4 == 0:
        assert _is_aligned(x, g, ee, inp.rel)
    refs = {True: A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee, inp.g), False: A.ref_grads(N, ei, et, inp.x, inp.rel, None, inp.g)}

    def run(with_ee, want_gx, want_gee, want_grel, kernels):
        wins = _bwd_windows(csr, D)
        assert D % 4 or _is_aligned(*(w.view for w in wins))
        want = (want_gx, want_gee and with_ee, want_grel)
        outs = tuple(w.view if k else None for w, k in zip(wins, want))
        got = nat.aggregate_bwd(csr, x, inp.rel, ee if with_ee else None, g, want_gx=want_gx, want_gee=want_gee, want_grel=want_grel,
                                out=outs)
        torch.cuda.synchronize()
        what = 'bwd %s %s %s' % (tag, A.case_id(case), kernels)
        gx_ref, gee_ref, grel_ref = refs[with_ee]
        gee_ref = A.select_rows(gee_ref, csr.perm)                           # edge-id order -> slot order
        for w, k, t, ref, name in zip(wins, want, got, (gx_ref, gee_ref, grel_ref), ('gx', 'gee', 'grel')):
            if not k:
                assert t is None and w.untouched(), '%s: %s was not asked for' % (what, name)
                continue
            assert t.data_ptr() == w.view.data_ptr()
            w.check('%s %s' % (what, name))
            _report('%s %s' % (what, name), t, ref)
        return [None if t is None else t.clone() for t in got]

    fused = run(True, True, True, True, 'gx+gee_grel_fused+grel_final')
    gee_alone = run(True, False, True, False, 'gee_alone')
    grel_alone = run(True, False, False, True, 'grel_partial_ee+grel_final')
    run(False, False, False, True, 'grel_partial_noee+grel_final')
    gx_alone = run(True, True, False, False, 'gx')
    run(False, True, False, False, 'gx_noee')
    assert torch.equal(fused[1], gee_alone[1]), 'fused gee differs from agg_bwd_gee_kernel'
    assert torch.equal(fused[2], grel_alone[2]), 'fused grel differs from agg_bwd_grel_partial_kernel'
    assert torch.equal(fused[0], gx_alone[0])
    again = nat.aggregate_bwd(csr, x, inp.rel, ee, g)                        # the wrapper's own allocations (out=None)
    assert all(torch.equal(a, b) for a, b in zip(again, fused))


@pytest.mark.parametrize('case', A.FAMILY_CASES['gee_grel_fused'], ids=_ids(A.FAMILY_CASES['gee_grel_fused']))
@pytest.mark.parametrize('small', [False, True], ids=['E>=4N', '2E<16'])
def test_backward_type_profile(pkg, case, small):
    """Relation slot runs of 0, 1, 15, 16, 17, 33 slots against kTypeChunk = 16, at every width; the graph of 2E < 16 slots is
    also the short-run gx kernel's (E < 4N), the larger one the long-run kernel's."""
    G = _graph(pkg, ('type', small))
    assert (G[4].num_edges_half < 4 * G[0]) == small
    _check_backward(pkg, G, case, 'type-small' if small else 'type')


@pytest.mark.parametrize('case', A.FAMILY_CASES['gx_hub_fold'], ids=_ids(A.FAMILY_CASES['gx_hub_fold']))
@pytest.mark.parametrize('hubs', [False, True], ids=['hubs-off', 'runs-as-hub-chunks'])
def test_backward_degree_profile(pkg, case, hubs):
    """gx_walk over runs of 0 .. 4 gs + 1 slots (batches of 4, 2 or 1), then over the same runs as hub chunks."""
    G = _degree_graph(pkg, A.case_geometry(case)[2], hubs)
    _check_backward(pkg, G, case, 'degree-hubs' if hubs else 'degree')


@pytest.mark.parametrize('case', A.FAMILY_CASES['gx_hub_fold'], ids=_ids(A.FAMILY_CASES['gx_hub_fold']))
def test_backward_hub_profile(pkg, case):
    """agg_bwd_gx_hub_kernel and the two agg_hub_fold_kernel launches: 1 .. 257 chunks per hub, hubs in one half only."""
    G = _graph(pkg, ('hub', None), thr=1, chunk=2)
    _check_backward(pkg, G, case, 'hub')


@pytest.mark.parametrize('case', A.SWITCH_CASES, ids=_ids(A.SWITCH_CASES))
@pytest.mark.parametrize('side', [0, 1], ids=['E=4N-1', 'E=4N'])
def test_backward_at_the_short_run_switch(pkg, case, side):
    G = _graph(pkg, ('switch', side))
    assert (G[4].num_edges_half < 4 * G[0]) == (side == 0)
    _check_backward(pkg, G, case, 'switch%d' % side)


def test_backward_long_type(pkg):
    """More than 64 * 16 * 16 slots of one relation at D = 4: the stage-2 loop of agg_bwd_grel_final_kernel runs twice."""
    _check_backward(pkg, _graph(pkg, ('long', None)), A.ALIGNED_CASES[0], 'long-type')


# ----------------------------------------------------------------------------------------------------------------
# destination-range backward
def _check_shard_backward(pkg, G, case, tag, ranges, whole=True):
    N, R, ei, et, csr = G
    nat = pkg._native
    D = case.d
    inp = _inputs('%s-%s' % (tag, A.case_id(case)), G, D)
    x = _place_x(inp.x, case.layout, strided=True)
    g = _place_g(inp.g, case.layout)
    ee = inp.ee.index_select(0, csr.perm).contiguous()
    E2 = ee.size(0)
    gee_ref = A.select_rows(A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee, inp.g)[1], csr.perm)
    slot_ids = torch.arange(E2, device=DEV).unsqueeze(1)
    gx_sum = torch.zeros((N, D), dtype=torch.float64, device=DEV)
    grel_sum = torch.zeros((2 * R + 1, D), dtype=torch.float64, device=DEV)
    last = None
    for n0, n1 in ranges:
        slots = csr.edge_table_shard(slot_ids, n0, n1).reshape(-1)           # slot of every shard row
        assert slots.numel() == sum(csr.shard_slot_counts(n0, n1))
        wins = _bwd_windows(csr, D, rows_gee=slots.numel())
        got = nat.aggregate_bwd_shard(csr, x, inp.rel, csr.edge_table_shard(ee, n0, n1), g[n0:n1], (n0, n1),
                                      out=tuple(w.view for w in wins))
        torch.cuda.synchronize()
        what = 'shard bwd %s %s [%d, %d)' % (tag, A.case_id(case), n0, n1)
        for w, name in zip(wins, ('gx', 'gee', 'grel')):
            w.check('%s %s' % (what, name))
        dst = ei[1]
        mine = (dst >= n0) & (dst < n1)                                      # the range's edges (both halves)
        gx_ref, _, grel_ref = A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee, inp.g, edge_mask=mine)
        _report(what + ' gx', got[0], gx_ref)
        _report(what + ' gee', got[1], A.select_rows(gee_ref, slots))
        _report(what + ' grel', got[2], grel_ref)
        if slots.numel() == 0:
            assert float(got[0].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        gx_sum += got[0].double()
        grel_sum += got[2].double()
        last = got
    if whole:       # the ranges partition the graph: the float64 sums over the ranks, same n and mag, same bar
        gx_ref, _, grel_ref = A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee, inp.g)
        _report('shard bwd %s %s sum of gx over %d ranks' % (tag, A.case_id(case), len(ranges)), gx_sum, gx_ref)
        _report('shard bwd %s %s sum of grel over %d ranks' % (tag, A.case_id(case), len(ranges)), grel_sum, grel_ref)
    if len(ranges) == 1 and ranges[0] == (0, N):
        one = nat.aggregate_bwd(csr, x, inp.rel, ee, g)
        shard_rows = csr.edge_table_shard(one[1], 0, N)
        assert torch.equal(last[0], one[0]) and torch.equal(last[1], shard_rows) and torch.equal(last[2], one[2])


@pytest.mark.parametrize('case', A.FAMILY_CASES['shard_gx_hub'], ids=_ids(A.FAMILY_CASES['shard_gx_hub']))
@pytest.mark.parametrize('world', [1, 3])
@pytest.mark.parametrize('graph', ['hub', 'type'])
def test_shard_backward(pkg, case, world, graph):
    """mgcn_aggregate_bwd_shard per rank against float64 (not only against the unsplit kernels, with which it shares its
    walks and folds): gee rows, each rank's gx / grel share, and their float64 sums over the ranks."""
    G = _graph(pkg, ('hub', None), thr=1, chunk=2) if graph == 'hub' else _graph(pkg, ('type', False))
    b = G[4].balanced_bounds(world, align=1)
    _check_shard_backward(pkg, G, case, '%s-W%d' % (graph, world), [(b[i], b[i + 1]) for i in range(world)])


@pytest.mark.parametrize('case', A.FAMILY_CASES['shard_gx'], ids=_ids(A.FAMILY_CASES['shard_gx']))
def test_shard_backward_of_a_range_without_slots(pkg, case):
    """An isolated node's range and an empty range own no slot: gx and grel are exact zeros, gee has no rows."""
    G = _graph(pkg, ('degree', A.case_geometry(case)[2]))
    assert sum(G[4].shard_slot_counts(0, 1)) == 0
    _check_shard_backward(pkg, G, case, 'degree-empty', [(0, 1), (5, 5), (0, 12)], whole=False)


# ----------------------------------------------------------------------------------------------------------------
# refusals
@pytest.mark.parametrize('case', A.REFUSED_CASES, ids=_ids(A.REFUSED_CASES))
def test_refused_widths_write_nothing(pkg, case):
    """More than 8 column chunks per lane: NativeError from every entry point, NaN-prefilled outputs untouched."""
    nat = pkg._native
    assert A.case_geometry(case) is None
    G = _graph(pkg, ('type', True))
    N, R, ei, et, csr = G
    D = case.d
    inp = _inputs('refused-' + A.case_id(case), G, D)
    ee = inp.ee.index_select(0, csr.perm).contiguous()
    x = _place_x(inp.x, case.layout)
    win = _out_window(N, D, case.layout)
    with pytest.raises(nat.NativeError):
        nat.aggregate_fwd(csr, x, inp.rel, ee, True, inp.loop_edge, win.view)
    torch.cuda.synchronize()
    assert win.untouched()
    if case.layout != A.OUTWIN:
        wins = _bwd_windows(csr, D)
        with pytest.raises(nat.NativeError):
            nat.aggregate_bwd(csr, x, inp.rel, ee, inp.g, out=tuple(w.view for w in wins))
        wins_s = _bwd_windows(csr, D)
        with pytest.raises(nat.NativeError):
            nat.aggregate_bwd_shard(csr, x, inp.rel, ee, inp.g, (0, N), out=tuple(w.view for w in wins_s))
        torch.cuda.synchronize()
        assert all(w.untouched() for w in wins + wins_s)


def test_backward_out_keyword_is_checked(pkg):
    nat = pkg._native
    G = _graph(pkg, ('type', True))
    N, R, ei, et, csr = G
    inp = _inputs('out-kw', G, 8)
    ee = inp.ee.index_select(0, csr.perm).contiguous()
    wins = _bwd_windows(csr, 8)
    with pytest.raises(nat.NativeError):                                      # wrong shape
        nat.aggregate_bwd(csr, inp.x, inp.rel, ee, inp.g, out=(wins[1].view, None, None))
    with pytest.raises(nat.NativeError):                                      # not contiguous
        nat.aggregate_bwd(csr, inp.x, inp.rel, ee, inp.g, out=(_pad_view(wins[0].view, 0, 1), None, None))
    with pytest.raises(nat.NativeError):                                      # given but not computed
        nat.aggregate_bwd(csr, inp.x, inp.rel, ee, inp.g, want_gx=False, out=tuple(w.view for w in wins))
    torch.cuda.synchronize()
    assert all(w.untouched() for w in wins)
    gx, gee, grel = nat.aggregate_bwd(csr, inp.x, inp.rel, ee, inp.g, out=(None, wins[1].view, None))
    assert gee.data_ptr() == wins[1].view.data_ptr() and gx is not None and grel is not None
    wins[1].check('out keyword')
