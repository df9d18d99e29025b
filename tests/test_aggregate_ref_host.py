"""Host-side checks of tests/aggregate_ref.py (no GPU): the float64 references agree with the oracle and with autograd,
every graph builder delivers the run lengths / chunk counts / relation runs it promises (asserted from the feeder's own
output), the grids keep every kernel instance, the hand-written geometry labels match pick_geometry, and the bar holds
for an f32 emulation of the same sums on every grid case. Figures are printed (`pytest -s`) before they are asserted."""
import pytest
import torch

from . import aggregate_ref as A
from .conftest import golden


def _csr(pkg, graph, thr=0, chunk=64):
    N, R, ei, et = graph
    return pkg._native.csr_build_host(N, 2 * R + 1, ei, et, hub_threshold=thr, hub_chunk=chunk)


# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['syn_a', 'syn_b', 'syn_c'])
def test_forward_reference_equals_the_oracle(oracle, case, monkeypatch):
    """Same halves, types, per-edge rows, self-loop block as oracle.aggregate_then_weight (before its weight multiply), run
    in float64. The oracle forms its norm in f32 (kept so: its compute_norm runs under the f32 default): that norm is handed
    to the reference here, and compared with the float64 norm separately."""
    g = golden(case)
    sd = {k: v.double() for k, v in g.state_dict().items()}
    ei, ea = g.t('dl_edge_index'), g.t('dl_edge_attr')
    ee = sd['edge_embeddings'].index_select(0, ea[1])
    x, rels = sd['entity_embedding'], sd['relation_embedding']
    N, E = x.size(0), ea.size(1) // 2
    old = torch.get_default_dtype()
    real_norm = oracle.compute_norm

    def norm_f32(idx, n):
        torch.set_default_dtype(old)
        try:
            return real_norm(idx, n)
        finally:
            torch.set_default_dtype(torch.float64)
    monkeypatch.setattr(oracle, 'compute_norm', norm_f32)
    torch.set_default_dtype(torch.float64)
    try:
        _, aggs = oracle.aggregate_then_weight(sd, 'conv1.', x, ei, ea[0], ee, rels)
    finally:
        torch.set_default_dtype(old)
    assert aggs[0].dtype == torch.float64
    rel = torch.cat([rels, sd['conv1.loop_rel']], 0)
    monkeypatch.undo()
    norms = [oracle.compute_norm(ei[:, :E], N), oracle.compute_norm(ei[:, E:], N)]
    ref = A.ref_forward(N, ei, ea[0], x, rel, ee, norms=norms)
    want = torch.cat(aggs[:2], 1)
    scale = float(want.abs().max())
    assert float((ref.value - want).abs().max()) <= 1e-12 * scale
    assert float((A.forward64(N, ei, ea[0], x, rel, ee, norms=norms) - want).abs().max()) <= 1e-12 * scale
    loop = A.ref_loop(x, rel, sd['conv1.loop_edge'].reshape(-1))
    assert float((loop - aggs[2]).abs().max()) <= 1e-12 * float(aggs[2].abs().max())
    for h in range(2):
        n64 = A.norm64(N, ei, h)
        assert float((norms[h].double() - n64).abs().max()) <= A.NORM_F32_MAX_U * A.U * float(n64.max())
        assert torch.equal(A.norm32(N, ei, h), norms[h])
    # n and mag are the term count and the sum of |term|
    deg_in = torch.bincount(ei[1, :E], minlength=N).double()
    assert torch.equal(ref.n[:, 0], deg_in) and bool((ref.mag >= ref.value.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('name', ['type', 'degree4'])
@pytest.mark.parametrize('with_ee', [True, False])
def test_gradient_sums_equal_autograd(name, with_ee):
    N, R, ei, et = A.type_profile() if name == 'type' else A.degree_profile(4)
    inp = A.make_inputs('host-grad-' + name, N, 2 * R + 1, ei.size(1), 5)
    x, rel, ee = (t.double().requires_grad_(True) for t in (inp.x, inp.rel, inp.ee))
    (A.forward64(N, ei, et, x, rel, ee if with_ee else None) * inp.g.double()).sum().backward()
    gx, gee, grel = A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee if with_ee else None, inp.g)
    tol = lambda t: 1e-12 * float(t.abs().max())
    assert float((gx.value - x.grad).abs().max()) <= tol(x.grad)
    assert float((grel.value - rel.grad).abs().max()) <= tol(rel.grad)
    assert float(grel.value[-1].abs().max()) == 0.0 and float(grel.n[-1].max()) == 0.0       # the self-loop row
    if with_ee:
        # d/d ee[e] = g * norm * x * rel * 1: the reference's gee is the kernel's (per unit of the table)
        assert float((gee.value - ee.grad).abs().max()) <= tol(ee.grad)
    out_deg = torch.bincount(ei[0], minlength=N).double()
    assert torch.equal(gx.n[:, 0], out_deg)
    assert torch.equal(grel.n[:, 0], torch.bincount(et, minlength=2 * R + 1).double())
    # a destination range's share: the masked sums add up to the whole
    mask = ei[1] < N // 2
    parts = [A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee, inp.g, edge_mask=m) for m in (mask, ~mask)]
    whole = A.ref_grads(N, ei, et, inp.x, inp.rel, inp.ee, inp.g)
    for k in (0, 2):
        assert float((parts[0][k].value + parts[1][k].value - whole[k].value).abs().max()) <= 1e-12
        assert torch.equal(parts[0][k].n + parts[1][k].n, whole[k].n)


# ----------------------------------------------------------------------------------------------------------------
def _run_lengths(csr, half):
    rp = csr['rowptr'][half].long()
    return set((rp[1:] - rp[:-1]).tolist())


@pytest.mark.parametrize('gs', [4, 8, 16, 32, 64])
def test_degree_profile_delivers_its_runs(pkg, gs):
    graph = A.degree_profile(gs)
    N, R, ei, et = graph
    csr = _csr(pkg, graph)
    runs = A.degree_runs(gs)
    assert set(runs) == {0, 1, 2, 3, 4, 5, 2 * gs - 1, 2 * gs, 2 * gs + 1, 4 * gs + 1}
    assert set(runs) <= _run_lengths(csr, 0), sorted(_run_lengths(csr, 0))
    assert set(runs[:-1]) <= _run_lengths(csr, 1), sorted(_run_lengths(csr, 1))
    rp = csr['rowptr'].long()
    assert (rp[0, 1:11] - rp[0, :10]).tolist() == runs                     # destinations 0..9, in that order
    deg = torch.bincount(ei.reshape(-1), minlength=N)
    assert int((deg == 0).sum()) >= 3 and int(deg[N - 1]) == 0             # isolated nodes, the last node among them
    E = ei.size(1) // 2
    assert int((ei[0, :E] == ei[1, :E]).sum()) >= 2                        # self edges
    pairs = (ei[0, :E] * N + ei[1, :E]) * (2 * R + 1) + et[:E]
    assert pairs.unique().numel() < E                                      # duplicate edges
    assert N <= 80 and E <= 1500
    assert bool(torch.equal(ei[0, E:], ei[1, :E]) and torch.equal(ei[1, E:], ei[0, :E]) and torch.equal(et[E:], et[:E] + R))
    # the same runs as hub chunks of a record window and one slot (the pre-pass walk): 2 gs - 1, 2 gs, 2 gs + 1, and 4 gs + 1 as
    # a chunk of 2 gs + 1 and one of 2 gs
    hub = _csr(pkg, graph, thr=5, chunk=2 * gs + 1)
    ch = hub['chunks'][:hub['num_chunks']].long()
    assert {2 * gs - 1, 2 * gs, 2 * gs + 1} <= set((ch[:, 1] - ch[:, 0]).tolist())
    assert 2 in set(hub['hubinfo'][0, :, 1].tolist()) and 5 in _run_lengths(hub, 0) and 6 not in _run_lengths(hub, 0)


def test_hub_profile_delivers_its_chunk_counts(pkg):
    graph = A.hub_profile()
    N, R, ei, et = graph
    csr = _csr(pkg, graph, thr=1, chunk=2)
    counts = csr['hubinfo'][:, :, 1].long()                                # [2, N]
    have = set(counts[counts > 0].tolist())
    assert {1, 2, 15, 16, 17, 32, 33, 257} <= have, sorted(have)
    assert counts[0, :7].tolist() + [int(counts[0, N - 1])] == list(A.HUB_CHUNK_COUNTS)    # first and last node are hubs
    assert int(counts[0, 0]) > A.K_FOLD_SPAN and int(counts[0, N - 1]) > A.K_FOLD_SPAN * A.K_FOLD_SPAN
    assert int(((counts[0] > 0) & (counts[1] == 0)).sum()) >= 8 and int(((counts[1] > 0) & (counts[0] == 0)).sum()) >= 1
    rp = csr['rowptr'].long()
    assert 1 in _run_lengths(csr, 0)                                       # ordinary runs next to the hubs
    chunks = csr['chunks'][:csr['num_chunks']].long()
    assert int((chunks[:, 1] - chunks[:, 0]).min()) == 1                   # ragged last chunks
    assert csr['num_chunks'] == int(counts.sum()) and ei.size(1) // 2 < 2000 and int(rp[1, N]) <= ei.size(1)


def test_type_profile_delivers_its_runs(pkg):
    graph = A.type_profile()
    N, R, ei, et = graph
    csr = _csr(pkg, graph)
    tp = csr['typeptr'].long()
    runs = (tp[1:] - tp[:-1]).tolist()
    assert runs == list(A.TYPE_RUNS) * 2 + [0]
    assert {0, 1, 15, 16, 17, 33} <= set(runs)
    starts = [int(tp[t]) for t in range(2 * R) if runs[t] > 0]
    assert any(s % A.K_TYPE_CHUNK == 0 and s > 0 for s in starts) and any(s % A.K_TYPE_CHUNK for s in starts)
    per_chunk = {}
    for t in range(2 * R):
        if runs[t]:
            per_chunk.setdefault(int(tp[t]) // A.K_TYPE_CHUNK, []).append(t)
    assert any(len(v) >= 2 for v in per_chunk.values())                    # several types start inside one chunk
    assert any(int(tp[t]) // 16 + 2 <= (int(tp[t + 1]) - 1) // 16 for t in range(2 * R) if runs[t])   # a run over three chunks
    assert ei.size(1) % A.K_TYPE_CHUNK != 0
    small = A.type_profile(small=True)
    assert small[2].size(1) < A.K_TYPE_CHUNK
    tps = _csr(pkg, small)['typeptr'].long()
    assert (tps[1:] - tps[:-1]).tolist() == [2, 0, 3, 2, 0, 3, 0]
    # the larger graph runs the long-run gx kernel, the small one the short-run kernel (E < 4N)
    assert ei.size(1) // 2 >= 4 * N and small[2].size(1) // 2 < 4 * small[0]


def test_long_type_and_switch_pair(pkg):
    graph = A.long_type()
    N, R, ei, et = graph
    tp = _csr(pkg, graph)['typeptr'].long()
    lo, hi = int(tp[0]), int(tp[1])
    assert hi - lo > 64 * 16 * 16
    # chunk rows of type 0 that stage 2 adds: more than 64 groups x 16 rows in flight
    assert (hi - 1) // A.K_TYPE_CHUNK - lo // A.K_TYPE_CHUNK > 64 * 16
    assert ei.size(1) // 2 >= 4 * N
    (N0, _, ei0, _), (N1, _, ei1, _) = A.switch_pair()
    assert N0 == N1 and ei0.size(1) // 2 == 4 * N0 - 1 and ei1.size(1) // 2 == 4 * N1
    assert A.case_geometry(A.SWITCH_CASES[0])[:2] == (4, 1)


# ----------------------------------------------------------------------------------------------------------------
def test_hand_written_geometry_labels():
    for c in A.FWD_CASES + A.BWD_CASES + A.FWD_GEOM_CASES + A.BWD_GEOM_CASES + A.REFUSED_CASES + A.SWITCH_CASES:
        assert A.geometry_label(A.case_geometry(c)) == c.label, A.case_id(c)
    # the exact edge of the refused set
    assert A.pick_geometry(2048, True) == (4, 8, 64) and A.pick_geometry(2052, True) is None
    assert A.pick_geometry(512, False) == (1, 8, 64) and A.pick_geometry(513, False) is None
    assert A.pick_geometry(516, True) == (4, 4, 64) and A.pick_geometry(516, False) is None
    assert [d for d in range(1, 2100) if A.pick_geometry(d, False) is None][0] == 513
    assert [d for d in range(4, 2100, 4) if A.pick_geometry(d, True) is None][0] == 2052


def test_every_kernel_instance_is_covered():
    """A later edit of the grids cannot silently drop a kernel instantiation: 13 families x 8 geometries."""
    families = ['fwd', 'hub_prepass', 'gee_grel_fused', 'gee_alone', 'grel_partial_ee', 'grel_partial_noee', 'gx_long',
                'gx_short', 'gx_hub_fold', 'grel_final', 'shard_gee_grel', 'shard_gx', 'shard_gx_hub']
    required = ['%s:v%dc%d' % (f, v, c) for f in families for v in (4, 1) for c in (1, 2, 4, 8)]
    required += ['agg_fwd_kernel<4,1,2>', 'agg_fwd_kernel<4,1,4>']
    assert len(required) == 13 * 8 + 2
    have = A.all_labels()
    missing = [l for l in required if l not in have]
    assert not missing, missing
    # every lane-group size, and the three ways into VEC = 1 at a width that is a multiple of 4
    assert {A.case_geometry(c)[2] for c in A.FWD_CASES} == {4, 8, 16, 32, 64}
    assert {c.layout for c in A.FWD_CASES} == {A.PLAIN, A.XCOL, A.XSTRIDE, A.OUTWIN}
    assert {c.layout for c in A.BWD_CASES} == {A.PLAIN, A.XCOL, A.XSTRIDE, A.GLD}


# ----------------------------------------------------------------------------------------------------------------
def test_inputs_have_no_ignorable_entry():
    a = A.make_inputs('a', 7, 5, 12, 9)
    b = A.make_inputs('b', 7, 5, 12, 9)
    for t in a:
        assert float(t.abs().min()) >= 0.5 and float(t.abs().max()) <= 2.0 and bool((t < 0).any()) and bool((t > 0).any())
    assert not torch.equal(a.x, b.x) and torch.equal(a.x, A.make_inputs('a', 7, 5, 12, 9).x)


def test_f32_emulation_stays_inside_the_bar():
    """The same sums in f32 on the CPU against the float64 references, every graph and width of the GPU grids. A ratio above
    1.0 means the bar or the reference is wrong. The worst ratio is recorded in aggregate_ref.py; it is a note, not the bar."""
    worst, worst_norm = 0.0, 0.0
    for label, (N, R, ei, et), widths in A.host_grid():
        for h in range(2):
            n64 = A.norm64(N, ei, h)
            assert bool((n64 > 0).all()), '%s: an edge with a zero norm tests nothing' % label
            rel_err = (A.norm32(N, ei, h).double() - n64).abs() / n64
            worst_norm = max(worst_norm, float(rel_err.max()) / A.U)
        for D in widths:
            inp = A.make_inputs('host-%s-%d' % (label, D), N, 2 * R + 1, ei.size(1), D)
            for ee in (inp.ee, None):
                fwd = A.emul_forward_f32(N, ei, et, inp.x, inp.rel, ee)
                r = [A.check(fwd, A.ref_forward(N, ei, et, inp.x, inp.rel, ee), '%s D=%d forward' % (label, D))]
                got = A.emul_grads_f32(N, ei, et, inp.x, inp.rel, ee, inp.g)
                refs = A.ref_grads(N, ei, et, inp.x, inp.rel, ee, inp.g)
                for k, what in enumerate(('gx', 'gee', 'grel')):
                    r.append(A.check(got[k], refs[k], '%s D=%d %s' % (label, D, what)))
                worst = max(worst, max(r))
            loop = (inp.x * inp.rel[-1]) * inp.loop_edge
            A.check_loop(loop, A.ref_loop(inp.x, inp.rel, inp.loop_edge), '%s D=%d loop' % (label, D))
    print('EMUL worst ratio %.4f (recorded %.4f); worst f32 norm error %.3f u' % (worst, A.EMUL_WORST_RATIO_MEASURED, worst_norm))
    assert worst_norm <= A.NORM_F32_MAX_U * (1 + 4 * A.U)          # (2.5 u is a first-order figure)
    assert worst <= 1.0
    assert A.EMUL_WORST_RATIO_MEASURED / 2 <= worst <= A.EMUL_WORST_RATIO_MEASURED * 2, 'the recorded worst ratio went stale'


def test_the_bar_notices_one_wrong_term():
    """A dropped, doubled or mis-indexed term of any element is far outside the bar (the sensitivity the inputs are built for)."""
    N, R, ei, et = A.degree_profile(64)
    D = 8
    inp = A.make_inputs('host-sens', N, 2 * R + 1, ei.size(1), D)
    ref = A.ref_forward(N, ei, et, inp.x, inp.rel, inp.ee)
    good = A.emul_forward_f32(N, ei, et, inp.x, inp.rel, inp.ee)
    assert A.worst_ratio(good, ref)[0] <= 1.0
    # the smallest possible term of the longest run (257 slots): dropped
    E = ei.size(1) // 2
    k = int((ei[1, :E] == 9).nonzero()[-1])
    term = (inp.x[ei[0, k]] * inp.rel[et[k]] * inp.ee[k]) * A.norm32(N, ei, 0)[k]
    bad = good.clone(); bad[9, :D] -= term
    assert A.worst_ratio(bad, ref)[0] > 20.0
    stale = good.clone(); stale[0, 0] = 1e-30                     # node 0 has no incoming edge in half 0: exactly 0.0
    assert A.worst_ratio(stale, ref)[1] == 1
    nan = good.clone(); nan[3, 1] = float('nan')
    assert A.worst_ratio(nan, ref)[0] == float('inf')
