"""Round-3 parity additions (`-m gpu`):

* BASELINE configs[4]'s layer widths under test: a config-5-shaped slice that the oracle still finishes
  on the host (N = 50 000, E = 500 000, R = 1000, D = 512; uniform and Zipf(1.1) tails): the fused launch 512 -> 200 and
  512 -> 512 against oracle.layer_forward (model.py:82-109 in the reference's per-edge order) at 5e-5, the two-launch
  path at 2e-6, and rank r of 8's destination range + table shard torch.equal to the full launch;
* the numerics claim of the fused layer's dense step (six bf16-split MFMA products, f32 accumulation) pinned against
  float64: on the bench workload max |out - f64| <= 1e-6 and <= 1.5 x the exact-f32 two-launch path's
  error; adversarial rows (2^+-20 dynamic range inside a row, denormals, exact cancellation, negative values) within the
  same bound relative to the row's magnitude; non-finite inputs poison their own rows only.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _graph(pkg, oracle, N, R, E, seed, zipf, duplicate_first=False, **csr_kw):
    tri = oracle.synthetic_triples(N, R, E, seed=seed, zipf=zipf)
    if duplicate_first:
        tri[1] = tri[0]                   # edges 0 and 1 (and E, E + 1) are the same (source, relation, destination)
    ei, ea = oracle.build_edge_list(tri, R)
    ei, ea = torch.from_numpy(ei), torch.from_numpy(ea)
    csr = pkg.GraphCSR(N, 2 * R + 1, ei, ea[0], torch.device(DEV), **csr_kw)
    return ei, ea, csr


def _layer(pkg, D, O, R, seed, bias=False):
    torch.manual_seed(seed)
    conv = pkg.MGCNConv(D, O, 2 * R, bias=bias).to(DEV).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        conv.ent_bn.running_mean.copy_(torch.randn(O, generator=g) * 0.05)
        conv.ent_bn.running_var.copy_(torch.rand(O, generator=g) * 0.5 + 0.05)
        conv.ent_bn.weight.copy_(torch.rand(O, generator=g) + 0.5)
        conv.ent_bn.bias.copy_(torch.randn(O, generator=g) * 0.1)
    return conv


def _fused(pkg, conv, csr, x, rel, table, node_range=None, ee_sub=(0, 0, 0), want_rel=True):
    nat, bn, O = pkg._native, conv.ent_bn, conv.out_channels
    _, wpack = conv.derived_weights()
    n0, n1 = (0, csr.num_nodes) if node_range is None else node_range
    out = torch.full((n1 - n0, O), float('nan'), device=DEV)
    rel_out = torch.empty((rel.size(0), O), device=DEV) if want_rel else None
    with torch.no_grad():
        nat.layer_fwd_fused(csr, x, rel, conv.loop_rel.reshape(-1), table, True, conv.loop_edge.reshape(-1), wpack, O, conv.bias,
                            bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out, node_range=node_range, ee_sub=ee_sub,
                            rels_weight=conv.rels_weight.detach().contiguous() if want_rel else None, rel_out=rel_out)
    return out, rel_out


def _layer_f64(conv, csr, x, rel, table_slot_order, ei, et, with_bound=False):
    """The layer in float64 with torch ops on the GPU (test infrastructure): model.py:82-109, eval mode. with_bound: also
    B[n, o] = sum_k sum_e |message_e[k]| |W[k, o]| * |gamma_o| / (3 sqrt(var_o + eps)): the condition of the output, i.e.
    what ONE unit roundoff on every product moves the pre-activation by (|tanh'| <= 1 carries it to the output)."""
    N, E = x.size(0), ei.size(1) // 2
    bn = conv.ent_bn
    dd = lambda t: t.detach().double()
    ee = torch.empty_like(table_slot_order, dtype=torch.float64)
    ee[csr.perm] = table_slot_order.double()                       # back to reference edge order
    ei, et = ei.to(DEV), et.to(DEV)
    rels = torch.cat([dd(rel), dd(conv.loop_rel)], 0)
    res = []
    for half, wname in ((slice(0, E), 'in_weight'), (slice(E, 2 * E), 'out_weight')):
        row, col = ei[0, half], ei[1, half]
        deg = torch.bincount(row, minlength=N).double()
        inv = deg.pow(-0.5)
        inv[torch.isinf(inv)] = 0
        norm = inv[row] * inv[col]
        msg = (dd(x)[row] * rels[et[half]] * ee[half]) * norm[:, None]
        agg = torch.zeros((N, x.size(1)), dtype=torch.float64, device=DEV).index_add_(0, col, msg)
        res.append(agg @ dd(getattr(conv, wname)))
        if with_bound:
            mag = torch.zeros((N, x.size(1)), dtype=torch.float64, device=DEV).index_add_(0, col, msg.abs())
            bound = bound + mag @ dd(getattr(conv, wname)).abs() if half.start else mag @ dd(getattr(conv, wname)).abs()
    a_loop = dd(x) * rels[-1] * dd(conv.loop_edge)
    loop = a_loop @ dd(conv.loop_weight)
    z = (res[0] + res[1] + loop) / 3
    if conv.bias is not None:
        z = z + dd(conv.bias)
    inv = dd(bn.weight) / torch.sqrt(dd(bn.running_var) + bn.eps)
    y = (z - dd(bn.running_mean)) * inv + dd(bn.bias)
    if with_bound:
        bound = (bound + a_loop.abs() @ dd(conv.loop_weight).abs()) * inv.abs() / 3
        return torch.tanh(y), bound
    return torch.tanh(y)


@pytest.mark.parametrize('zipf', [0.0, 1.1])
def test_config5_shaped_slice_dim512(pkg, oracle, zipf):
    N, R, E, D = 50000, 1000, 500000, 512
    ei, ea, csr = _graph(pkg, oracle, N, R, E, seed=3, zipf=zipf)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, D, generator=g) * 0.7
    rel = torch.randn(2 * R, D, generator=g) * 0.7
    ee = torch.randn(2 * E, D, generator=g) * 0.7                # reference edge order
    xd, reld = x.to(DEV), rel.to(DEV)
    table = ee.to(DEV).index_select(0, csr.perm)                   # slot order
    for O in (200, 512):
        conv = _layer(pkg, D, O, R, seed=40 + O)
        assert pkg._native.fused_supported(D, O)
        full, rel_out = _fused(pkg, conv, csr, xd, reld, table)
        sd = {'conv1.' + k: v.detach().cpu() for k, v in conv.state_dict().items()}
        want_ent, want_rel = oracle.layer_forward(sd, 'conv1.', x, ei, ea[0], ee, rel, training=False)
        assert float(want_ent.abs().mean()) > 0.05                                         # not vacuous
        # W after the sum + MFMA k order (six bf16-split products, f32 accumulation) vs the reference's per-edge f32 order.
        # With Zipf(1.1) tails the top destinations sum 10^4 messages: the REFERENCE's own sequential f32 scatter-add is
        # then the noisier side (measured against float64 below), hence the wider bar for that graph.
        np.testing.assert_allclose(full.cpu().numpy(), want_ent.numpy(), rtol=0, atol=5e-5 if zipf == 0 else 2e-4)
        np.testing.assert_allclose(rel_out.cpu().numpy(), want_rel.numpy(), rtol=0, atol=2e-5)
        ref64 = _layer_f64(conv, csr, xd, reld, table, ei, ea[0])
        err_fused = float((full.double() - ref64).abs().max())
        err_oracle = float((want_ent.to(DEV).double() - ref64).abs().max())
        del ref64
        # (f32 accumulation of K = 1536 products: ~2e-6 from float64 on a tanh output; the per-edge order of the reference
        # has shorter sums on a uniform graph, 5e-7, and longer ones on the hub rows of the Zipf graph)
        print('config-5 slice O=%d zipf=%.1f: max |fused - f64| = %.2e, max |reference order - f64| = %.2e' % (O, zipf, err_fused, err_oracle))
        assert err_fused <= 1e-5, (O, zipf, err_fused, err_oracle)
        two = torch.empty((N, O), device=DEV)
        with torch.no_grad():
            conv._two_launch_layer(csr, xd, reld, table, True, two)
        # exact-f32 MFMA dense step: two f32 summations of K = 1536 terms in different orders (2e-6 at K <= 768 without hubs;
        # a Zipf(1.1) hub row sums thousands of slots, its pre-activation is O(10) and one f32 ulp of it is 1e-6)
        assert float((two - full).abs().max()) <= 2e-5
        b = csr.balanced_bounds(8)
        for r in (0, 3, 7):                                                                  # rank r of 8 holds only its shard
            n0, n1 = b[r], b[r + 1]
            part, _ = _fused(pkg, conv, csr, xd, reld, csr.edge_table_shard(table, n0, n1), node_range=(n0, n1),
                             ee_sub=csr.shard_ee_sub(n0, n1), want_rel=False)
            assert torch.equal(part, full[n0:n1]), (O, r)


def test_fused_dense_step_is_f32_faithful_on_the_bench_workload(pkg, oracle):
    """bench.py's WN18RR-shaped 2-layer workload: both fused instances against float64."""
    N, R, E = 40943, 11, 86835
    ei, ea, csr = _graph(pkg, oracle, N, R, E, seed=0, zipf=0.0)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(N, 100, generator=g) * 0.3).to(DEV)
    rel = (torch.randn(2 * R, 100, generator=g) * 0.5).to(DEV)
    for D, O in ((100, 200), (200, 200)):
        conv = _layer(pkg, D, O, R, seed=50 + D)
        table = (torch.randn(2 * E, D, generator=g) * 0.5).to(DEV)
        fused, rel_out = _fused(pkg, conv, csr, x, rel, table)
        two = torch.empty((N, O), device=DEV)
        with torch.no_grad():
            conv._two_launch_layer(csr, x, rel, table, True, two)
        ref = _layer_f64(conv, csr, x, rel, table, ei, ea[0])
        err_fused = float((fused.double() - ref).abs().max())
        err_f32 = float((two.double() - ref).abs().max())
        assert err_fused <= 1e-6, (D, O, err_fused)
        assert err_fused <= 1.5 * err_f32 + 1e-7, (D, O, err_fused, err_f32)
        x, rel = fused, rel_out


def test_fused_dense_step_on_adversarial_rows(pkg, oracle):
    """Rows built to stress the three-way bf16 split of the aggregates: 2^+-20 dynamic range inside a row, denormal
    magnitudes, exact cancellation between two slots, negative values, +-2^k. The numeric contract of the fused dense step
    (include/mgcn_hip.h): |out - exact| <= 4 u B + 2e-7 with u = 2^-24 and B the row's condition (see _layer_f64) — the
    classical forward bound of an f32 dot product with a small constant; the exact-f32 MFMA path is held to the same bar.
    (On such rows the two paths differ from each other by up to 10x — both a hundred times inside the bound.)"""
    N, R, E, D, O = 600, 3, 2400, 128, 200
    ei, ea, csr = _graph(pkg, oracle, N, R, E, seed=5, zipf=0.0, duplicate_first=True, hub_threshold=0)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, D, generator=g)
    scale = torch.ones(N, D)
    scale[0:100] = torch.exp2(torch.randint(-20, 21, (100, D), generator=g).float())      # wide range inside a row
    scale[100:200] = 2.0 ** -130                                                            # denormal magnitudes
    x = x * scale
    x[200:300] = torch.exp2(torch.randint(-8, 9, (100, D), generator=g).float()) * torch.sign(x[200:300])   # +-2^k
    x[300:400] = -x[300:400].abs()                                                          # negative rows
    rel = torch.randn(2 * R, D, generator=g)
    ee = torch.randn(2 * E, D, generator=g)
    # exact cancellation: edges 0 / 1 (and their reverses E / E + 1) are duplicates with opposite per-edge rows
    ee[1], ee[E + 1] = -ee[0], -ee[E]
    conv = _layer(pkg, D, O, R, seed=60)
    xd, reld = x.to(DEV), rel.to(DEV)
    table = ee.to(DEV).index_select(0, csr.perm)
    fused, _ = _fused(pkg, conv, csr, xd, reld, table)
    two = torch.empty((N, O), device=DEV)
    with torch.no_grad():
        conv._two_launch_layer(csr, xd, reld, table, True, two)
    ref, bound = _layer_f64(conv, csr, xd, reld, table, ei, ea[0], with_bound=True)
    assert torch.isfinite(fused).all()
    u = 2.0 ** -24
    for name, got in (('fused', fused), ('exact-f32 two-launch', two)):
        excess = (got.double() - ref).abs() - (4 * u * bound + 2e-7)
        worst = int(torch.argmax(excess.max(1).values))
        assert float(excess.max()) <= 0, (name, worst, float((got.double() - ref).abs()[worst].max()), float(bound[worst].max()))
    big = u * bound > 1e-7                                    # (where the bound, not the 2e-7 floor, is what holds)
    ratio = ((fused.double() - ref).abs()[big] / (u * bound[big])).max()
    print('adversarial rows: max |fused - f64| / (u B) = %.3f over %d outputs' % (float(ratio), int(big.sum())))
    # non-finite inputs: split3(+-inf) is NaN, so an infinite layer input gives NaN in the rows that gather it (the
    # exact-f32 path gives +-1 or NaN there); every other row is unaffected, bit for bit
    bad = xd.clone()
    bad[17, 5] = float('inf')
    poisoned, _ = _fused(pkg, conv, csr, bad, reld, table)
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[17] = True
    src, dst = ei[0].to(DEV), ei[1].to(DEV)
    touched[dst[src == 17]] = True
    assert torch.equal(poisoned[~touched], fused[~touched])
    assert not torch.isfinite(poisoned[17]).all()


@pytest.mark.parametrize('D', [100, 200, 36])
def test_hub_fold_inside_the_prepass_launch(pkg, oracle, D):
    """The hub pre-pass is ONE launch (chunk sums + the two-level fold by the last lane group to arrive at a hub's counter,
    include/mgcn_hip.h (2)): a Zipf graph whose top hubs have more than 16 chunks (both fold levels) and hubs of 2..16
    chunks (one level). The aggregate matches a float64 scatter-add of the same messages (model.py:111-118), two launches
    are bit-identical (the fold order does not depend on which group arrives last), the arrival counters are zero again
    after every launch, and a destination range gives the rows of the full launch."""
    N, R, E = 3000, 7, 60000
    ei, ea, csr = _graph(pkg, oracle, N, R, E, seed=5, zipf=1.3, hub_threshold=16, hub_chunk=8)
    chunks = csr.chunks.cpu().numpy().reshape(-1, 4)[:csr.num_chunks]
    assert chunks[:, 3].max() > 16 and (chunks[:, 3] <= 16).any() and csr.num_chunks > 100
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(N, D, generator=g) * 0.5).to(DEV)
    rel = (torch.randn(2 * R + 1, D, generator=g) * 0.5).to(DEV)
    table = (torch.randn(2 * E, D, generator=g) * 0.5).to(DEV)            # slot order
    loop_edge = torch.ones(D, device=DEV)
    nat = pkg._native
    out = torch.empty((N, 3 * D), device=DEV)
    nat.aggregate_fwd(csr, x, rel, table, True, loop_edge, out)
    again = torch.empty_like(out)
    nat.aggregate_fwd(csr, x, rel, table, True, loop_edge, again)
    assert torch.equal(out, again)
    (buf, _), = [v for k, v in csr._hub_partials.items() if k[0] == D]
    counters = buf[csr.num_chunks * D:].view(torch.int32)
    assert counters.numel() == 2 * csr.num_chunks and int(counters.abs().max()) == 0
    # float64 reference of the two edge halves in slot order
    rec = csr.rec.cpu().numpy().reshape(-1, 4)
    src, typ, norm = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].copy().view(np.float32).astype(np.float64)
    sd = csr.slot_dst.cpu().numpy().view(np.uint32).astype(np.int64)      # bit 31 = half (csr_build.cpp), hub slots included
    dst, half = sd & 0x7fffffff, sd >> 31
    msg = x.cpu().double().numpy()[src] * rel.cpu().double().numpy()[typ] * table.cpu().double().numpy() * norm[:, None]
    want, mag = np.zeros((2, N, D)), np.zeros((2, N, D))
    for h in range(2):
        np.add.at(want[h], dst[half == h], msg[half == h])
        np.add.at(mag[h], dst[half == h], np.abs(msg[half == h]))
    got = out.cpu().double().numpy()
    for h in range(2):
        err = np.abs(got[:, h * D:(h + 1) * D] - want[h])
        assert (err <= 256 * 2.0 ** -24 * mag[h] + 1e-30).all(), (h, float(err.max()))   # (a sequential f32 sum of n terms: (n - 1) u)
    n0, n1 = 700, 2100
    part = torch.empty((n1 - n0, 3 * D), device=DEV)
    nat.aggregate_fwd(csr, x, rel, csr.edge_table_shard(table, n0, n1), True, loop_edge, part, node_range=(n0, n1),
                      ee_sub=csr.shard_ee_sub(n0, n1), out_row0=n0)
    assert torch.equal(part, out[n0:n1])
    # the same buffer (chunk-sum rows + counters) under OTHER inputs, as the next layer of equal width uses it: nothing of
    # the previous launch may survive in it (a stale chunk sum read by a fold would be off by far more than the bound)
    x2 = (-2.0 * x + 0.25).contiguous()
    out2 = torch.empty_like(out)
    nat.aggregate_fwd(csr, x2, rel, table, True, loop_edge, out2)
    msg2 = x2.cpu().double().numpy()[src] * rel.cpu().double().numpy()[typ] * table.cpu().double().numpy() * norm[:, None]
    got2 = out2.cpu().double().numpy()
    for h in range(2):
        want2, mag2 = np.zeros((N, D)), np.zeros((N, D))
        np.add.at(want2, dst[half == h], msg2[half == h])
        np.add.at(mag2, dst[half == h], np.abs(msg2[half == h]))
        assert (np.abs(got2[:, h * D:(h + 1) * D] - want2) <= 256 * 2.0 ** -24 * mag2 + 1e-30).all(), h


@pytest.mark.parametrize('zipf', [0.0, 1.2])
def test_work_balanced_runs_do_not_change_rows(pkg, oracle, zipf):
    """mgcn_layer_fwd_fused's row_bounds_dev (GraphCSR.workgroup_bounds: one work-balanced run of destinations per CU):
    the elastic kernel's rows are bit-identical with and without them, for the whole graph and for a destination
    range with its table shard, equal to the lockstep kernel's, and match the oracle (model.py:82-109). The reserved `tune`
    value (bits 10-11 = 1) and a packing for a generation that does not exist are refused, and a refused launch leaves the
    graph's hub buffers usable."""
    N, R, E, D, O = 5000, 11, 60000, 100, 200
    ei, ea, csr = _graph(pkg, oracle, N, R, E, seed=9, zipf=zipf)
    conv = _layer(pkg, D, O, R, seed=4, bias=True)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(N, D, generator=g) * 0.5).to(DEV)
    rel = (torch.randn(2 * R, D, generator=g) * 0.5).to(DEV)
    ee = (torch.randn(2 * E, D, generator=g) * 0.5).to(DEV)
    table = ee.index_select(0, csr.perm)
    nat = pkg._native
    bn = conv.ent_bn
    wcat, _ = conv.derived_weights()
    wpack = nat.pack_weights(wcat, generation=0)                            # (generations 2 and 3 share the shape's own packing)

    def launch(balance, tune, rng=None):
        n0, n1 = rng or (0, N)
        out = torch.empty((n1 - n0, O), device=DEV)
        tab = table if rng is None else csr.edge_table_shard(table, n0, n1)
        nat.layer_fwd_fused(csr, x, rel, conv.loop_rel.reshape(-1), tab, True, conv.loop_edge.reshape(-1),
                            wpack, O, conv.bias, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out, node_range=rng,
                            ee_sub=(0, 0, 0) if rng is None else csr.shard_ee_sub(n0, n1), tune=tune, balance=balance)
        return out
    bounds = csr.workgroup_bounds(0, N, 256, min_gain=0.0).cpu().numpy()
    assert bounds[0] == 0 and bounds[-1] == N and (np.diff(bounds) > 0).all() and len(bounds) == 257
    plain = launch(False, 0xc00)                 # the elastic kernel, equal runs
    assert torch.equal(launch(True, 0xc00), plain)
    assert torch.equal(launch(True, 0), plain)   # 63 lockstep tiles < 2 x CUs: the balanced launch is the elastic kernel
    assert torch.equal(launch(False, 0), plain)  # ... and the lockstep kernel's rows are the same bits
    part = launch(True, 0, (1234, 4321))
    assert torch.equal(part, plain[1234:4321])
    with pytest.raises(nat.NativeError):         # `tune` bits 10-11 = 1: the reserved value
        launch(False, 0x400)
    with pytest.raises(nat.NativeError):
        nat.pack_weights(wcat, generation=4)
    assert torch.equal(launch(True, 0), plain)   # after the refusals (zipf: the hub buffers are still usable)
    sd = {'conv1.' + k: v.detach().cpu() for k, v in conv.state_dict().items()}
    want, _ = oracle.layer_forward(sd, 'conv1.', x.cpu(), ei, ea[0], ee.cpu(), rel.cpu(), training=False)
    np.testing.assert_allclose(plain.cpu().numpy(), want.numpy(), rtol=0, atol=2e-4 if zipf else 5e-5)
