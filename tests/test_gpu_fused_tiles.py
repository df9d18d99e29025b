"""The fused layer forward where a workgroup walks SEVERAL tiles (`-m gpu`), every element held to float64.

The state a workgroup carries from one tile to the next — the double-buffered stage images, the row pointers and records
fetched one (tile, mode) ahead, the LDS counters between the two roles, the epilogue of a ragged last tile — is entered by
launches the rest of the suite hardly makes, and the launch arithmetic says which:

  generation 2 (layer_fused2.hip, fused2_launch): grid = min(tiles, CUs); a workgroup walks tiles bid, bid + grid, ...; so a
    second tile needs more than CUs x 64 rows. Tile height 64 unless 80-row tiles give the smaller makespan
    ceil(tiles / CUs) x height; outputs of at most 128 columns always take 80-row tiles.
  generation 3 (layer_fused3.hip, fused3_launch): one run of rows per workgroup, rpw = ceil(rows / CUs) rounded up to 16, or the
    caller's runs (`row_bounds=`), whose cap is per = ceil(rows / runs) rounded up to 16 (per <= 80) or to 80; tiles of
    NRT x 16 rows with NRT <= 5 if cap >= 80, 4 if cap >= 64, else 3, and 3 for outputs wider than 208 columns.

So the row counts here are functions of the device's CU count, each test restates this arithmetic (_gen2_geometry,
_gen3_geometry) and asserts that the tiles it means to reach are the ones it gets. Generation 3's tile height is FORCED to the
height the arithmetic allows (`tune` bits 0-3, which the launch clamps to the cap and refuses where it does not fit the LDS), so
the height is certain; the same launch with the height left to the kernel must give the same bits.

The yardstick is tests/fused_ref.py: float64 from the edge list, nothing of the library; the bar is the numeric contract of
include/mgcn_hip.h (2b), |out - exact| <= 4 * 2^-24 * B + 2e-7 per element. tests/test_fused_ref_host.py shows on the same inputs
(tests/fused_cases.py) that a plain f32 evaluation meets it (worst ratio 0.70), that the tanh is not saturated, and that dropping a
slot, swapping two rows, zeroing a k-block or shifting the BN scale by a column each break it. Beside the bar, the project's
bit-for-bit promises (torch.equal): the rows of the default launch, generation 2 == generation 3 where they share a packing,
rel_out == _native.matmul(rel, rels_weight).

One case departs from the list it was written from: runs [0, 48, 96, 161] have a run of 65 rows where 161 rows in 3 runs cap a
run at 64, which `row_bounds=` refuses (test_row_bounds_are_checked_before_any_launch); the 3-row-tile case is [0, 48, 97, 161]
(runs of one tile, 48 + 1 rows, 48 + 16 rows) with the height forced to 3. And "equal runs" at 100 -> 212 are two 48-row tiles
per run (outputs wider than 208 columns take 3 row tiles), so the 80-row tile followed by a 16-row tile is the same launch at
100 -> 200; both run. [0, 64, 128, 161] has no run of two tiles, so [0, 64, 161] with the height forced to 4 (64 | 64 + 33 rows)
runs beside it."""
import numpy as np
import pytest
import torch

from . import fused_cases, fused_ref
from .fused_cases import GEN2, GEN2_CASES, GEN3, GEN3_CASES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

_worst = {}
_device_cache = {}


def _cus():
    return int(torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count)


def _ceil(a, b):
    return -(-a // b)


def _gen2_geometry(rows, cus, O):
    """fused2_launch: (tile height, tiles, grid, tiles per workgroup, rows of the last tile)."""
    makespan = lambda bm: _ceil(_ceil(rows, bm), cus) * bm
    bm = 80 if O <= 128 else (64 if makespan(64) < makespan(80) else 80)
    tiles = _ceil(rows, bm)
    grid = min(tiles, cus)
    per_wg = [(tiles - b + grid - 1) // grid for b in range(grid)]
    assert sum(per_wg) == tiles
    return bm, tiles, grid, per_wg, rows - (tiles - 1) * bm


def _gen3_geometry(rows, cus, O, bounds, forced_nrt):
    """fused3_launch: (rows per tile, [tile sizes of every run])."""
    if bounds is None:
        cap = max(16, _ceil(_ceil(rows, cus), 16) * 16)
        runs = [min(cap, rows - k * cap) for k in range(_ceil(rows, cap))]
    else:
        runs = [hi - lo for lo, hi in zip(bounds[:-1], bounds[1:])]
        per = _ceil(rows, len(runs))
        cap = _ceil(per, 16) * 16 if per <= 80 else _ceil(per, 80) * 80
        assert max(runs) <= cap
    nrt_cap = 3 if O > 208 else (5 if cap >= 80 else 4 if cap >= 64 else 3)
    nrt = min(forced_nrt, nrt_cap)
    bm = 16 * nrt
    return bm, [[min(bm, r - k * bm) for k in range(_ceil(r, bm))] for r in runs]


class _Device(object):
    """A case's operands on the GPU; shared by the cases that share inputs."""

    def __init__(self, pkg, case, cus):
        i = fused_cases.build_inputs(case, cus)
        self.i, self.pkg, self.O = i, pkg, case.O
        self.csr = pkg.GraphCSR(i.N, 2 * i.R + 1, i.ei, i.et, torch.device(DEV), **i.hub_kw)
        conv = pkg.MGCNConv(case.D, case.O, 2 * i.R, bias=True)
        res = conv.load_state_dict(i.sd, strict=False)
        assert not res.unexpected_keys and all(k == 'ent_bn.num_batches_tracked' for k in res.missing_keys)
        self.conv = conv.to(DEV).eval()
        self.x, self.rel = i.x.to(DEV), i.rel.to(DEV)
        self.table = i.ee.to(DEV).index_select(0, self.csr.perm)                       # slot order (csr.perm: slot -> edge)
        if case.ee16:
            self.table = self.table.to(torch.bfloat16)                                 # exact: the inputs are bf16 values already
            assert torch.equal(self.table.float(), i.ee.to(DEV).index_select(0, self.csr.perm))
        self.packed = {}

    def wpack(self, gen):
        if gen not in self.packed:
            wcat, wp = self.conv.derived_weights()
            self.packed[gen] = wp if gen == 0 else self.pkg._native.pack_weights(wcat, generation=gen)
        return self.packed[gen]

    def launch(self, tune=0, balance=False, live=False, row_bounds=None, shard=False, wide=False, want_rel=False):
        nat, conv, bn, csr, i, O = self.pkg._native, self.conv, self.conv.ent_bn, self.csr, self.i, self.O
        n0, n1 = i.n0, i.n1
        rng = (n0, n1) if (n0, n1) != (0, i.N) else None
        x, out = self.x, torch.full((n1 - n0, O), float('nan'), device=DEV)
        if wide:                                                                       # column slices: ldx > D, ldo > O
            xw = torch.full((i.N, x.size(1) + 12), float('nan'), device=DEV)
            xw[:, 4:4 + x.size(1)] = x
            x = xw[:, 4:4 + x.size(1)]
            ow = torch.full((n1 - n0, O + 8), float('nan'), device=DEV)
            out = ow[:, 4:4 + O]
            assert x.stride(0) > x.size(1) and x.stride(0) % 4 == 0 and out.stride(0) > O and out.stride(0) % 4 == 0
        ee, sub = self.table, (0, 0, 0)
        if shard:
            ee, sub = csr.edge_table_shard(self.table, n0, n1), csr.shard_ee_sub(n0, n1)
            assert sub[0] > 0 and sub[1] > 0 and ee.size(0) < self.table.size(0)
        rel_out = torch.full((self.rel.size(0), O), float('nan'), device=DEV) if want_rel else None
        if row_bounds is not None:
            row_bounds = torch.tensor(row_bounds, dtype=torch.int32, device=DEV)
        with torch.no_grad():
            nat.layer_fwd_fused(csr, x, self.rel, conv.loop_rel.reshape(-1), ee, True, conv.loop_edge.reshape(-1),
                                self.wpack(nat.tune_generation(tune)), O, conv.bias, bn.running_mean, bn.running_var, bn.weight,
                                bn.bias, bn.eps, out, node_range=rng, ee_sub=sub, tune=tune, balance=balance, live=live,
                                rels_weight=conv.rels_weight.detach().contiguous() if want_rel else None, rel_out=rel_out,
                                row_bounds=row_bounds)
        if wide:
            pad = torch.ones(O + 8, dtype=torch.bool, device=DEV)
            pad[4:4 + O] = False
            assert bool(torch.isnan(ow[:, pad]).all())                                 # nothing written beside the slice
            out = out.contiguous()
        return (out, rel_out) if want_rel else out


def _device(pkg, case, cus):
    key = fused_cases._key(case, cus)
    if key not in _device_cache:
        _device_cache[key] = _Device(pkg, case, cus)
    return _device_cache[key]


def _hold_to_float64(case, cus, got, rel_got=None):
    """Every element against the float64 reference at the header's bar; prints the family's worst ratio so far."""
    out, rel_out, B, y = fused_cases.reference(case, cus)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == out.shape and np.isfinite(got).all()
    ratio = np.abs(got - out) / fused_ref.bar(B)
    worst = float(ratio.max())
    _worst[case.family] = max(_worst.get(case.family, 0.0), worst)
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print('%s [%s]: worst |got - float64| / bar = %.3f at row %d column %d (family so far: %.3f)'
          % (case.name, case.family, worst, at[0], at[1], _worst[case.family]))
    assert worst <= 1.0, (case.name, worst, at, float(got[at]), float(out[at]), float(B[at]))
    if rel_got is not None:
        # an f32 dot product of D terms, any order: |fl(a . w) - a . w| <= D u sum |a||w| (u = 2^-24)
        i = fused_cases.build_inputs(case, cus)
        mag = np.abs(i.rel.numpy().astype(np.float64)) @ np.abs(i.p['rels_weight'].astype(np.float64))
        assert (np.abs(rel_got.cpu().numpy().astype(np.float64) - rel_out) <= case.D * fused_ref.U * mag + 1e-30).all()


def _bit_for_bit_promises(pkg, case, d, got, rel_got, shard):
    nat = pkg._native
    assert torch.equal(rel_got, nat.matmul(d.rel, d.conv.rels_weight.detach().contiguous()))
    assert torch.equal(d.launch(tune=0, balance=True, live=None, shard=shard), got)          # the default launch's rows
    if case.O > 128 and case.O <= 208 and case.D <= 256:                                     # one packing for both generations
        other = GEN3 if case.gen == 2 else GEN2
        assert torch.equal(d.launch(tune=other, live=case.live, shard=shard), got)


@pytest.mark.parametrize('case', GEN2_CASES, ids=repr)
def test_generation2_second_tiles(pkg, case):
    cus = _cus()
    rows = case.rows(cus)
    bm, tiles, grid, per_wg, last = _gen2_geometry(rows, cus, case.O)
    # the geometry the case is there for: an uneven split, two tiles against one, and a last tile of a single row
    assert grid == cus and sorted(set(per_wg)) == [1, 2] and per_wg[0] == 2 and per_wg[-1] == 1
    assert bm == (80 if case.O <= 128 or '80row' in case.name else 64)
    assert last == 1 or cus % 4, (rows, bm, last)                    # (16 CUs more or less keep it; the MI355X has 256)
    d = _device(pkg, case, cus)
    i, csr = d.i, d.csr
    assert csr.live_rowptr is not None and csr.num_dead_slots > 0
    if case.hubs:                                                    # a hub in a tile that a workgroup walks second
        hub = csr.hubinfo.cpu()
        assert csr.num_chunks > 8 and bool((hub[:, bm * grid:, 1] > 0).any())
        assert bool((hub[:, rows - 1, 1] > 1).all())                 # ... the heaviest one its last, one-row tile
    else:
        assert csr.num_chunks == 0
    if case.R == 21:                                                 # the relation rows do not fit the LDS: read from memory
        assert 2 * case.R * case.D * 4 > 32 * 1024
    else:
        assert 2 * case.R * case.D * 4 <= 32 * 1024
    assert pkg._native.lib().mgcn_fused_kernel_generation(case.D, case.O, rows, 0) == 2
    shard = case.rng_pad > 0
    got, rel_got = d.launch(tune=GEN2, live=case.live, shard=shard, wide=case.wide, want_rel=True)
    _hold_to_float64(case, cus, got, rel_got)
    _bit_for_bit_promises(pkg, case, d, got, rel_got, shard)
    if shard:
        assert torch.equal(d.launch(tune=GEN2, live=case.live), got)                         # the range from the whole table
    pkg._native.check_fused_status(DEV)


_TILES = {                                         # (bounds, forced height) -> the tiles of every run, as the case means them
    ((0, 80, 161), 5): [[80], [80, 1]],
    ((0, 64, 128, 161), 4): [[64], [64], [33]],
    ((0, 64, 161), 4): [[64], [64, 33]],
    ((0, 48, 97, 161), 3): [[48], [48, 1], [48, 16]],
    ((0, 96, 161), 3): [[48, 48], [48, 17]],
    ((0, 80, 161), 3): [[48, 32], [48, 33]],       # 256-column passes: 3 row tiles beside two staging buffers
}


@pytest.mark.parametrize('case', GEN3_CASES, ids=repr)
def test_generation3_tiles_of_a_run(pkg, case):
    cus = _cus()
    rows = case.rows(cus)
    bm, run_tiles = _gen3_geometry(rows, cus, case.O, case.bounds, case.nrt)
    assert bm == 16 * case.nrt                                        # the height the case means is the one the cap allows
    if case.bounds is not None:
        assert rows == 161 and run_tiles == _TILES[(tuple(case.bounds), case.nrt)]
    elif case.O <= 208:                                               # equal runs of 96 rows: an 80-row tile, then a 16-row tile
        assert run_tiles[0] == [80, 16] and all(t == [80, 16] for t in run_tiles[:-1]) and len(run_tiles) > cus // 2
    else:
        assert run_tiles[0] == [48, 48] and all(t == [48, 48] for t in run_tiles[:-1]) and len(run_tiles) > cus // 2
    d = _device(pkg, case, cus)
    csr = d.csr
    assert csr.live_rowptr is not None and csr.num_dead_slots > 0
    if case.hubs:                                                     # the heaviest hub is the second tile of the second run
        hub = csr.hubinfo.cpu()
        assert csr.num_chunks > 8 and run_tiles[-1][-1] == 1 and bool((hub[:, rows - 1, 1] > 1).all())
    shard = case.rng_pad > 0
    tune = GEN3 | case.tune | case.nrt
    got, rel_got = d.launch(tune=tune, live=case.live, row_bounds=case.bounds, shard=shard, want_rel=True)
    _hold_to_float64(case, cus, got, rel_got)
    _bit_for_bit_promises(pkg, case, d, got, rel_got, shard)
    if not case.tune:                                                 # the same runs, the tile height left to the launch
        assert torch.equal(d.launch(tune=GEN3, live=case.live, row_bounds=case.bounds, shard=shard), got)
    if shard:
        assert torch.equal(d.launch(tune=tune, live=case.live, row_bounds=case.bounds), got)   # the range from the whole table
    pkg._native.check_fused_status(DEV)


def test_row_bounds_are_checked_before_any_launch(pkg):
    """`row_bounds=` raises NativeError for runs the launch does not assume, and `out` stays as it was."""
    nat = pkg._native
    case = GEN3_CASES[0]
    d = _device(pkg, case, _cus())
    want = d.launch(tune=GEN3, row_bounds=[0, 80, 161])
    for bad in ([0, 48, 96, 161],                       # a run of 65 rows: 161 rows in 3 runs allow 64
                [0, 80, 160], [0, 80, 80, 161], [0, 100, 90, 161], [1, 80, 161], [0]):
        with pytest.raises(nat.NativeError):
            d.launch(tune=GEN3, row_bounds=bad)
    conv, bn = d.conv, d.conv.ent_bn
    out = torch.full((161, case.O), float('nan'), device=DEV)
    for bad in (torch.tensor([0, 80, 161], dtype=torch.int32),                               # not on the device
                torch.tensor([0, 80, 161], dtype=torch.int64, device=DEV),
                torch.tensor([[0, 80, 161]], dtype=torch.int32, device=DEV),
                torch.tensor([0, 0, 80, 0, 161], dtype=torch.int32, device=DEV)[::2]):       # not contiguous
        with pytest.raises(nat.NativeError):
            nat.layer_fwd_fused(d.csr, d.x, d.rel, conv.loop_rel.reshape(-1), d.table, True, conv.loop_edge.reshape(-1),
                                d.wpack(3), case.O, conv.bias, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out,
                                tune=GEN3, live=False, row_bounds=bad)
    assert bool(torch.isnan(out).all())
    # one run per row is within the rule (161 runs of one row), and the rows do not depend on the runs
    assert torch.equal(d.launch(tune=GEN3, row_bounds=list(range(162))), want)
    nat.check_fused_status(DEV)
