"""The column cut of the fused layer kernels on the GPU (include/mgcn_hip.h (2b) "Column cut"): for 128 < D <= 256 generations 2
and 3 cut a row where its 128-byte lines say (D = 200: 96 | 104 instead of 128 | 72) and lanes past a chunk's width load the
chunk's last float4 instead of the row's head. The k-blocks, their order and the packed weights are those of the legacy cut
(`tune` bit 14), so in every case below

  * the rows of the new cut are torch.equal to the legacy cut's, and
  * every element meets the header's bar 4 * 2^-24 * B + 2e-7 against the float64 reference (tests/fused_ref.py).

Inputs and references are those of tests/fused_cases.py (cases built here from its Case; cached there per shape).
The poisoned launches hold x, the relation rows, the self-loop vectors and the per-edge table inside NaN: x as a column slice of a
wider buffer (every column >= D of its padded rows is NaN) with NaN rows before the first and after the last, the others with
NaN before and behind them (the per-edge table and the relation rows have no row stride: the launch reads them with stride D).
A lane that loaded anything outside its chunk's valid columns at either end of those arrays, or past D in any x row, would carry
NaN into a sum or, through 0 * NaN, into the zeros it stores."""
import numpy as np
import pytest
import torch

from . import fused_cases, fused_ref
from .fused_cases import GEN2, GEN3, Case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LEGACY = 1 << 14                       # `tune` bit 14: the legacy cut
B5 = [0, 80, 161]

_n161 = lambda c: 161
_one = lambda c: 80 * c + 1

WIDTHS = [Case('cut-%dx200' % D, 'cut widths', 2, D, 200, _n161) for D in (132, 160, 196, 200, 228, 256)]
WIDTHS.append(Case('cut-200x200-second-tile', 'cut widths', 2, 200, 200, _one))
VARIANTS = [
    Case('cut-200x200-live', 'cut variants', 2, 200, 200, _n161, live=True),
    Case('cut-200x200-canonical', 'cut variants', 2, 200, 200, _n161, live=False),
    Case('cut-200x200-hubs', 'cut variants', 2, 200, 200, _n161, hubs=True),
    Case('cut-200x200-strides', 'cut variants', 2, 200, 200, _n161, wide=True),
    Case('cut-200x200-range', 'cut variants', 2, 200, 200, _n161, rng_pad=16),
    Case('cut-200x200-rel21', 'cut variants', 2, 200, 200, _n161, R=21),
] + [Case('cut-200x%d' % O, 'cut narrow outputs', 2, 200, O, _n161) for O in (8, 64, 128)]

_cache = {}


def _cus():
    return int(torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count)


def _poisoned(t, rows_before=1, rows_after=1, cols_after=0):
    """`t` as a view into a NaN-filled buffer: NaN rows before and after, NaN columns behind every row (16-byte aligned)."""
    t2 = t.reshape(-1, t.size(-1)) if t.dim() > 1 else t.reshape(1, -1)
    if t.dim() == 1:                                   # a vector: 4 NaN floats before, 4 behind
        buf = torch.full((t.numel() + 8,), float('nan'), device=DEV, dtype=t.dtype)
        buf[4:4 + t.numel()] = t
        return buf[4:4 + t.numel()]
    buf = torch.full((t2.size(0) + rows_before + rows_after, t2.size(1) + cols_after), float('nan'), device=DEV, dtype=t.dtype)
    buf[rows_before:rows_before + t2.size(0), :t2.size(1)] = t2
    return buf[rows_before:rows_before + t2.size(0), :t2.size(1)]


class _Device(object):
    """A case's operands on the GPU (as tests/test_gpu_fused_tiles.py builds them); shared by the cases that share inputs."""

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
        self.packed = {}

    def wpack(self, gen):
        if gen not in self.packed:
            wcat, wp = self.conv.derived_weights()
            self.packed[gen] = wp if gen == 0 else self.pkg._native.pack_weights(wcat, generation=gen)
        return self.packed[gen]

    def launch(self, tune, live=False, row_bounds=None, shard=False, wide=False, poison=False):
        nat, conv, bn, csr, i, O = self.pkg._native, self.conv, self.conv.ent_bn, self.csr, self.i, self.O
        n0, n1 = i.n0, i.n1
        rng = (n0, n1) if (n0, n1) != (0, i.N) else None
        x, rel, out = self.x, self.rel, torch.full((n1 - n0, O), float('nan'), device=DEV)
        loop_rel, loop_edge = conv.loop_rel.detach().reshape(-1), conv.loop_edge.detach().reshape(-1)
        ee, sub = self.table, (0, 0, 0)
        if shard:
            ee, sub = csr.edge_table_shard(self.table, n0, n1), csr.shard_ee_sub(n0, n1)
            assert sub[0] > 0 and sub[1] > 0 and ee.size(0) < self.table.size(0)
        if wide or poison:                                                             # ldx > D (and, wide, ldo > O)
            x = _poisoned(x, cols_after=12)
            assert x.stride(0) == x.size(1) + 12 and x.data_ptr() % 16 == 0
        if wide:
            ow = torch.full((n1 - n0, O + 8), float('nan'), device=DEV)
            out = ow[:, 4:4 + O]
        if poison:
            rel, ee, loop_rel, loop_edge = _poisoned(rel), _poisoned(ee), _poisoned(loop_rel), _poisoned(loop_edge)
            assert rel.is_contiguous() and ee.is_contiguous() and ee.data_ptr() % 16 == 0 and loop_rel.data_ptr() % 16 == 0
        if row_bounds is not None:
            row_bounds = torch.tensor(row_bounds, dtype=torch.int32, device=DEV)
        with torch.no_grad():
            nat.layer_fwd_fused(csr, x, rel, loop_rel, ee, True, loop_edge, self.wpack(nat.tune_generation(tune)), O, conv.bias,
                                bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out, node_range=rng, ee_sub=sub,
                                tune=tune, balance=False, live=live, row_bounds=row_bounds)
        if wide:
            pad = torch.ones(O + 8, dtype=torch.bool, device=DEV)
            pad[4:4 + O] = False
            assert bool(torch.isnan(ow[:, pad]).all())                                 # nothing written beside the slice
            out = out.contiguous()
        return out


def _device(pkg, case, cus):
    key = fused_cases._key(case, cus)
    if key not in _cache:
        _cache[key] = _Device(pkg, case, cus)
    return _cache[key]


def _hold_to_float64(case, cus, got):
    out, _, B, _ = fused_cases.reference(case, cus)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == out.shape and np.isfinite(got).all()
    ratio = np.abs(got - out) / fused_ref.bar(B)
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print('%s: worst |got - float64| / bar = %.3f at row %d column %d' % (case.name, float(ratio.max()), at[0], at[1]))
    assert float(ratio.max()) <= 1.0, (case.name, float(ratio.max()), at, float(got[at]), float(out[at]), float(B[at]))


def _cut_moves(pkg, D):
    return pkg._native.fused_cut(D)[0] != pkg._native.fused_cut(D, legacy=True)[0]


@pytest.mark.parametrize('case', WIDTHS + VARIANTS, ids=repr)
def test_new_cut_gives_the_legacy_rows(pkg, case):
    cus = _cus()
    nat = pkg._native
    assert nat.fused_cut(200)[0] == [(0, 96), (96, 104)] and _cut_moves(pkg, 132) and not _cut_moves(pkg, 228) and not _cut_moves(pkg, 256)
    assert nat.lib().mgcn_fused_kernel_generation(case.D, case.O, case.rows(cus), 0) == 2
    d = _device(pkg, case, cus)
    if case.hubs:                                                    # the heaviest hub is the last row
        hub = d.csr.hubinfo.cpu()
        assert d.csr.num_chunks > 8 and bool((hub[:, case.rows(cus) - 1, 1] > 1).all())
    if case.R == 21:                                                 # the relation rows do not fit the LDS: read from memory
        assert 2 * case.R * case.D * 4 > 32 * 1024
    shard = case.rng_pad > 0
    kw = dict(live=case.live, shard=shard, wide=case.wide)
    got = d.launch(GEN2, **kw)
    _hold_to_float64(case, cus, got)
    assert torch.equal(got, d.launch(GEN2 | LEGACY, **kw))
    if case.name.endswith('canonical') or case.name.endswith('live'):    # the other walk of the slots: the same rows again
        assert torch.equal(got, d.launch(GEN2, live=not case.live))
    nat.check_fused_status(DEV)


@pytest.mark.parametrize('D', [132, 200, 256])
def test_generation3_with_the_cut_equals_generation2(pkg, D):
    cus = _cus()
    case = Case('cut-%dx200' % D, 'cut widths', 2, D, 200, _n161)
    d = _device(pkg, case, cus)
    want = d.launch(GEN2)
    got = d.launch(GEN3, row_bounds=B5)
    _hold_to_float64(case, cus, got)
    assert torch.equal(got, want)
    assert torch.equal(d.launch(GEN3 | LEGACY, row_bounds=B5), want)
    assert torch.equal(d.launch(GEN3, row_bounds=B5, live=True), want)
    pkg._native.check_fused_status(DEV)


@pytest.mark.parametrize('D', [132, 196, 200])
def test_idle_lanes_read_nothing_outside_their_chunk(pkg, D):
    cus = _cus()
    case = Case('cut-%dx200' % D, 'cut widths', 2, D, 200, _n161)
    d = _device(pkg, case, cus)
    want = d.launch(GEN2)
    for tune, bounds in ((GEN2, None), (GEN3, B5)):
        got = d.launch(tune, row_bounds=bounds, poison=True)
        assert not bool(torch.isnan(got).any())
        assert torch.equal(got, want)
    pkg._native.check_fused_status(DEV)
