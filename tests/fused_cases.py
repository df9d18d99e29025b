"""The cases of tests/test_gpu_fused_tiles.py and their inputs, built on the CPU from seeds alone, so that
tests/test_fused_ref_host.py checks on a machine without a GPU exactly the inputs the kernels are then held to.

A case's row count is a function of the device's CU count (`cus`): the launch arithmetic of the fused kernels — how many tiles
a workgroup walks, how tall they are, how ragged the last one is — depends on it (see the GPU test's module docstring). The
host test takes the MI355X's 256.

Graphs come from tests/live_graphs.py (about 30 % of the nodes are no source of a half: their slots are dead, so every graph has
a live view; E about 1.5 N per half; one destination of 40 slots, more than a 32-slot record chunk, near the END of the rows so
that it lies in a tile a workgroup reaches second). `hubs`: a Zipf(1.1) draw of extra destinations on top, the heaviest one
the LAST row (in every case with hubs the launch's last tile is that one row, walked second by its workgroup). Input scales are those of tests/test_gpu_live_slots.py::_Layer; the layer's parameters are
oracle.init_layer_state's (xavier weights, non-trivial BN statistics, gamma in [0.5, 1.5], a bias)."""
import importlib

import numpy as np
import torch

from .live_graphs import edge_list, random_halves

MI355X_CUS = 256
GEN2, GEN3 = 0x800, 0xc00            # `tune` bits 10-11: force the lockstep / the elastic kernel
NCH2 = 2 << 12                       # `tune` bits 12-13 = 2: 256-column passes (generation 3)


class Case(object):
    def __init__(self, name, family, gen, D, O, rows, R=3, hubs=False, rng_pad=0, bounds=None, tune=0, live=False, ee16=False,
                 wide=False, nrt=0):
        self.name, self.family, self.gen, self.D, self.O, self.R = name, family, gen, D, O, R
        self.rows = rows               # callable: cus -> rows of the launch
        self.hubs = hubs               # Zipf destinations, hub_threshold = 8, hub_chunk = 4
        self.rng_pad = rng_pad         # > 0: the launch is destinations [7, 7 + rows) of a graph of rows + rng_pad nodes
        self.bounds = bounds           # generation 3: the caller's runs (row_bounds=), else None
        self.tune = tune               # further `tune` bits
        self.live, self.ee16, self.wide = live, ee16, wide   # live view / bf16 table / x and out as column slices
        self.nrt = nrt                 # generation 3: row tiles per tile the case means to reach (forced: `tune` bits 0-3)

    def __repr__(self):
        return self.name


_one = lambda c: 80 * c + 1            # 64-row tiles on generation 2: some workgroups walk two tiles, the last tile has one row
_two = lambda c: 128 * c + 33          # 80-row tiles win the makespan rule: two tiles against one
_n161 = lambda c: 161

GEN2_CASES = [
    Case('g2-100x200', 'gen2 64-row tiles', 2, 100, 200, _one),
    Case('g2-200x200', 'gen2 64-row tiles', 2, 200, 200, _one),
    Case('g2-200x200-80row', 'gen2 80-row tiles', 2, 200, 200, _two),
    Case('g2-36x8', 'gen2 narrow outputs', 2, 36, 8, _one),
    Case('g2-36x64', 'gen2 narrow outputs', 2, 36, 64, _one),
    Case('g2-132x128', 'gen2 narrow outputs', 2, 132, 128, _one),
    Case('g2-100x200-range', 'gen2 range, shard, strides', 2, 100, 200, _one, rng_pad=16, wide=True),
    Case('g2-100x200-hubs', 'gen2 hubs', 2, 100, 200, _one, hubs=True),
    # (42 relation rows x 100 columns still fit the 32 KiB the relation table may take in LDS: the 200-wide first case it is)
    Case('g2-200x200-rel21', 'gen2 relation rows from memory', 2, 200, 200, _one, R=21),
    Case('g2-200x200-live', 'gen2 live view', 2, 200, 200, _one, live=True),
    Case('g2-100x200-bf16', 'gen2 bf16 table', 2, 100, 200, _one, ee16=True),
]

B5, B4, B3, B32, B4L = [0, 80, 161], [0, 64, 128, 161], [0, 48, 97, 161], [0, 96, 161], [0, 64, 161]
GEN3_CASES = [Case('g3-%dx%d-%s' % (D, O, '_'.join(map(str, b))), 'gen3 NRT=%d' % nrt, 3, D, O, _n161, bounds=b, nrt=nrt)
              for D, O in ((100, 200), (260, 200)) for b, nrt in ((B5, 5), (B4, 4), (B3, 3))]
GEN3_CASES += [Case('g3-%dx%d-0_96_161' % (D, O), 'gen3 32 column tiles', 3, D, O, _n161, bounds=B32, nrt=3)
               for D, O in ((100, 212), (1024, 512))]
GEN3_CASES += [
    # (the 4-row-tile runs above are one tile each; the same height forced where the second run has a later tile: 64 + 33 rows)
    Case('g3-100x200-0_64_161', 'gen3 NRT=4', 3, 100, 200, _n161, bounds=B4L, nrt=4),
    Case('g3-100x200-equal-runs', 'gen3 equal runs', 3, 100, 200, _one, nrt=5),
    Case('g3-100x212-equal-runs', 'gen3 equal runs', 3, 100, 212, _one, nrt=3),
    Case('g3-100x200-0_80_161-hubs', 'gen3 hubs', 3, 100, 200, _n161, bounds=B5, nrt=5, hubs=True),
    Case('g3-100x200-0_80_161-range', 'gen3 range, shard', 3, 100, 200, _n161, bounds=B5, nrt=5, rng_pad=16),
    Case('g3-200x200-0_80_161-live', 'gen3 live view', 3, 200, 200, _n161, bounds=B5, nrt=5, live=True),
    # (two staging buffers of 200 columns beside the image leave room for 3 row tiles: 48-row tiles, two in each run)
    Case('g3-200x200-0_80_161-256col', 'gen3 256-column passes', 3, 200, 200, _n161, bounds=B5, nrt=3, tune=NCH2),
]
CASES = GEN2_CASES + GEN3_CASES


def _edges(N, R, hubs, seed=11):
    big = N - 11                                                    # N = 161: row 150, in the second run of [0, 80, 161]
    halves = [list(h) for h in random_halves(N, R, 0.3, seed, big=(big, 40), max_in=2)]
    if hubs:
        rng = np.random.default_rng(seed + 1)
        extra = max(N // 4, 60)
        for h in halves:
            h.append((N - 1, int(h[0][1]), 0))                     # the last row is a source of the half: its slots are live
            srcs = np.unique(np.asarray([int(e[0]) for e in h]))   # destinations among the half's sources: live slots
            order = rng.permutation(srcs[srcs != big])
            last = int(np.flatnonzero(order == N - 1)[0])
            order[[0, last]] = order[[last, 0]]                    # the heaviest hub is the LAST row: a one-row tile walked second
            pr = 1.0 / np.arange(1, len(order) + 1) ** 1.1
            dst = order[rng.choice(len(order), size=extra, p=pr / pr.sum())]
            src = srcs[rng.integers(0, len(srcs), size=extra)]
            h += [(int(s), int(d), int(t)) for s, d, t in zip(src, dst, rng.integers(0, 2 * R, size=extra))]
    return edge_list(*halves)


_inputs = {}


def _key(case, cus):
    """What a case's inputs depend on: cases that differ only in how they are launched share inputs and reference."""
    return (int(case.rows(cus)), case.rng_pad, case.R, case.hubs, case.D, case.O, case.ee16)


class Inputs(object):
    pass


def build_inputs(case, cus=MI355X_CUS):
    """Everything of a case that does not need a GPU: graph size and edge list, the destination range, the layer's state dict
    and the same parameters as arrays for fused_ref, x, rel and the per-edge table in REFERENCE edge order (a bf16 case: already
    rounded to bf16 and widened, so the reference runs on the widened table). Cached per case and CU count."""
    key = _key(case, cus)
    if key in _inputs:
        return _inputs[key]
    oracle = importlib.import_module('oracle.mgcn_oracle')
    rows = int(case.rows(cus))
    N = rows + case.rng_pad
    i = Inputs()
    i.N, i.R, i.rows = N, case.R, rows
    i.n0, i.n1 = (7, 7 + rows) if case.rng_pad else (0, N)
    i.hub_kw = dict(hub_threshold=8, hub_chunk=4) if case.hubs else dict(hub_threshold=0)
    i.ei, i.et = _edges(N, case.R, case.hubs)
    g = torch.Generator().manual_seed(1)
    i.sd = oracle.init_layer_state('', case.D, case.O, g, bias=True)
    g = torch.Generator().manual_seed(2)
    E2 = i.ei.size(1)
    i.x = torch.randn(N, case.D, generator=g) * 0.4
    i.rel = torch.randn(2 * case.R, case.D, generator=g) * 0.5
    i.ee = torch.randn(E2, case.D, generator=g) * 0.5
    if case.ee16:
        i.ee = i.ee.to(torch.bfloat16).float()
    sd = i.sd
    i.p = dict(in_weight=sd['in_weight'].numpy(), out_weight=sd['out_weight'].numpy(), loop_weight=sd['loop_weight'].numpy(),
               rels_weight=sd['rels_weight'].numpy(), loop_rel=sd['loop_rel'].numpy().reshape(-1),
               loop_edge=sd['loop_edge'].numpy().reshape(-1), bias=sd['bias'].numpy(), bn_mean=sd['ent_bn.running_mean'].numpy(),
               bn_var=sd['ent_bn.running_var'].numpy(), bn_gamma=sd['ent_bn.weight'].numpy(), bn_beta=sd['ent_bn.bias'].numpy(),
               eps=1e-5)
    _inputs[key] = i
    return i


_refs = {}


def reference(case, cus=MI355X_CUS):
    """fused_ref.layer_f64 on the case's inputs, the rows of its destination range: (out, rel_out, B, y), computed once."""
    from . import fused_ref
    key = _key(case, cus)
    if key not in _refs:
        i = build_inputs(case, cus)
        out, rel_out, B, y = fused_ref.layer_f64(i.p, i.x.numpy(), i.rel.numpy(), i.ee.numpy(), i.ei.numpy(), i.et.numpy())
        for a in (out, rel_out, B, y):
            a.setflags(write=False)
        _refs[key] = (out[i.n0:i.n1], rel_out, B[i.n0:i.n1], y[i.n0:i.n1])
    return _refs[key]
