"""tests/fused_ref.py, the float64 yardstick of the fused layer kernels, checked where no GPU is needed:

* against oracle.layer_forward on the committed golden fixtures (which tests/test_oracle_golden.py pins to the reference bit for
  bit), to the f32 ordering noise test_build_order_within_rounding_of_reference_order already allows there (2e-5);
* on the exact inputs of every case of tests/test_gpu_fused_tiles.py (tests/fused_cases.py, at the MI355X's 256 CUs):
  - a straightforward f32 evaluation (numpy f32, messages summed in slot order, then `@`) stays within the bar
    4 * 2^-24 * B + 2e-7 of include/mgcn_hip.h (2b): the bar is one that the reference arithmetic alone meets;
  - the comparison is not emptied by tanh saturation: at most 10 % of a case's elements have |y| >= 2 and mean |out| > 0.05
    (a condition on the inputs, not a tolerance);
  - the bar is sharp: four value-only perturbations of the f32 evaluation each exceed it on at least one element — one slot
    dropped from one row, two destination rows of a tile swapped, one 32-wide k-block of one mode's weights zeroed, the BN scale
    taken from the neighbouring column;
* the host part of `_native.layer_fwd_fused(row_bounds=)`: the checks a caller's runs must pass before any launch."""
import numpy as np
import pytest
import torch

from . import fused_cases, fused_ref
from .conftest import ALL_CASES, golden


@pytest.mark.parametrize('name', ALL_CASES)
def test_reference_agrees_with_the_oracle_on_the_golden_fixtures(oracle, name):
    g = golden(name)
    sd = g.state_dict()
    ei, ea = g.t('dl_edge_index'), g.t('dl_edge_attr')
    ee = sd['edge_embeddings'].index_select(0, ea[1])
    want_ent, want_rel = oracle.layer_forward(sd, 'conv1.', sd['entity_embedding'], ei, ea[0], ee, sd['relation_embedding'])
    c = lambda k: sd['conv1.' + k].numpy()
    p = dict(in_weight=c('in_weight'), out_weight=c('out_weight'), loop_weight=c('loop_weight'), rels_weight=c('rels_weight'),
             loop_rel=c('loop_rel').reshape(-1), loop_edge=c('loop_edge').reshape(-1),
             bias=c('bias') if sd.get('conv1.bias') is not None else None, bn_mean=c('ent_bn.running_mean'),
             bn_var=c('ent_bn.running_var'), bn_gamma=c('ent_bn.weight'), bn_beta=c('ent_bn.bias'), eps=1e-5)
    out, rel_out, B, y = fused_ref.layer_f64(p, sd['entity_embedding'].numpy(), sd['relation_embedding'].numpy(), ee.numpy(),
                                             ei.numpy(), ea[0].numpy())
    assert out.dtype == np.float64 and out.shape == tuple(want_ent.shape) and B.shape == out.shape and (B >= 0).all()
    np.testing.assert_allclose(out, want_ent.numpy().astype(np.float64), rtol=0, atol=2e-5)
    np.testing.assert_allclose(rel_out, want_rel.numpy().astype(np.float64), rtol=0, atol=2e-5)
    np.testing.assert_allclose(np.tanh(y), out, rtol=0, atol=1e-15)
    assert float(np.abs(out).mean()) > 1e-3


def _perm(pkg, i):
    host = pkg._native.csr_build_host(i.N, 2 * i.R + 1, i.ei, i.et, **i.hub_kw)
    perm = host['perm'].numpy()
    assert sorted(perm.tolist()) == list(range(i.ei.size(1)))                 # a permutation of the edges: slot -> edge
    return perm, host


@pytest.mark.parametrize('case', fused_cases.CASES, ids=repr)
def test_f32_evaluation_meets_the_bar_and_the_bar_is_sharp(pkg, case):
    i = fused_cases.build_inputs(case)
    out, rel_out, B, y = fused_cases.reference(case)
    bar = fused_ref.bar(B)
    rows = slice(i.n0, i.n1)
    assert out.shape == (i.rows, case.O) and np.isfinite(out).all()
    # the conditions on the inputs: the tanh is not saturated, the outputs are not all near zero
    saturated = float((np.abs(y) >= 2).mean())
    assert saturated <= 0.10, saturated
    assert float(np.abs(out).mean()) > 0.05
    perm, host = _perm(pkg, i)
    if case.hubs:
        assert host['num_chunks'] > 8
    ev = lambda p=i.p, **kw: fused_ref.layer_f32_slots(p, i.x.numpy(), i.rel.numpy(), i.ee.numpy(), i.ei.numpy(), i.et.numpy(),
                                                       perm, **kw)[rows].astype(np.float64)
    got = ev()
    ratio = np.abs(got - out) / bar
    print('%s: f32 evaluation, worst |f32 - f64| / bar = %.3f; |y| >= 2 on %.1f %% of the elements, mean |out| = %.3f'
          % (case.name, float(ratio.max()), 100 * saturated, float(np.abs(out).mean())))
    assert float(ratio.max()) <= 1.0

    exceeds = lambda v: bool((np.abs(v - out) > bar).any())
    E = i.ei.size(1) // 2
    # one slot dropped from one row: a live in-half slot of the 40-slot destination
    big = i.N - 11
    assert i.n0 <= big < i.n1
    slots = np.flatnonzero((i.ei[1].numpy()[perm] == big) & (perm < E))
    assert len(slots) >= 40
    dropped = ev(drop_slot=int(slots[len(slots) // 2]))
    changed = np.flatnonzero((dropped != got).any(1))
    assert changed.tolist() == [big - i.n0] and exceeds(dropped)
    # two destination rows of a tile swapped (both in the same 16-row tile of the launch's last full tile)
    a, b = i.rows - 3, i.rows - 2
    assert a // 16 == b // 16
    swapped = got.copy()
    swapped[[a, b]] = swapped[[b, a]]
    assert exceeds(swapped)
    # one 32-wide k-block of one mode's weights zeroed
    w = np.array(i.p['in_weight'])
    w[32:64] = 0
    assert exceeds(ev(dict(i.p, in_weight=w)))
    # scale taken from the neighbouring column
    assert exceeds(ev(scale_shift=1))


def test_row_bounds_host_checks(pkg):
    nat = pkg._native
    assert [nat.row_bounds_cap(161, g) for g in (1, 2, 3, 4)] == [240, 160, 64, 48]
    assert nat.row_bounds_cap(80, 1) == 80 and nat.row_bounds_cap(81, 1) == 160 and nat.row_bounds_cap(5, 3) == 16
    for ok in ([0, 80, 161], [0, 64, 128, 161], [0, 48, 97, 161], [0, 96, 161], [0, 161], [0, 1, 161], list(range(162))):
        nat.check_row_bounds(ok, 161)
    nat.check_row_bounds(list(range(0, 16 * 4096 + 1, 16)), 16 * 4096)      # 4096 runs
    for bad in ([0, 48, 96, 161],                    # 65 rows in a run where 161 rows in 3 runs allow 64
                [0, 161, 161], [0, 80, 80, 161],     # an empty run
                [0, 100, 90, 161],                   # decreasing
                [1, 80, 161], [0, 80, 160], [0, 80, 162], [-1, 80, 161],
                [0], [], [161],
                list(range(0, 16 * 4097 + 1, 16))):     # 4097 runs
        with pytest.raises(nat.NativeError):
            nat.check_row_bounds(bad, 16 * 4097 if len(bad) > 1000 else 161)
    # the tensor itself: int32, one-dimensional, contiguous, on the launch's device
    x = torch.zeros(4, 4)
    for bad in ([0, 80, 161], torch.tensor([0, 80, 161]), torch.tensor([0, 80, 161], dtype=torch.int32),
                torch.tensor([[0, 80, 161]], dtype=torch.int32)):
        with pytest.raises(nat.NativeError):
            nat._checked_row_bounds(bad, 161, x)
