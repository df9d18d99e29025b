"""Host-side checks of tests/trunk_ref.py (no GPU): the float64 trunk reference against the oracle, the folded form the
pack kernel builds against the unfolded one, the constants of dense_ref.py re-measured at the lengths the trunk brings (a
test fails when an emulation comes within a factor 2 of its constant), the launch arithmetic LIMIT_GRID is there for (with the
workspace entry point, which needs no GPU), that the bar still bites at many taps, and the C ABI's new names. Figures are printed
(`pytest -s`)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from . import dense_ref as R
from . import trunk_ref as T
from .conftest import ROOT, golden

U = R.U
NAMES = ('mgcn_conve_packed_bytes', 'mgcn_conve_pack', 'mgcn_conve_trunk_workspace', 'mgcn_conve_trunk_fwd')
IDS = [T.case_id(c) for c in T.GRID]
ALL = T.GRID + T.LIMIT_GRID
ALL_IDS = [T.case_id(c) for c in ALL]


def test_grid_holds_the_required_shapes():
    assert T.PRODUCTION == (10, 20, 7, 200, False)
    for name, bias in (('toy_small', False), ('syn_a', True), ('syn_b', False)):
        hp = golden(name).hp
        assert (hp['k_w'], hp['k_h'], hp['kernel_size'], hp['num_filter'], bool(hp['bias'])) in T.GRID, name
        assert bool(hp['bias']) == bias
    for name in ('toy_d100', 'syn_c'):
        hp = golden(name).hp
        assert (hp['k_w'], hp['k_h'], hp['kernel_size'], hp['num_filter'], bool(hp['bias'])) == T.PRODUCTION
    assert (16, 32, 5, 32, True) in T.GRID
    assert any(c[2] == 1 for c in T.GRID)
    assert any(T.sizes(c)[2] % 32 != 0 for c in T.GRID)
    for c in T.GRID:
        assert c[0] * c[1] <= 512 and 1 <= c[2] <= min(2 * c[0], c[1])


def test_limit_grid_reaches_what_it_is_there_for(pkg):
    """The launch arithmetic of csrc/conve_trunk.hip restated per geometry of LIMIT_GRID (GRID itself stays as it is): a later
    change of a constant or of the list cannot silently empty a case."""
    assert T.GRID[0] == T.PRODUCTION and len(T.GRID) == 7 and not set(T.GRID) & set(T.LIMIT_GRID)
    assert T.LIMIT_BATCHES == (1, 63, 333)
    fig = {c: T.launch_figures(c) for c in T.LIMIT_GRID}
    lib = pkg._native.lib()
    for c in T.LIMIT_GRID:
        assert c[0] * c[1] <= 512 and 1 <= c[2] <= min(2 * c[0], c[1])
        assert pkg._native.conve_supported(*T.geometry(c))
    assert fig[(4, 8, 8, 8, True)]['T'] + 1 == 65 and fig[(4, 8, 8, 8, True)]['K'] == 8
    assert fig[(16, 32, 32, 3, False)]['T'] == 1024 and fig[(16, 32, 32, 3, False)]['NCG'] == 3 and 16 * 32 == 512
    assert fig[(16, 32, 17, 4, True)]['T'] + 1 == 290 > 256 and fig[(16, 32, 17, 4, True)]['P'] == 256
    assert fig[(10, 20, 9, 32, False)]['T'] + 1 == 82 and fig[(10, 20, 9, 32, False)]['P'] == 144
    assert (10, 20, 9, 32, False)[:2] == T.PRODUCTION[:2]
    assert (4, 8, 4, 300, True)[3] > 256 and fig[(4, 8, 4, 300, True)]['K'] == 7500
    assert (4, 8, 3, 1, False)[3] == 1                        # for (; f + 1 < F; f += 2) never iterates
    assert fig[(5, 8, 6, 7, True)]['K'] == 105
    assert {c[2] for c in T.LIMIT_GRID} >= {4, 6, 8, 9, 17, 32}            # the generic convolution (KS = 0) with a real kernel
    # one output position, and P <= 4: one segment, so plan_make returns nsplit = 0 and no batch has a workspace
    assert [c for c in T.LIMIT_GRID if fig[c]['P'] == 1] == [(4, 8, 8, 8, True), (16, 32, 32, 3, False)]
    assert fig[(2, 4, 3, 5, False)]['P'] == 4
    for c in T.LIMIT_GRID:
        nbytes = [lib.mgcn_conve_trunk_workspace(b, *T.geometry(c)) for b in (1, 2, 16, 63, 333, 8192, 8193, 100000)]
        if fig[c]['P'] <= 4:
            assert fig[c]['PQ'] == 1 and nbytes == [0] * 8, c
        else:
            assert fig[c]['PQ'] > 1 and all(n > 0 for n in nbytes[:6]) and nbytes[6:] == [0, 0], c
    # a second segment that is half zero-weight padding
    assert fig[(3, 5, 4, 3, True)]['P'] == 6 and fig[(3, 5, 4, 3, True)]['PQ'] == 2


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_reference_equals_oracle_in_float64(oracle, case):
    """Pins the interleaved image layout and the flatten order."""
    sd = {k: v.double() for k, v in T.weights(case).items()}
    s, r = T.queries(case, 5)
    want = oracle.conve_trunk(sd, T.hyper(case), s.double(), r.double())
    got, bar = T.ref_trunk(case, sd, s, r)
    err = float((got - want).abs().max())
    print('%s: |ref - oracle64| = %.3g, largest bar %.3g' % (T.case_id(case), err, float(bar.max())))
    assert err <= 1e-12
    assert float(got.max()) > 0.1 and float((got > 0).double().mean()) > 0.2      # the relus leave something to compare


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_folded_form_equals_unfolded_in_float64(case):
    sd = T.weights(case)
    s, r = T.queries(case, 5)
    want, _ = T.ref_trunk(case, sd, s, r)
    got = T.ref_trunk_folded(case, sd, s, r)
    err = float((got - want).abs().max())
    print('%s: |folded - unfolded| = %.3g' % (T.case_id(case), err))
    assert err <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('k', [49, 39200])
@pytest.mark.parametrize('left', ['signed', 'nonneg'])
def test_sequential_f32_chain_at_trunk_lengths(k, left):
    """C_DOT = 10 rests on 2.50 u mag measured up to K = 300; the trunk brings K = ks^2 = 49 and K = F H W = 39 200 (with
    non-negative left operands after the relu)."""
    g = R.gen(R.seed_of(10, k, left == 'signed'))
    a, b = R.pm_uniform((8, k), g), R.pm_uniform((k, 8), g)
    if left == 'nonneg':
        a = a.abs()
    want, mag = R.ref_matmul(a, b)
    ratio = float(((R.emul_dot_f32(a, b).double() - want).abs() / (U * mag)).max())
    print('sequential f32 chain, K = %d, %s left operand: %.2f u mag (C_DOT = %.1f)' % (k, left, ratio, R.C_DOT))
    assert ratio <= R.C_DOT / 2


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_torch_cpu_f32_trunk_sits_inside_the_bar(oracle, case):
    sd = T.weights(case)
    s, r = T.queries(case, 7)
    want, bar, pre64, m1 = T.ref_trunk(case, sd, s, r, want_conv=True)
    hp = T.hyper(case)
    # conv stage in torch-CPU f32: bn0 -> conv2d -> bn1, before the relu
    bn = lambda x, n: F.batch_norm(x, sd['conv2.%s.running_mean' % n], sd['conv2.%s.running_var' % n], sd['conv2.%s.weight' % n],
                                   sd['conv2.%s.bias' % n], False, 0.1, T.BN_EPS)
    img = torch.stack([s, r], dim=2).reshape(-1, 1, 2 * case[0], case[1])
    pre32 = bn(F.conv2d(bn(img, 'bn0'), sd['conv2.conv_e.weight'], sd.get('conv2.conv_e.bias')), 'bn1')
    r1 = float(((pre32.double() - pre64).abs() / (U * m1)).max())
    got = oracle.conve_trunk(sd, hp, s, r)
    ry = R.max_ratio(got, want, bar)
    print('%s: torch-CPU f32 conv stage %.2f u m1 (bar %.1f), output %.3f of bar_y, |y32 - y64| = %.3g'
          % (T.case_id(case), r1, R.C_DOT + R.C_EPI, ry, float((got.double() - want).abs().max())))
    assert r1 <= (R.C_DOT + R.C_EPI) / 2
    assert ry <= 0.5


@pytest.mark.parametrize('case', [(16, 32, 32, 3, False), (16, 32, 17, 4, True)], ids=T.case_id)
def test_the_bar_bites_at_many_taps(case):
    """Worst-case as bar_y is, at 1024 and 289 taps it still fails a trunk that drops the last tap of one filter or reads the
    image one column off (float64 evaluations on the CPU, so nothing but the fault is in the difference)."""
    assert case in T.LIMIT_GRID
    k_w, k_h, ks, f, _ = case
    sd = T.weights(case)
    s, r = T.queries(case, 7)
    want, bar = T.ref_trunk(case, sd, s, r)
    cut = dict(sd)
    cut['conv2.conv_e.weight'] = sd['conv2.conv_e.weight'].clone()
    cut['conv2.conv_e.weight'][f - 1, 0, ks - 1, ks - 1] = 0.0
    assert R.max_ratio(T.ref_trunk(case, cut, s, r)[0], want, bar) > 1.0
    img = torch.stack([s, r], dim=2).reshape(7, 2 * k_w, k_h).roll(1, dims=2).reshape(7, k_w * k_h, 2)
    assert R.max_ratio(T.ref_trunk(case, sd, img[:, :, 0].contiguous(), img[:, :, 1].contiguous())[0], want, bar) > 1.0


def test_header_and_binding_carry_the_trunk_entry_points(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    declared = set(re.findall(r'\b(mgcn_\w+)\s*\(', header))
    for name in NAMES:
        assert name in declared, name
        assert name in pkg._native.EXPORTS, name
    assert '#define MGCN_ABI_VERSION 4' in header and pkg._native.ABI_VERSION == 4
