"""tests/trunk_train_ref.py checked on the CPU (`-m "not gpu"`): the float64 reference against the torch modules of ConvE
in float64 with the same masks, the masks' draw order against model._drawn_dropout (dist._trunk's draws), the bars against their vacuity caps, what
the training-mode trunk's entry points (paragraph (9) of include/mgcn_hip.h) do without a GPU, and the limit cases: their
launch arithmetic, the two conditions on their inputs (caps, relu margin) and four faults that must break a bar there."""
import copy
import os
import types

import pytest
import torch

from . import dense_ref as R
from . import trunk_ref as T
from . import trunk_train_ref as TT

EINVAL, EUNSUPPORTED = 1, 3
HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_OF = {'d_conv_w': 'conv_e.weight', 'd_conv_b': 'conv_e.bias', 'd_g0': 'bn0.weight', 'd_b0': 'bn0.bias', 'd_g1': 'bn1.weight',
            'd_b1': 'bn1.bias', 'd_fc_w': 'fc.weight', 'd_fc_b': 'fc.bias'}


def conve_module(pkg, case, **over):
    params = types.SimpleNamespace(**dict(T.hyper(case), **over))
    conv = pkg.model.ConvE(params, 10)
    res = conv.load_state_dict({k[len('conv2.'):]: v for k, v in T.weights(case).items()}, strict=False)
    assert not res.unexpected_keys
    return conv.train()


@pytest.mark.parametrize('case,B', [(T.GRID[2], 17), (T.GRID[6], 5), (T.GRID[1], 2), (T.PRODUCTION, 16)]
                         + [(c, 17 if T.launch_figures(c)['P'] == 1 else 5) for c in T.LIMIT_GRID],
                         ids=lambda v: T.case_id(v) if isinstance(v, tuple) else str(v))
def test_reference_equals_the_torch_modules_in_float64(pkg, case, B):
    """ConvE's own torch branch (through dist._trunk, which draws the masks from a generator) cast to double, against the
    reference fed the same masks: z, every gradient and the running statistics to 1e-12 relative."""
    conv = conve_module(pkg, case, feat_drop=0.2, hidden_drop=0.0).double()
    _, s, r, _, _, gz = TT.inputs(case, B, 0.2)
    K = T.sizes(case)[2]
    gen = torch.Generator().manual_seed(31)
    twin = torch.Generator()
    twin.set_state(gen.get_state())
    h, w, _ = T.sizes(case)
    keep = torch.empty((B, case[3], h, w), dtype=torch.float64).bernoulli_(0.8, generator=twin).bool().reshape(B, K)
    seen = {}
    hook = conv.fc.register_forward_hook(lambda m, i, o: seen.__setitem__('z', o))
    sg, rg = s.double().requires_grad_(True), r.double().requires_grad_(True)
    pkg.dist._trunk(conv, sg, rg, gen)
    hook.remove()
    seen['z'].backward(gz.double())
    want = TT.run(case, T.weights(case), s, r, keep, 1.0 / 0.8, gz, torch.float64)
    got = {'z': seen['z'], 'ds': sg.grad, 'dr': rg.grad, 'rm0': conv.bn0.running_mean, 'rv0': conv.bn0.running_var,
           'rm1': conv.bn1.running_mean, 'rv1': conv.bn1.running_var}
    params = dict(conv.named_parameters())
    got.update({k: params[v].grad for k, v in PARAM_OF.items() if v in params})
    for name, v in got.items():
        ref = want[name]
        scale = float(ref.abs().max())
        if name in TT.cancelling_of(case):                      # ~0 in exact arithmetic: relative to the terms that cancel
            scale = float(TT.run(case, T.weights(case), s, r, keep, 1.0 / 0.8, gz, torch.float64, with_mag=True)[1][name].abs().max())
        err = float((v.detach().reshape(ref.shape) - ref).abs().max())
        assert err <= 1e-12 * scale, (name, err, scale)


def test_masks_are_drawn_as_dist_dropout_draws_them(pkg):
    """The HIP path's recipe (bernoulli_ on an f32 tensor of [B, F H W], then on one of [B, O], from the same generator)
    gives the masks dist._trunk's torch path applies: recomputing that path with them reproduces its bits."""
    case, B = T.GRID[1], 9
    conv = conve_module(pkg, case, feat_drop=0.2, hidden_drop=0.3)
    manual = copy.deepcopy(conv)
    s, r = T.queries(case, B)
    gen = torch.Generator().manual_seed(5)
    twin = torch.Generator()
    twin.set_state(gen.get_state())
    y = pkg.dist._trunk(conv, s, r, gen)
    m1 = torch.empty((B, conv.flat_sz), dtype=torch.float32).bernoulli_(0.8, generator=twin)
    m2 = torch.empty((B, case[0] * case[1]), dtype=torch.float32).bernoulli_(0.7, generator=twin)
    o = case[0] * case[1]
    x = torch.cat([s.view(-1, 1, o), r.view(-1, 1, o)], dim=1).transpose(2, 1).reshape(-1, 1, 2 * case[0], case[1])
    x = torch.relu(manual.bn1(manual.conv_e(manual.bn0(x))))
    x = x * m1.view_as(x) * (1.0 / 0.8)
    z = manual.fc(x.view(-1, manual.flat_sz))
    z = z * m2 * (1.0 / (1.0 - 0.3))
    assert torch.equal(torch.relu(manual.bn2(z)), y)


def test_header_and_binding_carry_the_training_trunk(pkg):
    names = ('mgcn_conve_train_workspace', 'mgcn_conve_train_fwd', 'mgcn_conve_train_bwd')
    with open(os.path.join(os.path.dirname(HERE), 'include', 'mgcn_hip.h')) as fh:
        header = fh.read()
    for n in names:
        assert n in pkg._native.EXPORTS and n + '(' in header
    assert '#define MGCN_ABI_VERSION 4' in header


def test_entry_points_refuse_bad_arguments_without_a_gpu(pkg):
    """All argument checks precede the first launch: the library answers MGCN_EINVAL / MGCN_EUNSUPPORTED on a machine with no
    GPU (the pointers are made-up, 16-byte aligned addresses that are never followed)."""
    lib = pkg._native.lib()
    geom = (4, 8, 3, 8, 32)
    k_w, k_h, ks, f, o = geom
    B, K = 5, 8 * 6 * 6
    nbytes = lib.mgcn_conve_train_workspace(B, *geom)
    assert nbytes >= 2 * B * K * 4 and nbytes % 16 == 0
    assert lib.mgcn_conve_train_workspace(B, *geom) == nbytes                      # a function of (B, geometry) alone
    assert lib.mgcn_conve_train_workspace(B + 1, *geom) > nbytes
    for refused in ((B, 32, 32, 3, 2, 1024), (0,) + geom, (-1,) + geom, (1 << 20,) + geom, (B, k_w, k_h, ks, f, o + 1),
                    (B, k_w, k_h, k_h + 1, f, o), (B, k_w, k_h, ks, 0, o), (1, 1, 2, 2, 3, 2)):
        assert lib.mgcn_conve_train_workspace(*refused) == 0, refused
    P = 0x10000

    def fwd(batch=B, geom=geom, s=P, lds=o, r=P, ldr=o, cw=P, fw=P, ldw=K, g0=P, b1=P, rm0=P, rv1=P, z=P, ldz=o, saved=P, ws=P,
            ws_bytes=nbytes):
        return lib.mgcn_conve_train_fwd(batch, *geom, s, lds, r, ldr, cw, None, fw, ldw, None, g0, P, rm0, P, 0.1, 1e-5, P, b1, P, rv1, 0.1,
                                        1e-5, None, 1.0, z, ldz, saved, ws, ws_bytes, None)

    def bwd(batch=B, geom=geom, s=P, r=P, cw=P, fw=P, ldw=K, g1=P, saved=P, gz=P, ldg=o, ldds=o, lddr=o, lddw=K, ws=P, ws_bytes=nbytes):
        return lib.mgcn_conve_train_bwd(batch, *geom, s, o, r, o, cw, fw, ldw, P, P, g1, P, None, 1.0, saved, gz, ldg, P, ldds, P, lddr,
                                        P, P, P, P, P, P, P, lddw, P, ws, ws_bytes, None)

    bad_f = [dict(s=None), dict(r=None), dict(cw=None), dict(fw=None), dict(g0=None), dict(b1=None), dict(rm0=None), dict(rv1=None),
             dict(z=None), dict(saved=None), dict(ws=None), dict(ws=P + 4), dict(ws_bytes=nbytes - 1), dict(lds=o - 1), dict(ldr=o - 1),
             dict(ldz=o - 1), dict(ldw=K - 1), dict(batch=-1), dict(geom=(k_w, k_h, ks, f, o + 1)), dict(geom=(k_w, k_h, k_h + 1, f, o)),
             dict(geom=(k_w, k_h, 0, f, o)), dict(geom=(k_w, k_h, ks, 0, o))]
    for kw in bad_f:
        assert fwd(**kw) == EINVAL, kw
        assert lib.mgcn_last_error()
    bad_b = [dict(s=None), dict(r=None), dict(cw=None), dict(fw=None), dict(g1=None), dict(saved=None), dict(gz=None), dict(ws=None),
             dict(ws=P + 8), dict(ws_bytes=nbytes - 1), dict(ldg=o - 1), dict(ldds=o - 1), dict(lddr=o - 1), dict(ldw=K - 1),
             dict(lddw=K - 1), dict(batch=-1), dict(geom=(k_w, k_h, ks, f, o + 1))]
    for kw in bad_b:
        assert bwd(**kw) == EINVAL, kw
    for call in (fwd, bwd):
        assert call(geom=(32, 32, 3, 2, 1024)) == EUNSUPPORTED
        assert call(batch=0) == EUNSUPPORTED and call(batch=1 << 20) == EUNSUPPORTED
        assert call(batch=1, geom=(1, 2, 2, 3, 2)) == EUNSUPPORTED                  # one value per bn1 channel


def test_switch_with_cpu_tensors_takes_the_torch_path(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    case = T.GRID[1]
    on, off = conve_module(pkg, case, conve_trunk_train='hip'), conve_module(pkg, case)
    s, r = T.queries(case, 6)
    outs = []
    for m in (on, off):
        torch.manual_seed(2)
        outs.append(m.trunk(s, r))
    assert torch.equal(outs[0], outs[1]) and not hasattr(on, '_trunk_train_count')
    monkeypatch.setenv('MGCN_TRUNK_TRAIN', 'hip')
    outs = []
    for m in (on, off):                                     # the environment variable cannot put CPU tensors on the GPU path either
        torch.manual_seed(3)
        outs.append(m.trunk(s, r, generator=None))
    assert torch.equal(outs[0], outs[1]) and not hasattr(off, '_trunk_train_count')
    # a one-value channel still raises torch's own error
    one = (1, 2, 2, 3, False)
    m = conve_module(pkg, one, conve_trunk_train='hip')
    with pytest.raises(ValueError):
        m.trunk(*T.queries(one, 1))


CAPPED_CASES = [c for c in TT.grid_cases() if c[2] < 1.0]


@pytest.mark.parametrize('case,B,p,seed', [c + (0,) for c in CAPPED_CASES] + TT.limit_cases(),
                         ids=TT.case_ids(CAPPED_CASES + TT.limit_cases()))
def test_bars_stay_under_their_vacuity_caps(case, B, p, seed):
    """No bar of the GPU parity grid may exceed 1e-4 of the tensor (of its terms, for the three that cancel): a kernel wrong
    in the fourth digit must fail. Printed as bar / cap."""
    ref = TT.reference(case, B, p, seed)
    caps = TT.vacuity(ref)
    print('%s B=%d p=%g: %s' % (T.case_id(case), B, p, ' '.join('%s=%.3g' % kv for kv in sorted(caps.items()))))
    for name, ratio in caps.items():
        assert ratio <= 1.0, (name, ratio)
    for name in TT.STATS:
        assert ref.bar[name] <= 1e-5 * max(1.0, float(ref.ref[name].abs().max())), name


# ------------------------------------------------------------------------------------------------ the limits of the domain
LIMIT_IDS = TT.case_ids(TT.limit_cases())


@pytest.mark.parametrize('case,B,p,seed', TT.limit_cases(), ids=LIMIT_IDS)
def test_limit_cases_keep_their_relu_masks(case, B, p, seed):
    """The smallest float64 |a| before the relu is at least 4 x the largest |a32 - a64| of the same inputs in torch-CPU f32
    (4: what derived_bar gives a kernel over the CPU's f32 error), and f32 flips no mask: otherwise one activation at 1e-8
    decides the case. The recorded seed is the first from 0 that meets this and the caps."""
    ref = TT.reference(case, B, p, seed)
    print('%s B=%d p=%g seed=%d: min |a64| = %.3g, max |a32 - a64| = %.3g, margin %.3g, %d masks flipped'
          % (T.case_id(case), B, p, seed, ref.a_min, ref.a_err, TT.margin(ref), ref.a_flips))
    assert ref.a_flips == 0
    assert TT.margin(ref) >= 4.0
    for earlier in range(seed):
        other = TT.Reference(case, *TT.inputs(case, B, p, earlier))
        assert TT.margin(other) < 4.0 or max(TT.vacuity(other).values()) > 1.0, earlier


def test_module_case_at_kernel_size_9_keeps_its_relu_masks():
    """test_module_against_float64's ks = 9 case draws its masks on the device, but the activations before the relu depend on
    trunk_ref's weights and queries alone: the same margin, at the batch it uses."""
    case, B = TT.MODULE_KS9
    assert case == (10, 20, 9, 32, False) and case in T.LIMIT_GRID
    ref = TT.reference(case, B, 0.2)
    assert ref.a_flips == 0 and TT.margin(ref) >= 4.0


def test_limit_cases_reach_what_they_are_there_for(pkg):
    """The launch arithmetic of csrc/conve_train.hip restated per case: a later change of a constant or of the list cannot
    silently empty one."""
    cases = TT.limit_cases()
    assert len(set(cases)) == len(cases)
    geoms = [c[0] for c in cases]
    assert all(g in geoms for g in T.LIMIT_GRID)
    fig = {g: T.launch_figures(g) for g in geoms}
    ps = [c[2] for c in cases]
    assert all(a != b for a, b in zip(ps, ps[1:])) and set(ps) == {0.0, 0.2}            # the masks alternate
    # tt_tap_kernel: 64 threads while T + 1 <= 64, else 256 with t = threadIdx.x + s * 256 in slot s < TT_SLOTS_T = 5
    assert fig[(4, 8, 8, 8, True)]['T'] + 1 == 65
    assert fig[(10, 20, 9, 32, False)]['T'] + 1 == 82 and fig[(10, 20, 9, 32, False)]['P'] == 144
    assert 256 < fig[(16, 32, 17, 4, True)]['T'] + 1 <= 512 and fig[(16, 32, 17, 4, True)]['P'] == 256      # slots 0 and 1
    assert fig[(16, 32, 32, 3, False)]['T'] == 1024 == 4 * 256                                             # t == T: slot 4, thread 0
    assert TT.MOST_TAPS[0] == (16, 32, 32, 3, False) and TT.MANY_TAPS[0] == (16, 32, 17, 4, True)
    assert sum(fig[g]['T'] + 1 > 64 for g in set(geoms)) == 4
    assert fig[(16, 32, 32, 3, False)]['NCG'] == 3 and fig[(16, 32, 32, 3, False)]['K'] == 3
    # the generic convolution (ks not 3, 5, 7) with a real kernel
    assert {g[2] for g in geoms} >= {4, 6, 8, 9, 17, 32}
    # one output position: bn1 over the batch alone, which needs rows
    for case, B, _, _ in cases:
        if fig[case]['P'] == 1:
            assert case[2] == case[1] == 2 * case[0] and fig[case]['K'] == case[3] and B >= 16
    assert [g for g in T.LIMIT_GRID if fig[g]['P'] == 1] == [(4, 8, 8, 8, True), (16, 32, 32, 3, False)]
    assert fig[(2, 4, 3, 5, False)]['P'] == 4 and fig[(3, 5, 4, 3, True)]['P'] == 6
    # F > 256: a second block of tt_bn1_finish_kernel / tt_prep_kernel; F = 1
    assert (4, 8, 4, 300, True) in geoms and 300 > 256 and fig[(4, 8, 4, 300, True)]['K'] == 7500
    assert (4, 8, 3, 1, False) in geoms
    assert fig[(5, 8, 6, 7, True)]['K'] == 105
    # tt_gh_kernel's 64-row blocks at a small geometry; the batch limit
    assert [(B) for case, B, _, _ in cases if case == TT.SMALL] == [64, 65, 257]
    full = [B for case, B, _, _ in cases if case == TT.LIMIT_B4096]
    assert full == [4096, 4095] and TT.FULL_BATCH[:2] == (TT.LIMIT_B4096, 4096) and fig[TT.LIMIT_B4096]['P'] > 1
    assert -(-4096 // 16) == 256 and -(-4095 // 16) == 256                   # gb[256], gg[256]: one entry per thread
    lib = pkg._native.lib()
    for case, B, _, _ in cases:
        assert lib.mgcn_conve_train_workspace(B, *T.geometry(case)) > 0, (case, B)
    for case in set(geoms):
        geom = T.geometry(case)
        assert lib.mgcn_conve_train_workspace(4096, *geom) > 0 and lib.mgcn_conve_train_workspace(4097, *geom) == 0
        assert pkg._native.conve_train_supported(4096, geom) and not pkg._native.conve_train_supported(4097, geom)
        assert (lib.mgcn_conve_train_workspace(1, *geom) > 0) == (fig[case]['P'] > 1)      # B P >= 2


def _breaks(ref, name, value):
    return float((value.double().reshape(ref.ref[name].shape) - ref.ref[name]).abs().max()) > ref.bar[name]


def _broken(ref, outs):
    return sorted(k for k, v in outs.items() if k in ref.bar and _breaks(ref, k, v))


@pytest.mark.parametrize('spec', [TT.MANY_TAPS, TT.FULL_BATCH], ids=TT.case_ids([TT.MANY_TAPS, TT.FULL_BATCH]))
def test_the_bars_bite_at_the_limits(spec):
    """Value-only faults a kernel could have at these shapes, applied to the float64 computation on the CPU: each must break
    the bar of at least one output (and, where the fault sits in one output, of that output)."""
    case, B, p, seed = spec
    k_w, k_h, ks, f, bias = case
    ref = TT.reference(case, B, p, seed)
    sd, s, r, keep, inv_keep, gz = TT.inputs(case, B, p, seed)
    full = TT.run(case, sd, s, r, keep, inv_keep, gz, extra=('gc',))
    # 1. the last tap of one filter dropped: from the convolution, and from d conv weight alone
    cut = dict(sd)
    cut['conv2.conv_e.weight'] = sd['conv2.conv_e.weight'].clone()
    cut['conv2.conv_e.weight'][f - 1, 0, ks - 1, ks - 1] = 0.0
    broken = _broken(ref, TT.run(case, cut, s, r, keep, inv_keep, gz))
    print('%s: last tap of the last filter dropped from the convolution breaks %s' % (T.case_id(case), broken))
    assert 'z' in broken
    dw = full['d_conv_w'].clone()
    dw[f - 1, 0, ks - 1, ks - 1] = 0.0
    assert _breaks(ref, 'd_conv_w', dw)
    # 2. the image shifted by one column
    img = torch.stack([s, r], dim=2).reshape(B, 2 * k_w, k_h).roll(1, dims=2).reshape(B, k_w * k_h, 2)
    broken = _broken(ref, TT.run(case, sd, img[:, :, 0].contiguous(), img[:, :, 1].contiguous(), keep, inv_keep, gz))
    print('%s: image shifted by one column breaks %s' % (T.case_id(case), broken))
    assert 'z' in broken and 'd_conv_w' in broken
    # 3. the conv bias left out. Under a training-mode bn1 the whole of d conv bias is 0 in exact arithmetic (a kernel that
    # left ALL of it out would be right), so what must show is a part left out: the conv-bias sums of the last block of 16
    # rows missing from d conv bias; and, with a conv bias, the bias missing from the convolution (bn1 removes it from
    # everything but its own mean)
    gc = full['gc']
    assert _breaks(ref, 'd_conv_b', gc[:B - 16].sum((0, 2, 3)))
    if bias:
        nob = {k: v for k, v in sd.items() if k != 'conv2.conv_e.bias'}
        broken = _broken(ref, TT.run((k_w, k_h, ks, f, False), nob, s, r, keep, inv_keep, gz))
        print('%s: conv bias left out of the convolution breaks %s' % (T.case_id(case), broken))
        assert 'mu1' in broken and 'rm1' in broken
    # 4. the last block of 16 rows dropped from a batch sum: d fc.bias, d fc.weight, d conv weight, the bn0 mean
    h = B - 16
    assert _breaks(ref, 'd_fc_b', gz[:h].double().sum(0))
    part = TT.run(case, sd, s, r, keep, inv_keep, torch.cat([gz[:h], torch.zeros_like(gz[h:])]))
    assert float((part['z'] - full['z']).abs().max()) == 0.0            # (the forward is the same: only the sums lose rows)
    assert _breaks(ref, 'd_fc_w', part['d_fc_w'])
    x = torch.stack([s, r], dim=2).double()
    assert _breaks(ref, 'mu0', x[:h].sum().reshape(1) / x.numel())
    pat = TT._patches(_x0(ref, x, sd).reshape(B, 2 * k_w, k_h), ks)
    assert _breaks(ref, 'd_conv_w', torch.einsum('bfhw,bhwt->ft', gc[:h], pat[:h]))


def _x0(ref, x, sd):
    """bn0's output in float64 from the reference's own statistics."""
    return (x - ref.ref['mu0']) * ref.ref['rstd0'] * sd['conv2.bn0.weight'].double() + sd['conv2.bn0.bias'].double()
