"""tests/trunk_train_ref.py checked on the CPU (`-m "not gpu"`): the float64 reference against the torch modules of ConvE
in float64 with the same masks, the masks' draw order against dist._dropout, the bars against their vacuity caps, and
what the training-mode trunk's entry points (paragraph (9) of include/mgcn_hip.h) do without a GPU."""
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


@pytest.mark.parametrize('case,B', [(T.GRID[2], 17), (T.GRID[6], 5), (T.GRID[1], 2), (T.PRODUCTION, 16)],
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


@pytest.mark.parametrize('case,B,p', [c for c in TT.grid_cases() if c[2] < 1.0],
                         ids=lambda v: T.case_id(v) if isinstance(v, tuple) else str(v))
def test_bars_stay_under_their_vacuity_caps(case, B, p):
    """No bar of the GPU parity grid may exceed 1e-4 of the tensor (of its terms, for the three that cancel): a kernel wrong
    in the fourth digit must fail. Printed as bar / cap."""
    ref = TT.reference(case, B, p)
    caps = TT.vacuity(ref)
    print('%s B=%d p=%g: %s' % (T.case_id(case), B, p, ' '.join('%s=%.3g' % kv for kv in sorted(caps.items()))))
    for name, ratio in caps.items():
        assert ratio <= 1.0, (name, ratio)
    for name in TT.STATS:
        assert ref.bar[name] <= 1e-5 * max(1.0, float(ref.ref[name].abs().max())), name
