"""The training-mode HIP ConvE trunk (csrc/conve_train.hip, paragraph (9) of include/mgcn_hip.h) on a real MI355X: held to
the float64 reference and the bars of tests/trunk_train_ref.py through the C ABI and through ConvE.trunk, to its promises
(same inputs, same bits; a NULL gradient pointer leaves the others' bits alone; refusals write nothing), to the goldens'
training step with the switch on, and to the one-rank promise of dist.train_step_sharded. Every parity case prints
`RATIO family id worst-error / bar` (pytest -s) before it asserts."""
import copy
import os
import types

import numpy as np
import pytest
import torch

from . import dense_ref as R
from . import trunk_ref as T
from . import trunk_train_ref as TT
from .conftest import FULL_CASES, GOLDEN, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL, EUNSUPPORTED = 1, 3
SMALL = (4, 8, 3, 8, False)
GRADS = ('ds', 'dr', 'd_conv_w', 'd_conv_b', 'd_g0', 'd_b0', 'd_g1', 'd_b1', 'd_fc_w', 'd_fc_b')


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _report(family, cid, ratio):
    print('RATIO %s %s %.4f' % (family, cid, ratio))
    assert ratio <= 1.0, '%s %s: worst |got - float64| is %.3f x its bar' % (family, cid, ratio)


def _wide(t, extra):
    """t as a column window of a tensor with `extra` spare NaN columns (row stride > its width)."""
    w = torch.full((t.size(0), t.size(1) + extra), float('nan'), device=DEV)
    w[:, :t.size(1)] = t.to(DEV)
    return w[:, :t.size(1)]


class Call(object):
    """One forward + backward through the C ABI: inputs as windows (ld > O), every output a window of a guarded buffer."""

    def __init__(self, nat, case, B, p, skip=(), seed=0):
        self.lib, self.case, self.B = nat.lib(), case, B
        self.geom = T.geometry(case)
        k_w, k_h, ks, F, O = self.geom
        K = T.sizes(case)[2]
        sd, s, r, keep, inv_keep, gz = TT.inputs(case, B, p, seed)
        d = lambda k: sd['conv2.' + k].to(DEV).contiguous() if 'conv2.' + k in sd else None
        self.s, self.r, self.gz = _wide(s, 3), _wide(r, 1), _wide(gz, 2)
        self.keep, self.inv_keep = (None if keep is None else keep.to(DEV).contiguous()), inv_keep
        self.w = {k: d(k) for k in ('conv_e.weight', 'conv_e.bias', 'fc.weight', 'fc.bias', 'bn0.weight', 'bn0.bias', 'bn1.weight',
                                    'bn1.bias')}
        self.run_stats = {k: d(k) for k in ('bn0.running_mean', 'bn0.running_var', 'bn1.running_mean', 'bn1.running_var')}
        self.nbytes = self.lib.mgcn_conve_train_workspace(B, *self.geom)
        assert self.nbytes > 0
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV)
        G = lambda rows, cols, extra: R.Guarded(rows, cols, cols + extra, DEV)
        self.out = {'z': G(B, O, 5), 'saved': G(1, 2 + 2 * F, 3), 'ds': G(B, O, 1), 'dr': G(B, O, 2), 'd_conv_w': G(1, F * ks * ks, 1),
                    'd_conv_b': G(1, F, 1), 'd_g0': G(1, 1, 1), 'd_b0': G(1, 1, 1), 'd_g1': G(1, F, 1), 'd_b1': G(1, F, 1),
                    'd_fc_w': G(O, K, 3), 'd_fc_b': G(1, O, 1)}
        self.skip = set(skip)
        self.K, self.O, self.F = K, O, F

    def _p(self, t):
        return None if t is None else t.data_ptr()

    def fwd(self, **over):
        a = dict(batch=self.B, geom=self.geom, s=self.s.data_ptr(), lds=self.s.stride(0), r=self.r.data_ptr(), cw=self._p(self.w['conv_e.weight']),
                 fw=self._p(self.w['fc.weight']), ldw=self.K, g0=self._p(self.w['bn0.weight']), rm0=self._p(self.run_stats['bn0.running_mean']),
                 z=self.out['z'].ptr(), ldz=self.out['z'].ld, saved=self.out['saved'].ptr(), ws=self.ws.data_ptr(), ws_bytes=self.nbytes)
        a.update(over)
        w, rs = self.w, self.run_stats
        return self.lib.mgcn_conve_train_fwd(
            a['batch'], *a['geom'], a['s'], a['lds'], a['r'], self.r.stride(0), a['cw'], self._p(w['conv_e.bias']), a['fw'], a['ldw'],
            self._p(w['fc.bias']), a['g0'], self._p(w['bn0.bias']), a['rm0'], self._p(rs['bn0.running_var']), TT.BN_MOMENTUM, TT.BN_EPS,
            self._p(w['bn1.weight']), self._p(w['bn1.bias']), self._p(rs['bn1.running_mean']), self._p(rs['bn1.running_var']), TT.BN_MOMENTUM,
            TT.BN_EPS, self._p(self.keep), self.inv_keep, a['z'], a['ldz'], a['saved'], a['ws'], a['ws_bytes'], _stream())

    def bwd(self, **over):
        a = dict(batch=self.B, geom=self.geom, gz=self.gz.data_ptr(), ldg=self.gz.stride(0), ws=self.ws.data_ptr(), ws_bytes=self.nbytes,
                 saved=self.out['saved'].ptr(), ldds=self.out['ds'].ld)
        a.update(over)
        w = self.w
        o = lambda k: None if k in self.skip else self.out[k].ptr()
        return self.lib.mgcn_conve_train_bwd(
            a['batch'], *a['geom'], self.s.data_ptr(), self.s.stride(0), self.r.data_ptr(), self.r.stride(0), self._p(w['conv_e.weight']),
            self._p(w['fc.weight']), self.K, self._p(w['bn0.weight']), self._p(w['bn0.bias']), self._p(w['bn1.weight']), self._p(w['bn1.bias']),
            self._p(self.keep), self.inv_keep, a['saved'], a['gz'], a['ldg'], o('ds'), a['ldds'], o('dr'), self.out['dr'].ld, o('d_conv_w'),
            o('d_conv_b'), o('d_g0'), o('d_b0'), o('d_g1'), o('d_b1'), o('d_fc_w'), self.out['d_fc_w'].ld, o('d_fc_b'), a['ws'], a['ws_bytes'],
            _stream())

    def check_guards(self, what):
        for k, gd in self.out.items():
            if k in self.skip:
                assert gd.untouched(), '%s: %s was written through a NULL pointer' % (what, k)
            else:
                gd.check('%s %s' % (what, k))

    def results(self):
        """name -> tensor, with the names of trunk_train_ref."""
        F = self.F
        sv = self.out['saved'].view.reshape(-1)
        got = {'z': self.out['z'].view, 'mu0': sv[0:1], 'rstd0': sv[1:2], 'mu1': sv[2:2 + F], 'rstd1': sv[2 + F:2 + 2 * F],
               'rm0': self.run_stats['bn0.running_mean'], 'rv0': self.run_stats['bn0.running_var'],
               'rm1': self.run_stats['bn1.running_mean'], 'rv1': self.run_stats['bn1.running_var']}
        for k in GRADS:
            if k not in self.skip:
                got[k] = self.out[k].view
        return got


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('case,B,p,seed', [c + (0,) for c in TT.grid_cases()] + TT.limit_cases(),
                         ids=TT.case_ids(TT.grid_cases() + TT.limit_cases()))
def test_grid_parity_through_the_c_abi(pkg, case, B, p, seed):
    """The grid, and the limits of the domain (trunk_train_ref.limit_cases: up to 1024 taps, P = 1, F = 1 and F > 256,
    B = 4096), to the same bars."""
    cid = '%s-B%d-p%g%s' % (T.case_id(case), B, p, '-s%d' % seed if seed else '')
    ref = TT.reference(case, B, p, seed)
    c = Call(pkg._native, case, B, p, seed=seed)
    assert c.fwd() == 0, c.lib.mgcn_last_error()
    assert c.bwd() == 0, c.lib.mgcn_last_error()
    torch.cuda.synchronize()
    c.check_guards(cid)
    worst = {}
    for name, got in c.results().items():
        worst[name] = ref.ratio(name, got)
    print('RATIOS %s %s' % (cid, ' '.join('%s=%.3f' % kv for kv in sorted(worst.items()))))
    for name, ratio in worst.items():
        _report('trunk_train_' + name, cid, ratio)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('case,B,p,seed', [(SMALL, 17, 0.2, 0), (T.PRODUCTION, 130, 0.2, 0), TT.MOST_TAPS, TT.FULL_BATCH],
                         ids=['small', 'production', 'taps-1024', 'batch-4096'])
def test_same_inputs_same_bits_and_null_gradients(pkg, case, B, p, seed):
    runs = []
    for skip in ((), (), ('d_fc_w', 'ds', 'd_conv_b'), ('d_conv_w', 'd_conv_b', 'd_fc_b', 'dr', 'd_g0', 'd_b0')):
        c = Call(pkg._native, case, B, p, skip=skip, seed=seed)
        assert c.fwd() == 0 and c.bwd() == 0, c.lib.mgcn_last_error()
        torch.cuda.synchronize()
        c.check_guards('repeat')
        runs.append(c.results())
    for name, v in runs[0].items():
        assert torch.equal(v, runs[1][name]), name
        for other in runs[2:]:
            if name in other:
                assert torch.equal(v, other[name]), '%s changed when another gradient pointer was NULL' % name


# ---------------------------------------------------------------------------------------------------------------- 3
def test_refusals_write_nothing(pkg):
    case, B = SMALL, 5
    c = Call(pkg._native, case, B, 0.2)
    lib = c.lib
    k_w, k_h, ks, f, o = c.geom
    stats_before = {k: v.clone() for k, v in c.run_stats.items()}
    bad_f = [('null s', dict(s=None)), ('null conv weight', dict(cw=None)), ('null fc weight', dict(fw=None)), ('null z', dict(z=None)),
             ('null saved', dict(saved=None)), ('null bn weight', dict(g0=None)), ('null running mean', dict(rm0=None)),
             ('null workspace', dict(ws=None)), ('misaligned workspace', dict(ws=c.ws.data_ptr() + 4, ws_bytes=c.nbytes - 4)),
             ('workspace one byte short', dict(ws_bytes=c.nbytes - 1)), ('lds < O', dict(lds=o - 1)), ('ldz < O', dict(ldz=o - 1)),
             ('ldw < K', dict(ldw=c.K - 1)), ('negative batch', dict(batch=-1)), ('k_w k_h != O', dict(geom=(k_w, k_h, ks, f, o + 1))),
             ('kernel too large', dict(geom=(k_w, k_h, k_h + 1, f, o))), ('no filters', dict(geom=(k_w, k_h, ks, 0, o)))]
    for what, kw in bad_f:
        assert c.fwd(**kw) == EINVAL, what
        assert lib.mgcn_last_error()
    assert c.fwd(geom=(32, 32, 3, 2, 1024)) == EUNSUPPORTED
    assert c.fwd(batch=0) == EUNSUPPORTED and c.fwd(batch=1 << 20) == EUNSUPPORTED
    assert lib.mgcn_conve_train_workspace(B, 32, 32, 3, 2, 1024) == 0 and lib.mgcn_conve_train_workspace(1, 1, 2, 2, 3, 2) == 0
    bad_b = [('null gz', dict(gz=None)), ('null saved', dict(saved=None)), ('ldg < O', dict(ldg=o - 1)), ('ldds < O', dict(ldds=o - 1)),
             ('workspace one byte short', dict(ws_bytes=c.nbytes - 1)), ('null workspace', dict(ws=None)),
             ('k_w k_h != O', dict(geom=(k_w, k_h, ks, f, o + 1)))]
    for what, kw in bad_b:
        assert c.bwd(**kw) == EINVAL, what
    assert c.bwd(geom=(32, 32, 3, 2, 1024)) == EUNSUPPORTED
    # the batch limit: 4096 is taken, 4097 refused by all three entry points and by the wrapper's question
    assert lib.mgcn_conve_train_workspace(4096, *c.geom) > 0 and lib.mgcn_conve_train_workspace(4097, *c.geom) == 0
    assert c.fwd(batch=4097) == EUNSUPPORTED and lib.mgcn_last_error()
    assert c.bwd(batch=4097) == EUNSUPPORTED
    assert pkg._native.conve_train_supported(4096, c.geom) and not pkg._native.conve_train_supported(4097, c.geom)
    torch.cuda.synchronize()
    assert all(gd.untouched() for gd in c.out.values())
    assert all(torch.equal(v, c.run_stats[k]) for k, v in stats_before.items())
    assert c.fwd() == 0 and c.bwd() == 0                                   # and the good call works
    torch.cuda.synchronize()
    c.check_guards('good call')
    ref = TT.reference(case, B, 0.2)
    for name, got in c.results().items():
        assert ref.ratio(name, got) <= 1.0, name


# ---------------------------------------------------------------------------------------------------------------- 4
def conve_module(pkg, case, sd=None, **over):
    params = types.SimpleNamespace(**dict(T.hyper(case), **over))
    conv = pkg.model.ConvE(params, 10)
    sd = T.weights(case) if sd is None else sd
    res = conv.load_state_dict({k[len('conv2.'):]: v for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys
    return conv.to(DEV).train()


PARAM_OF = {'d_conv_w': 'conv_e.weight', 'd_conv_b': 'conv_e.bias', 'd_g0': 'bn0.weight', 'd_b0': 'bn0.bias', 'd_g1': 'bn1.weight',
            'd_b1': 'bn1.bias', 'd_fc_w': 'fc.weight', 'd_fc_b': 'fc.bias'}


@pytest.mark.parametrize('case,B', [((3, 8, 3, 6, True), 17), (T.PRODUCTION, 128), TT.MODULE_KS9], ids=['small', 'production', 'ks9'])
def test_module_against_float64(pkg, monkeypatch, case, B):
    """ConvE.trunk(s, r, generator=g) + backward with the switch on against the float64 reference fed the masks drawn from a
    clone of g's state; the reference carries the torch tail (hidden_drop -> bn2 -> relu) in its own dtype, and the bars
    are widened by that tail's Lipschitz factor max |gamma2| rstd2 (at least 1) alone."""
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    sd = T.weights(case)
    conv = conve_module(pkg, case, sd=sd, conve_trunk_train='hip', feat_drop=0.2, hidden_drop=0.3)
    s, r = T.queries(case, B)
    O, K = case[0] * case[1], T.sizes(case)[2]
    gy = R.pm_uniform((B, O), R.gen(R.seed_of(13, B, *T.geometry(case))))
    gen = torch.Generator(device=DEV).manual_seed(77)
    twin = torch.Generator(device=DEV)
    twin.set_state(gen.get_state())
    keep = torch.empty((B, K), device=DEV).bernoulli_(0.8, generator=twin).bool().cpu()
    hid = torch.empty((B, O), device=DEV).bernoulli_(0.7, generator=twin).cpu()
    lip = [1.0]

    def tail(z, dtype):
        zd = z * hid.to(dtype) * (1.0 / 0.7)
        mu, var = zd.mean(0), zd.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + TT.BN_EPS)
        if dtype == torch.float64:
            lip[0] = max(1.0, float((sd['conv2.bn2.weight'].double().abs() * rstd).max()) / 0.7)
        y = torch.relu((zd - mu) * rstd * sd['conv2.bn2.weight'].to(dtype) + sd['conv2.bn2.bias'].to(dtype))
        return y, (y * gy.to(dtype)).sum()

    ref = TT.Reference(case, sd, s, r, keep, 1.0 / 0.8, None, tail=tail)
    sg, rg = s.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    y = conv.trunk(sg, rg, generator=gen)
    assert conv._trunk_train_count == 1
    (y * gy.to(DEV)).sum().backward()
    got = {'y': y, 'ds': sg.grad, 'dr': rg.grad, 'rm0': conv.bn0.running_mean, 'rv0': conv.bn0.running_var,
           'rm1': conv.bn1.running_mean, 'rv1': conv.bn1.running_var}
    params = dict(conv.named_parameters())
    got.update({k: params[v].grad for k, v in PARAM_OF.items() if v in params})
    assert int(conv.bn0.num_batches_tracked) == 1 and int(conv.bn1.num_batches_tracked) == 1
    cid = '%s-B%d' % (T.case_id(case), B)
    print('bn2 Lipschitz factor %.3f' % lip[0])
    for name, v in got.items():                    # the running statistics of bn0 / bn1 do not pass through the tail: their own bars
        _report('trunk_train_module_' + name, cid, ref.ratio(name, v) / (1.0 if name in TT.STATS else lip[0]))


def test_dispatch(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    monkeypatch.delenv('MGCN_TRUNK', raising=False)
    case = SMALL
    s, r = (t.to(DEV) for t in T.queries(case, 40))
    taken = lambda m: getattr(m, '_trunk_train_count', 0)

    def same_as_torch(on, off, seed, **kw):
        before = taken(on)
        outs = []
        for m in (on, off):
            torch.manual_seed(seed)
            outs.append(m.trunk(s, r, **kw))
        assert torch.equal(outs[0], outs[1]) and taken(on) == before
        assert torch.equal(on.bn1.running_var, off.bn1.running_var)

    on, off = conve_module(pkg, case, conve_trunk_train='hip'), conve_module(pkg, case)
    y = on.trunk(s, r)
    assert taken(on) == 1 and taken(off) == 0
    # the switch off: today's code on today's modules (F.dropout's own stream)
    torch.manual_seed(3)
    y_off = off.trunk(s, r)
    twin = conve_module(pkg, case)
    torch.manual_seed(3)
    x = torch.cat([s.view(-1, 1, 32), r.view(-1, 1, 32)], dim=1).transpose(2, 1).reshape(-1, 1, 8, 8)
    x = twin.feature_drop(torch.relu(twin.bn1(twin.conv_e(twin.bn0(x)))))
    parent = torch.relu(twin.bn2(twin.hidden_drop(twin.fc(x.view(-1, twin.flat_sz))))).contiguous()
    assert torch.equal(y_off, parent)
    # eval mode, the environment variable, momentum=None, conve_trunk='hip' alone: the torch path's bits
    a, b = conve_module(pkg, case, conve_trunk_train='hip').eval(), conve_module(pkg, case).eval()
    same_as_torch(a, b, 4)
    a, b = conve_module(pkg, case, conve_trunk_train='hip'), conve_module(pkg, case)
    monkeypatch.setenv('MGCN_TRUNK_TRAIN', 'torch')
    same_as_torch(a, b, 5)
    monkeypatch.setenv('MGCN_TRUNK_TRAIN', 'hip')
    assert taken(b) == 0
    b.trunk(s, r)
    assert taken(b) == 1                                                    # ... and it overrides in the other direction
    monkeypatch.delenv('MGCN_TRUNK_TRAIN')
    a, b = conve_module(pkg, case, conve_trunk_train='hip'), conve_module(pkg, case)
    a.bn1.momentum = b.bn1.momentum = None
    same_as_torch(a, b, 6)
    a, b = conve_module(pkg, case, conve_trunk='hip'), conve_module(pkg, case)
    same_as_torch(a, b, 7)
    wide = (32, 32, 3, 2, False)
    sd = T.weights(wide)
    a, b = conve_module(pkg, wide, sd=sd, conve_trunk_train='hip'), conve_module(pkg, wide, sd=sd)
    sw, rw = (t.to(DEV) for t in T.queries(wide, 9))
    outs = []
    for m in (a, b):
        torch.manual_seed(8)
        outs.append(m.trunk(sw, rw))
    assert torch.equal(outs[0], outs[1]) and taken(a) == 0
    # one row past the batch limit: the torch path's bits, and no HIP launch counted
    a, b = conve_module(pkg, case, conve_trunk_train='hip'), conve_module(pkg, case)
    s_full, r_full = (t.to(DEV) for t in T.queries(case, 4097))
    assert pkg._native.conve_train_supported(4096, T.geometry(case)) and not pkg._native.conve_train_supported(4097, T.geometry(case))
    outs = []
    for m in (a, b):
        torch.manual_seed(9)
        outs.append(m.trunk(s_full, r_full))
    assert torch.equal(outs[0], outs[1]) and taken(a) == 0
    assert torch.equal(a.bn1.running_var, b.bn1.running_var) and torch.equal(a.bn0.running_mean, b.bn0.running_mean)
    a.trunk(s_full[:4096], r_full[:4096])
    assert taken(a) == 1                                                    # ... and 4096 rows take the kernels
    # dist._trunk with a generator: its torch path and the HIP path see the same masks, so they agree to rounding
    gen = lambda: torch.Generator(device=DEV).manual_seed(21)
    a, b = conve_module(pkg, case, conve_trunk_train='hip'), conve_module(pkg, case)
    ya, yb = pkg.dist._trunk(a, s, r, gen()), pkg.dist._trunk(b, s, r, gen())
    assert taken(a) == 1 and taken(b) == 0
    assert float((ya - yb).abs().max()) <= 1e-4 * float(yb.abs().max())
    assert ((ya == 0) != (yb == 0)).float().mean() < 0.01                    # the same elements dropped / rectified


# ---------------------------------------------------------------------------------------------------------------- 5
def _loader(pkg, g, **over):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**dict(g.hp, **over))
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    return dl, params


def _model(pkg, g, **over):
    dl, params = _loader(pkg, g, **over)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    missing = model.load_state_dict(g.state_dict(), strict=False)
    assert not missing.unexpected_keys
    return model.to(DEV), dl, params


# conv2.* gradients that cancel analytically under a training-mode bn1: both paths hold rounding noise there
CANCELLING_KEYS = ('conv2.conv_e.bias', 'conv2.bn0.weight', 'conv2.bn0.bias')


def _golden_grads(g, model, torch_model, what):
    inv = model._slot_csr.inv_perm
    for k, ref in g.grads().items():
        grad_of = lambda m: (lambda p: p.grad if p.grad is not None else torch.zeros_like(p))(dict(m.named_parameters())[k])
        got = grad_of(model)
        if k == 'edge_embeddings':
            got = got.index_select(0, inv)
        scale = float(ref.abs().max()) + 1e-12
        floor = 2e-6 if k.startswith('conv2.') else 1e-9
        atol = 2e-5 * scale + floor
        if k in CANCELLING_KEYS:
            torch_dev = float((grad_of(torch_model).cpu() - ref).abs().max())
            hip_dev = float((got.cpu() - ref).abs().max())
            print('%s %s: existing bar %.3g, torch path off the golden by %.3g, HIP path by %.3g' % (what, k, atol, torch_dev, hip_dev))
            if hip_dev > atol:            # only a key seen above its floor takes the larger of that bar and 4 x the torch path's deviation
                atol = max(atol, 4.0 * torch_dev)
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=2e-3, atol=atol, err_msg=k)


@pytest.mark.parametrize('case', FULL_CASES)
def test_train_step_gradients_vs_golden_with_the_hip_trunk(pkg, monkeypatch, case):
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    g = golden(case)
    models = []
    for switch in ('hip', 'torch'):
        model, dl, params = _model(pkg, g, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, conve_trunk_train=switch)
        model.conv1.drop.p = 0.0
        model.train()
        trip, lab = g.t('train_triple').to(DEV), g.t('train_label').to(DEV)
        pred = model(trip[:, 0], trip[:, 1], dl.graph)
        loss = model.loss(pred, lab)
        loss.backward()
        models.append((model, pred, loss))
    (model, pred, loss), (torch_model, _, _) = models
    assert model.conv2._trunk_train_count == 1 and not hasattr(torch_model.conv2, '_trunk_train_count')
    print('%s: largest |score - golden| = %.3g' % (case, float(np.abs(pred.detach().cpu().numpy() - g['train_score']).max())))
    np.testing.assert_allclose(pred.detach().cpu().numpy(), g['train_score'], rtol=0, atol=2e-5)
    assert abs(float(loss) - float(g['train_loss'])) < 1e-5
    _golden_grads(g, model, torch_model, case)
    sd_after = model.state_dict()
    for k in g.z.files:
        if k.startswith('train_after_') and 'num_batches' not in k:
            np.testing.assert_allclose(sd_after[k[len('train_after_'):]].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('case', FULL_CASES)
def test_fused_bce_step_vs_golden_with_the_hip_trunk(pkg, monkeypatch, case):
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    g = golden(case)
    models = []
    for switch in ('hip', 'torch'):
        model, dl, params = _model(pkg, g, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, conve_trunk_train=switch)
        model.conv1.drop.p = 0.0
        model.train()
        trip = g.t('train_triple').to(DEV)
        idx = dl.train_index().to(DEV)
        loss = model.forward_loss(trip[:, 0], trip[:, 1], dl.graph, idx, lbl_smooth=0.0)
        loss.backward()
        models.append((model, loss))
    (model, loss), (torch_model, _) = models
    assert model.conv2._trunk_train_count == 1
    assert abs(float(loss.detach()) - float(g['train_loss'])) < 1e-5
    _golden_grads(g, model, torch_model, case + ' fused')


# ---------------------------------------------------------------------------------------------------------------- 6
def _sharded_models(pkg, case, dropout):
    over = dict(gcn_drop=dropout, hidden_drop=dropout, feat_drop=dropout, conve_trunk_train='hip')
    dl, params = _loader(pkg, golden(case), **over)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    assert not model.load_state_dict(golden(case).state_dict(), strict=False).unexpected_keys
    model.conv1.drop.p = dropout / 3
    return model.to(DEV), dl


def _batches(dl, steps, B=8):
    q = dl.train_queries()
    g = torch.Generator().manual_seed(1)
    return [q[torch.randperm(q.size(0), generator=g)[:B]].to(DEV) for _ in range(steps)]


def test_sharded_step_on_one_rank(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    case = 'syn_b'
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    try:
        ref, dl = _sharded_models(pkg, case, 0.0)
        sm, dl_s = _sharded_models(pkg, case, 0.0)
        idx = dl.train_index().to(DEV)
        opt_r, opt_s = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.optim.Adam(sm.parameters(), lr=1e-3)
        for q in _batches(dl, 2):
            opt_r.zero_grad()
            loss_r = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
            loss_r.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
            opt_r.step()
            loss_s = pkg.dist.train_step_sharded(sm, dl_s.graph, q[:, 0], q[:, 1], idx, opt_s, lbl_smooth=0.1, clip=0.5)
            assert torch.equal(loss_s, loss_r.detach())
        assert ref.conv2._trunk_train_count == 2 and sm.conv2._trunk_train_count == 2
        for k, v in ref.state_dict().items():
            assert torch.equal(sm.state_dict()[k], v), k
        # dropout > 0 and a device generator: two identical calls, identical bits
        states = []
        for _ in range(2):
            m, dlm = _sharded_models(pkg, case, 0.3)
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)
            gen = torch.Generator(device=DEV).manual_seed(9)
            torch.manual_seed(9)
            losses = [pkg.dist.train_step_sharded(m, dlm.graph, q[:, 0], q[:, 1], idx, opt, lbl_smooth=0.1, clip=0.5, generator=gen)
                      for q in _batches(dlm, 2)]
            assert m.conv2._trunk_train_count == 2
            states.append((losses, copy.deepcopy(m.state_dict())))
    finally:
        torch.use_deterministic_algorithms(False)
    assert all(torch.equal(a, b) for a, b in zip(states[0][0], states[1][0]))
    for k, v in states[0][1].items():
        assert torch.equal(v, states[1][1][k]), k
