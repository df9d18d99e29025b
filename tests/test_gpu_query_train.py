"""The training step's HIP query path (csrc/query_train.hip, paragraph (11) of include/mgcn_hip.h) on a real MI355X: the
row-gradient scatter held bit for bit to the sequential loop of tests/query_train_ref.py, the trunk's tail to float64 and the
bars of that file, both to their promises (same inputs, same bits; a NULL gradient pointer leaves the others' bits alone;
refusals write nothing; a column's results do not depend on the other columns of the call), the modules with the switch
params.query_path_train on, the goldens' training step, and two runs from one seed giving the same bits without
torch.use_deterministic_algorithms. Every parity case prints `RATIO family id worst-error / bar` (pytest -s) before it asserts."""
import copy
import os
import types

import numpy as np
import pytest
import torch

from . import dense_ref as R
from . import query_train_ref as Q
from . import trunk_ref as T
from . import trunk_train_ref as TT
from .conftest import FULL_CASES, GOLDEN, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL, EUNSUPPORTED = 1, 3
SWITCHES = ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN', 'MGCN_TRUNK')


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _report(family, cid, ratio):
    print('RATIO %s %s %.4f' % (family, cid, ratio))
    assert ratio <= 1.0, '%s %s: worst |got - float64| is %.3f x its bar' % (family, cid, ratio)


def _wide(t, extra, dtype=None):
    """t as a column window of a tensor with `extra` spare guard columns (row stride > its width): NaN, or 0xA5 bytes for a mask."""
    if t.dtype == torch.bool:
        w = torch.full((t.size(0), t.size(1) + extra), 0xA5, dtype=torch.uint8, device=DEV)
        w[:, :t.size(1)] = t.to(DEV).to(torch.uint8)
    else:
        w = torch.full((t.size(0), t.size(1) + extra), float('nan'), device=DEV)
        w[:, :t.size(1)] = t.to(DEV)
    return w[:, :t.size(1)]


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


# ---------------------------------------------------------------------------------------------------------------- 1
def _scatter(lib, idx, d, num_rows, out_extra, d_extra=2):
    """One call through the C ABI: d a window with NaN guard columns, out a window of a guarded buffer (out_extra = 0: its rows
    are contiguous, the flat fill). Returns the Guarded."""
    B, dim = d.shape
    dw = _wide(d, d_extra)
    out = R.Guarded(num_rows, dim, dim + out_extra, DEV)
    nbytes = lib.mgcn_query_rows_bwd_workspace(B)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    idx_dev = idx.to(DEV)
    rc = lib.mgcn_query_rows_bwd(B, num_rows, dim, idx_dev.data_ptr(), dw.data_ptr(), dw.stride(0), out.ptr(), out.ld, ws.data_ptr(),
                                 nbytes, _stream())
    assert rc == 0, lib.mgcn_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('pattern', Q.PATTERNS)
@pytest.mark.parametrize('B', Q.SCATTER_BATCHES)
def test_scatter_equals_the_sequential_loop(pkg, B, pattern):
    lib = pkg._native.lib()
    ran = 0
    for num_rows in Q.SCATTER_ROWS:
        idx = Q.scatter_index(pattern, B, num_rows)
        if idx is None:
            continue
        for dim in Q.SCATTER_DIMS:
            d = Q.scatter_addends(B, dim)
            want = Q.scatter_loop(idx, d, num_rows)
            for out_extra in (0, 3):
                out = _scatter(lib, idx, d, num_rows, out_extra)
                what = '%s B=%d rows=%d dim=%d ld=%d' % (pattern, B, num_rows, dim, dim + out_extra)
                out.check(what)
                assert torch.equal(out.view.cpu(), want), what
                ran += 1
    if pattern not in ('distinct', 'first_last'):
        assert ran == 2 * len(Q.SCATTER_ROWS) * len(Q.SCATTER_DIMS)


def test_scatter_longest_chain_and_flat_fill_offsets(pkg):
    """B = 4096 addends on one row (dim 4), and a contiguous out whose base is 1, 2 or 3 floats off a 16-byte boundary (the flat
    fill's scalar head and tail), each inside a guarded buffer."""
    lib = pkg._native.lib()
    B, dim, num_rows = 4096, 4, 7
    idx = Q.scatter_index('equal', B, num_rows)
    d = Q.scatter_addends(B, dim)
    want = Q.scatter_loop(idx, d, num_rows)
    assert not torch.equal(want, Q.scatter_loop(idx, d, num_rows, reverse=True))
    for out_extra in (0, 1):
        out = _scatter(lib, idx, d, num_rows, out_extra)
        out.check('longest chain')
        assert torch.equal(out.view.cpu(), want)
    B, dim, num_rows = 65, 3, 11
    idx, d = Q.scatter_index('random', B, num_rows), Q.scatter_addends(B, dim)
    want = Q.scatter_loop(idx, d, num_rows)
    nbytes = lib.mgcn_query_rows_bwd_workspace(B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dd, idx_dev = d.to(DEV), idx.to(DEV)
    for off in (1, 2, 3):
        raw = torch.full((num_rows * dim + 16,), R.GUARD_F32, dtype=torch.int32, device=DEV)
        out = raw.view(torch.float32)[off:off + num_rows * dim].view(num_rows, dim)
        assert lib.mgcn_query_rows_bwd(B, num_rows, dim, idx_dev.data_ptr(), dd.data_ptr(), dim, out.data_ptr(), dim, ws.data_ptr(), nbytes,
                                       _stream()) == 0, lib.mgcn_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), off
        assert bool((raw[:off] == R.GUARD_F32).all()) and bool((raw[off + num_rows * dim:] == R.GUARD_F32).all()), off


def test_scatter_wrapper_and_refusals(pkg):
    """_native.query_rows_bwd (a fresh out, and a given window), and refusals that write nothing."""
    nat = pkg._native
    B, dim, num_rows = 63, 200, 5
    idx, d = Q.scatter_index('random', B, num_rows), Q.scatter_addends(B, dim)
    want = Q.scatter_loop(idx, d, num_rows)
    assert torch.equal(nat.query_rows_bwd(idx.to(DEV), d.to(DEV), num_rows).cpu(), want)
    gd = R.Guarded(num_rows, dim, dim + 4, DEV)
    nat.query_rows_bwd(idx.to(DEV), _wide(d, 1), num_rows, out=gd.view)
    torch.cuda.synchronize()
    gd.check('wrapper window')
    assert torch.equal(gd.view.cpu(), want)
    lib = nat.lib()
    out = R.Guarded(num_rows, dim, dim + 2, DEV)
    nbytes = lib.mgcn_query_rows_bwd_workspace(B)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    dd, idx_dev = d.to(DEV), idx.to(DEV)

    def call(batch=B, rows=num_rows, dim_=dim, idx_=idx_dev.data_ptr(), d_=dd.data_ptr(), ldd=dim, out_=out.ptr(), ldo=out.ld, ws_=ws.data_ptr(),
             ws_bytes=nbytes):
        return lib.mgcn_query_rows_bwd(batch, rows, dim_, idx_, d_, ldd, out_, ldo, ws_, ws_bytes, _stream())

    for what, kw in [('null idx', dict(idx_=None)), ('null d', dict(d_=None)), ('null out', dict(out_=None)), ('null workspace', dict(ws_=None)),
                     ('misaligned workspace', dict(ws_=ws.data_ptr() + 4)), ('workspace one byte short', dict(ws_bytes=nbytes - 1)),
                     ('ldd < dim', dict(ldd=dim - 1)), ('ldo < dim', dict(ldo=dim - 1)), ('negative batch', dict(batch=-1)),
                     ('no rows', dict(rows=0)), ('no columns', dict(dim_=0))]:
        assert call(**kw) == EINVAL, what
        assert lib.mgcn_last_error()
    assert call(batch=0) == EUNSUPPORTED and call(batch=4097) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched() and bool((ws == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    out.check('good call')
    assert torch.equal(out.view.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- 2
class TailCall(object):
    """One forward + backward of the tail through the C ABI: inputs as windows (ld > O), every output a window of a guarded
    buffer. `cols` = (c0, width): the call sees only that column window of the same tensors."""

    def __init__(self, nat, B, O, p, skip=(), cols=None):
        self.lib, self.B, self.O = nat.lib(), B, O
        z, keep, inv_keep, gamma, beta, rm, rv, gx = Q.tail_inputs(B, O, p)
        self.z, self.gx = _wide(z, 3), _wide(gx, 2)
        self.keep, self.inv_keep = (None if keep is None else _wide(keep, 5)), inv_keep
        self.gamma, self.beta, self.rm, self.rv = (t.to(DEV).contiguous() for t in (gamma, beta, rm, rv))
        self.c0, self.width = cols if cols is not None else (0, O)
        G = lambda rows, extra: R.Guarded(rows, O, O + extra, DEV)
        self.out = {'x': G(B, 5), 'saved': G(2, 3), 'gz': G(B, 1), 'd_gamma': G(1, 2), 'd_beta': G(1, 1)}
        self.skip = set(skip)

    def _at(self, t, elem=4):
        """The address of column c0 of t's first row (None stays None)."""
        if t is None:
            return None
        return (t.ptr() if isinstance(t, R.Guarded) else t.data_ptr()) + elem * self.c0

    def fwd(self, **over):
        o = self.out
        a = dict(batch=self.B, dim=self.width, z=self._at(self.z), ldz=self.z.stride(0), keep=self._at(self.keep, 1),
                 ldk=0 if self.keep is None else self.keep.stride(0), inv_keep=self.inv_keep, gamma=self._at(self.gamma), beta=self._at(self.beta),
                 rm=self._at(self.rm), rv=self._at(self.rv), momentum=Q.BN_MOMENTUM, eps=Q.BN_EPS, x=self._at(o['x']), ldx=o['x'].ld,
                 saved=self._at(o['saved']), ldsv=o['saved'].ld)
        a.update(over)
        return self.lib.mgcn_conve_tail_fwd(a['batch'], a['dim'], a['z'], a['ldz'], a['keep'], a['ldk'], a['inv_keep'], a['gamma'], a['beta'],
                                            a['rm'], a['rv'], a['momentum'], a['eps'], a['x'], a['ldx'], a['saved'], a['ldsv'], _stream())

    def bwd(self, **over):
        o = self.out
        p = lambda k: None if k in self.skip else self._at(o[k])
        a = dict(batch=self.B, dim=self.width, z=self._at(self.z), ldz=self.z.stride(0), keep=self._at(self.keep, 1),
                 ldk=0 if self.keep is None else self.keep.stride(0), inv_keep=self.inv_keep, x=self._at(o['x']), ldx=o['x'].ld,
                 saved=self._at(o['saved']), ldsv=o['saved'].ld, gamma=self._at(self.gamma), gx=self._at(self.gx), ldg=self.gx.stride(0),
                 gz=p('gz'), ldgz=o['gz'].ld, d_gamma=p('d_gamma'), d_beta=p('d_beta'))
        a.update(over)
        return self.lib.mgcn_conve_tail_bwd(a['batch'], a['dim'], a['z'], a['ldz'], a['keep'], a['ldk'], a['inv_keep'], a['x'], a['ldx'],
                                            a['saved'], a['ldsv'], a['gamma'], a['gx'], a['ldg'], a['gz'], a['ldgz'], a['d_gamma'], a['d_beta'],
                                            _stream())

    def check_guards(self, what):
        """Everything outside the call's column window still holds the guard pattern."""
        c0, c1 = self.c0, self.c0 + self.width
        for k, gd in self.out.items():
            if k in self.skip:
                assert gd.untouched(), '%s: %s was written through a NULL pointer' % (what, k)
                continue
            probe = gd.raw.clone()
            probe[:gd.rows, c0:c1] = gd.pattern
            assert bool((probe == gd.pattern).all()), '%s: %s wrote outside rows [0, %d) x columns [%d, %d)' % (what, k, gd.rows, c0, c1)

    def results(self):
        """name -> tensor over the call's columns, with the names of query_train_ref."""
        c = slice(self.c0, self.c0 + self.width)
        sv = self.out['saved'].view
        got = {'x': self.out['x'].view[:, c], 'mean': sv[0, c], 'rstd': sv[1, c], 'rm': self.rm[c], 'rv': self.rv[c]}
        for k in ('gz', 'd_gamma', 'd_beta'):
            if k not in self.skip:
                got[k] = self.out[k].view[:, c] if k == 'gz' else self.out[k].view[0, c]
        return got


TAIL_CASES = [(B, O, p) for B in Q.TAIL_BATCHES for O in Q.TAIL_DIMS for p in Q.TAIL_PS]


@pytest.mark.parametrize('B,O,p', TAIL_CASES)
def test_tail_grid_through_the_c_abi(pkg, B, O, p):
    cid = 'B%d-O%d-p%g' % (B, O, p)
    ref = Q.tail_reference(B, O, p)
    c = TailCall(pkg._native, B, O, p)
    assert c.fwd() == 0, c.lib.mgcn_last_error()
    assert c.bwd() == 0, c.lib.mgcn_last_error()
    torch.cuda.synchronize()
    c.check_guards(cid)
    if c.keep is not None:                          # the masks' guard columns too
        assert bool((c.keep._base[:, O:] == 0xA5).all())
    worst = {name: ref.ratio(name, got) for name, got in c.results().items()}
    print('RATIOS %s %s' % (cid, ' '.join('%s=%.3f' % kv for kv in sorted(worst.items()))))
    for name, ratio in worst.items():
        _report('query_tail_' + name, cid, ratio)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('B,O,p', [(17, 32, 0.3), (130, 200, 0.3), (63, 200, 0.0)])
def test_tail_same_inputs_same_bits_and_null_gradients(pkg, B, O, p):
    runs = []
    for skip in ((), (), ('gz',), ('d_gamma', 'd_beta'), ('gz', 'd_beta')):
        c = TailCall(pkg._native, B, O, p, skip=skip)
        assert c.fwd() == 0 and c.bwd() == 0, c.lib.mgcn_last_error()
        torch.cuda.synchronize()
        c.check_guards('repeat')
        runs.append(c.results())
    for name, v in runs[0].items():
        assert torch.equal(v, runs[1][name]), name
        for other in runs[2:]:
            if name in other:
                assert torch.equal(v, other[name]), '%s changed when another gradient pointer was NULL' % name
    c = TailCall(pkg._native, B, O, p, skip=('gz', 'd_gamma', 'd_beta'))            # nothing asked for: nothing done
    assert c.fwd() == 0 and c.bwd() == 0
    torch.cuda.synchronize()
    c.check_guards('all NULL')


def test_tail_refusals_write_nothing(pkg):
    B, O = 5, 32
    c = TailCall(pkg._native, B, O, 0.3)
    lib = c.lib
    before = (c.rm.clone(), c.rv.clone())
    nan = float('nan')
    bad_f = [('null z', dict(z=None)), ('null gamma', dict(gamma=None)), ('null beta', dict(beta=None)), ('null running mean', dict(rm=None)),
             ('null running var', dict(rv=None)), ('null x', dict(x=None)), ('null saved', dict(saved=None)), ('ldz < O', dict(ldz=O - 1)),
             ('ldk < O', dict(ldk=O - 1)), ('ldx < O', dict(ldx=O - 1)), ('ldsv < O', dict(ldsv=O - 1)), ('negative batch', dict(batch=-1)),
             ('no columns', dict(dim=0)), ('negative inv_keep', dict(inv_keep=-1.0)), ('NaN inv_keep', dict(inv_keep=nan)),
             ('momentum > 1', dict(momentum=1.5)), ('negative eps', dict(eps=-1.0))]
    for what, kw in bad_f:
        assert c.fwd(**kw) == EINVAL, what
        assert lib.mgcn_last_error()
    for batch in (0, 1, 4097):
        assert c.fwd(batch=batch) == EUNSUPPORTED and c.bwd(batch=batch) == EUNSUPPORTED, batch
    bad_b = [('null z', dict(z=None)), ('null x', dict(x=None)), ('null saved', dict(saved=None)), ('null gamma', dict(gamma=None)),
             ('null gx', dict(gx=None)), ('ldg < O', dict(ldg=O - 1)), ('ldgz < O', dict(ldgz=O - 1)), ('ldx < O', dict(ldx=O - 1)),
             ('negative batch', dict(batch=-1)), ('no columns', dict(dim=0))]
    for what, kw in bad_b:
        assert c.bwd(**kw) == EINVAL, what
    torch.cuda.synchronize()
    assert all(gd.untouched() for gd in c.out.values())
    assert torch.equal(before[0], c.rm) and torch.equal(before[1], c.rv)
    assert c.fwd() == 0 and c.bwd() == 0                                   # and the good call works
    torch.cuda.synchronize()
    c.check_guards('good call')
    ref = Q.tail_reference(B, O, 0.3)
    for name, got in c.results().items():
        assert ref.ratio(name, got) <= 1.0, name


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('B,p', [(130, 0.3), (17, 0.0)])
def test_tail_column_independence(pkg, B, p):
    """The tail on O = 200, and again on the 16-column window [64, 80) of the same tensors: the same bits in those columns."""
    O = 200
    full, part = TailCall(pkg._native, B, O, p), TailCall(pkg._native, B, O, p, cols=(64, 16))
    for c in (full, part):
        assert c.fwd() == 0 and c.bwd() == 0, c.lib.mgcn_last_error()
    torch.cuda.synchronize()
    part.check_guards('window')
    assert torch.equal(part.rm[:64], Q.tail_inputs(B, O, p)[5][:64].to(DEV)) and torch.equal(part.rv[80:], Q.tail_inputs(B, O, p)[6][80:].to(DEV))
    got, want = part.results(), full.results()
    for name in Q.OUTPUTS:
        assert torch.equal(got[name], want[name][..., 64:80]), name
    ref = Q.tail_reference(B, O, p)
    for name, v in got.items():
        _report('query_tail_window_' + name, 'B%d-p%g' % (B, p), ref.ratio(name, v, cols=slice(64, 80)))


# ---------------------------------------------------------------------------------------------------------------- 5
def conve_module(pkg, case, sd=None, **over):
    params = types.SimpleNamespace(**dict(T.hyper(case), **over))
    conv = pkg.model.ConvE(params, 10)
    sd = T.weights(case) if sd is None else sd
    res = conv.load_state_dict({k[len('conv2.'):]: v for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys
    return conv.to(DEV).train()


def _sum_rows(idx, d, num_rows):
    """out[idx[b]] += d[b] in float64 (the reference of a gather's gradient)."""
    return torch.zeros((num_rows, d.size(1)), dtype=torch.float64).index_add_(0, idx, d.double())


PARAM_OF = {'d_conv_w': 'conv_e.weight', 'd_conv_b': 'conv_e.bias', 'd_g0': 'bn0.weight', 'd_b0': 'bn0.bias', 'd_g1': 'bn1.weight',
            'd_b1': 'bn1.bias', 'd_fc_w': 'fc.weight', 'd_fc_b': 'fc.bias'}


@pytest.mark.parametrize('case,B', [((3, 8, 3, 6, True), 17), (T.PRODUCTION, 128)], ids=['small', 'production'])
def test_gathers_and_trunk_against_float64(pkg, case, B):
    """query_rows (both tables, indices with repeats) + ConvE.trunk + backward with both training switches on, against the
    float64 reference of trunk_train_ref fed the gathered rows and the masks drawn from a clone of the
    generator; the reference carries the tail in its own dtype. Bars: trunk_train_ref's, widened by the tail's Lipschitz
    factor max |gamma2| rstd2 / keep (at least 1) as in test_gpu_trunk_train. A table's gradient is a sum of up to n of the
    per-query gradients: n times their bar, plus (n - 1) u of the sum of their magnitudes for the f32 additions themselves."""
    sd = T.weights(case)
    feat = 0.2
    conv = conve_module(pkg, case, sd=sd, conve_trunk_train='hip', query_path_train='hip', feat_drop=feat, hidden_drop=0.3)
    owner = types.SimpleNamespace(training=True, params=conv.params)
    O, K = case[0] * case[1], T.sizes(case)[2]
    n_ent, n_rel = 40, 6
    g = R.gen(R.seed_of(31, B, *T.geometry(case)))
    ent, rel_t = R.pm_uniform((n_ent, O), g), R.pm_uniform((n_rel, O), g)
    src, rel = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, n_rel, (B,), generator=g)
    src[:4] = src[0]                                     # one source at least four times
    s, r = ent[src], rel_t[rel]
    gy = R.pm_uniform((B, O), g)
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
    ent_d, rel_d = ent.to(DEV).requires_grad_(True), rel_t.to(DEV).requires_grad_(True)
    y = conv.trunk(pkg.model.query_rows(owner, ent_d, src.to(DEV)), pkg.model.query_rows(owner, rel_d, rel.to(DEV)), generator=gen)
    assert owner._query_rows_count == 2 and conv._tail_train_count == 1
    assert conv._trunk_train_count == 1
    (y * gy.to(DEV)).sum().backward()
    assert int(conv.bn2.num_batches_tracked) == 1
    cid = '%s-B%d' % (T.case_id(case), B)
    print('bn2 Lipschitz factor %.3f' % lip[0])
    got = {'y': y, 'rm0': conv.bn0.running_mean, 'rv0': conv.bn0.running_var, 'rm1': conv.bn1.running_mean, 'rv1': conv.bn1.running_var}
    params = dict(conv.named_parameters())
    got.update({k: params[v].grad for k, v in PARAM_OF.items() if v in params})
    for name, v in got.items():
        _report('query_module_' + name, cid, ref.ratio(name, v) / (1.0 if name in TT.STATS else lip[0]))
    for name, table, idx, key in (('d_all_ent', ent_d, src, 'ds'), ('d_all_rel', rel_d, rel, 'dr')):
        n = int(torch.bincount(idx).max())
        want = _sum_rows(idx, ref.ref[key], table.size(0))
        bar = n * lip[0] * ref.bar[key] + (n - 1) * R.U * float(_sum_rows(idx, ref.ref[key].abs(), table.size(0)).max())
        _report('query_module_' + name, cid, R.max_ratio(table.grad.cpu(), want, bar))
        unnamed = torch.ones(table.size(0), dtype=torch.bool)
        unnamed[idx] = False
        assert bool((table.grad.cpu()[unnamed] == 0).all())


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


ALL_ON = dict(conve_trunk_train='hip', query_path_train='hip')


def test_forward_loss_step_against_float64(pkg):
    """MGCN.forward_loss + backward with the switches on (syn_b, dropout 0, a batch with repeated sources and relations): the
    loss and the gradients that reach the encoder's two outputs, against float64 autograd of everything after the encoder
    (gathers, trunk, tail, scores, BCE) fed the encoder's own f32 outputs. Bars: derived_bar of the same computation in
    torch-CPU f32, floored at 8 u of the terms of the last additions, widened by the tail's Lipschitz factor as above."""
    g = golden('syn_b')
    model, dl, params = _model(pkg, g, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, **ALL_ON)
    model.conv1.drop.p = 0.0
    model.train()
    case = (int(params.k_w), int(params.k_h), int(params.kernel_size), int(params.num_filter), bool(params.bias))
    sd = {k: v.clone() for k, v in g.state_dict().items() if k.startswith('conv2.')}
    q = dl.train_queries()
    pick = torch.randperm(q.size(0), generator=R.gen(5))[:12]
    batch = torch.cat([q[pick], q[pick[:1]].repeat(4, 1)]).to(DEV)                 # B = 16: one (source, relation) five times
    src, rel = batch[:, 0], batch[:, 1]
    idx = dl.train_index().to(DEV)
    seen = {}
    encode = model.encode

    def recording_encode(data):
        ae, ar = encode(data)
        ae.retain_grad()
        ar.retain_grad()
        seen['ent'], seen['rel'] = ae, ar
        return ae, ar

    model.encode = recording_encode
    loss = model.forward_loss(src, rel, dl.graph, idx, lbl_smooth=0.1)
    loss.backward()
    assert model._query_rows_count == 2 and model.conv2._tail_train_count == 1 and model.conv2._trunk_train_count == 1
    ae, ar = seen['ent'].detach().cpu(), seen['rel'].detach().cpu()
    n_ent = ae.size(0)
    labels = pkg._native.label_rows(idx.query_keys(src, rel), idx.keys, idx.ptr, idx.tails, n_ent, lbl_smooth=0.1).cpu()
    src_c, rel_c = src.cpu(), rel.cpu()
    leaf, lip, losses = {}, [1.0], {}

    def tail(z, dtype):
        mu, var = z.mean(0), z.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + TT.BN_EPS)
        if dtype == torch.float64:
            lip[0] = max(1.0, float((sd['conv2.bn2.weight'].double().abs() * rstd).max()))
        y = torch.relu((z - mu) * rstd * sd['conv2.bn2.weight'].to(dtype) + sd['conv2.bn2.bias'].to(dtype))
        ent = ae.to(dtype).clone().requires_grad_(True)
        leaf[dtype] = ent
        score = torch.sigmoid(y @ ent.t() + sd['conv2.bias'].to(dtype))
        losses[dtype] = torch.nn.functional.binary_cross_entropy(score, labels.to(dtype))
        return y, losses[dtype]

    runs = {}
    for dtype in (torch.float64, torch.float32):
        out = TT.run(case, sd, ae[src_c], ar[rel_c], None, 1.0, None, dtype, with_mag=(dtype == torch.float64), tail=tail)
        out, mag = out if dtype == torch.float64 else (out, None)
        runs[dtype] = {'loss': losses[dtype].detach().double().reshape(1),
                       'd_all_ent': _sum_rows(src_c, out['ds'], n_ent) + leaf[dtype].grad.double(),
                       'd_all_rel': _sum_rows(rel_c, out['dr'], ar.size(0))}
        if mag is not None:
            mags = {'loss': runs[dtype]['loss'].abs(), 'd_all_ent': _sum_rows(src_c, mag['ds'], n_ent) + leaf[dtype].grad.double().abs(),
                    'd_all_rel': _sum_rows(rel_c, mag['dr'], ar.size(0))}
    got = {'loss': loss.detach().reshape(1), 'd_all_ent': seen['ent'].grad, 'd_all_rel': seen['rel'].grad}
    print('bn2 Lipschitz factor %.3f' % lip[0])
    for name, v in got.items():
        want = runs[torch.float64][name]
        cpu_err = float((runs[torch.float32][name] - want).abs().max())
        bar = R.derived_bar(cpu_err, 8 * R.U * float(mags[name].max())) * lip[0]
        assert bar <= 1e-4 * float(want.abs().max()), (name, bar)              # the vacuity rule of query_train_ref
        _report('query_forward_loss_' + name, 'syn_b-B16', R.max_ratio(v.cpu(), want, bar))


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


@pytest.mark.parametrize('fused', [False, True], ids=['forward', 'forward_loss'])
@pytest.mark.parametrize('case', FULL_CASES)
def test_train_step_vs_golden_with_the_hip_query_path(pkg, case, fused):
    """The goldens' training step as test_gpu_trunk_train does it (same bars), with every switch on."""
    g = golden(case)
    models = []
    for over in (ALL_ON, {}):
        model, dl, params = _model(pkg, g, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, **over)
        model.conv1.drop.p = 0.0
        model.train()
        trip = g.t('train_triple').to(DEV)
        if fused:
            pred, loss = None, model.forward_loss(trip[:, 0], trip[:, 1], dl.graph, dl.train_index().to(DEV), lbl_smooth=0.0)
        else:
            pred = model(trip[:, 0], trip[:, 1], dl.graph)
            loss = model.loss(pred, g.t('train_label').to(DEV))
        loss.backward()
        models.append((model, pred, loss))
    (model, pred, loss), (torch_model, _, _) = models
    B = g.t('train_triple').size(0)
    expect = 1 if B >= 2 else 0                          # (a one-query batch keeps torch's tail)
    assert model._query_rows_count == 2 and getattr(model.conv2, '_tail_train_count', 0) == expect
    assert not hasattr(torch_model, '_query_rows_count') and not hasattr(torch_model.conv2, '_tail_train_count')
    if pred is not None:
        print('%s: largest |score - golden| = %.3g' % (case, float(np.abs(pred.detach().cpu().numpy() - g['train_score']).max())))
        np.testing.assert_allclose(pred.detach().cpu().numpy(), g['train_score'], rtol=0, atol=2e-5)
    assert abs(float(loss.detach()) - float(g['train_loss'])) < 1e-5
    _golden_grads(g, model, torch_model, case)
    if not fused:
        sd_after = model.state_dict()
        for k in g.z.files:
            if k.startswith('train_after_') and 'num_batches' not in k:
                np.testing.assert_allclose(sd_after[k[len('train_after_'):]].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6)
        if g.has('train_after_conv2.bn2.num_batches_tracked'):
            assert int(sd_after['conv2.bn2.num_batches_tracked']) == int(g['train_after_conv2.bn2.num_batches_tracked'])


def test_dispatch(pkg, monkeypatch):
    """The counters move only with the switch on, in training mode, with autograd; with the switch off the outputs and
    gradients are those of a model that never heard of it (today's expressions, on torch's own stream)."""
    case = (4, 8, 3, 8, False)
    s, r = (t.to(DEV) for t in T.queries(case, 40))
    tails = lambda m: getattr(m, '_tail_train_count', 0)

    def same_as_torch(on, off, seed, **kw):
        before = tails(on)
        outs = []
        for m in (on, off):
            torch.manual_seed(seed)
            outs.append(m.trunk(s, r, **kw))
        assert torch.equal(outs[0], outs[1]) and tails(on) == before
        assert torch.equal(on.bn2.running_var, off.bn2.running_var)

    on, off = conve_module(pkg, case, query_path_train='hip'), conve_module(pkg, case)
    on.trunk(s, r)
    assert tails(on) == 1 and tails(off) == 0 and int(on.bn2.num_batches_tracked) == 1
    # the switch off: today's code on today's modules (F.dropout's own stream)
    torch.manual_seed(3)
    y_off = off.trunk(s, r)
    twin = conve_module(pkg, case)
    torch.manual_seed(3)
    x = torch.cat([s.view(-1, 1, 32), r.view(-1, 1, 32)], dim=1).transpose(2, 1).reshape(-1, 1, 8, 8)
    x = twin.feature_drop(torch.relu(twin.bn1(twin.conv_e(twin.bn0(x)))))
    parent = torch.relu(twin.bn2(twin.hidden_drop(twin.fc(x.view(-1, twin.flat_sz))))).contiguous()
    assert torch.equal(y_off, parent)
    # eval mode, no autograd, the environment variable, momentum=None, no running statistics, a one-query batch
    a, b = conve_module(pkg, case, query_path_train='hip').eval(), conve_module(pkg, case).eval()
    same_as_torch(a, b, 4)
    a, b = conve_module(pkg, case, query_path_train='hip'), conve_module(pkg, case)
    with torch.no_grad():
        same_as_torch(a, b, 5)
    monkeypatch.setenv('MGCN_QUERY_TRAIN', 'torch')
    same_as_torch(a, b, 6)
    monkeypatch.setenv('MGCN_QUERY_TRAIN', 'hip')
    assert tails(b) == 0
    b.trunk(s, r)
    assert tails(b) == 1                                                    # ... and it overrides in the other direction
    monkeypatch.delenv('MGCN_QUERY_TRAIN')
    a, b = conve_module(pkg, case, query_path_train='hip'), conve_module(pkg, case)
    a.bn2.momentum = b.bn2.momentum = None
    same_as_torch(a, b, 7)
    a, b = conve_module(pkg, case, query_path_train='hip'), conve_module(pkg, case)
    with pytest.raises(ValueError):                                         # torch's own "more than 1 value per channel"
        a.trunk(s[:1], r[:1])
    assert tails(a) == 0
    # the HIP conv block alone keeps the torch tail's bits: the switch off changes nothing there either
    gen = lambda: torch.Generator(device=DEV).manual_seed(21)
    a = conve_module(pkg, case, conve_trunk_train='hip')
    bn2_before, seen = copy.deepcopy(a.bn2), {}
    hook = a.bn2.register_forward_hook(lambda m, i, o: seen.__setitem__('in', i[0]))
    ya = a.trunk(s, r, generator=gen())
    hook.remove()
    assert torch.equal(ya, torch.relu(bn2_before(seen['in']))) and torch.equal(a.bn2.running_var, bn2_before.running_var)
    assert tails(a) == 0 and a._trunk_train_count == 1
    # dist._trunk with a generator: its torch tail and the HIP tail see the same masks, so they agree to rounding
    for block in ('torch', 'hip'):
        a, b = conve_module(pkg, case, conve_trunk_train=block, query_path_train='hip'), conve_module(pkg, case, conve_trunk_train=block)
        ya, yb = pkg.dist._trunk(a, s, r, gen()), pkg.dist._trunk(b, s, r, gen())
        assert tails(a) == 1 and tails(b) == 0
        assert float((ya - yb).abs().max()) <= 1e-4 * float(yb.abs().max())
        assert ((ya == 0) != (yb == 0)).float().mean() < 0.01                # the same elements dropped / rectified
    # the gathers: a table without a gradient, int32 indices, eval mode and no_grad keep index_select
    owner = types.SimpleNamespace(training=True, params=types.SimpleNamespace(query_path_train='hip'))
    table = torch.randn(9, 4, device=DEV, requires_grad=True)
    idx = torch.tensor([3, 3, 1, 3], device=DEV)
    rows = lambda o, t, i: pkg.model.query_rows(o, t, i)
    assert rows(owner, table, idx).grad_fn.name().startswith('_QueryRowsFn') and owner._query_rows_count == 1
    assert torch.equal(rows(owner, table.detach(), idx), table.detach()[idx])
    assert torch.equal(rows(owner, table, idx.int()), table.detach()[idx])
    with torch.no_grad():
        rows(owner, table, idx)
    owner.training = False
    rows(owner, table, idx)
    off_owner = types.SimpleNamespace(training=True, params=types.SimpleNamespace())
    assert not rows(off_owner, table, idx).grad_fn.name().startswith('_QueryRowsFn')
    assert owner._query_rows_count == 1 and not hasattr(off_owner, '_query_rows_count')


# ---------------------------------------------------------------------------------------------------------------- 6
def _fresh(pkg, case, dropout, **over):
    over = dict(dict(gcn_drop=dropout, hidden_drop=dropout, feat_drop=dropout, **ALL_ON), **over)
    dl, params = _loader(pkg, golden(case), **over)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    assert not model.load_state_dict(golden(case).state_dict(), strict=False).unexpected_keys
    model.conv1.drop.p = dropout / 3
    return model.to(DEV), dl


def _repeating_batches(dl, steps, B=16):
    """Batches in which one query (its source and its relation) occurs five times: rows of d all_ent and d all_rel with more than
    three addends, whose order would show."""
    q = dl.train_queries()
    g = torch.Generator().manual_seed(1)
    out = []
    for _ in range(steps):
        pick = torch.randperm(q.size(0), generator=g)[:B - 4]
        batch = torch.cat([q[pick], q[pick[:1]].repeat(4, 1)])
        assert int(torch.bincount(batch[:, 0]).max()) >= 4 and int(torch.bincount(batch[:, 1]).max()) >= 4
        out.append(batch[torch.randperm(B, generator=g)].to(DEV))
    return out


def test_two_runs_one_seed_same_bits_without_the_determinism_flag(pkg):
    """forward_loss + backward + ClipAdam.clip_and_step, two steps at dropout 0.3, twice from the same seeds: every loss and
    every state_dict entry has the same bits, with torch.use_deterministic_algorithms off."""
    assert not torch.are_deterministic_algorithms_enabled()
    states = []
    for _ in range(2):
        model, dl = _fresh(pkg, 'syn_b', 0.3)
        model.train()
        idx = dl.train_index().to(DEV)
        opt = pkg.ClipAdam(model.parameters(), lr=1e-3)
        torch.manual_seed(9)
        losses = []
        for q in _repeating_batches(dl, 2):
            opt.zero_grad()
            loss = model.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
            loss.backward()
            opt.clip_and_step(0.5)
            losses.append(loss.detach().clone())
        assert model._query_rows_count == 4 and model.conv2._tail_train_count == 2 and model.conv2._trunk_train_count == 2
        assert opt._hip_step_count == 2
        states.append((losses, copy.deepcopy(model.state_dict())))
    assert all(torch.equal(a, b) for a, b in zip(states[0][0], states[1][0]))
    for k, v in states[0][1].items():
        assert torch.equal(v, states[1][1][k]), k


def test_sharded_step_on_one_rank_without_the_determinism_flag(pkg):
    """dist.train_step_sharded on one rank against the one-GPU step at dropout 0, bit for bit, and two identical sharded runs at
    dropout 0.3 from one device generator -- the promises of test_gpu_trunk_train's sharded test, without the global flag."""
    assert not torch.are_deterministic_algorithms_enabled()
    ref, dl = _fresh(pkg, 'syn_b', 0.0)
    sm, dl_s = _fresh(pkg, 'syn_b', 0.0)
    idx = dl.train_index().to(DEV)
    opt_r, opt_s = pkg.ClipAdam(ref.parameters(), lr=1e-3), pkg.ClipAdam(sm.parameters(), lr=1e-3)
    ref.train()
    for q in _repeating_batches(dl, 2):
        opt_r.zero_grad()
        loss_r = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
        loss_r.backward()
        opt_r.clip_and_step(0.5)
        loss_s = pkg.dist.train_step_sharded(sm, dl_s.graph, q[:, 0], q[:, 1], idx, opt_s, lbl_smooth=0.1, clip=0.5)
        assert torch.equal(loss_s, loss_r.detach())
    for m in (ref, sm):
        assert m._query_rows_count == 4 and m.conv2._tail_train_count == 2 and m.conv2._trunk_train_count == 2
    for k, v in ref.state_dict().items():
        assert torch.equal(sm.state_dict()[k], v), k
    states = []
    for _ in range(2):
        m, dlm = _fresh(pkg, 'syn_b', 0.3)
        opt = pkg.ClipAdam(m.parameters(), lr=1e-3)
        gen = torch.Generator(device=DEV).manual_seed(9)
        torch.manual_seed(9)
        losses = [pkg.dist.train_step_sharded(m, dlm.graph, q[:, 0], q[:, 1], idx, opt, lbl_smooth=0.1, clip=0.5, generator=gen)
                  for q in _repeating_batches(dlm, 2)]
        assert m._query_rows_count == 4 and m.conv2._tail_train_count == 2
        states.append((losses, copy.deepcopy(m.state_dict())))
    assert all(torch.equal(a, b) for a, b in zip(states[0][0], states[1][0]))
    for k, v in states[0][1].items():
        assert torch.equal(v, states[1][1][k]), k
