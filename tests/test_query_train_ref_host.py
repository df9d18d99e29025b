"""tests/query_train_ref.py checked on the CPU (`-m "not gpu"`): the scatter loop against torch autograd of index_select and
its sensitivity to the order of the addends, the tail's float64 reference against Dropout -> BatchNorm1d -> relu in float64
(running statistics included), the bars against their vacuity caps, and what the entry points of paragraph (11) of
include/mgcn_hip.h do without a GPU."""
import os
import types

import pytest
import torch

from . import query_train_ref as Q

EINVAL, EUNSUPPORTED = 1, 3
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ('mgcn_query_rows_bwd_workspace', 'mgcn_query_rows_bwd', 'mgcn_conve_tail_fwd', 'mgcn_conve_tail_bwd')


@pytest.mark.parametrize('pattern', Q.PATTERNS)
def test_scatter_loop_is_index_select_backward_and_order_shows(pattern):
    """In float64 the loop equals autograd's gradient of index_select exactly up to rounding (1e-12 relative); in f32 the
    reversed loop gives other bits for every pattern that puts three or more addends on a row."""
    seen_order = False
    for B in Q.SCATTER_BATCHES:
        for num_rows in Q.SCATTER_ROWS:
            idx = Q.scatter_index(pattern, B, num_rows)
            if idx is None:
                continue
            assert idx.dtype == torch.int64 and idx.shape == (B,) and int(idx.min()) >= 0 and int(idx.max()) < num_rows
            d = Q.scatter_addends(B, 4)
            table = torch.zeros((num_rows, 4), dtype=torch.float64, requires_grad=True)
            torch.index_select(table, 0, idx).backward(d.double())
            want = Q.scatter_loop(idx, d, num_rows)
            scale = float(d.abs().double().sum())
            assert float((table.grad - want.double()).abs().max()) <= 1e-6 * scale
            named = torch.zeros(num_rows, dtype=torch.bool)
            named[idx] = True
            assert bool((want[~named] == 0).all())
            most = int(torch.bincount(idx, minlength=num_rows).max())
            if most >= 8:                               # (with three addends the two orders can still round alike)
                assert not torch.equal(want, Q.scatter_loop(idx, d, num_rows, reverse=True)), (pattern, B, num_rows)
                seen_order = True
    assert seen_order == (pattern not in ('distinct', 'first_last'))


def test_patterns_are_what_they_say():
    idx = Q.scatter_index('first_last', 65, 300)
    assert int(idx[0]) == int(idx[-1]) and idx[:-1].unique().numel() == 64
    assert Q.scatter_index('distinct', 257, 300).unique().numel() == 257
    assert Q.scatter_index('distinct', 63, 5) is None and Q.scatter_index('first_last', 2, 300) is None
    assert set(Q.scatter_index('ends', 64, 300).tolist()) == {0, 299}
    assert Q.scatter_index('equal', 257, 5).unique().tolist() == [2]
    assert sorted(Q.scatter_index('alternate', 65, 300).unique().tolist()) == [100, 200]


@pytest.mark.parametrize('B,O,p', [(2, 32, 0.3), (17, 200, 0.3), (130, 32, 0.0), (16, 1, 1.0)])
def test_tail_reference_equals_the_torch_modules_in_float64(B, O, p):
    """model._drawn_dropout's expression -> nn.BatchNorm1d -> relu in double, fed the same mask: x, the three gradients and
    the running statistics to 1e-12 relative."""
    z, keep, inv_keep, gamma, beta, rm, rv, gx = Q.tail_inputs(B, O, p)
    bn = torch.nn.BatchNorm1d(O, eps=Q.BN_EPS, momentum=Q.BN_MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    zd = z.double().requires_grad_(True)
    u = zd if keep is None else zd * keep.double() * inv_keep
    x = torch.relu(bn(u))
    x.backward(gx.double())
    want = Q.tail_run(z, keep, inv_keep, gamma, beta, rm, rv, gx)
    got = {'x': x, 'gz': zd.grad, 'd_gamma': bn.weight.grad, 'd_beta': bn.bias.grad, 'rm': bn.running_mean, 'rv': bn.running_var}
    for name, v in got.items():
        scale = max(float(want[name].abs().max()), 1e-30)
        assert float((v.detach() - want[name]).abs().max()) <= 1e-12 * max(scale, 1.0), name


def test_dropout_order_is_drawn_dropouts(pkg):
    """u = (z * mask) * (1 / keep), the expression of model._drawn_dropout, bit for bit in f32."""
    z = Q.tail_inputs(17, 32, 0.3)[0]
    g = torch.Generator().manual_seed(3)
    twin = torch.Generator()
    twin.set_state(g.get_state())
    want = pkg.model._drawn_dropout(z, 0.3, g)
    mask = torch.empty_like(z).bernoulli_(0.7, generator=twin)
    assert torch.equal(want, (z * mask.bool().float()) * (1.0 / 0.7))


CASES = [(B, O, p) for B in Q.TAIL_BATCHES for O in Q.TAIL_DIMS for p in Q.TAIL_PS]


@pytest.mark.parametrize('B,O,p', CASES)
def test_bars_stay_under_their_vacuity_caps(B, O, p):
    """No bar of the GPU grid may exceed 1e-4 of its tensor, and every pre-activation of the float64 reference lies further
    from 0 than x's bar: an evaluation that is inside the bar rectifies the same elements, so the backward, which is
    discontinuous there, is compared on the same relu mask. Printed as bar / cap."""
    ref = Q.tail_reference(B, O, p)
    caps = Q.tail_vacuity(ref)
    print('B=%d O=%d p=%g margin=%.3g: %s' % (B, O, p, ref.margin, ' '.join('%s=%.3g' % kv for kv in sorted(caps.items()))))
    for name, ratio in caps.items():
        assert ratio <= 1.0, (name, ratio)
    assert ref.margin > 2.0 * ref.bar['x'], (ref.margin, ref.bar['x'])
    if p >= 1.0:
        assert all(ref.bar[k] == 0.0 for k in ('gz', 'd_gamma'))


def test_header_and_binding_carry_the_query_path(pkg):
    with open(os.path.join(os.path.dirname(HERE), 'include', 'mgcn_hip.h')) as fh:
        header = fh.read()
    for n in NAMES:
        assert n in pkg._native.EXPORTS and n + '(' in header
    assert '#define MGCN_ABI_VERSION 4' in header and pkg._native.ABI_VERSION == 4
    assert pkg._native.lib().mgcn_abi_version() == 4


def test_entry_points_refuse_bad_arguments_without_a_gpu(pkg):
    """All argument checks precede the first launch: the library answers MGCN_EINVAL / MGCN_EUNSUPPORTED on a machine with no
    GPU (the pointers are made-up, 16-byte aligned addresses that are never followed)."""
    lib = pkg._native.lib()
    P = 0x10000
    B, N, D = 5, 7, 12
    assert lib.mgcn_query_rows_bwd_workspace(B) >= B * 12 and lib.mgcn_query_rows_bwd_workspace(B) % 16 == 0
    assert lib.mgcn_query_rows_bwd_workspace(4096) >= 4096 * 12
    for refused in (0, -1, 4097, 1 << 20):
        assert lib.mgcn_query_rows_bwd_workspace(refused) == 0
    nbytes = lib.mgcn_query_rows_bwd_workspace(B)

    def rows(batch=B, num_rows=N, dim=D, idx=P, d=P, ldd=D, out=P, ldo=D, ws=P, ws_bytes=nbytes):
        return lib.mgcn_query_rows_bwd(batch, num_rows, dim, idx, d, ldd, out, ldo, ws, ws_bytes, None)

    for kw in [dict(idx=None), dict(d=None), dict(out=None), dict(ws=None), dict(ws=P + 8), dict(ws_bytes=nbytes - 1), dict(ws_bytes=0),
               dict(ldd=D - 1), dict(ldo=D - 1), dict(batch=-1), dict(num_rows=0), dict(num_rows=-3), dict(dim=0)]:
        assert rows(**kw) == EINVAL, kw
        assert lib.mgcn_last_error()
    for kw in [dict(batch=0), dict(batch=4097, ws_bytes=1 << 20), dict(num_rows=(1 << 50) + 1)]:
        assert rows(**kw) == EUNSUPPORTED, kw

    def fwd(batch=B, dim=D, z=P, ldz=D, keep=None, ldk=D, inv_keep=1.0, gamma=P, beta=P, rm=P, rv=P, momentum=0.1, eps=1e-5, x=P, ldx=D,
            saved=P, ldsv=D):
        return lib.mgcn_conve_tail_fwd(batch, dim, z, ldz, keep, ldk, inv_keep, gamma, beta, rm, rv, momentum, eps, x, ldx, saved, ldsv, None)

    def bwd(batch=B, dim=D, z=P, ldz=D, keep=None, ldk=D, inv_keep=1.0, x=P, ldx=D, saved=P, ldsv=D, gamma=P, gx=P, ldg=D, gz=P, ldgz=D):
        return lib.mgcn_conve_tail_bwd(batch, dim, z, ldz, keep, ldk, inv_keep, x, ldx, saved, ldsv, gamma, gx, ldg, gz, ldgz, P, P, None)

    nan = float('nan')
    for kw in [dict(z=None), dict(gamma=None), dict(beta=None), dict(rm=None), dict(rv=None), dict(x=None), dict(saved=None),
               dict(ldz=D - 1), dict(ldx=D - 1), dict(ldsv=D - 1), dict(keep=P, ldk=D - 1), dict(batch=-1), dict(dim=0), dict(inv_keep=-1.0),
               dict(inv_keep=nan), dict(momentum=1.5), dict(momentum=nan), dict(eps=-1.0)]:
        assert fwd(**kw) == EINVAL, kw
        assert lib.mgcn_last_error()
    for kw in [dict(z=None), dict(x=None), dict(saved=None), dict(gamma=None), dict(gx=None), dict(ldz=D - 1), dict(ldx=D - 1),
               dict(ldsv=D - 1), dict(ldg=D - 1), dict(ldgz=D - 1), dict(keep=P, ldk=D - 1), dict(batch=-1), dict(dim=0), dict(inv_keep=nan)]:
        assert bwd(**kw) == EINVAL, kw
    for call in (fwd, bwd):
        for batch in (0, 1, 4097):                       # B = 1: one value per channel has no batch statistics
            assert call(batch=batch) == EUNSUPPORTED, batch
            assert lib.mgcn_last_error()
    assert not pkg._native.conve_tail_supported(1, 200) and pkg._native.conve_tail_supported(2, 1)
    assert not pkg._native.query_rows_supported(0) and pkg._native.query_rows_supported(4096) and not pkg._native.query_rows_supported(4097)


def test_switch_with_cpu_tensors_takes_the_torch_path(pkg, monkeypatch):
    """The switch acts on f32 GPU tensors only: on the CPU the gathers and the tail are today's torch code, bit for bit, with
    params.query_path_train and with the environment variable."""
    from . import trunk_ref as T
    monkeypatch.delenv('MGCN_QUERY_TRAIN', raising=False)
    monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
    case = T.GRID[1]

    def conve(**over):
        conv = pkg.model.ConvE(types.SimpleNamespace(**dict(T.hyper(case), **over)), 10)
        assert not conv.load_state_dict({k[len('conv2.'):]: v for k, v in T.weights(case).items()}, strict=False).unexpected_keys
        return conv.train()

    s, r = T.queries(case, 6)
    for env in (None, 'hip'):
        if env:
            monkeypatch.setenv('MGCN_QUERY_TRAIN', env)
        on, off = conve(query_path_train='hip'), conve()
        outs = []
        for m in (on, off):
            torch.manual_seed(2)
            outs.append(m.trunk(s, r))
        assert torch.equal(outs[0], outs[1]) and not hasattr(on, '_tail_train_count') and not hasattr(off, '_tail_train_count')
        owner = types.SimpleNamespace(training=True, params=types.SimpleNamespace(query_path_train='hip'))
        table = torch.randn(9, 4, requires_grad=True)
        idx = torch.tensor([3, 3, 1, 3])
        pkg.model.query_rows(owner, table, idx).sum().backward()
        assert not hasattr(owner, '_query_rows_count') and torch.equal(table.grad[3], torch.full((4,), 3.0))
