"""csrc/train_layer.hip held to float64 at its block edges (`-m gpu`): the training epilogue (4t) forward / backward, its
split stages (4s) bit for bit, and the split-K weight-gradient product mgcn_matmul_tn_f32. N runs around the 128-row
statistic blocks, O around the 256-column trips of combine_sum_kernel / partial_kernel and the 256-column blocks of
fold_kernel / stats_finish_kernel. References, grids and bars: tests/dense_ref.py. Every case prints
`RATIO family id worst-error / bar` (pytest -s) before it asserts."""
import pytest
import torch

from . import dense_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
UNSUPPORTED = 3
U = R.U


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _report(family, cid, ratio):
    print('RATIO %s %s %.4f' % (family, cid, ratio))
    assert ratio <= 1.0, '%s %s: worst |got - float64| is %.3f x its bar' % (family, cid, ratio)


def _dev(t):
    return None if t is None else t.to(DEV)


def _wide(u, extra):
    """The three products as column windows of tensors with row stride O + extra (ldu > O), NaN in the spare columns."""
    out = []
    for t in u:
        w = torch.full((t.shape[0], t.shape[1] + extra), float('nan'), device=DEV)
        w[:, :t.shape[1]] = t
        out.append(w[:, :t.shape[1]])
    return out


@pytest.mark.parametrize('case', R.TRAIN_CASES, ids=R.case_id)
def test_training_epilogue_vs_float64(pkg, case):
    """(4t): z, y, saved mean / rstd, running statistics, gz, gu, ggamma, gbeta against float64 autograd of
    F.batch_norm(training=True) + tanh. Bars: dense_ref.derived_bar -- 4 x torch-CPU f32 autograd's own error on the same
    inputs, floored at 8 u of the terms being added, capped by test_training_layer_kernels_vs_torch_autograd's bars."""
    nat = pkg._native
    N, O, with_bias, with_running, extra = case
    cid = R.case_id(case)
    u, bias, gamma, beta, rm, rv, gy = R.train_inputs(N, O, with_bias, with_running)
    r64 = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy)
    r32 = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy, dtype=torch.float32)
    cpu_err = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64 if r64[k] is not None}
    du, dbias, dgamma, dbeta, drm, drv, dgy = _wide([t.to(DEV) for t in u], extra), _dev(bias), _dev(gamma), _dev(beta), _dev(rm), _dev(rv), _dev(gy)
    y, z, mean, rstd = nat.bn_tanh_train_fwd(*du, dbias, dgamma, dbeta, drm, drv, R.BN_MOMENTUM, R.BN_EPS)
    gz, gu, gg, gb = nat.bn_tanh_train_bwd(z, y, dgy, mean, rstd, dgamma)
    torch.cuda.synchronize()
    got = dict(z=z, y=y, mean=mean, rstd=rstd, rm=drm, rv=drv, gz=gz, gu=gu, ggamma=gg, gbeta=gb)
    # z = (a + b + c) / 3 (+ bias): two adds, a division, an add -- each within u / 2 of its result
    zmag = sum(t.double().abs() for t in u) + (bias.double().abs() if with_bias else 0.0)
    _report('train_z', cid, R.max_ratio(z.cpu(), r64['z'], 2 * U * zmag + 1e-45))
    z64 = r64['z']
    zabs = float(z64.abs().max())
    rstd_max = float(r64['rstd'].max())
    S = float((gamma.double().abs() * r64['rstd']).max())                       # |d y / d z| <= |gamma| rstd
    gp = gy.double() * (1 - r64['y'] ** 2)
    gp_max = float(gp.abs().max())
    xh_max = float(((z64 - r64['mean']) * r64['rstd']).abs().max())
    bars = {
        # name: (floor = 8 u x the result and the largest term of its last additions, today's bar or None)
        'mean': (8 * U * zabs, None),
        'rstd': (8 * U * rstd_max, None),
        'y': (8 * U, 2e-6),
        'gz': (8 * U * S * gp_max * (1 + xh_max * xh_max), 2e-5 * float(r64['gz'].abs().max())),
        'gu': (8 * U * S * gp_max * (1 + xh_max * xh_max) / 3, 2e-5 * float(r64['gu'].abs().max())),
        'ggamma': (8 * U * (float(r64['ggamma'].abs().max()) + gp_max * xh_max), 2e-5 * float(r64['ggamma'].abs().max())),
        'gbeta': (8 * U * (float(r64['gbeta'].abs().max()) + gp_max), 2e-5 * float(r64['gbeta'].abs().max())),
    }
    if with_running:
        bars['rm'] = (8 * U * float(r64['rm'].abs().max()), 1e-7)
        bars['rv'] = (8 * U * float(r64['rv'].abs().max()), 1e-5 * float(r64['rv'].abs().min()) + 1e-7)
    for name, (floor, today) in bars.items():
        bar = R.derived_bar(cpu_err[name], floor, today)
        _report('train_' + name, cid, R.max_ratio(got[name].cpu(), r64[name], bar))
    assert torch.equal(gu.cpu(), gz.cpu() / torch.full((N, O), 3.0))          # gu = gz / 3, an IEEE division
    if not with_running:                                                         # NULL running statistics: nothing else to check
        assert drm is None and drv is None


@pytest.mark.parametrize('case', R.TRAIN_ILL_CASES, ids=R.case_id)
def test_training_epilogue_ill_conditioned_columns(pkg, case):
    """Columns with mean 100 and spread 1e-2 (the reason the variance is two-pass). f32 cannot give xhat to the usual bar
    here (torch-CPU f32 batch_norm itself is ~1e-3 off float64), so: (1) save_mean / save_rstd against float64 statistics
    of the RETURNED z -- mean to the column-sum bar with K = N, rstd to 4 x the relative error of a two-pass f32 CPU emulation on
    that same z (dense_ref.ill_rstd_bar); (2) y against float64 tanh((z - mean) rstd gamma + beta)
    evaluated from the returned statistics."""
    nat = pkg._native
    N, O = case
    cid = R.case_id(case)
    g = R.gen(R.seed_of(6, N, O))
    zin = R.ill_conditioned_z(N, O, g)
    gamma, beta = R.pm_uniform((O,), g) * 1.5, R.randn_scaled((O,), g, 0.1)
    dz = zin.to(DEV)
    y, z, mean, rstd = nat.bn_tanh_train_fwd(dz, dz, dz, None, gamma.to(DEV), beta.to(DEV), None, None, R.BN_MOMENTUM, R.BN_EPS)
    torch.cuda.synchronize()
    z64 = z.double()
    _report('ill_z', cid, R.max_ratio(z, zin.to(DEV).double(), 2 * U * 3 * zin.to(DEV).double().abs()))
    mean64 = z64.mean(0)
    rstd64 = 1 / torch.sqrt(z64.var(0, unbiased=False) + R.BN_EPS)
    _report('ill_mean', cid, R.max_ratio(mean, mean64, R.colsum_bar(z64.abs().sum(0) / N, N)))
    _report('ill_rstd', cid, R.max_ratio(rstd, rstd64, R.ill_rstd_bar(z, R.BN_EPS) * rstd64))
    # (2) from the returned statistics: z - mean is exact (Sterbenz), two products and an add follow
    t64 = (z64 - mean.double()) * rstd.double() * gamma.to(DEV).double() + beta.to(DEV).double()
    y64 = torch.tanh(t64)
    arg_bar = R.C_EPI * U * (t64.abs() + beta.to(DEV).double().abs())
    _report('ill_y', cid, R.max_ratio(y, y64, R.tanh_bar(y64, arg_bar)))


@pytest.mark.parametrize('case', R.TRAIN_SPLIT_CASES, ids=R.case_id)
def test_split_stages_equal_unsplit_past_256_columns(pkg, case):
    """(4s) with two "ranks" whose first rows are multiples of 128 equals (4t) bit for bit, at widths that take the second
    column trip of combine_sum_kernel / partial_kernel and the second block of fold_kernel / stats_finish_kernel."""
    nat = pkg._native
    N, cut, O = case
    u, bias, gamma, beta, rm0, rv0, gy = [_dev(t) if not isinstance(t, list) else [v.to(DEV) for v in t] for t in R.train_inputs(N, O, True, True)]
    rm, rv = rm0.clone(), rv0.clone()
    y, z, mean, rstd = nat.bn_tanh_train_fwd(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS)
    gz, gu, gg, gb = nat.bn_tanh_train_bwd(z, y, gy, mean, rstd, gamma)
    pieces = [(0, cut), (cut, N)]
    assert cut % 128 == 0
    st1 = [nat.bn_train_stage_sum(*[t[a:b] for t in u], bias) for a, b in pieces]
    assert torch.equal(torch.cat([s[0] for s in st1]), z)
    parts = torch.cat([s[1] for s in st1])
    st2 = [nat.bn_train_stage_center(s[0], parts, N) for s in st1]
    parts2 = torch.cat([s[1] for s in st2])
    ys = []
    for s, c in zip(st1, st2):
        assert torch.equal(c[0], mean)
        m, v = rm0.clone(), rv0.clone()
        yy, rs = nat.bn_train_stage_finish(s[0], parts2, N, c[0], gamma, beta, m, v, R.BN_MOMENTUM, R.BN_EPS)
        assert torch.equal(rs, rstd) and torch.equal(m, rm) and torch.equal(v, rv)
        ys.append(yy)
    assert torch.equal(torch.cat(ys), y)
    bw = [nat.bn_train_bwd_stage_sums(z[a:b], y[a:b], gy[a:b], mean, rstd) for a, b in pieces]
    allp = torch.cat(bw, dim=1)
    outs = [nat.bn_train_bwd_stage_apply(z[a:b], y[a:b], gy[a:b], mean, rstd, gamma, allp[0], allp[1], N) for a, b in pieces]
    assert torch.equal(torch.cat([o[0] for o in outs]), gz) and torch.equal(torch.cat([o[1] for o in outs]), gu)
    for o in outs:
        assert torch.equal(o[2], gg) and torch.equal(o[3], gb)
    # and the unsplit values themselves are right past column 256
    r64 = R.ref_train_epilogue(*[t.cpu() for t in u], bias.cpu(), gamma.cpu(), beta.cpu(), rm0.cpu(), rv0.cpu(), R.BN_MOMENTUM, R.BN_EPS,
                               gy.cpu())
    assert float((y.cpu().double() - r64['y'])[:, 256:].abs().max()) <= 2e-6
    assert float((gb.cpu().double() - r64['gbeta'])[256:].abs().max()) <= 2e-5 * float(r64['gbeta'].abs().max())


# ----------------------------------------------------------------------------------------------------------------
# mgcn_matmul_tn_f32
def _tn_abi(pkg, a, b, m, n, k, ldc):
    lib = pkg._native.lib()
    c = R.Guarded(m, n, ldc, DEV)
    nbytes = lib.mgcn_matmul_tn_workspace(k, m, n)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=DEV)
    rc = lib.mgcn_matmul_tn_f32(k, m, n, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.ptr(), ldc, ws.data_ptr(), nbytes,
                                _stream())
    torch.cuda.synchronize()
    return rc, c


@pytest.mark.parametrize('case', R.MATMUL_TN_CASES, ids=R.case_id)
def test_matmul_tn_f32(pkg, case):
    K, M, N = case
    cid = R.case_id(case)
    a, b = [t.to(DEV) for t in R.matmul_tn_inputs(K, M, N)]
    want, mag = R.ref_matmul_tn(a, b)
    rc, c = _tn_abi(pkg, a, b, M, N, K, N + (3 if (K + M + N) % 2 else 4))       # ldc > N, guard columns and rows
    assert rc == 0, pkg._native.lib().mgcn_last_error()
    c.check('matmul_tn_f32')
    _report('matmul_tn', cid, R.max_ratio(c.view, want, R.dot_bar(mag, K)))
    got = c.view.contiguous()
    assert torch.equal(pkg._native.matmul_tn(a, b), got)                         # the wrapper (ldc = N), and a second call: reproducible
    # strided operands: the aggregate's halves (A a column window of a [K, 2M] tensor), B with an odd row stride
    wide = torch.cat([torch.full_like(a, float('nan')), a], dim=1)
    assert torch.equal(pkg._native.matmul_tn(wide[:, M:], R.layout(b, 'oddstride')), got)


@pytest.mark.parametrize('M,N', [(209, 16), (16, 257)])
def test_matmul_tn_f32_unsupported_writes_nothing(pkg, M, N):
    K = 257
    a, b = [t.to(DEV) for t in R.matmul_tn_inputs(K, M, N)]
    rc, c = _tn_abi(pkg, a, b, M, N, K, N + 4)
    assert rc == UNSUPPORTED
    assert c.untouched()
    assert not pkg._native.matmul_tn_supported(M, N)
