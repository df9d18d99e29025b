"""csrc/train_layer.hip held to float64 at its block edges (`-m gpu`): the training epilogue (4t) forward / backward, its
split stages (4s) -- bit for bit at cuts that are multiples of 128, against float64 and rank against rank at the ragged
cuts training produces --, what the wrappers must refuse, and the split-K weight-gradient product mgcn_matmul_tn_f32. N runs around the 128-row
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
    inputs = R.train_inputs(N, O, with_bias, with_running)
    u, bias, gamma, beta, rm, rv, gy = inputs
    r64 = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy)
    r32 = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy, dtype=torch.float32)
    cpu_err = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64 if r64[k] is not None}
    du, dbias, dgamma, dbeta, drm, drv, dgy = _wide([t.to(DEV) for t in u], extra), _dev(bias), _dev(gamma), _dev(beta), _dev(rm), _dev(rv), _dev(gy)
    y, z, mean, rstd = nat.bn_tanh_train_fwd(*du, dbias, dgamma, dbeta, drm, drv, R.BN_MOMENTUM, R.BN_EPS)
    gz, gu, gg, gb = nat.bn_tanh_train_bwd(z, y, dgy, mean, rstd, dgamma)
    torch.cuda.synchronize()
    got = dict(z=z, y=y, mean=mean, rstd=rstd, rm=drm, rv=drv, gz=gz, gu=gu, ggamma=gg, gbeta=gb)
    # the bars (z: two adds, a division, an add; the rest derived_bar over floors and today's caps): dense_ref.train_bars, shared
    # with the split stages below
    for name, bar in R.train_bars(inputs, r64, cpu_err).items():
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
# (4s) at the cuts training produces: rank boundaries that are no multiples of 128
def _pieces(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


def _split_forward(nat, N, O, cuts, u, bias, gamma, beta, rm0, rv0):
    """Stages 1-3 rank by rank, the partials concatenated in rank order (what _Exchange.gather_blocks hands every rank). Checks
    the shapes of what each rank returns; returns per-rank lists z, y and the per-rank statistics (mean, rstd, rm, rv)."""
    pieces = _pieces(cuts)
    blocks = [nat.bn_blocks(b - a) for a, b in pieces]
    st1 = [nat.bn_train_stage_sum(*[t[a:b] for t in u], bias) for a, b in pieces]
    for (a, b), nb, (zz, part) in zip(pieces, blocks, st1):
        assert tuple(zz.shape) == (b - a, O) and tuple(part.shape) == (nb, O)
    sums = torch.cat([s[1] for s in st1])
    assert sums.size(0) == len(R.rank_blocks(cuts))
    st2 = [nat.bn_train_stage_center(s[0], sums, N) for s in st1]
    for nb, (mean, part) in zip(blocks, st2):
        assert tuple(mean.shape) == (O,) and tuple(part.shape) == (nb, O)
    sqs = torch.cat([c[1] for c in st2])
    ys, stats = [], []
    for (a, b), s, c in zip(pieces, st1, st2):
        m = None if rm0 is None else rm0.clone()
        v = None if rv0 is None else rv0.clone()
        yy, rs = nat.bn_train_stage_finish(s[0], sqs, N, c[0], gamma, beta, m, v, R.BN_MOMENTUM, R.BN_EPS)
        assert tuple(yy.shape) == (b - a, O) and tuple(rs.shape) == (O,)
        ys.append(yy)
        stats.append(dict(mean=c[0], rstd=rs, rm=m, rv=v))
    return [s[0] for s in st1], ys, stats


def _split_backward(nat, N, O, cuts, zs, ys, gy, stats, gamma):
    """The two backward stages rank by rank, each rank with ITS copy of the statistics; returns per-rank (gz, gu, ggamma, gbeta)."""
    pieces = _pieces(cuts)
    bw = [nat.bn_train_bwd_stage_sums(z, y, gy[a:b], st['mean'], st['rstd']) for (a, b), z, y, st in zip(pieces, zs, ys, stats)]
    for (a, b), p in zip(pieces, bw):
        assert tuple(p.shape) == (2, nat.bn_blocks(b - a), O)
    allp = torch.cat(bw, dim=1)
    outs = [nat.bn_train_bwd_stage_apply(z, y, gy[a:b], st['mean'], st['rstd'], gamma, allp[0], allp[1], N)
            for (a, b), z, y, st in zip(pieces, zs, ys, stats)]
    for (a, b), o in zip(pieces, outs):
        assert tuple(o[0].shape) == (b - a, O) and tuple(o[1].shape) == (b - a, O) and tuple(o[2].shape) == (O,) and tuple(o[3].shape) == (O,)
    return outs


def _same_bits_on_every_rank(stats, names):
    for name in names:
        for r, st in enumerate(stats):
            if stats[0][name] is None:
                assert st[name] is None
            else:
                assert torch.equal(st[name], stats[0][name]), 'rank %d: %s differs from rank 0' % (r, name)


@pytest.mark.parametrize('case', R.TRAIN_RAGGED_CASES, ids=R.ragged_id)
def test_split_stages_ragged_vs_float64(pkg, case):
    """(4s) with the ranks cut where GraphCSR.balanced_bounds cuts them (multiples of 32 or of 1, not of 128; ranks without
    rows anywhere): z is (4t)'s z bit for bit (row-local), every rank -- one without rows included -- ends with the same bits
    for mean, rstd, ggamma, gbeta and the running statistics, a rank's partials have bn_blocks(rows) rows, and all results meet
    float64 under the bars of (4t) (dense_ref.train_bars; the f32 emulation of these very blocks uses at most 0.65 of them:
    tests/test_dense_ref_host.py). They are not (4t)'s bits: the blocks differ."""
    nat = pkg._native
    N, O, with_bias, with_running, cuts = case
    cid = R.ragged_id(case)
    inputs, r64, bars = R.train_reference(N, O, with_bias, with_running)
    u, bias, gamma, beta, rm0, rv0, gy = [[v.to(DEV) for v in t] if isinstance(t, list) else _dev(t) for t in inputs]
    u = _wide(u, R.TRAIN_RAGGED_LDU_EXTRA.get((N, O, cuts), 0))
    zs, ys, stats = _split_forward(nat, N, O, cuts, u, bias, gamma, beta, rm0, rv0)
    outs = _split_backward(nat, N, O, cuts, zs, ys, gy, stats, gamma)
    _, z_unsplit, _, _ = nat.bn_tanh_train_fwd(*u, bias, gamma, beta, None, None, R.BN_MOMENTUM, R.BN_EPS)
    torch.cuda.synchronize()
    z = torch.cat(zs)
    assert torch.equal(z, z_unsplit)
    for st, o in zip(stats, outs):
        st['ggamma'], st['gbeta'] = o[2], o[3]
    _same_bits_on_every_rank(stats, ('mean', 'rstd', 'rm', 'rv', 'ggamma', 'gbeta'))
    gz, gu = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    got = dict(z=z, y=torch.cat(ys), gz=gz, gu=gu, **stats[0])
    for name, ratio in R.train_ratios(got, r64, bars).items():
        _report('ragged_' + name, cid, ratio)
    assert torch.equal(gu.cpu(), gz.cpu() / torch.full((N, O), 3.0))          # gu = gz / 3, an IEEE division
    if not with_running:
        assert 'rm' not in bars and stats[0]['rm'] is None


def test_split_stages_zero_row_ranks_first_and_last_equal_unsplit(pkg):
    """Ranks without rows at both ends (a skewed graph's balanced_bounds), the others cut at multiples of 128: the blocks are
    (4t)'s blocks, so everything is (4t)'s bit for bit -- on the empty ranks too."""
    nat = pkg._native
    N, O, cuts = R.TRAIN_SPLIT_EMPTY_ENDS
    assert cuts[0] == cuts[1] and cuts[-2] == cuts[-1] and all(c % 128 == 0 for c in cuts[:-2])
    inputs, _, _ = R.train_reference(N, O, True, True)
    u, bias, gamma, beta, rm0, rv0, gy = [[v.to(DEV) for v in t] if isinstance(t, list) else _dev(t) for t in inputs]
    rm, rv = rm0.clone(), rv0.clone()
    y, z, mean, rstd = nat.bn_tanh_train_fwd(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS)
    gz, gu, gg, gb = nat.bn_tanh_train_bwd(z, y, gy, mean, rstd, gamma)
    zs, ys, stats = _split_forward(nat, N, O, cuts, u, bias, gamma, beta, rm0, rv0)
    outs = _split_backward(nat, N, O, cuts, zs, ys, gy, stats, gamma)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(zs), z) and torch.equal(torch.cat(ys), y)
    assert torch.equal(torch.cat([o[0] for o in outs]), gz) and torch.equal(torch.cat([o[1] for o in outs]), gu)
    for st, o in zip(stats, outs):
        assert torch.equal(st['mean'], mean) and torch.equal(st['rstd'], rstd) and torch.equal(st['rm'], rm) and torch.equal(st['rv'], rv)
        assert torch.equal(o[2], gg) and torch.equal(o[3], gb)
    for i in (0, -1):                                                            # the empty ranks: [0, O] everywhere
        assert tuple(zs[i].shape) == (0, O) and tuple(ys[i].shape) == (0, O) and tuple(outs[i][0].shape) == (0, O)


@pytest.mark.parametrize('case', R.TRAIN_RAGGED_ILL_CASES, ids=R.ragged_id)
def test_split_stages_ragged_ill_conditioned_columns(pkg, case):
    """test_training_epilogue_ill_conditioned_columns on the staged outputs at ragged cuts: the statistics against float64
    statistics of the returned z (colsum_bar, ill_rstd_bar), y against float64 tanh from the returned statistics."""
    nat = pkg._native
    N, O, cuts = case
    cid = R.ragged_id(case)
    g = R.gen(R.seed_of(6, N, O))
    zin = R.ill_conditioned_z(N, O, g)
    gamma, beta = (R.pm_uniform((O,), g) * 1.5).to(DEV), R.randn_scaled((O,), g, 0.1).to(DEV)
    dz = zin.to(DEV)
    zs, ys, stats = _split_forward(nat, N, O, cuts, [dz, dz, dz], None, gamma, beta, None, None)
    torch.cuda.synchronize()
    _same_bits_on_every_rank(stats, ('mean', 'rstd'))
    z, y, mean, rstd = torch.cat(zs), torch.cat(ys), stats[0]['mean'], stats[0]['rstd']
    z64 = z.double()
    _report('ragged_ill_z', cid, R.max_ratio(z, dz.double(), 2 * U * 3 * dz.double().abs()))
    mean64 = z64.mean(0)
    rstd64 = 1 / torch.sqrt(z64.var(0, unbiased=False) + R.BN_EPS)
    _report('ragged_ill_mean', cid, R.max_ratio(mean, mean64, R.colsum_bar(z64.abs().sum(0) / N, N)))
    _report('ragged_ill_rstd', cid, R.max_ratio(rstd, rstd64, R.ill_rstd_bar(z, R.BN_EPS) * rstd64))
    t64 = (z64 - mean.double()) * rstd.double() * gamma.double() + beta.double()
    y64 = torch.tanh(t64)
    arg_bar = R.C_EPI * U * (t64.abs() + beta.double().abs())
    _report('ragged_ill_y', cid, R.max_ratio(y, y64, R.tanh_bar(y64, arg_bar)))


# ----------------------------------------------------------------------------------------------------------------
# The seam: what the wrappers of (4t) / (4s) must refuse. The kernels index z[r * O + col] (no leading dimension) and read O
# elements of every per-column vector, so a window, a short block or a short vector is a wrong-stride or out-of-bounds read.
def _seam_tensors(nat, N, O, cut, dev):
    """Valid operands of every wrapper for two ranks [0, cut), [cut, N): the forward's own outputs."""
    u, bias, gamma, beta, rm, rv, gy = [[v.to(dev) for v in t] if isinstance(t, list) else t.to(dev) for t in R.train_inputs(N, O, True, True)]
    y, z, mean, rstd = nat.bn_tanh_train_fwd(*u, bias, gamma, beta, rm.clone(), rv.clone(), R.BN_MOMENTUM, R.BN_EPS)
    zs, ys, stats = _split_forward(nat, N, O, (0, cut, N), u, bias, gamma, beta, rm, rv)
    sums = torch.cat([nat.bn_train_stage_sum(*[t[a:b] for t in u], bias)[1] for a, b in ((0, cut), (cut, N))])
    sqs = torch.cat([nat.bn_train_stage_center(zz, sums, N)[1] for zz in zs])
    allp = torch.cat([nat.bn_train_bwd_stage_sums(zs[i], ys[i], gy[a:b], mean, rstd) for i, (a, b) in enumerate(((0, cut), (cut, N)))], dim=1)
    return dict(u=u, bias=bias, gamma=gamma, beta=beta, rm=rm, rv=rv, gy=gy, y=y, z=z, mean=mean, rstd=rstd, z0=zs[0], y0=ys[0],
                gy0=gy[:cut], mean_s=stats[0]['mean'], rstd_s=stats[0]['rstd'], sums=sums, sqs=sqs, gp=allp[0], gxp=allp[1])


def _bad_forms(t):
    """(label, tensor) of a per-column vector with O - 1 and O + 1 elements."""
    return (('short', t[:-1].clone()), ('long', torch.cat([t, t[:1]])))


def _seam_calls(nat, T, N, cut):
    """(name, thunk) of every call that must raise NativeError. Blocks: a column window of a NaN-filled wider tensor, or one
    row short; vectors: O - 1 / O + 1 elements; partials: another width."""
    mom, eps = R.BN_MOMENTUM, R.BN_EPS
    win = lambda t: R.layout(t, 'window')
    narrow = lambda p: p[:, :-1].contiguous()
    fwd = dict(bias=T['bias'], gamma=T['gamma'], beta=T['beta'], running_mean=T['rm'], running_var=T['rv'])
    for k in fwd:
        for label, bad in _bad_forms(fwd[k]):
            a = dict(fwd, **{k: bad})
            yield 'bn_tanh_train_fwd %s %s' % (k, label), (lambda a=a: nat.bn_tanh_train_fwd(
                *T['u'], a['bias'], a['gamma'], a['beta'], a['running_mean'], a['running_var'], mom, eps))
    for label, bad in _bad_forms(T['bias']):
        yield 'bn_train_stage_sum bias %s' % label, (lambda bad=bad: nat.bn_train_stage_sum(*[t[:cut] for t in T['u']], bad))

    # the wrappers that take z / y: (name, function of a dict of named operands, the valid operands)
    full = dict(z=T['z'], y=T['y'], gy=T['gy'], mean=T['mean'], rstd=T['rstd'], gamma=T['gamma'])
    rank = dict(z=T['z0'], y=T['y0'], gy=T['gy0'], mean=T['mean_s'], rstd=T['rstd_s'], gamma=T['gamma'], beta=T['beta'],
                running_mean=T['rm'], running_var=T['rv'], sums=T['sums'], sqs=T['sqs'], gp=T['gp'], gxp=T['gxp'])
    table = [
        ('bn_tanh_train_bwd', lambda a: nat.bn_tanh_train_bwd(a['z'], a['y'], a['gy'], a['mean'], a['rstd'], a['gamma']), full,
         ('z', 'y'), ('y', 'gy'), ('mean', 'rstd', 'gamma'), ()),
        ('bn_train_stage_center', lambda a: nat.bn_train_stage_center(a['z'], a['sums'], N), rank, ('z',), (), (), ('sums',)),
        ('bn_train_stage_finish', lambda a: nat.bn_train_stage_finish(a['z'], a['sqs'], N, a['mean'], a['gamma'], a['beta'], a['running_mean'],
                                                                      a['running_var'], mom, eps), rank,
         ('z',), (), ('mean', 'gamma', 'beta', 'running_mean', 'running_var'), ('sqs',)),
        ('bn_train_bwd_stage_sums', lambda a: nat.bn_train_bwd_stage_sums(a['z'], a['y'], a['gy'], a['mean'], a['rstd']), rank,
         ('z', 'y'), ('y', 'gy'), ('mean', 'rstd'), ()),
        ('bn_train_bwd_stage_apply', lambda a: nat.bn_train_bwd_stage_apply(a['z'], a['y'], a['gy'], a['mean'], a['rstd'], a['gamma'], a['gp'],
                                                                            a['gxp'], N), rank,
         ('z', 'y'), ('y', 'gy'), ('mean', 'rstd', 'gamma'), ('gp', 'gxp')),
    ]
    for name, fn, ok, windows, short_rows, vectors, partials in table:
        for k in windows:
            yield '%s %s window' % (name, k), (lambda fn=fn, a=dict(ok, **{k: win(ok[k])}): fn(a))
        for k in short_rows:
            yield '%s %s one row short' % (name, k), (lambda fn=fn, a=dict(ok, **{k: ok[k][:-1]}): fn(a))
        for k in vectors:
            for label, bad in _bad_forms(ok[k]):
                yield '%s %s %s' % (name, k, label), (lambda fn=fn, a=dict(ok, **{k: bad}): fn(a))
        for k in partials:
            yield '%s %s narrower' % (name, k), (lambda fn=fn, a=dict(ok, **{k: narrow(ok[k])}): fn(a))


def test_training_wrappers_refuse_what_the_kernels_cannot_index(pkg):
    """Every wrapper of (4t) / (4s) refuses, before any launch, a z or y that is a column window of a wider tensor (the
    kernels would read it at row stride O), a y / gy with a row missing, a per-column vector of O - 1 or O + 1 elements and
    partials of another width; the running statistics passed to a refused call keep their bits. gy alone is taken in any
    layout (autograd hands it over that way) and gives the bits of the contiguous call."""
    nat = pkg._native
    N, O, cut = 130, 6, 97
    T = _seam_tensors(nat, N, O, cut, DEV)
    torch.cuda.synchronize()
    rm0, rv0 = T['rm'].clone(), T['rv'].clone()
    accepted = []
    count = 0
    for name, call in _seam_calls(nat, T, N, cut):
        count += 1
        try:
            call()
            accepted.append(name)
        except nat.NativeError:
            pass
    torch.cuda.synchronize()
    print('SEAM %d calls, accepted: %s' % (count, accepted))
    assert not accepted, accepted
    assert count >= 56
    assert torch.equal(T['rm'], rm0) and torch.equal(T['rv'], rv0)
    # gy in any layout: the bits of the contiguous call
    want = nat.bn_tanh_train_bwd(T['z'], T['y'], T['gy'], T['mean'], T['rstd'], T['gamma'])
    want_s = nat.bn_train_bwd_stage_sums(T['z0'], T['y0'], T['gy0'], T['mean_s'], T['rstd_s'])
    want_a = nat.bn_train_bwd_stage_apply(T['z0'], T['y0'], T['gy0'], T['mean_s'], T['rstd_s'], T['gamma'], T['gp'], T['gxp'], N)
    forms = [lambda t, k=k: R.layout(t, k) for k in R.LAYOUTS] + [lambda t: t.t().contiguous().t()]
    for form in forms:
        gy, gy0 = form(T['gy']), form(T['gy0'])
        got = nat.bn_tanh_train_bwd(T['z'], T['y'], gy, T['mean'], T['rstd'], T['gamma'])
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(nat.bn_train_bwd_stage_sums(T['z0'], T['y0'], gy0, T['mean_s'], T['rstd_s']), want_s)
        got_a = nat.bn_train_bwd_stage_apply(T['z0'], T['y0'], gy0, T['mean_s'], T['rstd_s'], T['gamma'], T['gp'], T['gxp'], N)
        assert all(torch.equal(a, b) for a, b in zip(got_a, want_a))


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
