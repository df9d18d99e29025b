"""csrc/dense.hip held to float64 at its tile edges (`-m gpu`): scoring values (score_fwd / score_target / score_rank /
score_topk), mgcn_matmul_f32, mgcn_dense_bn_tanh_fwd, mgcn_score_bce_fwd, filter_mask / label_rows. References, grids,
operand layouts, guard buffers and bars come from tests/dense_ref.py, whose constants tests/test_dense_ref_host.py
measures on the CPU. One parametrised case per shape; every case prints `RATIO family id worst-error / bar`
(pytest -s) before it asserts. Nothing is skipped or filtered by a margin: rank counts and top-k lists are compared
with a recount over a score block that was itself checked against float64."""
import ctypes

import pytest
import torch

from . import dense_ref as R
from .test_gpu_topk import expected as topk_expected

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
UNSUPPORTED = 3


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _report(family, cid, ratio):
    print('RATIO %s %s %.4f' % (family, cid, ratio))
    assert ratio <= 1.0, '%s %s: worst |got - float64| is %.3f x its bar' % (family, cid, ratio)


# ----------------------------------------------------------------------------------------------------------------
# scoring
def _check_scoring(pkg, x, ent, bias, label, cid, row0=0):
    """x [B, dim], ent [n, dim], bias [n] on the device, in whatever layout: the four entry points of (5) / (7)."""
    nat, lib = pkg._native, pkg._native.lib()
    B, dim = x.shape
    n = ent.shape[0]
    p64, z64, mag = R.ref_scores(x, ent, bias)
    logit_bar = R.split_logit_bar(mag) if label == R.SPLIT else R.dot_bar(mag, dim)
    bar = R.sigmoid_bar(p64, logit_bar)

    # (a) the score block through the C ABI with lds > n_local and guard rows
    out = R.Guarded(B, n, n + (3 if (B + n) % 2 else 4), DEV)
    rc = lib.mgcn_score_fwd(B, n, dim, x.data_ptr(), x.stride(0), ent.data_ptr(), ent.stride(0), bias.data_ptr(), out.ptr(), out.ld,
                            _stream())
    assert rc == 0, lib.mgcn_last_error()
    torch.cuda.synchronize()
    out.check('score_fwd')
    score = out.view.contiguous()
    _report('score_fwd', cid, R.max_ratio(score, p64, bar))
    assert torch.equal(nat.score_fwd(x, ent, bias), score)            # the wrapper's own (lds = n_local) block

    # (b) targets: ids below, inside and above the shard; the ones outside must leave `out` untouched
    g = R.gen(R.seed_of(7, B, n, dim))
    lo = max(row0 - 3, 0)
    obj = torch.randint(lo, row0 + n + 3, (B,), generator=g).to(DEV)
    obj[0] = row0 + n - 1
    inside = (obj >= row0) & (obj < row0 + n)
    tg = R.Guarded(1, B, B + 5, DEV)
    nat.score_target(x, ent, bias, obj, ent_row0=row0, out=tg.view[0])
    torch.cuda.synchronize()
    tg.check('score_target')
    assert bool((tg.raw[0, :B][~inside] == R.GUARD_F32).all()), 'score_target wrote a query whose target is outside the shard'
    rows = torch.arange(B, device=DEV)[inside]
    loc = (obj - row0)[inside]
    got_t = tg.view[0][inside]
    _report('score_target', cid, R.max_ratio(got_t, p64[rows, loc], bar[rows, loc]))
    assert torch.equal(got_t, score[rows, loc])

    # (c) filtered counts against a recount over the checked block; both filter forms; ldm wider than the row
    # queries whose target lives elsewhere: a value that ties. (At B = 1 the clone keeps the column's stride n: the
    # wrapper used to refuse that one-element tensor as "not contiguous".)
    target = score[:, 0].clone()
    target[inside] = got_t
    hit = (torch.rand((B, n), generator=g) < 0.1).to(DEV)
    words = (n + 31) // 32
    mask = R.pack_bits(hit, words + 1)
    ids = torch.arange(n, device=DEV).unsqueeze(0)
    ob = (obj - row0).unsqueeze(1)
    keep = ~hit & (ids != ob)
    tt = target.unsqueeze(1)
    want = torch.stack([((score > tt) & keep).sum(1), ((score == tt) & keep & (ids < ob)).sum(1), ((score == tt) & keep).sum(1)], 1)
    for kw in (dict(mask=mask), dict(label=hit.float())):
        cnt = R.Guarded(B, 3, 3, DEV, torch.int64)
        cnt.view.zero_()
        nat.score_rank(x, ent, bias, obj, target, ent_row0=row0, counts=cnt.view, **kw)
        torch.cuda.synchronize()
        cnt.check('score_rank')
        assert torch.equal(cnt.view, want), ('score_rank', cid, list(kw))

    # (d) top-k over the same block
    k = 5
    got_s, got_i = nat.score_topk(x, ent, bias, k, mask=mask, ent_row0=row0)
    want_s, want_i = topk_expected(score, k, hit, row0)
    assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s), ('score_topk', cid)


@pytest.mark.parametrize('case', R.SCORE_CASES, ids=R.case_id)
def test_scoring_values(pkg, case):
    B, n, dim, label = case
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim))]
    _check_scoring(pkg, x, ent, bias, label, R.case_id(case))


@pytest.mark.parametrize('case', R.SCORE_RANDN_CASES, ids=R.case_id)
def test_scoring_values_randn(pkg, case):
    """The distributions of the existing tests: saturated sigmoids (scale 4) and small products (scale 0.05)."""
    B, n, dim, scale, label = case
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim), scale)]
    _check_scoring(pkg, x, ent, bias, label, R.case_id(case))


@pytest.mark.parametrize('kind', R.LAYOUTS[1:])
@pytest.mark.parametrize('case', R.SCORE_LAYOUT_CASES, ids=R.case_id)
def test_scoring_operand_layouts(pkg, case, kind):
    """x and ent as windows of wider tensors: aligned (same path), base off by one float, odd row stride (guarded path)."""
    B, n, dim, label = case
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim))]
    if kind != 'window':
        label = R.G_NT
    _check_scoring(pkg, R.layout(x, kind), R.layout(ent, kind), bias, label, R.case_id(case) + '-' + kind)


@pytest.mark.parametrize('case', R.SCORE_SHARD_CASES, ids=R.case_id)
def test_scoring_entity_shard_row0_37(pkg, case):
    B, n, dim, label = case
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim, 37))]
    _check_scoring(pkg, x, ent, bias, label, R.case_id(case) + '-row0', row0=37)


# ----------------------------------------------------------------------------------------------------------------
# mgcn_matmul_f32
def _matmul_abi(pkg, a, b, cid):
    lib = pkg._native.lib()
    m, k = a.shape
    n = b.shape[1]
    want, mag = R.ref_matmul(a, b)
    c = R.Guarded(m, n, n + (3 if (m + k + n) % 2 else 4), DEV)
    rc = lib.mgcn_matmul_f32(m, k, n, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.ptr(), c.ld, _stream())
    assert rc == 0, lib.mgcn_last_error()
    torch.cuda.synchronize()
    c.check('matmul_f32')
    _report('matmul_f32', cid, R.max_ratio(c.view, want, R.dot_bar(mag, k)))
    return c.view.contiguous()


@pytest.mark.parametrize('case', R.MATMUL_CASES, ids=R.case_id)
def test_matmul_f32(pkg, case):
    m, k, n, _ = case
    a, b = [t.to(DEV) for t in R.matmul_inputs(m, k, n)]
    got = _matmul_abi(pkg, a, b, R.case_id(case))
    assert torch.equal(pkg._native.matmul(a, b), got)                  # the wrapper (ldc = n): same values


@pytest.mark.parametrize('kind', R.LAYOUTS[1:])
@pytest.mark.parametrize('case', R.MATMUL_LAYOUT_CASES, ids=R.case_id)
def test_matmul_f32_operand_layouts(pkg, case, kind):
    m, k, n, _ = case
    a, b = [t.to(DEV) for t in R.matmul_inputs(m, k, n)]
    _matmul_abi(pkg, R.layout(a, kind), R.layout(b, kind), R.case_id(case) + '-' + kind)


def test_fused_layer_relation_projection_equals_small_matmul(pkg, oracle):
    """The header: rel_out of the fused launch has the arithmetic of mgcn_matmul_f32's small-matrix kernel, bit for bit --
    here on a synthetic fused layer shape (D = 100 -> O = 200, 14 relation rows), and both against float64."""
    from .test_gpu_round3 import _fused, _graph, _layer
    N, Rn, E, D, O = 700, 7, 4000, 100, 200
    ei, ea, csr = _graph(pkg, oracle, N, Rn, E, seed=5, zipf=0.0)
    conv = _layer(pkg, D, O, Rn, seed=9)
    g = R.gen(11)
    x, rel = R.pm_uniform((N, D), g).to(DEV), R.pm_uniform((2 * Rn, D), g).to(DEV)
    table = R.pm_uniform((2 * E, D), g).to(DEV)
    _, rel_out = _fused(pkg, conv, csr, x, rel, table)
    small = pkg._native.matmul(rel, conv.rels_weight.detach().contiguous())
    assert torch.equal(rel_out, small)
    want, mag = R.ref_matmul(rel, conv.rels_weight.detach())
    _report('rel_out', 'fused-100-200', R.max_ratio(rel_out, want, R.dot_bar(mag, D)))


# ----------------------------------------------------------------------------------------------------------------
# mgcn_dense_bn_tanh_fwd
@pytest.mark.parametrize('case', R.BN_TANH_CASES, ids=R.case_id)
def test_dense_bn_tanh_fwd(pkg, case):
    N, D, O, with_bias, lda_extra, ldo_extra, _ = case
    a, w, bias, mean, var, gamma, beta = [None if t is None else t.to(DEV) for t in R.bn_tanh_inputs(N, D, O, with_bias)]
    want, bar = R.ref_dense_bn_tanh(a, w, bias, mean, var, gamma, beta, R.BN_EPS)
    wide = torch.full((N, 3 * D + lda_extra), float('nan'), device=DEV)
    wide[:, :3 * D] = a
    out = R.Guarded(N, O, O + ldo_extra, DEV)
    pkg._native.dense_bn_tanh_fwd(wide[:, :3 * D], w, bias, mean, var, gamma, beta, R.BN_EPS, out.view)
    torch.cuda.synchronize()
    out.check('dense_bn_tanh_fwd')
    _report('dense_bn_tanh', R.case_id(case), R.max_ratio(out.view, want, bar))


def test_dense_bn_tanh_refuses_a_strided_weight(pkg):
    """The wrapper takes w_cat contiguous only (the C entry point has no ldw): a column window is refused, not copied."""
    a, w, bias, mean, var, gamma, beta = [None if t is None else t.to(DEV) for t in R.bn_tanh_inputs(33, 4, 32, True)]
    out = torch.empty((33, 32), device=DEV)
    with pytest.raises(pkg._native.NativeError):
        pkg._native.dense_bn_tanh_fwd(a, R.layout(w, 'window'), bias, mean, var, gamma, beta, R.BN_EPS, out)


# ----------------------------------------------------------------------------------------------------------------
# mgcn_score_bce_fwd
def _bce_call(pkg, x, ent, bias, mask, hot, cold, inv, B, n, dim):
    lib = pkg._native.lib()
    np_ = int(lib.mgcn_score_bce_partials(B, n))
    parts = R.Guarded(1, np_, np_ + 8, DEV)
    G = R.Guarded(n, B, B + 4, DEV)
    rc = lib.mgcn_score_bce_fwd(B, n, dim, x.data_ptr(), x.stride(0), ent.data_ptr(), ent.stride(0), bias.data_ptr(), mask.data_ptr(),
                                mask.size(1), ctypes.c_float(hot), ctypes.c_float(cold), ctypes.c_float(inv), G.ptr(), G.ld, parts.ptr(),
                                _stream())
    torch.cuda.synchronize()
    return rc, parts, G


def _check_bce(pkg, B, n, dim, cid, smooth, logit_scale=None, num_entities=None):
    nat = pkg._native
    x, ent, bias, hit = R.bce_inputs(B, n, dim, logit_scale)
    x, ent, bias, hit = x.to(DEV), ent.to(DEV), bias.to(DEV), hit.to(DEV)
    total = n if num_entities is None else num_entities
    hot, cold = nat.smoothed_targets(smooth, total)
    inv = 1.0 / (float(B) * float(total))
    mask = R.pack_bits(hit, (n + 31) // 32 + 2)                        # ldm wider than the row
    rc, parts, G = _bce_call(pkg, x, ent, bias, mask, hot, cold, inv, B, n, dim)
    assert rc == 0, nat.lib().mgcn_last_error()
    parts.check('loss_partial')
    G.check('grad_logit')
    assert bool(torch.isfinite(parts.view).all()), 'a loss partial was never written'
    z64, mag = R.ref_logits(x, ent, bias)
    y = torch.where(hit, torch.tensor(hot, device=DEV), torch.tensor(cold, device=DEV))
    loss64, g64, p64 = R.ref_bce(z64, y, inv)
    loss_s, g_s, p_s = R.ref_bce(z64, y, inv, saturate_f32=True)       # == the line above where f32 p does not saturate
    sat = p_s != p64
    loss = float(parts.view.double().sum()) * inv
    loss_bar = R.bce_loss_bar(float(loss_s), R.emul_bce_loss_f32(z64, y, inv))
    print('RATIO bce_loss %s %.4f (bar %.3g relative)' % (cid, abs(loss - float(loss_s)) / loss_bar, loss_bar / abs(float(loss_s))))
    assert abs(loss - float(loss_s)) <= loss_bar, (cid, loss, float(loss_s), float(loss64))
    got = G.view.t()                                                  # [B, n]
    logit_bar = R.dot_bar(mag, dim)
    bar = R.bce_grad_bar(g64, p64, y, logit_bar, inv)
    # Saturated entries (torch-CPU f32 p exactly 0 or 1) are held to torch's f32 value alone, all others to float64:
    # g_s is that reference. Only at the edge of saturation -- 1 - p64 within [u / 4, 4 u], widened by the logit's own bar,
    # where an f32 sigmoid may round p to 1 or to 1 - u depending on its last bit -- either side of the jump is taken:
    # float64's (p - y) inv_count, or 0, the formula's value at p == 1.
    q64 = torch.sigmoid(-z64)                                         # 1 - p64 without cancellation
    edge = (q64 >= R.U / 4 * torch.exp(-logit_bar)) & (q64 <= 4 * R.U * torch.exp(logit_bar))
    err = (got.double() - g_s).abs() / bar
    either = torch.minimum((got.double() - g64).abs(), got.double().abs()) / bar
    ratio = float(torch.where(edge, either, err).max())
    print('bce_grad %s: %d saturated entries, %d at the edge of saturation' % (cid, int(sat.sum()), int(edge.sum())))
    assert bool(torch.isfinite(got).all())
    _report('bce_grad', cid, ratio)
    return int(sat.sum())


@pytest.mark.parametrize('case', R.BCE_CASES, ids=R.case_id)
def test_score_bce_fwd(pkg, case):
    B, n, dim, smooth, _ = case
    _check_bce(pkg, B, n, dim, R.case_id(case), smooth=smooth)


@pytest.mark.parametrize('scale', [40.0, 120.0])
@pytest.mark.parametrize('case', [(68, 33, 36), (212, 1000, 200)], ids=R.case_id)
def test_score_bce_fwd_saturated_logits(pkg, case, scale):
    """Logits up to +-40 (f32 p reaches exactly 1) and +-120 (log clamped at -100, p (1 - p) under the 1e-12 floor)."""
    B, n, dim = case
    for smooth in (0.0, 0.1):
        nsat = _check_bce(pkg, B, n, dim, R.case_id(case) + '-z%d-s%g' % (scale, smooth), smooth, logit_scale=scale)
        assert nsat > 0


def test_score_bce_fwd_row_shard(pkg):
    """A row shard of a larger table: num_entities > n in the mean's count and in the smoothed targets."""
    _check_bce(pkg, 132, 1000, 36, '132-1000-36-of-4099', smooth=0.1, num_entities=4099)


@pytest.mark.parametrize('B,dim', [(6, 36), (36, 6)])
def test_score_bce_fwd_unsupported_writes_nothing(pkg, B, dim):
    n = 33
    x, ent, bias, hit = [t.to(DEV) for t in R.bce_inputs(B, n, dim)]
    rc, parts, G = _bce_call(pkg, x, ent, bias, R.pack_bits(hit), 1.0, 0.0, 1.0 / (B * n), B, n, dim)
    assert rc == UNSUPPORTED
    assert parts.untouched() and G.untouched()


# ----------------------------------------------------------------------------------------------------------------
# filter_mask / label_rows
TAIL_COUNTS = [0, 1, 63, 64, 65, 257, 1000]


def _index(num_entities):
    """Keys 10, 20, ..., 70 holding 0, 1, 63, 64, 65, 257 and 1000 distinct tails each."""
    g = R.gen(99)
    keys = torch.arange(1, len(TAIL_COUNTS) + 1, dtype=torch.int64) * 10
    ptr, tails = [0], []
    for c in TAIL_COUNTS:
        tails.append(torch.sort(torch.randperm(num_entities, generator=g)[:c])[0].to(torch.int32))
        ptr.append(ptr[-1] + c)
    return keys, torch.tensor(ptr, dtype=torch.int64), torch.cat(tails)


QKEYS = [70, 60, 5, 25, 10, 99, 50, 20, 40, 30]     # present keys, one absent between keys, below the first, above the last


@pytest.mark.parametrize('row0,n_local', [(0, 1), (0, 33), (37, 1000), (64, 31)])
@pytest.mark.parametrize('batch', [1, 3, 4, 5])
def test_filter_mask_and_label_rows(pkg, batch, row0, n_local):
    nat = pkg._native
    keys, ptr, tails = _index(1100)
    hits = []
    for start in range(0, len(QKEYS), batch):                          # every query key, `batch` at a time
        qkey = torch.tensor((QKEYS + QKEYS)[start:start + batch], dtype=torch.int64)
        hit = R.ref_filter(qkey, keys, ptr, tails, row0, n_local)
        hits.append(int(hit.sum()))
        dq, dk, dp, dt = qkey.to(DEV), keys.to(DEV), ptr.to(DEV), tails.to(DEV)
        words = (n_local + 31) // 32
        m = R.Guarded(batch, words + 2, words + 2, DEV, torch.int32)   # the whole ldm row is zeroed by contract
        nat.filter_mask(dq, dk, dp, dt, n_local, ent_row0=row0, out=m.view)
        torch.cuda.synchronize()
        m.check('filter_mask')                                         # rows past `batch` untouched
        assert torch.equal(m.view.cpu(), R.pack_bits(hit, words + 2))
        lab = R.Guarded(batch, n_local, n_local + 3, DEV)
        nat.label_rows(dq, dk, dp, dt, n_local, lbl_smooth=0.1, num_entities=1100, ent_row0=row0, out=lab.view)
        torch.cuda.synchronize()
        lab.check('label_rows')
        hot, cold = nat.smoothed_targets(0.1, 1100)
        want = torch.where(hit, torch.tensor(hot), torch.tensor(cold))
        assert torch.equal(lab.view.cpu(), want)
    assert n_local < 1000 or max(hits) > 256                           # the 1000-tail key took several trips of the stride
