"""Host-side checks of tests/dense_ref.py (no GPU): the grids keep every kernel path, the float64 references agree with
stock torch, and the error bars hold -- with the margin they claim -- for a float32 emulation of each operation on the
grids' own inputs. This is where the constants of dense_ref.py are measured: every test prints its figure
(`pytest -s`) and fails when the figure comes within a factor 2 of the constant derived from it."""
import pytest
import torch
import torch.nn.functional as F

from . import dense_ref as R

U = R.U


def test_every_path_label_is_covered():
    """A later edit of the grids cannot silently drop a kernel instantiation."""
    required = [
        'SIGMOID:split', 'TARGET:split', 'RANK:split',
        'SIGMOID:tile/guarded/NT-operand', 'TARGET:tile/guarded/NT-operand', 'RANK:tile/guarded/NT-operand',
        'SIGMOID:tile/fast/NT=2/NT-operand', 'SIGMOID:tile/fast/NT=4/NT-operand', 'SIGMOID:tile/fast/NT=8/NT-operand',
        'SIGMOID:tile/fast/NT=13/NT-operand',
        'TARGET:tile/fast/NT=2/NT-operand', 'TARGET:tile/fast/NT=4/NT-operand', 'TARGET:tile/fast/NT=8/NT-operand',
        'TARGET:tile/fast/NT=13/NT-operand',
        'RANK:tile/fast/NT=2/NT-operand', 'RANK:tile/fast/NT=4/NT-operand', 'RANK:tile/fast/NT=8/NT-operand',
        'RANK:tile/fast/NT=13/NT-operand',
        'tile/fast/NT=2/NT-operand/BCE', 'tile/fast/NT=4/NT-operand/BCE', 'tile/fast/NT=8/NT-operand/BCE',
        'tile/fast/NT=13/NT-operand/BCE', 'tile/fast/NT=8/strips128/NT-operand/BCE', 'tile/fast/NT=13/strips208/NT-operand/BCE',
        'tile/fast/NT=2/NN/dma/NONE', 'tile/fast/NT=4/NN/dma/NONE', 'tile/fast/NT=8/NN/dma/NONE', 'tile/fast/NT=13/NN/dma/NONE',
        'tile/fast/NT=2/NN/dma/BN_TANH', 'tile/fast/NT=4/NN/dma/BN_TANH', 'tile/fast/NT=8/NN/dma/BN_TANH',
        'tile/fast/NT=13/NN/dma/BN_TANH',
        'tile/guarded/NN', 'tile/guarded/NN/BN_TANH', 'small_matmul',
    ]
    have = R.all_labels()
    missing = [l for l in required if l not in have]
    assert not missing, missing
    # the three ways out of the small-matrix kernel, each alone
    tile = [c for c in R.MATMUL_CASES if c[3] != R.SMALL]
    assert any(m == 1025 and k <= 2048 and n <= 4096 for m, k, n, _ in tile)
    assert any(m <= 1024 and k == 2052 and n <= 4096 for m, k, n, _ in tile)
    assert any(m <= 1024 and k <= 2048 and n == 4100 for m, k, n, _ in tile)
    assert all(m <= 1024 and k <= 2048 and n <= 4096 for m, k, n, l in R.MATMUL_CASES if l == R.SMALL)


AXES = [
    ('score', R.SCORE_CASES, [(0, [1, 3, 4, 15, 16, 17, 63, 64, 65, 128, 209, 333]), (1, [1, 15, 16, 17, 31, 32, 33, 255, 257, 4099]),
                              (2, [4, 8, 28, 32, 36, 60, 64, 68, 100, 200, 348, 352, 356, 384, 512, 6, 35, 198, 353])]),
    ('matmul', R.MATMUL_CASES, [(0, [1, 31, 32, 33, 1024, 1025, 5003]), (1, [1, 3, 4, 15, 16, 17, 100, 2048, 2052]),
                                (2, [1, 4, 32, 36, 64, 68, 128, 132, 208, 212, 256, 416, 1028, 1040, 4100])]),
    ('bn_tanh', R.BN_TANH_CASES, [(0, [1, 33, 97, 5003]), (1, [4, 5, 12, 20, 100, 172]),
                                  (2, [4, 18, 32, 36, 64, 128, 132, 200, 208, 212, 256, 416])]),
    ('train', R.TRAIN_CASES, [(0, [2, 127, 128, 129, 5003]), (1, [1, 3, 200, 256, 257, 300, 513])]),
    ('matmul_tn', R.MATMUL_TN_CASES, [(0, [1, 3, 4, 5, 255, 256, 257, 1023, 65537, 70001]), (1, [1, 15, 16, 17, 100, 208]),
                                      (2, [1, 16, 127, 128, 129, 200, 256])]),
    ('bce', R.BCE_CASES, [(0, [4, 32, 36, 64, 68, 128, 132, 208, 212, 256, 416]), (1, [1, 31, 33, 1000, 4099]), (2, [4, 36, 200])]),
]


@pytest.mark.parametrize('name,cases,axes', AXES, ids=[a[0] for a in AXES])
def test_every_axis_value_occurs_twice(name, cases, axes):
    """Not the full product, but every value of each axis at least twice, against two different values of the others."""
    for ax, values in axes:
        for v in values:
            others = {tuple(c[i] for i in range(len(axes)) if i != ax) for c in cases if c[ax] == v}
            assert len(others) >= 2 or (len(axes) == 1), (name, ax, v, others)
    if name == 'score':
        assert (1, 1, 4) in [c[:3] for c in cases]


def test_references_agree_with_stock_torch():
    """The references are checked against something that is not themselves, to 1e-12, on the grids' small cases."""
    for B, n, d, _ in [c for c in R.SCORE_CASES if c[0] * c[1] <= 20000]:
        x, e, b = R.score_inputs(B, n, d, R.seed_of(B, n, d))
        p, z, mag = R.ref_scores(x, e, b)
        want = torch.sigmoid(torch.einsum('bk,nk->bn', x.double(), e.double()) + b.double()[None, :])
        assert float((p - want).abs().max()) <= 1e-12
        assert bool((mag >= z.abs() - 1e-12).all())
    for N, D, O, wb, _, _, _ in [c for c in R.BN_TANH_CASES if c[0] <= 97]:
        a, w, bias, mean, var, gamma, beta = R.bn_tanh_inputs(N, D, O, wb)
        y, bar = R.ref_dense_bn_tanh(a, w, bias, mean, var, gamma, beta, R.BN_EPS)
        pre = torch.einsum('nk,ko->no', a.double(), w.double()) / 3 + (bias.double() if wb else 0)
        want = torch.tanh(F.batch_norm(pre, mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, R.BN_EPS))
        assert float((y - want).abs().max()) <= 1e-12
        assert bool((bar > 0).all())
    for K, M, N in [c for c in R.MATMUL_TN_CASES if c[0] <= 1023]:
        a, b = R.matmul_tn_inputs(K, M, N)
        c, mag = R.ref_matmul_tn(a, b)
        assert float((c - torch.einsum('km,kn->mn', a.double(), b.double())).abs().max()) <= 1e-12
    # BCE against BCELoss and its autograd in float64 (moderate logits: no clamp is active in either)
    x, e, b, hit = R.bce_inputs(36, 33, 4)
    z, _ = R.ref_logits(x, e, b)
    zz = z.clone().requires_grad_(True)
    y = torch.where(hit, torch.tensor(0.9), torch.tensor(0.01)).double()
    loss = torch.nn.BCELoss()(torch.sigmoid(zz), y)
    loss.backward()
    l2, g2, _ = R.ref_bce(z, y, 1.0 / z.numel())
    assert abs(float(loss.detach()) - float(l2)) <= 1e-12 and float((zz.grad - g2).abs().max()) <= 1e-12
    # saturated logits: the clamps are those of torch (a loss term is 100, not inf)
    l3, g3, _ = R.ref_bce(torch.tensor([[-800.0, 800.0]], dtype=torch.float64), torch.tensor([[1.0, 0.0]], dtype=torch.float64), 0.5)
    want3 = torch.nn.BCELoss()(torch.sigmoid(torch.tensor([[-800.0, 800.0]], dtype=torch.float64)), torch.tensor([[1.0, 0.0]], dtype=torch.float64))
    assert abs(float(l3) - float(want3)) <= 1e-9 and bool(torch.isfinite(g3).all())
    # the training epilogue: autograd against the closed form
    u, bias, gamma, beta, rm, rv, gy = R.train_inputs(129, 3, True, True)
    r = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy)
    z = ((u[0].double() + u[1].double() + u[2].double()) / 3 + bias.double())
    mean, var = z.mean(0), z.var(0, unbiased=False)
    xh = (z - mean) / torch.sqrt(var + R.BN_EPS)
    yy = torch.tanh(xh * gamma.double() + beta.double())
    gp = gy.double() * (1 - yy * yy)
    gz = gamma.double() / torch.sqrt(var + R.BN_EPS) * (gp - gp.mean(0) - xh * (gp * xh).mean(0))
    assert float((r['y'] - yy).abs().max()) <= 1e-12 and float((r['gz'] - gz).abs().max()) <= 1e-12
    assert float((r['ggamma'] - (gp * xh).sum(0)).abs().max()) <= 1e-12 and float((r['gbeta'] - gp.sum(0)).abs().max()) <= 1e-12
    assert float((r['rv'] - (0.9 * rv.double() + 0.1 * z.var(0, unbiased=True))).abs().max()) <= 1e-12
    # filter bits
    keys, ptr, tails = torch.tensor([3, 9]), torch.tensor([0, 2, 5]), torch.tensor([1, 40, 0, 37, 41], dtype=torch.int32)
    hit = R.ref_filter(torch.tensor([9, 4, 3]), keys, ptr, tails, 37, 5)
    assert hit.tolist() == [[True, False, False, False, True], [False] * 5, [False, False, False, True, False]]
    assert R.pack_bits(hit).tolist() == [[17], [0], [8]]
    assert R.pack_bits(torch.ones(1, 32, dtype=torch.bool)).tolist() == [[-1]]


def _sub(t, rows, cols=None):
    """A spread of at most `rows` rows (and `cols` columns): first, last and evenly spaced ones."""
    def pick(n, m):
        return torch.unique(torch.linspace(0, n - 1, min(n, m)).round().long())
    t = t[pick(t.shape[0], rows)]
    return t if cols is None else t[:, pick(t.shape[1], cols)]


def _dot_operands():
    """(name, K, A [m, K], B [K, n]) of every grid with a dot product, cut down to a spread of rows and columns."""
    for B, n, d, l in R.SCORE_CASES:
        x, e, _ = R.score_inputs(B, n, d, R.seed_of(B, n, d))
        yield 'score' + R.case_id((B, n, d)), d, _sub(e, 24), _sub(x, 24).t().contiguous(), l
    for m, k, n, l in R.MATMUL_CASES:
        a, b = R.matmul_inputs(m, k, n)
        yield 'matmul' + R.case_id((m, k, n)), k, _sub(a, 16), _sub(b.t().contiguous(), 32).t().contiguous(), l
    for k, m, n in R.MATMUL_TN_CASES:
        a, b = R.matmul_tn_inputs(k, m, n)
        yield 'matmul_tn' + R.case_id((k, m, n)), k, _sub(a.t().contiguous(), 8), _sub(b.t().contiguous(), 8).t().contiguous(), 'tn'
    for N, D, O, wb, _, _, l in R.BN_TANH_CASES:
        a, w = R.bn_tanh_inputs(N, D, O, wb)[:2]
        yield 'bn_tanh' + R.case_id((N, D, O)), 3 * D, _sub(a, 16), _sub(w.t().contiguous(), 32).t().contiguous(), l


def test_dot_product_bar_holds_for_a_sequential_f32_chain():
    """c of dense_ref.dot_bar: a sequential f32 chain on the grids' own inputs, ratio |err| / (u mag) per case."""
    worst, worst_split, where = 0.0, 0.0, None
    for name, k, a, b, label in _dot_operands():
        got = R.emul_dot_f32(a, b)
        want, mag = R.ref_matmul(a, b)
        ratio = float(((got.double() - want).abs() / (U * mag)).max())
        assert ratio <= min(k + 2.0, R.C_DOT), (name, ratio)
        if ratio > worst:
            worst, where = ratio, name
        if label == R.SPLIT:     # the split kernels' contract 4 u mag + 2e-7 (a bf16-split chain is not emulated here: an f32 chain's figure)
            worst_split = max(worst_split, float(((got.double() - want).abs() / R.split_logit_bar(mag)).max()))
    print('sequential f32 chain: worst |err| / (u mag) = %.3f at %s (constant %.2f); against the split bar %.3f'
          % (worst, where, R.C_DOT, worst_split))
    assert worst <= R.C_DOT / 2, 'the emulation is within a factor 2 of C_DOT: re-measure DOT_RATIO_MEASURED (%.3f)' % worst


def _grid_logits():
    zs = []
    for B, n, d, _ in R.SCORE_CASES:
        zs.append(R.ref_logits(*R.score_inputs(B, n, d, R.seed_of(B, n, d)))[0].flatten()[:20000])
    for B, n, d, s, _ in R.SCORE_RANDN_CASES:
        zs.append(R.ref_logits(*R.score_inputs(B, n, d, R.seed_of(B, n, d), s))[0].flatten()[:20000])
    return torch.cat(zs)


def test_sigmoid_and_tanh_constants():
    """c_s: torch-CPU f32 sigmoid of the grids' logits (rounded to f32) against float64 of the same f32 value; the tanh
    constant the same way over the grids' BN arguments."""
    z = _grid_logits().float()
    r_sig = float((torch.sigmoid(z).double() - torch.sigmoid(z.double())).abs().max()) / U
    ts = []
    for N, D, O, wb, _, _, _ in R.BN_TANH_CASES:
        a, w, bias, mean, var, gamma, beta = R.bn_tanh_inputs(N, D, O, wb)
        pre = _sub(a, 64).double() @ w.double() / 3 + (bias.double() if wb else 0)
        ts.append(((pre - mean.double()) / torch.sqrt(var.double() + R.BN_EPS) * gamma.double() + beta.double()).flatten())
    t = torch.cat(ts).float()
    r_tanh = float((torch.tanh(t).double() - torch.tanh(t.double())).abs().max()) / U
    print('torch-CPU f32 sigmoid: %.3f u (c_s = %.2f); tanh: %.3f u (constant %.2f)' % (r_sig, R.C_SIG, r_tanh, R.C_TANH))
    assert r_sig <= R.C_SIG / 2 and r_tanh <= R.C_TANH / 2
    # the whole scoring bar on an f32 evaluation: logits by the f32 chain, torch f32 sigmoid
    used = 0.0
    for B, n, d, label in R.SCORE_CASES:
        x, e, b = R.score_inputs(B, n, d, R.seed_of(B, n, d))
        x, e, b = _sub(x, 24), _sub(e, 24), _sub(b[:, None], 24)[:, 0]
        p64, z64, mag = R.ref_scores(x, e, b)
        p32 = torch.sigmoid(R.emul_dot_f32(x, e.t().contiguous()) + b)
        bar = R.sigmoid_bar(p64, R.dot_bar(mag, d))
        used = max(used, R.max_ratio(p32, p64, bar))
    print('f32 chain + f32 sigmoid uses %.3f of the scoring bar' % used)
    assert used <= 0.5


def test_bn_tanh_eval_bar_holds_for_torch_cpu_f32():
    """C_EPI: the affine BN step in torch-CPU f32 from the f32-rounded pre-activation, in units of
    u (S (|pre| + |mean|) + |t| + |beta|); then the whole (4) bar on an f32 evaluation (f32 chain + torch f32)."""
    r_epi, used = 0.0, 0.0
    for N, D, O, wb, _, _, _ in R.BN_TANH_CASES:
        a, w, bias, mean, var, gamma, beta = R.bn_tanh_inputs(N, D, O, wb)
        a = _sub(a, 32)
        y64, bar = R.ref_dense_bn_tanh(a, w, bias, mean, var, gamma, beta, R.BN_EPS)
        pre64 = a.double() @ w.double() / 3 + (bias.double() if wb else 0)
        inv64 = 1 / torch.sqrt(var.double() + R.BN_EPS)
        t64 = (pre64 - mean.double()) * inv64 * gamma.double() + beta.double()
        pre32 = pre64.float()
        t32 = (pre32 - mean) * (1.0 / torch.sqrt(var + R.BN_EPS)) * gamma + beta
        unit = U * (gamma.abs().double() * inv64 * (pre64.abs() + mean.abs().double()) + t64.abs() + beta.abs().double())
        r_epi = max(r_epi, float(((t32.double() - t64).abs() / unit).max()))
        v32 = R.emul_dot_f32(a, w) / 3.0
        if wb:
            v32 = v32 + bias
        y32 = torch.tanh((v32 - mean) * (1.0 / torch.sqrt(var + R.BN_EPS)) * gamma + beta)
        used = max(used, R.max_ratio(y32, y64, bar))
    print('affine BN step in f32: %.3f units (C_EPI = %.2f); an f32 evaluation uses %.3f of the (4) bar' % (r_epi, R.C_EPI, used))
    assert r_epi <= R.C_EPI / 2 and used <= 0.5


def test_ill_conditioned_statistics():
    """Columns with mean 100 and spread 1e-2: a one-pass E[z^2] - E[z]^2 in f32 is useless there (the reason the kernels'
    variance is two-pass), a two-pass f32 variance after a sequential f32 mean gives rstd to the 6e-4 relative
    this was designed on; dense_ref.ill_rstd_bar turns the per-case figure printed here into the device test's bar."""
    worst, worst_sum = 0.0, 0.0
    for n, o in R.TRAIN_ILL_CASES:
        z = R.ill_conditioned_z(n, o, R.gen(R.seed_of(6, n, o)))
        var64 = z.double().var(0, unbiased=False)
        rstd64 = 1 / torch.sqrt(var64 + R.BN_EPS)
        one_pass = (z * z).mean(0) - z.mean(0) ** 2
        assert float((one_pass.double() - var64).abs().max()) > 2 * float(var64.max())      # off by more than the variance itself
        mean, rstd = R.emul_two_pass_rstd_f32(z, R.BN_EPS)
        rel = float(((rstd.double() - rstd64).abs() / rstd64).max())
        print('N = %d: two-pass f32 rstd relative error %.3g' % (n, rel))
        worst = max(worst, rel)
        ratio = R.max_ratio(mean, z.double().mean(0), U * z.double().abs().sum(0) / n)
        print('N = %d: sequential f32 column mean %.3g u mag (constant %.1f, rigorous %d)' % (n, ratio, R.C_COLSUM, n + 2))
        assert ratio <= min(n + 2.0, R.C_COLSUM)
        worst_sum = max(worst_sum, ratio)
    assert worst_sum <= R.C_COLSUM / 2
    assert worst_sum > R.C_DOT          # the +- dot-product constant does not hold for same-sign sums: hence colsum_bar
    assert worst <= 6e-4


def test_training_bars_are_not_looser_than_the_existing_test_at_its_shape():
    """At N, O = 5003, 200 (test_training_layer_kernels_vs_torch_autograd) the derived bars are capped by that test's own:
    2e-6 on y, 2e-5 x scale on the gradients; torch-CPU f32 itself stays inside them."""
    u, bias, gamma, beta, rm, rv, gy = R.train_inputs(5003, 200, True, True)
    r64 = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy)
    r32 = R.ref_train_epilogue(*u, bias, gamma, beta, rm, rv, R.BN_MOMENTUM, R.BN_EPS, gy, dtype=torch.float32)
    err_y = float((r32['y'].double() - r64['y']).abs().max())
    assert R.derived_bar(err_y, 8 * U, 2e-6) <= 2e-6 and err_y <= 2e-6
    for k in ('gz', 'ggamma', 'gbeta'):
        scale = float(r64[k].abs().max())
        err = float((r32[k].double() - r64[k]).abs().max())
        assert err <= 2e-5 * scale, (k, err, scale)
    assert R.derived_bar(1e-7, 1e-9, 2e-6) == 4e-7 and R.derived_bar(0.0, 1e-7, 2e-6) == 1e-7
    assert R.derived_bar(4e-7, 5e-6, 2e-6) == 2e-6                       # today's bar caps the floor where f32 meets it
    assert R.derived_bar(1e-6, 1e-9, 2e-6) == 4e-6                       # and does not apply where f32 cannot


def test_ragged_cuts_are_the_ones_training_produces():
    """TRAIN_RAGGED_CASES: well-formed partitions that between them hold a cut that is no multiple of 128 in every case but
    the all-in-one-rank ones, ranks without rows first, in the middle and last, a rank of one row, of exactly 128 and of 129,
    one row per rank, NULL running statistics, no bias, and widths on both sides of the 256-column trip."""
    seen = set()
    for N, O, wb, wr, cuts in R.TRAIN_RAGGED_CASES:
        assert cuts[0] == 0 and cuts[-1] == N and all(b >= a for a, b in zip(cuts[:-1], cuts[1:])), cuts
        rows = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
        live = [n for n in rows if n > 0]
        assert sum(len(range(0, n, R.RB)) for n in rows) == len(R.rank_blocks(cuts))
        if len(live) > 1:
            assert any(c % R.RB for c in cuts[1:-1]) or 128 in rows, cuts
        seen.update(k for k, hit in (('first', rows[0] == 0), ('last', rows[-1] == 0), ('middle', 0 in rows[1:-1]),
                                     ('one', 1 in rows), ('128', 128 in rows), ('129', 129 in rows), ('each', len(rows) == N),
                                     ('norun', not wr), ('nobias', not wb), ('wide', O > 256), ('narrow', O <= 256),
                                     ('ldu', (N, O, cuts) in R.TRAIN_RAGGED_LDU_EXTRA)) if hit)
    assert seen == {'first', 'last', 'middle', 'one', '128', '129', 'each', 'norun', 'nobias', 'wide', 'narrow', 'ldu'}, seen
    assert all(any((n, o, c) == k for n, o, _, _, c in R.TRAIN_RAGGED_CASES) for k in R.TRAIN_RAGGED_LDU_EXTRA)
    assert R.rank_blocks((0, 0, 130, 130, 300)) == [(0, 128), (128, 130), (130, 258), (258, 300)]


def _live_ranks(cuts):
    return sum(1 for a, b in zip(cuts[:-1], cuts[1:]) if b > a)


def test_split_stage_emulation_meets_the_4t_bars_on_ragged_cuts():
    """(4s) at cuts that are no multiples of 128: the f32 restatement of the stages (per-rank blocks, rank-then-block fold)
    against float64 under the UNCHANGED bars of (4t), dense_ref.train_bars. A partition moves the association of the sums, and
    the bars -- derived from torch-CPU f32 in yet another association -- have room for it. The worst ratio is recorded next
    to the cases and must not go stale."""
    worst, where = 0.0, None
    for case in R.TRAIN_RAGGED_CASES:
        N, O, wb, wr, cuts = case
        inputs, r64, bars = R.train_reference(N, O, wb, wr)
        ratios = R.train_ratios(R.emul_train_split_f32(inputs, cuts), r64, bars)
        name = max(ratios, key=ratios.get)
        print('EMUL %s worst %s %.4f' % (R.ragged_id(case), name, ratios[name]))
        assert ratios[name] <= 1.0, (R.ragged_id(case), ratios)
        if ratios[name] > worst:
            worst, where = ratios[name], (R.ragged_id(case), name)
    print('EMUL worst ratio %.4f at %s (recorded %.4f)' % (worst, where, R.TRAIN_RAGGED_EMUL_WORST_RATIO_MEASURED))
    assert R.TRAIN_RAGGED_EMUL_WORST_RATIO_MEASURED / 2 <= worst <= R.TRAIN_RAGGED_EMUL_WORST_RATIO_MEASURED * 2, \
        'the recorded worst ratio went stale'


def test_split_stage_bars_notice_per_rank_statistics():
    """Vacuity: the two mistakes a split epilogue can make without any test at aligned cuts noticing -- a rank that centres on
    the mean of ITS rows, a rank that divides by ITS row count -- are outside the bars on every case with two ranks that have
    rows, even judged by the rank with the most rows (5002 of 5003)."""
    for case in R.TRAIN_RAGGED_CASES:
        N, O, wb, wr, cuts = case
        if _live_ranks(cuts) < 2:
            continue
        inputs, r64, bars = R.train_reference(N, O, wb, wr)
        for wrong in ('own_mean', 'own_count'):
            ratios = R.train_ratios(R.emul_train_split_f32(inputs, cuts, wrong=wrong), r64, bars)
            assert ratios['z'] <= 1.0                                     # z is row-local: neither mistake touches it
            stat = max(ratios['mean'], ratios['rstd'])
            print('WRONG %s %s: statistics %.3g, y %.3g, gz %.3g x their bars' % (wrong, R.ragged_id(case), stat, ratios['y'], ratios['gz']))
            assert stat > 1.0 and ratios['y'] > 1.0 and ratios['gz'] > 1.0, (wrong, R.ragged_id(case), ratios)


def test_split_stage_emulation_on_ill_conditioned_columns():
    """Columns with mean 100 and spread 1e-2 at ragged cuts: the emulated mean within colsum_bar, rstd within ill_rstd_bar
    (both taken on the z the stages return, as the device test does)."""
    w_mean, w_rstd = 0.0, 0.0
    for N, O, cuts in R.TRAIN_RAGGED_ILL_CASES:
        g = R.gen(R.seed_of(6, N, O))
        zin = R.ill_conditioned_z(N, O, g)
        gamma, beta = R.pm_uniform((O,), g) * 1.5, R.randn_scaled((O,), g, 0.1)
        e = R.emul_train_split_f32(([zin, zin, zin], None, gamma, beta, None, None, torch.zeros_like(zin)), cuts)
        z64 = e['z'].double()
        r_mean = R.max_ratio(e['mean'], z64.mean(0), R.colsum_bar(z64.abs().sum(0) / N, N))
        rstd64 = 1 / torch.sqrt(z64.var(0, unbiased=False) + R.BN_EPS)
        r_rstd = R.max_ratio(e['rstd'], rstd64, R.ill_rstd_bar(e['z'], R.BN_EPS) * rstd64)
        print('ILL N = %d, %d ranks: mean %.3f of colsum_bar, rstd %.3f of ill_rstd_bar' % (N, len(cuts) - 1, r_mean, r_rstd))
        assert r_mean <= 1.0 and r_rstd <= 1.0
        w_mean, w_rstd = max(w_mean, r_mean), max(w_rstd, r_rstd)
    print('ILL worst: mean %.3f, rstd %.3f' % (w_mean, w_rstd))


def test_layouts_and_guards():
    t = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    for kind in R.LAYOUTS:
        v = R.layout(t, kind)
        assert torch.equal(v, t) and v.stride(1) == 1
    assert R.layout(t, 'window').stride(0) % 4 == 0 and R.layout(t, 'window').storage_offset() % 4 == 0
    assert R.layout(t, 'offset1').stride(0) % 4 == 0 and R.layout(t, 'offset1').storage_offset() % 4 == 1
    assert R.layout(t, 'oddstride').stride(0) % 4 != 0
    for dt in (torch.float32, torch.int32, torch.int64):
        g = R.Guarded(3, 5, 7, 'cpu', dt)
        g.view.fill_(1)
        g.check('inside')
        assert not g.untouched()
        g.buf[3, 0] = 1
        with pytest.raises(AssertionError):
            g.check('outside')
    g = R.Guarded(2, 2, 4, 'cpu')
    assert bool(torch.isnan(g.buf).all()) and g.untouched()


def test_bce_loss_bar_f32_cannot_hold_1e6_on_saturated_logits():
    """Why dense_ref.bce_loss_bar has its second term: torch-CPU f32 BCELoss misses float64 (with f32 saturation) by more
    than 1e-6 relative once logits reach +-40, and stays inside 1e-6 on small logits."""
    for scale, beyond in ((None, False), (40.0, True)):
        x, e, b, hit = R.bce_inputs(68, 33, 4 if scale is None else 36, scale)
        z, _ = R.ref_logits(x, e, b)
        y = torch.where(hit, torch.tensor(0.9), torch.tensor(0.01))
        ref = float(R.ref_bce(z, y, 1.0 / z.numel(), saturate_f32=True)[0])
        cpu = R.emul_bce_loss_f32(z, y, 1.0 / z.numel())
        print('logit scale %s: torch-CPU f32 loss off by %.3g relative' % (scale, abs(cpu - ref) / abs(ref)))
        assert (abs(cpu - ref) > 1e-6 * abs(ref)) == beyond
        assert abs(cpu - ref) <= R.bce_loss_bar(ref, cpu)


def test_bce_gradient_bar_holds_for_torch_cpu_f32():
    """dense_ref.bce_grad_bar on an f32 evaluation of the whole operation (logits by the sequential f32 chain, torch-CPU
    f32 sigmoid, BCELoss's and sigmoid's backward formulas in f32): inside the bar everywhere, while a bar with the plain
    p (1 - p) slope is broken under the 1e-12 floor, where the logit's own rounding error meets a slope of order 1."""
    used, plain = 0.0, 0.0
    for B, n, d, scale in ((68, 33, 36, None), (68, 33, 36, 40.0), (212, 1000, 200, 40.0), (68, 33, 36, 120.0)):
        x, e, b, hit = R.bce_inputs(B, n, d, scale)
        z, mag = R.ref_logits(x, e, b)
        inv = 1.0 / z.numel()
        for hot, cold in ((1.0, 0.0), (0.9, 0.01)):
            y = torch.where(hit, torch.tensor(hot), torch.tensor(cold))
            _, g64, p64 = R.ref_bce(z, y, inv)
            _, g_s, p_s = R.ref_bce(z, y, inv, saturate_f32=True)
            p32 = torch.sigmoid(R.emul_dot_f32(x, e.t().contiguous()) + b)
            pq = (1.0 - p32) * p32
            g32 = ((p32 - y) / torch.clamp(pq, min=1e-12) * pq * inv).double()
            sat = p_s != p64
            ref = torch.where(sat, g_s, g64)
            bar = R.bce_grad_bar(g64, p64, y, R.dot_bar(mag, d), inv)
            used = max(used, float(((g32 - ref).abs() / bar).max()))
            old = 4 * R.U * g64.abs() + inv * R.sigmoid_bar(p64, R.dot_bar(mag, d))
            plain = max(plain, float(((g32 - ref).abs() / old).max()))
    print('an f32 BCE gradient uses %.3f of bce_grad_bar (%.1f x the plain-slope bar)' % (used, plain))
    assert used <= 0.5 and plain > 1.0
