"""tests/autograd_ref.py checked on the CPU: the layout makers give the strides and alignments the device test relies on, the
downstream ops it uses really hand a custom Function those layouts, every float64 restatement agrees with plain float64 torch
autograd of the oracle's formula (oracle/mgcn_oracle.py) on the same inputs, the loss cases satisfy the condition of the
power-of-two scaling, and an f32 emulation of the scaled sums stays inside the bars of section (3) (its share is printed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import aggregate_ref as A
from . import autograd_ref as AR
from . import cand_ce_ref as E
from . import cand_train_ref as C
from . import dense_ref as R
from . import query_train_ref as Q
from . import trunk_ref as T
from . import trunk_train_ref as TT

TIGHT = 1e-11          # float64 against float64, results of order 1 and sums of at most a few thousand terms


def _close(got, want, what, tol=TIGHT):
    want = want.reshape(got.shape)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, '%s: %.3g apart (scale %.3g)' % (what, err, scale)


# ---------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize('shape', [(5, 3), (17, 24), (130, 18), (33, 12), (3, 15)])
def test_layout_makers(shape):
    r, c = shape
    G = R.pm_uniform(shape, R.gen(R.seed_of(1, r, c)))
    for kind in AR.FREE_LAYOUTS + AR.EXPANDED_LAYOUTS:
        view, base = AR.make_layout(G, kind)
        strides, align = AR.expected_layout(kind, r, c)
        assert base.data_ptr() % 16 == 0
        assert tuple(view.shape) == shape and tuple(view.stride()) == strides and view.data_ptr() % 16 == align, (kind, view.stride())
        if kind in AR.FREE_LAYOUTS:
            assert torch.equal(view, G), kind
        elif kind == 'rowexp':
            assert torch.equal(view, G[0].expand(r, c))
        else:
            assert torch.equal(view, G[0, 0].expand(r, c))
    # (c): off the 16-byte grid in the base and in the row stride; (b) and (e) keep NaN outside the window
    view, base = AR.make_layout(G, 'offset3')
    assert view.stride(0) % 4 != 0 and view.storage_offset() == 3 and bool(torch.isnan(base[:, :3]).all())
    assert bool(torch.isnan(AR.make_layout(G, 'window5')[1][:, c:]).all())
    rows = AR.make_layout(G, 'rows')[1]
    assert bool(torch.isnan(rows[0]).all()) and bool(torch.isnan(rows[-1]).all())


def test_bits_compare_nan_equal_and_see_one_flipped_bit():
    t = torch.tensor([[1.0, float('nan')], [0.0, -0.0]])
    assert AR.same_bits(t, t.clone()) and not torch.equal(t, t.clone())
    u = t.clone()
    u[1, 0] = -0.0
    assert not AR.same_bits(t, u)


class _Probe(torch.autograd.Function):
    """A trivial custom Function that records the gradient it is handed."""
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x * 2.0

    @staticmethod
    def backward(ctx, g):
        _Probe.seen.append((tuple(g.stride()), g.storage_offset(), g.data_ptr() % 16))
        return g * 2.0


def test_downstream_ops_hand_over_the_layouts_as_they_are():
    """What the device test relies on: autograd passes the gradient exactly as the downstream op produced it (or as it was given)."""
    r, c = 5, 3
    x = torch.randn(r, c, requires_grad=True)
    G = torch.randn(r, c)

    def seen(run):
        _Probe.seen = []
        y = _Probe.apply(x)
        hooked = []
        y.register_hook(lambda g: hooked.append((tuple(g.stride()), g.storage_offset(), g.data_ptr() % 16)))
        run(y)
        assert hooked == _Probe.seen            # the hook sees the very layout the backward receives
        return _Probe.seen[0]

    assert seen(lambda y: y.sum().backward())[0] == (0, 0)
    assert seen(lambda y: (y.sum(0) * torch.randn(c)).sum().backward())[0] == (0, 1)
    base = torch.randn(r, c + 3)
    got = seen(lambda y: torch.cat([torch.randn(r, 3), y], 1).backward(base))
    assert got == ((c + 3, 1), 3, 12)
    for kind in AR.FREE_LAYOUTS + AR.EXPANDED_LAYOUTS:
        view, _ = AR.make_layout(G, kind)
        assert seen(lambda y: torch.autograd.grad(y, x, grad_outputs=view))[0] == AR.expected_layout(kind, r, c)[0], kind


# ---------------------------------------------------------------------------------------------------------------- (4) restatements
def test_aggregate_restatement_against_the_oracle(oracle):
    case = AR.aggregate_case()
    e = case.extra
    ref = AR.aggregate_reference(case, case.G)
    x, rel, ee = (t.double().requires_grad_(True) for t in case.inputs.values())
    E2, D = e['ei'].size(1), e['D']
    halves = []
    for h in range(2):
        sl = slice(h * E2 // 2, (h + 1) * E2 // 2)
        halves.append(oracle._propagate(x, e['ei'][:, sl], e['et'][sl], A.norm64(e['N'], e['ei'], h), ee[sl], rel, torch.eye(D, dtype=torch.float64)))
    out = torch.cat(halves, 1)
    out.backward(case.G.double())
    _close(out.detach(), ref['out'].value, 'aggregate forward')
    for name, leaf in (('x', x), ('rel', rel), ('ee', ee)):
        _close(leaf.grad, ref[name].value, 'aggregate d ' + name)
    assert int(ref['x'].n.max()) > 8 and float(A.bar_of(ref['x']).max()) < 1e-4 * float(ref['x'].value.abs().max())


@pytest.mark.parametrize('masks', ['none', 'keys'])
def test_layer_restatement_against_plain_autograd(masks):
    """model.py:103-106 as the oracle's layer_forward writes it (dropout on the in / out products, / 3, bias, batch norm, tanh),
    with the keep-masks injected."""
    case = AR.layer_case()
    m_in, m_out = AR.layer_key_masks(case) if masks == 'keys' else (None, None)
    inv_keep = 1.0 / (1.0 - case.extra['p']) if masks == 'keys' else 1.0
    r64, bars = AR.layer_reference(case, m_in, m_out, inv_keep, case.G)
    leaves = [t.double().requires_grad_(True) for t in case.inputs.values()]
    agg, a_loop, w_in, w_out, w_loop, bias, gamma, beta = leaves
    d = AR.LAYER_D
    in_res, out_res, loop_res = agg[:, :d] @ w_in, agg[:, d:] @ w_out, a_loop @ w_loop
    if m_in is not None:
        in_res, out_res = in_res * m_in.double() * inv_keep, out_res * m_out.double() * inv_keep
        assert 0.5 < float(m_in.double().mean()) < 0.9 and not torch.equal(m_in, m_out)
    rm, rv = case.extra['rm'].double().clone(), case.extra['rv'].double().clone()
    out = (in_res + out_res + loop_res) / 3 + bias
    y = torch.tanh(F.batch_norm(out, rm, rv, gamma, beta, True, AR.BN_MOMENTUM, AR.BN_EPS))
    y.backward(case.G.double())
    _close(y.detach(), r64['y'], 'layer y')
    _close(rm, r64['rm'], 'layer running mean')
    _close(rv, r64['rv'], 'layer running var')
    for name, leaf in zip(AR.LAYER_NAMES, leaves):
        _close(leaf.grad, r64[name], 'layer d ' + name)
        if name != 'bias':          # (d bias cancels analytically before a batch norm: its bar is 8 u of its terms, not of its value)
            assert 0 < bars[name] < 1e-3 * float(r64[name].abs().max()), (name, bars[name])       # no bar is vacuous


def test_trunk_and_tail_restatements_against_the_oracle(oracle):
    """oracle.conve_trunk in training mode without dropout, float64, against the chain trunk_train_ref.run -> query_train_ref.tail_run
    -> trunk_train_ref.run on the trunk case's geometry."""
    case, B, _ = AR.TRUNK
    sd = T.weights(case)
    s, r = T.queries(case, B)
    O = case[0] * case[1]
    G = R.pm_uniform((B, O), R.gen(R.seed_of(2, B, O)))
    sd64 = {k: v.double().clone().requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
    s64, r64 = s.double().requires_grad_(True), r.double().requires_grad_(True)
    hp = dict(T.hyper(case), feat_drop=0.0, hidden_drop=0.0)
    x = oracle.conve_trunk(sd64, hp, s64, r64, training=True)
    x.backward(G.double())
    z = TT.run(case, sd, s, r, None, 1.0, torch.zeros(B, O))['z']
    t = lambda k: sd['conv2.bn2.' + k]
    tail = Q.tail_run(z, None, 1.0, t('weight'), t('bias'), t('running_mean'), t('running_var'), G)
    _close(tail['x'], x.detach(), 'trunk + tail forward')
    _close(tail['d_gamma'], sd64['conv2.bn2.weight'].grad, 'd bn2 weight')
    _close(tail['d_beta'], sd64['conv2.bn2.bias'].grad, 'd bn2 bias')
    back = TT.run(case, sd, s, r, None, 1.0, tail['gz'])
    _close(back['ds'], s64.grad, 'ds')
    _close(back['dr'], r64.grad, 'dr')
    for name, key in (('d_conv_w', 'conv_e.weight'), ('d_conv_b', 'conv_e.bias'), ('d_fc_w', 'fc.weight'), ('d_fc_b', 'fc.bias'),
                      ('d_g0', 'bn0.weight'), ('d_b0', 'bn0.bias'), ('d_g1', 'bn1.weight'), ('d_b1', 'bn1.bias')):
        _close(back[name], sd64['conv2.' + key].grad, name)
    for k, name in (('bn0.running_mean', 'rm0'), ('bn0.running_var', 'rv0'), ('bn1.running_mean', 'rm1'), ('bn1.running_var', 'rv1')):
        _close(back[name], sd64['conv2.' + k].detach(), name)


def test_the_cases_are_the_references_own_inputs():
    """The trunk and tail cases hand the device exactly what the shared references were computed on."""
    case = AR.trunk_case()
    sd, s, r, keep, inv_keep, gz = TT.inputs(*AR.TRUNK)
    assert torch.equal(case.inputs['s'], s) and torch.equal(case.G, gz) and torch.equal(case.extra['keep'], keep)
    assert torch.equal(case.inputs['fc_w'], sd['conv2.fc.weight']) and case.inputs['conv_b'] is not None
    z, keep, inv_keep, gamma, beta, rm, rv, gx = Q.tail_inputs(*AR.TAIL)
    tc = AR.tail_case()
    assert torch.equal(tc.inputs['z'], z) and torch.equal(tc.G, gx) and torch.equal(tc.extra['keep'], keep)
    ref = AR.tail_reference()
    assert all(v <= 1.0 for v in Q.tail_vacuity(ref).values())
    idx = AR.rows_case().extra['idx']
    assert int(torch.bincount(idx).max()) >= 4 and idx.numel() == AR.ROWS_B


def test_rows_and_dropout_restatements():
    case = AR.rows_case()
    want = AR.rows_reference(case, case.G)
    table = case.inputs['table'].double().requires_grad_(True)
    torch.index_select(table, 0, case.extra['idx']).backward(case.G.double())
    n = int(torch.bincount(case.extra['idx']).max())
    mag = torch.zeros(table.shape, dtype=torch.float64).index_add_(0, case.extra['idx'], case.G.double().abs())
    assert bool(((want.double() - table.grad).abs() <= C.gamma(n) * mag).all())
    assert not torch.equal(want, Q.scatter_loop(case.extra['idx'], case.G, AR.ROWS_N, reverse=True))     # the order shows in the bits
    case = AR.dropout_case()
    got = AR.dropout_reference(case, case.G)
    kept = got != 0
    inv = np.float32(1.0 / (1.0 - case.extra['p']))
    assert 0.5 < float(kept.float().mean()) < 0.9
    assert torch.equal(got[kept], torch.from_numpy((case.G[kept].numpy() * inv).astype(np.float32)))
    assert torch.equal(kept, AR.dropout_reference(case, case.inputs['x']) != 0)                       # same bits forward and backward


def test_score_restatement_against_the_oracle(oracle):
    case = AR.score_case()
    r64, bars = AR.score_reference(case, case.G)
    x, ent, bias = (t.double().requires_grad_(True) for t in case.inputs.values())
    s = oracle.score_all(x, ent, bias)
    s.backward(case.G.double())
    _close(s.detach(), r64['s'], 'scores')
    for name, leaf in (('x', x), ('ent', ent), ('bias', bias)):
        _close(leaf.grad, r64[name], 'score d ' + name)
        assert float((bars[name] / r64[name].abs().clamp(min=1e-3)).max()) < 1e-3, name


# ---------------------------------------------------------------------------------------------------------------- (3) scalar losses
def _loss_cases():
    return [(AR.bce_case(*c), AR.score_bce_reference) for c in AR.BCE] + [(AR.cand_bce_case(), AR.cand_bce_reference),
                                                                           (AR.cand_ce_case(), AR.cand_ce_reference)]


def _autograd_loss(case, oracle):
    """The loss of a loss case by plain float64 torch ops on fresh leaves: (loss, leaves)."""
    x, ent, bias = (t.double().requires_grad_(True) for t in case.inputs.values())
    e = case.extra
    if 'hit' in e:
        hot, cold = AR.smoothed(e['smooth'], e['n'])
        y = torch.where(e['hit'], torch.tensor(hot), torch.tensor(cold)).double()
        return F.binary_cross_entropy(oracle.score_all(x, ent, bias), y), (x, ent, bias)
    live, row = C.live_rows(e['cand'], 0, e['N'])
    z = (ent[row] * x[:, None, :]).sum(2) + bias[row]
    B, K = row.shape
    if 'hot' in e:
        y = torch.where(e['label'], torch.tensor(e['hot']), torch.tensor(e['cold'])).double()
        return F.binary_cross_entropy(torch.sigmoid(z[live]), y[live], reduction='sum') / (B * K), (x, ent, bias)
    loss = 0.0
    for b in range(B):
        pos = e['label'][b] & live[b]
        if not bool(pos.any()):
            continue
        lp = torch.log_softmax(z[b][live[b]], 0)
        q = (1.0 - e['eps']) * pos[live[b]].double() / int(pos.sum()) + e['eps'] / int(live[b].sum())
        loss = loss - (q * lp).sum() / B
    return loss, (x, ent, bias)


@pytest.mark.parametrize('which', range(4), ids=['bce-small', 'bce', 'cand_bce', 'cand_ce'])
def test_loss_restatements_scaling_condition_and_f32_share(oracle, which):
    case, reference = _loss_cases()[which]
    r1 = reference(case)[0]
    assert AR.scale_safe([r1[k] for k in ('x', 'ent', 'bias')]), 'a reference gradient is below 2^-100 without being zero'
    assert any(bool((r1[k] != 0).any()) for k in ('x', 'ent', 'bias'))
    gl = 3.0
    r64, b1, mags, aux = reference(case, gl)
    loss, leaves = _autograd_loss(case, oracle)
    (loss * gl).backward()
    assert abs(float(loss.detach()) - r64['loss']) <= TIGHT * max(1.0, abs(r64['loss']))
    for name, leaf in zip(('x', 'ent', 'bias'), leaves):
        _close(leaf.grad, r64[name], '%s d %s' % (case.name, name))
    if 'cand' in case.extra:
        dead = ~aux['live']
        assert int(dead.sum()) >= 4 and case.extra['cand'].size(1) % 64 != 0               # dead positions, K no multiple of 64
        emul = AR.emul_list_f32(aux, case, gl)
    else:
        q = torch.sigmoid(-aux['z'])
        assert bool((q > 64 * R.U).all()), 'a probability at the edge of f32 saturation: dense_ref.bce_grad_bar alone does not cover it'
        emul = AR.emul_score_bce_f32(aux, case, gl)
    bars = AR.scaled_bars(b1, mags, gl)
    share = AR.worst_share(emul, r64, bars)
    print('SHARE %s gl=%g %s' % (case.name, gl, ' '.join('%s=%.4f' % kv for kv in sorted(share.items()))))
    assert max(share.values()) <= 1.0, share
    for k in bars:              # no bar is vacuous: far below the gradient's own scale wherever the gradient is not tiny
        big = r64[k].abs() > 1e-3 * float(r64[k].abs().max())
        assert float((torch.as_tensor(bars[k]).expand_as(r64[k])[big] / r64[k].abs()[big]).max()) < 1e-2, k
