"""The torch.autograd.Function classes of kgc-gcn_amd/autograd.py and kgc-gcn_amd/dist.py on a real MI355X, held to what autograd may
hand them rather than to what loss.backward() of the production graph happens to: (1) every layout of the upstream gradient gives
the bits of the contiguous one and leaves the handed tensor alone, (2) freezing inputs changes no bit of what is still computed,
(3) a scalar loss weight scales exactly (powers of two), within the family's bar times |gl| (3.0), and the same as a tensor,
(4) a random upstream gradient meets the float64 restatement of the Function's formula, (5) two backwards through one graph give
the same bits and leave the saved tensors alone, (6) the shard forms (the rank's rows and a world-1 exchange made explicit) give the bits of
the plain forms (every trailing argument at its default). Cases, layouts,
restatements and bars: tests/autograd_ref.py (checked on the CPU by tests/test_autograd_ref_host.py). Every float64 check prints
`RATIO family id worst / bar` (pytest -s) before it asserts.

Which layouts reach a kernel uncopied (asserted in test_gradient_layouts where a wrapper call shows it, HANDED_THROUGH):
  _TrunkTrainFn, _QueryRowsFn, _TrunkTailFn, _CounterDropoutFn    (a) (b) (c) (e) as they are; (d) (f) (g) copied;
  _AggregateFn (plain, with node_range), _GatherRowsFn            (a) (e) as they are; (b) (c) (d) (f) (g) copied;
  _LayerTrainFn (plain, with an exchange)                         the same, the copy being _native._bn_grad's / .contiguous();
  _ScoreFn                                                        none: torch's gs * s * (1 - s) reads any layout, the kernels its result;
  _AllReduceGradFn                                                every layout copied; _RankZeroGradFn: every layout handed on, no kernel;
  the loss Functions                                              a scalar, folded in by broadcasting.
Worst share of a bar on the MI355X, per family (section (4), then (3) unit / x 3; the shard forms give the plain forms' figures):
  aggregate 0.476 (d ee)   layer p = 0 0.209, torch masks 0.267, keys 0.384 (d a_loop / d agg)   trunk 0.356 (ds)   tail 0.161 (x)
  score 0.133 (s)   score BCE (4, 1, 4) 0.053 / 0.045, (36, 33, 4) 0.052 / 0.059 (d x)   list BCE 0.166 / 0.141, list CE 0.173 / 0.174 (d ent)
  row gather, dropout and the identity Functions: bit for bit.
The f32 emulation of the host test uses at most 0.059 (score BCE), 0.089 (list BCE) and 0.092 (list CE) of the x 3 bars."""
import collections

import pytest
import torch

from . import aggregate_ref as A
from . import autograd_ref as AR
from . import dense_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MOM, EPS = AR.BN_MOMENTUM, AR.BN_EPS


def _report(family, cid, ratio):
    print('RATIO %s %s %.4f' % (family, cid, ratio))
    assert ratio <= 1.0, '%s %s: worst |got - float64| is %.3f x its bar' % (family, cid, ratio)


# ---------------------------------------------------------------------------------------------------------------- the Functions
class Spec(object):
    """One Function on one case: `leaves(trainable)` -> (OrderedDict of device leaves, state dict of in-place tensors),
    `apply(leaves, state)` -> output, `check64(y, grads, state, G)` the float64 check of section (4)."""

    def __init__(self, name, case, call, state=None, prepare=None, check64=None):
        self.name, self.case, self.call, self.state_of, self.prepare, self.check64 = name, case, call, state, prepare, check64
        self.scalar = case.G is None

    def leaves(self, trainable=None):
        out = collections.OrderedDict()
        for k, v in self.case.inputs.items():
            t = v.to(DEV)
            if self.prepare is not None:
                t = self.prepare(k, t)
            out[k] = t.clone().requires_grad_(trainable is None or k in trainable)
        return out, ({k: v.to(DEV).clone() for k, v in self.state_of.items()} if self.state_of else {})

    def apply(self, leaves, state):
        return self.call(leaves, state)


_csr_cache = {}


def _csr(pkg):
    if 'csr' not in _csr_cache:
        e = AR.aggregate_case().extra
        _csr_cache['csr'] = pkg.GraphCSR(e['N'], 2 * e['R'] + 1, e['ei'], e['et'], DEV, hub_threshold=0, hub_chunk=64)
    return _csr_cache['csr']


def _exchange(pkg, n):
    return pkg.dist._Exchange([0, n], 0, None, 1)


def _agg_check(pkg, shard):
    def check(y, grads, state, G):
        case = AR.aggregate_case()
        csr = _csr(pkg)
        ref = AR.aggregate_reference(case, G)
        perm = csr.perm.cpu().long()
        ee_ref = A.select_rows(ref['ee'], perm)
        if shard:
            slots = csr.edge_table_shard(torch.arange(perm.numel(), device=DEV).unsqueeze(1), 0, case.extra['N']).reshape(-1).cpu()
            ee_ref = A.select_rows(ee_ref, slots)
        for name, got, want in (('out', y, ref['out']), ('x', grads['x'], ref['x']), ('rel', grads['rel'], ref['rel']), ('ee', grads['ee'], ee_ref)):
            ratio, bad_zero, _ = A.worst_ratio(got.detach().cpu(), want)
            print('RATIO autograd_%s %s %.4f (term-less elements that are not 0.0: %d)' % ('shard_aggregate' if shard else 'aggregate', name, ratio, bad_zero))
            A.check(got.detach().cpu(), want, name)
    return check


def _layer_check(form, label=None):
    def check(y, grads, state, G):
        case = AR.layer_case()
        inv_keep = 1.0 / (1.0 - case.extra['p'])
        if form == 'p0':
            m_in, m_out, inv_keep = None, None, 1.0
        elif form == 'keys':
            m_in, m_out = AR.layer_key_masks(case)
        else:                                   # torch's masks: the bool tensors the Function saved
            saved = [t for t in y.grad_fn.saved_tensors if t is not None and t.dtype == torch.bool]
            assert len(saved) == 2
            m_in, m_out = (t.cpu() for t in saved)
            assert 0.5 < float(m_in.float().mean()) < 0.9 and not torch.equal(m_in, m_out)
        r64, bars = AR.layer_reference(case, m_in, m_out, inv_keep, G)
        got = dict(grads, y=y, rm=state['rm'], rv=state['rv'])
        for name, share in AR.worst_share(got, r64, bars).items():
            _report('autograd_' + (label or 'layer_' + form), name, share)
    return check


def _trunk_check(y, grads, state, G):
    ref = AR.trunk_reference()
    got = {'z': y, 'rm0': state['rm0'], 'rv0': state['rv0'], 'rm1': state['rm1'], 'rv1': state['rv1']}
    got.update({AR.TRUNK_GRAD_OF[k]: v for k, v in grads.items()})
    assert len(got) == 15
    for name, v in got.items():
        _report('autograd_trunk', name, ref.ratio(name, v))


def _tail_check(y, grads, state, G):
    ref = AR.tail_reference()
    got = {'x': y, 'rm': state['rm'], 'rv': state['rv'], 'gz': grads['z'], 'd_gamma': grads['gamma'], 'd_beta': grads['beta']}
    for name, v in got.items():
        _report('autograd_tail', name, ref.ratio(name, v))


def _rows_check(y, grads, state, G):
    case = AR.rows_case()
    assert torch.equal(y.detach().cpu(), case.inputs['table'][case.extra['idx']])
    assert torch.equal(grads['table'].cpu(), AR.rows_reference(case, G)), 'd table is not the sequential loop bit for bit'


def _dropout_check(y, grads, state, G):
    case = AR.dropout_case()
    assert torch.equal(y.detach().cpu(), AR.dropout_reference(case, case.inputs['x']))
    assert torch.equal(grads['x'].cpu(), AR.dropout_reference(case, G))


def _score_check(y, grads, state, G):
    r64, bars = AR.score_reference(AR.score_case(), G)
    for name, share in AR.worst_share(dict(grads, s=y), r64, bars).items():
        _report('autograd_score', name, share)


def _identity_check(y, grads, state, G):
    assert AR.same_bits(grads['y'].cpu(), G) and AR.same_bits(y.detach().cpu(), AR.identity_case().inputs['y'])


def matrix_specs(pkg):
    M, Dm = pkg.model, pkg.dist
    specs = []
    agg = AR.aggregate_case()
    N = agg.extra['N']
    csr = _csr(pkg)
    slot = lambda k, t: t.index_select(0, csr.perm.long()).contiguous() if k == 'ee' else t
    shard = lambda k, t: csr.edge_table_shard(slot(k, t), 0, N) if k == 'ee' else t
    specs.append(Spec('aggregate', agg, lambda l, s: M._AggregateFn.apply(l['x'], l['rel'], l['ee'], csr), prepare=slot,
                      check64=_agg_check(pkg, False)))
    specs.append(Spec('shard_aggregate', agg, lambda l, s: M._AggregateFn.apply(l['x'], l['rel'], l['ee'], csr, (0, N)), prepare=shard,
                      check64=_agg_check(pkg, True)))

    lay = AR.layer_case()
    e = lay.extra
    keys = (e['keys'][0], e['keys'][1], e['row0'])

    def layer_call(p, drop_keys, sharded=False):
        def call(l, s):
            a = tuple(l.values()) + (s['rm'], s['rv'], MOM, EPS, p)
            with torch.random.fork_rng(devices=[0]):      # (the session's generators are left as they were)
                torch.manual_seed(20260101)     # the torch-mask form draws from the device generator: the same masks every call
                if sharded:
                    return M._LayerTrainFn.apply(*a, drop_keys, _exchange(pkg, AR.LAYER_N))
                return M._LayerTrainFn.apply(*a, drop_keys)
        return call
    st = dict(rm=e['rm'], rv=e['rv'])
    specs.append(Spec('layer_p0', lay, layer_call(0.0, None), state=st, check64=_layer_check('p0')))
    specs.append(Spec('layer_torch_masks', lay, layer_call(e['p'], None), state=st, check64=_layer_check('torch')))
    specs.append(Spec('layer_keys', lay, layer_call(e['p'], keys), state=st, check64=_layer_check('keys')))
    specs.append(Spec('shard_layer_p0', lay, layer_call(0.0, None, True), state=st, check64=_layer_check('p0', 'shard_layer_p0')))
    specs.append(Spec('shard_layer_keys', lay, layer_call(e['p'], keys, True), state=st, check64=_layer_check('keys', 'shard_layer_keys')))

    tr = AR.trunk_case()
    keep, stats = tr.extra['keep'].to(DEV), tr.extra['stats']

    def trunk_call(l, s):
        return M._TrunkTrainFn.apply(*l.values(), (s['rm0'], s['rv0'], MOM, AR.TT.BN_EPS), (s['rm1'], s['rv1'], MOM, AR.TT.BN_EPS), keep,
                                     tr.extra['inv_keep'], tr.extra['geom'])
    specs.append(Spec('trunk', tr, trunk_call, state=dict(rm0=stats['bn0.running_mean'], rv0=stats['bn0.running_var'],
                                                           rm1=stats['bn1.running_mean'], rv1=stats['bn1.running_var']), check64=_trunk_check))

    ta = AR.tail_case()
    tkeep = ta.extra['keep'].to(DEV)
    specs.append(Spec('tail', ta, lambda l, s: M._TrunkTailFn.apply(l['z'], l['gamma'], l['beta'], s['rm'], s['rv'], AR.Q.BN_MOMENTUM, AR.Q.BN_EPS,
                                                                    tkeep, ta.extra['inv_keep']),
                      state=dict(rm=ta.extra['rm'], rv=ta.extra['rv']), check64=_tail_check))

    ro = AR.rows_case()
    idx = ro.extra['idx'].to(DEV)
    specs.append(Spec('rows', ro, lambda l, s: M._QueryRowsFn.apply(l['table'], idx), check64=_rows_check))

    dr = AR.dropout_case()
    specs.append(Spec('dropout', dr, lambda l, s: M._CounterDropoutFn.apply(l['x'], dr.extra['key'], dr.extra['row0'], dr.extra['p']),
                      check64=_dropout_check))

    specs.append(Spec('score', AR.score_case(), lambda l, s: M._ScoreFn.apply(l['x'], l['ent'], l['bias']), check64=_score_check))

    ident = AR.identity_case()
    ex = _exchange(pkg, ident.G.size(0))
    specs.append(Spec('gather_rows', ident, lambda l, s: Dm._GatherRowsFn.apply(l['y'], ex, False), check64=_identity_check))
    specs.append(Spec('gather_rows_reduce', ident, lambda l, s: Dm._GatherRowsFn.apply(l['y'], ex, True), check64=_identity_check))
    specs.append(Spec('all_reduce_grad', ident, lambda l, s: Dm._AllReduceGradFn.apply(l['y'], ex), check64=_identity_check))
    specs.append(Spec('rank_zero_grad', ident, lambda l, s: Dm._RankZeroGradFn.apply(l['y'], ex), check64=_identity_check))
    return collections.OrderedDict((s.name, s) for s in specs)


MATRIX = ('aggregate', 'shard_aggregate', 'layer_p0', 'layer_torch_masks', 'layer_keys', 'shard_layer_p0', 'shard_layer_keys', 'trunk', 'tail',
          'rows', 'dropout', 'score', 'gather_rows', 'gather_rows_reduce', 'all_reduce_grad', 'rank_zero_grad')


def loss_specs(pkg):
    """name -> (plain Spec, shard Spec, reference function)."""
    M, Dm = pkg.model, pkg.dist
    out = collections.OrderedDict()
    for c in AR.BCE:
        case = AR.bce_case(*c)
        n = case.extra['n']
        mask = R.pack_bits(case.extra['hit']).to(DEV)
        hot, cold = pkg._native.smoothed_targets(case.extra['smooth'], n)
        assert (hot, cold) == AR.smoothed(case.extra['smooth'], n)
        out[case.name] = (Spec(case.name, case, lambda l, s, mask=mask, hot=hot, cold=cold: M._ScoreBCEFn.apply(l['x'], l['ent'], l['bias'], mask, hot, cold)),
                          Spec(case.name + '_shard', case, lambda l, s, mask=mask, hot=hot, cold=cold, n=n: M._ScoreBCEFn.apply(
                              l['x'], l['ent'], l['bias'], mask, hot, cold, n)), AR.score_bce_reference)
    case = AR.cand_bce_case()
    e = case.extra
    cand, label = e['cand'].to(DEV), e['label'].to(DEV)
    out['cand_bce'] = (Spec('cand_bce', case, lambda l, s: M._CandBCEFn.apply(l['x'], l['ent'], l['bias'], cand, label, e['hot'], e['cold'])),
                       Spec('cand_bce_shard', case, lambda l, s: M._CandBCEFn.apply(l['x'], l['ent'], l['bias'], cand, label, e['hot'], e['cold'], 0)),
                       AR.cand_bce_reference)
    case2 = AR.cand_ce_case()
    e2 = case2.extra
    cand2, label2 = e2['cand'].to(DEV), e2['label'].to(DEV)
    ex = _exchange(pkg, e2['N'])
    out['cand_ce'] = (Spec('cand_ce', case2, lambda l, s: M._CandCEFn.apply(l['x'], l['ent'], l['bias'], cand2, label2, e2['eps'])),
                      Spec('cand_ce_shard', case2, lambda l, s: M._CandCEFn.apply(l['x'], l['ent'], l['bias'], cand2, label2, e2['eps'], 0, ex)),
                      AR.cand_ce_reference)
    return out


LOSSES = ('bce-4-1-4', 'bce-36-33-4', 'cand_bce', 'cand_ce')
LOSS_FORMS = [(n, f) for n in LOSSES for f in ('plain', 'shard')]


def _any_spec(pkg, name):
    if name in MATRIX:
        return matrix_specs(pkg)[name]
    base, form = name.rsplit(':', 1)
    return loss_specs(pkg)[base][0 if form == 'plain' else 1]


def _grads(outputs, leaves, grad_outputs=None):
    ins = [t for t in leaves.values() if t.requires_grad]
    got = torch.autograd.grad(outputs, ins, grad_outputs=grad_outputs, retain_graph=True)
    torch.cuda.synchronize()
    return collections.OrderedDict(zip([k for k, t in leaves.items() if t.requires_grad], got))


def _same(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert AR.same_bits(a[k], b[k]), '%s: d %s differs' % (what, k)
        assert bool(torch.isfinite(a[k]).all()), '%s: d %s is not finite' % (what, k)


# ---------------------------------------------------------------------------------------------------------------- (1)
# Which layouts reach the wrapper uncopied: Function -> (the _native entry its backward calls, the position of the gradient among
# its arguments, the layouts handed through as they are). Every other layout must arrive as a copy. (The layer Functions hand
# every layout on and _native._bn_grad copies inside the wrapper; _ScoreFn's kernels only see torch's elementwise product.)
_STRIDE_RULE = ('contiguous', 'window5', 'offset3', 'rows')       # last stride 1, rows at least a row apart
_CONTIGUOUS = ('contiguous', 'rows')                              # .contiguous()
HANDED_THROUGH = {'trunk': ('conve_train_bwd', 13, _STRIDE_RULE), 'tail': ('conve_tail_bwd', 6, _STRIDE_RULE),
                  'rows': ('query_rows_bwd', 1, _STRIDE_RULE), 'dropout': ('dropout_apply', 0, _STRIDE_RULE),
                  'aggregate': ('aggregate_bwd', 4, _CONTIGUOUS), 'shard_aggregate': ('aggregate_bwd_shard', 4, _CONTIGUOUS)}


@pytest.mark.parametrize('name', MATRIX)
def test_gradient_layouts(pkg, name, monkeypatch):
    spec = matrix_specs(pkg)[name]
    reached = []
    if name in HANDED_THROUGH:
        entry, pos, through = HANDED_THROUGH[name]
        inner = getattr(pkg._native, entry)

        def recording(*args, **kw):
            reached.append(args[pos].data_ptr())
            return inner(*args, **kw)
        monkeypatch.setattr(pkg._native, entry, recording)
    leaves, state = spec.leaves()
    y = spec.apply(leaves, state)
    r, c = y.shape
    G = spec.case.G.to(DEV)
    assert tuple(G.shape) == (r, c)
    seen = []
    y.register_hook(lambda g: seen.append((tuple(g.stride()), g.data_ptr() % 16)))
    want = None
    for kind in AR.FREE_LAYOUTS:
        view, base = AR.make_layout(G, kind)
        before = AR.bits(base).clone()
        if kind == 'offset3':                   # a real downstream torch.cat([other, y], 1): its backward hands y a narrow view
            other = torch.randn((r, 3), device=DEV)
            got = _grads(torch.cat([other, y], 1), leaves, base)
        else:
            got = _grads(y, leaves, view)
        assert seen[-1] == AR.expected_layout(kind, r, c), (kind, seen[-1])
        assert torch.equal(AR.bits(base), before), '%s: the handed gradient was written' % kind
        if name in HANDED_THROUGH:
            assert (reached[-1] == view.data_ptr()) == (kind in through), '%s %s: handed through %s' % (name, kind, reached[-1] == view.data_ptr())
        if want is None:
            want = got
        _same(got, want, '%s %s' % (name, kind))
        if name == 'all_reduce_grad':           # its docstring's promise: a storage of its own
            assert got['y'].untyped_storage().data_ptr() != base.untyped_storage().data_ptr() and got['y'].is_contiguous()
    # (f) a row-expanded gradient, handed in directly and by a real downstream y.sum(0) * v
    view, base = AR.make_layout(G, 'rowexp')
    before = AR.bits(base).clone()
    clone = _grads(y, leaves, view.contiguous())
    assert seen[-1][0] == (c, 1)
    got = _grads(y, leaves, view)
    assert seen[-1][0] == (0, 1)
    assert torch.equal(AR.bits(base), before)
    assert name not in HANDED_THROUGH or reached[-1] != view.data_ptr()         # an expanded gradient is always copied
    _same(got, clone, name + ' rowexp')
    got = _grads((y.sum(0) * base).sum(), leaves)
    assert seen[-1][0] == (0, 1)
    _same(got, clone, name + ' rowexp by sum(0)')
    # (g) a scalar-expanded gradient by a plain y.sum()
    clone = _grads(y, leaves, torch.ones((r, c), device=DEV))
    got = _grads(y.sum(), leaves)
    assert seen[-1][0] == (0, 0)
    _same(got, clone, name + ' scalar')
    assert len(seen) == len(AR.FREE_LAYOUTS) + 5


# ---------------------------------------------------------------------------------------------------------------- (2)
def _patterns(names):
    out = []
    for n in names:
        for p in (frozenset([n]), frozenset(names) - {n}):
            if p and p != frozenset(names) and p not in out:
                out.append(p)
    return out


@pytest.mark.parametrize('name', MATRIX + tuple('%s:%s' % nf for nf in LOSS_FORMS))
def test_frozen_inputs(pkg, name):
    spec = _any_spec(pkg, name)
    G = None if spec.scalar else spec.case.G.to(DEV)

    def run(trainable):
        leaves, state = spec.leaves(trainable)
        y = spec.apply(leaves, state)
        y.backward(G)
        torch.cuda.synchronize()
        return leaves, state, y.detach()

    names = list(spec.case.inputs)
    full, state0, y0 = run(None)
    assert all(t.grad is not None for t in full.values())
    for pat in _patterns(names):
        leaves, state, y = run(pat)
        what = '%s with only %s trainable' % (name, sorted(pat))
        assert AR.same_bits(y, y0), what
        for k, t in leaves.items():
            if k in pat:
                assert t.grad is not None and AR.same_bits(t.grad, full[k].grad), '%s: d %s differs' % (what, k)
            else:
                assert t.grad is None, '%s: the frozen %s has a gradient' % (what, k)
        for k in state0:
            assert AR.same_bits(state[k], state0[k]), '%s: %s differs' % (what, k)
    for k, v in (spec.state_of or {}).items():                  # the in-place state did move
        assert not torch.equal(state0[k].cpu(), v), k


# ---------------------------------------------------------------------------------------------------------------- (3)
@pytest.mark.parametrize('name,form', LOSS_FORMS)
def test_scalar_loss_weights(pkg, name, form):
    plain, shard, reference = loss_specs(pkg)[name]
    spec = plain if form == 'plain' else shard
    leaves, state = spec.leaves()
    loss = spec.apply(leaves, state)
    assert loss.dim() == 0
    unit = _grads(loss, leaves)
    # a power of two scales exactly
    quarter = _grads(loss * 0.25, leaves)
    for k in unit:
        assert AR.same_bits(quarter[k], unit[k] * 0.25), '%s: d %s under 0.25 is not a quarter of the unit gradient bit for bit' % (spec.name, k)
        assert bool((unit[k] != 0).any())
    # 3.0 against float64: the family's unit bar times 3 plus the one rounding of gl (autograd_ref's docstring)
    gl = 3.0
    three = _grads(loss * gl, leaves)
    r64, b1, mags, _ = reference(spec.case, gl)
    for k, share in AR.worst_share(three, r64, AR.scaled_bars(b1, mags, gl)).items():
        _report('autograd_loss_x3_' + spec.name, k, share)
    for k, share in AR.worst_share(unit, reference(spec.case)[0], b1).items():
        _report('autograd_loss_unit_' + spec.name, k, share)
    # gl as a tensor: 0-dim, a 0-dim view into a larger tensor, and what a downstream (loss * w).sum() accumulates
    _same(_grads(loss, leaves, torch.tensor(gl, device=DEV)), three, spec.name + ' 0-dim gl')
    seen = []
    loss.register_hook(lambda g: seen.append((g.dim(), g.storage_offset())))
    _same(_grads(loss, leaves, torch.full((4,), gl, device=DEV)[2]), three, spec.name + ' gl as a view')
    assert seen[-1] == (0, 2)
    _same(_grads(loss, leaves, torch.full((1, 1), gl, device=DEV).expand(3, 5)[1, 2]), three, spec.name + ' gl as an expanded view')
    _same(_grads((loss * torch.full((4,), 0.75, device=DEV)).sum(), leaves), three, spec.name + ' gl from a broadcast')


# ---------------------------------------------------------------------------------------------------------------- (4)
@pytest.mark.parametrize('name', MATRIX)
def test_random_gradient_against_float64(pkg, name):
    spec = matrix_specs(pkg)[name]
    leaves, state = spec.leaves()
    y = spec.apply(leaves, state)
    grads = _grads(y, leaves, spec.case.G.to(DEV))
    spec.check64(y, grads, state, spec.case.G)


# ---------------------------------------------------------------------------------------------------------------- (5)
@pytest.mark.parametrize('name', MATRIX + tuple('%s:%s' % nf for nf in LOSS_FORMS))
def test_twice_through_one_graph(pkg, name):
    spec = _any_spec(pkg, name)
    leaves, state = spec.leaves()
    y = spec.apply(leaves, state)
    G = torch.tensor(0.7, device=DEV) if spec.scalar else spec.case.G.to(DEV)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert saved or name in ('gather_rows', 'gather_rows_reduce', 'all_reduce_grad', 'rank_zero_grad', 'dropout')
    # The trunk's workspace (uint8) is the one saved tensor a backward may write: by the header's contract (include/mgcn_hip.h (9)) its
    # first section c [B, K] is what the forward leaves for the backward, which reads it, and every later section is the backward's
    # own scratch. Held here: c keeps its bits, and the whole workspace has the same bits after the second backward as after the first.
    keeps = lambda t: 4 * AR.TRUNK[1] * AR.T.sizes(AR.TRUNK[0])[2] if (name == 'trunk' and t.dtype == torch.uint8) else t.numel()
    assert name != 'trunk' or sum(t.dtype == torch.uint8 and keeps(t) < t.numel() for t in saved) == 1
    snap = [t.clone() for t in saved]
    ins = [t for t in leaves.values()]
    runs, after = [], []
    for _ in range(2):
        y.backward(G, retain_graph=True, inputs=ins)
        torch.cuda.synchronize()
        runs.append(collections.OrderedDict((k, t.grad.clone()) for k, t in leaves.items()))
        for t in ins:
            t.grad = None
        for t, s in zip(saved, snap):
            n = keeps(t)
            assert AR.same_bits(t.reshape(-1)[:n], s.reshape(-1)[:n]), '%s: a saved tensor of shape %s changed in a backward' % (name, tuple(t.shape))
        after.append([t.clone() for t in saved])
    _same(runs[1], runs[0], name + ' second backward')
    for a, b in zip(*after):
        assert AR.same_bits(a, b), '%s: a saved tensor differs after the second backward' % name


# ---------------------------------------------------------------------------------------------------------------- (6)
@pytest.mark.parametrize('name', LOSSES)
def test_shard_forms_give_the_plain_forms_bits(pkg, name):
    plain, shard, _ = loss_specs(pkg)[name]
    got = []
    for spec in (plain, shard):
        leaves, state = spec.leaves()
        loss = spec.apply(leaves, state)
        got.append((loss.detach(), _grads(loss, leaves), _grads(loss * 0.6180339887, leaves),
                    _grads(loss, leaves, torch.tensor(-1.3, device=DEV))))
    assert AR.same_bits(got[0][0], got[1][0]), 'loss'
    for i, what in ((1, 'unit gradient'), (2, 'gl = 0.618...'), (3, 'gl = -1.3 as a tensor')):
        _same(got[1][i], got[0][i], '%s shard form under %s' % (name, what))
    assert not AR.same_bits(got[0][1]['x'], got[0][2]['x'])
