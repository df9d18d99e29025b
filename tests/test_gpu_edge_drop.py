"""Edge dropout and own-triple removal on a real MI355X (`-m gpu`; include/mgcn_hip.h (19)): the rewritten
records byte for byte against the host twin (which tests/test_edge_drop_host.py holds to the restatement), by value and through
the device step word; the flags against their restatement; the aggregation forward and backward on the view against the float64
sums of the kept sub-graph under aggregate_ref's own bars; and the whole training step with both switches on: repeatable,
equal to the sharded step at one rank, equal to the captured step, bit for bit. With the switches off nothing is launched."""
import copy

import numpy as np
import pytest
import torch

from . import aggregate_ref as ar
from . import edge_drop_ref as er
from .test_gpu_cand_captured import FIRST_STEP
from .test_gpu_cand_captured import SEED as DRAW_SEED
from .test_gpu_captured_step import CLIP, SMOOTH, SWITCHES, _assert_same_state, _twin, _word
from .test_gpu_query_train import DEV, _repeating_batches

pytestmark = pytest.mark.gpu
GRAPHS = er.graphs()
NODE = {'degree': 5, 'hub': 0, 'type': 3}
WIDTHS = (4, 65, 100)
P_STEP = 0.5

_built = {}


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES + ('MGCN_EDGE_DROP', 'MGCN_EDGE_DROP_QUERIES'):
        monkeypatch.delenv(name, raising=False)


def _graph(pkg, name):
    """(host layout, host table, GraphCSR on the device, its state), built once per module."""
    if name not in _built:
        N, R, ei, et, thr, chunk = GRAPHS[name]
        host = pkg._native.csr_build_host(N, 2 * R + 1, ei, et, hub_threshold=thr, hub_chunk=chunk)
        csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, DEV, hub_threshold=thr, hub_chunk=chunk)
        assert torch.equal(csr.rec.cpu(), host['rec']) and csr.num_chunks == host['num_chunks']
        st = csr.edge_drop_state()
        _built[name] = (host, st.table.cpu(), csr, st)
    return _built[name]


def _forced(name, kind):
    f = er.forced_of(kind, GRAPHS[name][2], NODE[name])
    return None if f is None else torch.from_numpy(f)


# ------------------------------------------------------------------------------------------------- bytes
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_records_equal_the_host_twin(pkg, name):
    """Every case of edge_drop_ref.DROP_CASES, by value and through the device word; then the word is overwritten with the next
    step's and the SAME call gives the next step's records."""
    nat = pkg._native
    host, table, csr, st = _graph(pkg, name)
    word = _word(nat, er.SEED, er.STEP)
    dkey = nat.DeviceKey(word, nat.EDGE_DROP_SITE)
    for label, p, kind in er.DROP_CASES:
        f = _forced(name, kind)
        fd = None if f is None else f.to(DEV)
        key = nat.dropout_key(er.SEED, er.STEP, nat.EDGE_DROP_SITE)
        if p <= 0 and f is None:
            assert nat.edge_drop_records(csr, st, key, p) is csr.rec and nat.edge_drop_records(csr, st, dkey, p) is csr.rec
            continue
        want, cinv = nat.edge_drop_records_host(host, table, key, p, f)
        got = nat.edge_drop_records(csr, st, key, p, fd)
        assert got is not csr.rec and torch.equal(got.cpu(), want), (name, label)
        assert torch.equal(st.cinv.cpu().view(torch.int32), cinv.contiguous().view(torch.int32)), (name, label)
        out = torch.full_like(csr.rec, -1)
        assert nat.edge_drop_records(csr, st, dkey, p, fd, out=out) is out and torch.equal(out.cpu(), want), (name, label)
    word.copy_(_word(nat, er.SEED, er.STEP + 1))
    want, _ = nat.edge_drop_records_host(host, table, nat.dropout_key(er.SEED, er.STEP + 1, nat.EDGE_DROP_SITE), 0.5, None)
    got = nat.edge_drop_records(csr, st, dkey, 0.5)
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(want, nat.edge_drop_records_host(host, table, nat.dropout_key(er.SEED, er.STEP, nat.EDGE_DROP_SITE), 0.5, None)[0])
    assert torch.equal(csr.rec.cpu(), host['rec'])                 # the canonical records stay as they are


def test_records_beyond_one_grid(pkg):
    """A graph whose degree launch (2 N x 8 lanes) and record launch (2 E lanes) both exceed 2048 workgroups, so both kernels
    take their strided loop, with skewed destinations (hubs of several chunks): the bits are the host twin's."""
    nat = pkg._native
    N, R, E = 40000, 3, 300001
    g = torch.Generator().manual_seed(3)
    s = torch.randint(0, N, (E,), generator=g)
    o = (torch.rand(E, generator=g) ** 3 * N).long().clamp(max=N - 1)
    r = torch.randint(0, R, (E,), generator=g)
    ei, et = torch.stack((torch.cat((s, o)), torch.cat((o, s)))), torch.cat((r, r + R))
    host = nat.csr_build_host(N, 2 * R + 1, ei, et)
    csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, DEV)
    st = csr.edge_drop_state()
    assert 2 * N * 8 > 2048 * 256 and 2 * E > 2048 * 256 and csr.num_chunks > 0 and st.max_run > 64
    f = torch.from_numpy(er.every_third(E))
    key = nat.dropout_key(5, 6, nat.EDGE_DROP_SITE)
    want, _ = nat.edge_drop_records_host(host, st.table.cpu(), key, 0.3, f)
    assert torch.equal(nat.edge_drop_records(csr, st, key, 0.3, f.to(DEV)).cpu(), want)
    # the flags at this size: a few hundred queries, one of them a hub source
    qs = (ei[0, :300] * (2 * R) + et[:300]).tolist() + (ei[0, E:E + 300] * (2 * R) + et[E:E + 300]).tolist() + [-1, N * 2 * R]
    got = nat.edge_flags_from_queries(torch.tensor(qs, device=DEV), st, E)
    want = np.zeros(E, dtype=np.uint8)
    keys = (ei[0] * (2 * R) + et).numpy()
    want[np.nonzero(np.isin(keys, np.array(qs)))[0] % E] = 1
    assert np.array_equal(got.cpu().numpy(), want) and 0 < int(want.sum()) < E


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_flags_equal_the_restatement(pkg, name):
    nat = pkg._native
    N, R, ei, et, _, _ = GRAPHS[name]
    E = ei.size(1) // 2
    _, _, csr, st = _graph(pkg, name)
    for label, qs in er.query_cases(ei, et, R, N).items():
        st.forced.fill_(1)                                        # the call zero-fills first
        got = nat.edge_flags_from_queries(torch.tensor(qs, dtype=torch.int64, device=DEV), st, E)
        assert got is st.forced and np.array_equal(got.cpu().numpy(), er.flags(ei, et, R, qs)), (name, label)


# ------------------------------------------------------------------------------------------------- forward and backward
@pytest.mark.parametrize('D', WIDTHS)
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_aggregation_on_the_view_against_float64(pkg, name, D):
    """_AggregateFn forward and backward on GraphCSR.with_records(rec') against ref_forward / ref_grads of the KEPT edge list
    (float64 norms of the kept sub-graph; a dropped edge is no term at all): aggregate_ref.check's bars as they are, exact zeros
    where the kept graph has no term, and gee of a dropped slot exactly 0."""
    nat = pkg._native
    N, R, ei, et, _, _ = GRAPHS[name]
    E = ei.size(1) // 2
    _, _, csr, st = _graph(pkg, name)
    inp = ar.make_inputs('edge_drop-%s-%d' % (name, D), N, 2 * R + 1, 2 * E, D)
    for label, p, kind in (('p05', 0.5, None), ('p02_forced', 0.2, 'third'), ('p0_node', 0.0, 'node')):
        f = _forced(name, kind)
        kept = er.kept_edges(er.SEED, er.STEP, p, E, None if f is None else f.numpy())
        assert 0 < int(kept.sum()) < E
        rec = nat.edge_drop_records(csr, st, nat.dropout_key(er.SEED, er.STEP, nat.EDGE_DROP_SITE), p, None if f is None else f.to(DEV))
        view = csr.with_records(rec)
        ei_k, et_k, ids = er.kept_list(ei, et, kept)
        x = inp.x.to(DEV).requires_grad_()
        rel = inp.rel.to(DEV).requires_grad_()
        ee = inp.ee.to(DEV).index_select(0, csr.perm).contiguous().requires_grad_()      # slot order
        out = pkg.model._AggregateFn.apply(x, rel, ee, view)
        out.backward(inp.g.to(DEV))
        what = 'edge_drop %s D%d %s' % (name, D, label)
        ar.check(out.detach().cpu(), ar.ref_forward(N, ei_k, et_k, inp.x, inp.rel, inp.ee[ids]), what + ' fwd')
        gx_ref, gee_k, grel_ref = ar.ref_grads(N, ei_k, et_k, inp.x, inp.rel, inp.ee[ids], inp.g)
        ar.check(x.grad.cpu(), gx_ref, what + ' gx')
        ar.check(rel.grad.cpu(), grel_ref, what + ' grel')
        full = torch.zeros((2 * E, D), dtype=torch.float64)
        full[ids] = gee_k.value
        gee_ref = ar.Ref(full, torch.ones_like(full), full.abs())      # a dropped edge: bar 0, so exactly 0.0
        gee = ee.grad.cpu()
        ar.check(gee, ar.select_rows(gee_ref, csr.perm.cpu()), what + ' gee')
        dropped = torch.from_numpy(~np.concatenate((kept, kept)))[csr.perm.cpu()]
        assert int(dropped.sum()) > 0 and bool((gee[dropped] == 0).all()), what      # (a product with norm +0.0f: +0.0 or -0.0)
        # the canonical graph gives something else: the view was read
        assert not torch.equal(pkg.model._AggregateFn.apply(x.detach(), rel.detach(), ee.detach(), csr), out.detach())


# ------------------------------------------------------------------------------------------------- the whole step
def _on(model, p=P_STEP, queries=True):
    model.params.edge_drop, model.params.edge_drop_queries = p, queries
    return model


def _table_step(pkg, m, dl, idx, opt, q, i):
    opt.zero_grad()
    loss = m.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=SMOOTH)
    loss.backward()
    opt.clip_and_step(CLIP)
    return loss.detach().clone()


def _list_step(pkg, m, dl, idx, opt, q, i, loss='softmax', num_neg=20):
    cand, labels = pkg.harness.draw_candidates(q, idx, m.entity_embedding.size(0), num_neg, DRAW_SEED, FIRST_STEP + i, labels=True)
    opt.zero_grad()
    out = m.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, labels=labels, lbl_smooth=SMOOTH, loss=loss)
    out.backward()
    opt.clip_and_step(CLIP)
    return out.detach().clone()


def _table_sharded(pkg, m, dl, idx, opt, q, i):
    return pkg.dist.train_step_sharded(m, dl.graph, q[:, 0], q[:, 1], idx, opt, lbl_smooth=SMOOTH, clip=CLIP).clone()


def _list_sharded(pkg, m, dl, idx, opt, q, i, loss='softmax', num_neg=20):
    cand, labels = pkg.harness.draw_candidates(q, idx, m.entity_embedding.size(0), num_neg, DRAW_SEED, FIRST_STEP + i, labels=True)
    return pkg.dist.train_step_sharded_candidates(m, dl.graph, q[:, 0], q[:, 1], cand, idx, opt, labels=labels, lbl_smooth=SMOOTH, clip=CLIP,
                                                  loss=loss).clone()


def _run(pkg, step_fn, steps=3, layers=2, on=True):
    m, dl, idx, opt = _twin(pkg, layers)
    if on:
        _on(m)
    losses = [step_fn(pkg, m, dl, idx, opt, q, i) for i, q in enumerate(_repeating_batches(dl, steps))]
    return m, opt, losses


@pytest.mark.parametrize('form', ['table', 'list'])
def test_step_repeats_and_equals_the_sharded_step_at_one_rank(pkg, form):
    """forward_loss / forward_loss_candidates with edge_drop = 0.5 and edge_drop_queries, two layers, three steps: two runs from
    one seed give the same bits; dist.train_step_sharded(_candidates) at one rank gives the same bits again; one rewrite per step;
    and the switches do change the step."""
    one, sharded = (_table_step, _table_sharded) if form == 'table' else (_list_step, _list_sharded)
    a, opt_a, la = _run(pkg, one)
    b, opt_b, lb = _run(pkg, one)
    c, opt_c, lc = _run(pkg, sharded)
    off, _, lo = _run(pkg, one, on=False)
    assert all(torch.equal(x, y) for x, y in zip(la, lb)) and all(torch.equal(x, y) for x, y in zip(la, lc))
    _assert_same_state(a, opt_a, b, opt_b)
    _assert_same_state(a, opt_a, c, opt_c)
    assert a._edge_drop_count == b._edge_drop_count == c._edge_drop_count == 3 and not hasattr(off, '_edge_drop_count')
    assert all(bool(torch.isfinite(x)) for x in la) and not any(torch.equal(x, y) for x, y in zip(la, lo))


@pytest.mark.parametrize('form', ['table', 'list'])
def test_captured_step_is_the_eager_loop(pkg, form):
    """CapturedTrainStep / CapturedCandidateStep with both switches on against the eager twin over six calls (two eager, the
    capture with its first replay, three replays), load_dropout_state between two replays included: losses, state, Adam moments
    and the dropout state, bit for bit, from ONE capture (the rewrite follows the device step word; the flags follow the batch)."""
    a, dl_a, idx_a, opt_a = _twin(pkg, 2)
    b, dl_b, idx_b, opt_b = _twin(pkg, 2)
    _on(a), _on(b)
    if form == 'table':
        step = pkg.CapturedTrainStep(a, dl_a.graph, idx_a, opt_a, lbl_smooth=SMOOTH, clip=CLIP, warmup=2)
        eager = lambda q, i: _table_step(pkg, b, dl_b, idx_b, opt_b, q, i)
    else:
        step = pkg.CapturedCandidateStep(a, dl_a.graph, idx_a, opt_a, 20, DRAW_SEED, draw_step=FIRST_STEP, loss='softmax', lbl_smooth=SMOOTH,
                                         clip=CLIP, warmup=2)
        eager = lambda q, i: _list_step(pkg, b, dl_b, idx_b, opt_b, q, i)
    for i, q in enumerate(_repeating_batches(dl_a, 6)):
        if i == 4:
            for m in (a, b):
                m.load_dropout_state({'dropout_seed': 77, 'dropout_step': 40})
        got, want = step(q[:, 0], q[:, 1]).clone(), eager(q, i)
        assert torch.equal(got, want), (i, float(got), float(want))
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 4, 2, False)
    _assert_same_state(a, opt_a, b, opt_b)
    assert a.dropout_state() == {'dropout_seed': 77, 'dropout_step': 42}
    step.model.params.edge_drop = 0.25                             # a switch is part of the capture key
    q = _repeating_batches(dl_a, 1)[0]
    b.params.edge_drop = 0.25
    assert torch.equal(step(q[:, 0], q[:, 1]).clone(), eager(q, 6)) and step.captures == 2


def test_switches_off_and_eval_mode_launch_nothing(pkg):
    """Training-mode encode with the switches absent, set to their defaults, or with edge_drop_queries on but no queries handed
    over: the same tensors, no rewrite. Eval mode with both switches on: the tensors of the model without them."""
    outs = []
    for setup in (None, (0.0, False), (0.0, True)):
        m, dl, idx, opt = _twin(pkg, 2)
        if setup is not None:
            _on(m, *setup)
        outs.append([t.detach().clone() for t in m.encode(dl.graph)])
        assert not hasattr(m, '_edge_drop_count') and not hasattr(dl.graph.csr(m.relation_embedding.size(0) + 1), '_edge_drop')
    assert all(torch.equal(x, y) for o in outs[1:] for x, y in zip(outs[0], o))
    m, dl, idx, opt = _twin(pkg, 2)
    q = _repeating_batches(dl, 1)[0]
    on = [t.detach().clone() for t in _on(m, 0.0, True).encode(dl.graph, queries=(q[:, 0], q[:, 1]))]
    assert m._edge_drop_count == 1 and not torch.equal(on[0], outs[0][0])      # own-triple removal alone changes the encoder
    evs = []
    for on in (False, True):
        m, dl, idx, opt = _twin(pkg, 2)
        if on:
            _on(m)
        m.eval()
        with torch.no_grad():
            evs.append([t.clone() for t in m.encode(dl.graph, queries=(q[:, 0], q[:, 1]))])
        assert not hasattr(m, '_edge_drop_count')
    assert all(torch.equal(x, y) for x, y in zip(*evs))


def test_refusals(pkg):
    m, dl, idx, opt = _twin(pkg, 1)
    _on(m)
    m.params.dropout = 'torch'
    q = _repeating_batches(dl, 1)[0]
    with pytest.raises(pkg._native.NativeError, match='counter'):
        m.forward_loss(q[:, 0], q[:, 1], dl.graph, idx)
    with pytest.raises(pkg._native.NativeError, match='counter'):
        pkg.dist.train_step_sharded(m, dl.graph, q[:, 0], q[:, 1], idx, opt)
    _, _, csr, st = _graph(pkg, 'type')
    with pytest.raises(pkg._native.NativeError):
        pkg._native.edge_drop_records(csr, st, 1, 0.5, out=csr.rec)
    with pytest.raises(pkg._native.NativeError):
        pkg._native.edge_drop_records(csr, st, 1, 0.5, torch.zeros(3, dtype=torch.uint8, device=DEV))
    short = copy.copy(st)
    short.table = st.table[:st.max_run].contiguous()
    with pytest.raises(pkg._native.NativeError, match='table'):
        pkg._native.edge_drop_records(csr, short, 1, 0.5)
