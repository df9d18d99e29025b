"""The weighted candidate draw and the softmax's logQ term (include/mgcn_hip.h (17)) on a real MI355X (`-m gpu`):

  * mgcn_cand_draw_alias against its host twin (which tests/test_cand_alias_host.py holds to the Python-integer definition), the
    equal-weights table against mgcn_cand_draw, the _dev form against the by-value form, one captured _dev draw under two words;
  * forward_loss_candidates(loss='softmax', logq=...) against the float64 reference of tests/cand_ce_ref.py given the same f32
    bias - logq, within that module's bars; logq = 0 against the call without logq, bit for bit; 'bce' refuses logq;
  * the steps: eager against captured, the sharded step at one rank, three shards of the scoring stage in one process, two gloo
    processes that draw their own lists from a broadcast sampler; the uniform sampler against no sampler, bit for bit.
Integers, or reproducible float paths: the comparisons are torch.equal except where a float64 reference or a second process is
involved."""
import os

import numpy as np
import pytest
import torch

from . import cand_alias_ref as A
from . import cand_ce_ref as E
from . import cand_draw_ref as R
from . import cand_train_ref as C
from . import dense_ref as D
from .test_gpu_cand_ce import _same_state, check_against_float64, forward, same_bits
from .test_gpu_captured_step import CLIP, SMOOTH, SWITCHES, _assert_same_state, _twin, _word
from .test_gpu_query_train import DEV, _repeating_batches
from .test_gpu_train_sharded import _PORTS, _assemble, _batches, _models, _np

pytestmark = pytest.mark.gpu
GRID_N, GRID_B, GRID_K = (1, 2, 5, 4097), (1, 3, 130), (1, 2, 3, 65, 130)
WEIGHTS = {1: [3], 2: [1, 2 ** 32 - 1], 5: [3, 0, 7, 1, 9], 4097: A.zipf_weights(4097)}


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES + ('MGCN_EE',):
        monkeypatch.delenv(name, raising=False)


def _on(dev, *ts):
    return [t.to(dev) for t in ts]


@pytest.fixture(scope='module')
def host_blocks(pkg):
    """N -> (table on the CPU, host twin's (cand, label) at the largest (B, K), key, row0): computed once, shared, never changed."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    out = {}
    for i, N in enumerate(GRID_N):
        table = pkg.NegativeSampler.from_weights(torch.tensor(WEIGHTS[N], dtype=torch.int64)).table
        k, row0 = R.key(1234, 5 + i), (0, 3, 2 ** 32 + 5, 2 ** 40 - 1)[i]
        want = nat.cand_draw_host(R.grid_queries(max(GRID_B)), keys, ptr, tails, N, max(GRID_K), k, row0=row0, table=table)
        out[N] = (table, want, k, row0)
    return out


# ------------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize('N', GRID_N)
def test_kernel_equals_host_twin(pkg, host_blocks, N):
    """Every (B, K) of the grid is a corner of the host twin's largest block; written into padded windows of poisoned buffers,
    with and without labels."""
    nat = pkg._native
    table, (want_c, want_l), k, row0 = host_blocks[N]
    dkeys, dptr, dtails = _on(DEV, *R.grid_index())
    dq, dt = R.grid_queries(max(GRID_B)).to(DEV), table.to(DEV)
    want_c, want_l = want_c.to(DEV), want_l.to(DEV)
    for B in GRID_B:
        for K in GRID_K:
            cbuf = torch.full((B, K + 3), -77, dtype=torch.int64, device=DEV)
            lbuf = torch.full((B, K + 5), 77, dtype=torch.uint8, device=DEV)
            cand, label = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, k, row0=row0, table=dt, out=(cbuf[:, :K], lbuf[:, :K]))
            assert torch.equal(cand, want_c[:B, :K]) and torch.equal(label, want_l[:B, :K]), (N, B, K)
            assert bool((cbuf[:, K:] == -77).all()) and bool((lbuf[:, K:] == 77).all()), (N, B, K)
            only, none = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, k, row0=row0, labels=False, table=dt)
            assert none is None and torch.equal(only, cand)
    if N > 1:
        assert int(want_c[:, 1:].min()) >= 0 and int(want_c[:, 1:].max()) < N


@pytest.mark.parametrize('N', GRID_N)
def test_equal_weights_table_gives_the_uniform_draw(pkg, N):
    nat = pkg._native
    dkeys, dptr, dtails = _on(DEV, *R.grid_index())
    dq = R.grid_queries(130).to(DEV)
    s = pkg.NegativeSampler.uniform(N).to(DEV)
    assert s.table.is_cuda and s.logq.is_cuda and s.to(DEV) is s and not bool(s.logq.view(torch.int32).any())
    for K in GRID_K:
        k = R.key(9, K)
        got = nat.cand_draw(dq, dkeys, dptr, dtails, N, K, k, row0=2 ** 32 + 5, table=s.table)
        want = nat.cand_draw(dq, dkeys, dptr, dtails, N, K, k, row0=2 ** 32 + 5)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (N, K)


@pytest.mark.parametrize('N', GRID_N)
def test_device_key_form_equals_the_by_value_form(pkg, host_blocks, N):
    nat = pkg._native
    dkeys, dptr, dtails = _on(DEV, *R.grid_index())
    dq, dt = R.grid_queries(130).to(DEV), host_blocks[N][0].to(DEV)
    for seed, step in ((1234, 5), (2 ** 63, 2 ** 32), (2 ** 64 - 1, 2 ** 64 - 1)):
        dk = nat.DeviceKey(_word(nat, seed, step), nat.CAND_DRAW_SITE)
        key = nat.dropout_key(seed, step, nat.CAND_DRAW_SITE)
        for B, K in ((1, 1), (3, 2), (130, 3), (3, 65), (130, 130)):
            got = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, dk, row0=3, table=dt)
            want = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, key, row0=3, table=dt)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (N, B, K, seed)


def test_a_captured_draw_follows_the_word(pkg, host_blocks):
    """ONE mgcn_cand_draw_alias_dev captured in a graph, launched twice with two different words written in between: the two
    eager by-value draws."""
    nat = pkg._native
    N, B, K = 4097, 130, 65
    dkeys, dptr, dtails = _on(DEV, *R.grid_index())
    dq, dt = R.grid_queries(B).to(DEV), host_blocks[N][0].to(DEV)
    pairs = ((7, 2 ** 32 - 1), (7, 2 ** 32))
    word = _word(nat, 1, 1)
    dk = nat.DeviceKey(word, nat.CAND_DRAW_SITE)
    cbuf = torch.full((B, K), -77, dtype=torch.int64, device=DEV)
    lbuf = torch.full((B, K), 77, dtype=torch.uint8, device=DEV)
    nat.cand_draw(dq, dkeys, dptr, dtails, N, K, dk, row0=3, table=dt)            # (the kernel is loaded ahead of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nat.cand_draw(dq, dkeys, dptr, dtails, N, K, dk, row0=3, table=dt, out=(cbuf, lbuf))
    seen = []
    for pair in pairs:
        word.copy_(_word(nat, *pair))
        graph.replay()
        want = nat.cand_draw(dq, dkeys, dptr, dtails, N, K, nat.dropout_key(pair[0], pair[1], nat.CAND_DRAW_SITE), row0=3, table=dt)
        assert torch.equal(cbuf, want[0]) and torch.equal(lbuf, want[1]), pair
        seen.append(cbuf.clone())
    assert not torch.equal(seen[0], seen[1])


def test_corrupt_table_writes_dead_positions_only(pkg):
    """The table of tests/test_cand_alias_host.py's corrupt case: the kernel writes what the host twin writes, and every written
    id is -1 or inside [0, N)."""
    nat = pkg._native
    N = 7
    table = A.table_tensor([3 << 32, N << 32, A.M64 & (-1 << 32), (2 ** 31) << 32, 0 << 32, 6 << 32, (N + 1) << 32 | 0x80000000])
    keys, ptr, tails = R.grid_index()
    q, k = R.grid_queries(67), R.key(5, 6)
    want = nat.cand_draw_host(q, keys, ptr, tails, N, 65, k, table=table)
    got = nat.cand_draw(q.to(DEV), *_on(DEV, keys, ptr, tails), N, 65, k, table=table.to(DEV))
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    neg = got[0][:, 1:]
    assert bool(((neg == -1) | ((neg >= 0) & (neg < N))).all()) and int((neg == -1).sum()) > 0


def test_wrapper_refusals_write_nothing(pkg):
    nat = pkg._native
    dkeys, dptr, dtails = _on(DEV, *R.grid_index())
    q = R.grid_queries(4).to(DEV)
    table = pkg.NegativeSampler.uniform(7).table
    cbuf = torch.full((4, 8), -77, dtype=torch.int64, device=DEV)
    for bad in (table, table.to(DEV)[:6], table.to(DEV).int(), torch.zeros((7, 2), dtype=torch.int64, device=DEV)[:, 0]):
        with pytest.raises(nat.NativeError):
            nat.cand_draw(q, dkeys, dptr, dtails, 7, 8, 1, table=bad, out=cbuf, labels=False)
    with pytest.raises(nat.NativeError, match='sampler holds'):
        pkg.harness.draw_candidates(torch.zeros((4, 2), dtype=torch.int64, device=DEV), None, 7, 7, 1, 1, sampler=pkg.NegativeSampler.uniform(7))
    torch.cuda.synchronize()
    assert bool((cbuf == -77).all())


# ------------------------------------------------------------------------------------------------- the loss
N_ENT = 97


def _stub(model, x, ent, bias):
    """model.encode / model.conv2.trunk / model.conv2.bias replaced by leaves of the test's own shape: forward_loss_candidates
    itself runs, on a scoring stage of any dim."""
    rel = torch.zeros((1, ent.size(1)), device=DEV)
    model.encode = lambda data: (ent, rel)
    model.conv2.trunk = lambda a, b: x
    model.conv2.bias = torch.nn.Parameter(bias)


LOSS_GRID = [(dim, K) for dim in (4, 200) for K in (1, 65, 257)]


@pytest.mark.parametrize('dim,K', LOSS_GRID, ids=['%d-%d' % c for c in LOSS_GRID])
def test_softmax_with_logq_against_float64(pkg, dim, K):
    """forward_loss_candidates(loss='softmax', logq=...) on lists with -1 and out-of-table ids (cand_ce_ref.DEAD) and the planted
    edge rows: loss and the gradients of x, all_ent and bias against cand_ce_ref.ref_list_ce given the SAME f32 bias - logq as
    its bias, within that module's bars (d bias passes straight through the subtraction). Then logq = 0 against no logq."""
    nat = pkg._native
    B, eps = 8, 0.1
    model, dl, params = _models(pkg, 'syn_b')
    model.train()
    x, ent, bias, cand, label = E.problem(B, K, N_ENT, dim, D.seed_of(171, dim, K))
    sampler = pkg.NegativeSampler.from_weights(torch.tensor(A.zipf_weights(N_ENT, scale=1 << 12)))
    logq = sampler.logq
    assert float(logq.max()) > 1.0 and float(logq.min()) < -1.0
    xd, ed = x.to(DEV).requires_grad_(True), ent.to(DEV).requires_grad_(True)
    _stub(model, xd, ed, bias.to(DEV))
    src = rel = torch.zeros(B, dtype=torch.int64, device=DEV)
    dcand, dlabel = cand.to(DEV), label.to(DEV)

    def run(**kw):
        for t in (xd, ed, model.conv2.bias):
            t.grad = None
        loss = model.forward_loss_candidates(src, rel, dcand, dl.graph, labels=dlabel, lbl_smooth=eps, loss='softmax', **kw)
        loss.backward()
        return loss.detach(), xd.grad.clone(), ed.grad.clone(), model.conv2.bias.grad.clone()

    loss, dx, d_ent, d_bias = run(logq=sampler.to(DEV).logq)
    eff = bias - logq                                            # one f32 subtraction: the bits the device forms
    assert same_bits((model.conv2.bias.detach() - logq.to(DEV)), eff)
    inv = 1.0 / B
    ref = E.ref_list_ce(x, ent, eff, cand, label, eps, inv)
    zbar, rowbar = E.logit_bars(ref, dim)
    lbar = E.loss_bar(ref, rowbar, inv, B * ((K + 63) // 64))
    r_loss = abs(float(loss) - ref['loss']) / lbar if lbar else abs(float(loss) - ref['loss'])
    bx, be, bb = E.grad_bars(ref, x, ent, rowbar, inv)
    r_x = D.max_ratio(dx.cpu(), ref['dx'], bx + E.F32_TINY)
    r_e = D.max_ratio(d_ent.cpu(), ref['d_ent'], be + E.F32_TINY)
    r_b = D.max_ratio(d_bias.cpu(), ref['d_bias'], bb + E.F32_TINY)
    print('RATIO cand_alias_logq %d-%d loss %.4f dx %.4f d_ent %.4f d_bias %.4f' % (dim, K, r_loss, r_x, r_e, r_b))
    assert r_loss <= 1.0 and r_x <= 1.0 and r_e <= 1.0 and r_b <= 1.0
    if K > 1:
        plain = E.ref_list_ce(x, ent, bias, cand, label, eps, inv)
        assert abs(plain['loss'] - ref['loss']) > 100 * lbar       # the correction is far above the bars: the test can see it
    zero = run(logq=torch.zeros(N_ENT, device=DEV))
    none = run()
    for a, b in zip(zero, none):
        assert same_bits(a, b)
    with pytest.raises(nat.NativeError, match='softmax only'):
        model.forward_loss_candidates(src, rel, dcand, dl.graph, labels=dlabel, loss='bce', logq=sampler.to(DEV).logq)
    for bad in (logq, logq.to(DEV)[:-1], logq.to(DEV).double()):
        with pytest.raises(nat.NativeError, match='logq must be'):
            model.forward_loss_candidates(src, rel, dcand, dl.graph, labels=dlabel, loss='softmax', logq=bad)


@pytest.mark.parametrize('dim', [36, 200])
def test_three_shards_of_the_scoring_stage_with_logq(pkg, dim):
    """Rows [0, a), [a, a) (empty) and [a, N) as tests/test_gpu_cand_ce.py plays them, each shard with bias[n0:n1] - logq[n0:n1]:
    the slices of the whole subtraction bit for bit; the counts are exact, the shards' g blocks are disjoint and add up to the
    whole launch's g, the losses add up, all within cand_ce_ref's bars against float64 on the same f32 bias - logq."""
    nat = pkg._native
    B, K, a, inv, eps = 8, 130, 37, 1.0 / 8, 0.1
    x, ent, bias, cand, label = E.problem(B, K, N_ENT, dim, D.seed_of(172, dim))
    cand[0, 3], cand[0, 4] = a - 1, a
    logq = pkg.NegativeSampler.from_weights(torch.tensor(A.zipf_weights(N_ENT, scale=1 << 12))).logq
    eff = bias - logq
    ref = E.ref_list_ce(x, ent, eff, cand, label, eps, inv)
    xd, ed, bd, cd, ld_, lq = (t.to(DEV) for t in (x, ent, bias, cand, label, logq))
    whole = forward(nat, xd, ed, bd - lq, cd, ld_, eps, inv)
    rowbar = check_against_float64(nat, whole, ref, dim, inv, 'alias-shard-whole-%d' % dim)
    bounds = [0, a, a, N_ENT]
    stats, zs = [], []
    for r in range(3):
        n0, n1 = bounds[r], bounds[r + 1]
        b_r = bd[n0:n1] - lq[n0:n1]
        assert same_bits(b_r, (bd - lq)[n0:n1])
        z, units = nat.cand_ce_logits(xd, ed[n0:n1], b_r, cd, ld_, ent_row0=n0)
        zs.append(z)
        stats.append(nat.cand_ce_merge(units))
    glob = nat.cand_ce_merge(torch.stack(stats).contiguous(), part_dim=0)
    m, s, nl, npos = (t.cpu() for t in nat.cand_ce_stat_fields(glob))
    assert torch.equal(nl.long(), ref['n_live']) and torch.equal(npos.long(), ref['n_pos'])
    assert same_bits(m, nat.cand_ce_stat_fields(whole['stat'])[0])
    g_sum, loss_sum = torch.zeros((B, K), device=DEV), 0.0
    seen = torch.zeros((B, K), dtype=torch.int64)
    for r in range(3):
        n0, n1 = bounds[r], bounds[r + 1]
        live, _ = C.live_rows(cand, n0, n1 - n0)
        seen += live.long()
        loss_r, g_r, _ = nat.cand_ce_finish(zs[r], cd, ld_, glob, eps, n1 - n0, ent_row0=n0)
        assert not bool(g_r.cpu()[~live].any()), r
        g_sum, loss_sum = g_sum + g_r, loss_sum + float(loss_r)
    assert torch.equal(seen, ref['live'].long())
    gbar = E.g_bar(ref, rowbar, inv)
    lbar = E.loss_bar(ref, rowbar, inv, whole['parts'].numel())
    r_g, r_g64 = D.max_ratio(g_sum.cpu(), whole['g'].cpu().double(), gbar), D.max_ratio(g_sum.cpu(), ref['g'], gbar)
    r_l, r_l64 = abs(loss_sum - float(whole['loss'])) / lbar, abs(loss_sum - ref['loss']) / lbar
    print('RATIO cand_alias_shards dim=%d g %.4f g64 %.4f loss %.4f loss64 %.4f' % (dim, r_g, r_g64, r_l, r_l64))
    assert r_g <= 1.0 and r_g64 <= 1.0 and r_l <= 1.0 and r_l64 <= 1.0


# ------------------------------------------------------------------------------------------------- the steps
SEED, NEG = 99, 9


def _sampler(pkg, dl, idx, which):
    n = dl.num_entity
    if which == 'uniform':
        return pkg.NegativeSampler.uniform(n).to(DEV)
    s = pkg.NegativeSampler.from_degrees(index=idx, num_entities=n).to(DEV)
    assert float(s.logq.max()) > 0.1 and float(s.logq.min()) < -0.1          # the training index of the fixture is skewed
    return s


@pytest.mark.parametrize('which', ['weighted', 'uniform'])
@pytest.mark.parametrize('loss', ['bce', 'softmax'])
def test_eager_and_captured_epochs_agree(pkg, loss, which):
    """One layer, every HIP switch on, counter dropout 0.3, ClipAdam: three one-step epochs of
    harness.train_sampled_negatives(sampler=s, draw_seed=...) with captured=True (two eager warm-up steps, then the capture and
    its replay) against the default loop on a twin: every loss, the lists, every parameter, Adam moment and the dropout state
    bit for bit. With the uniform sampler, a third twin trained WITHOUT a sampler agrees as well."""
    twins = [_twin(pkg) for _ in range(3 if which == 'uniform' else 2)]
    samplers = []
    for m, dl, idx, opt in twins:
        m.params.lbl_smooth, m.params.clip_grad = SMOOTH, CLIP
        samplers.append(_sampler(pkg, dl, idx, which))
    samplers[2:] = [None] * (len(twins) - 2)
    batches = _repeating_batches(twins[0][1], 3)
    for i, q in enumerate(batches):
        losses = []
        for t, ((m, dl, idx, opt), s) in enumerate(zip(twins, samplers)):
            losses.append(pkg.harness.train_sampled_negatives(m, q, idx, dl.graph, opt, m.params, 16, NEG, generator=torch.Generator().manual_seed(i),
                                                              draw_seed=SEED, first_step=2 ** 32 - 2 + i, loss=loss, sampler=s,
                                                              captured=True if t == 0 else None))
        assert all(v == losses[0] for v in losses) and np.isfinite(losses[0]), (i, losses)
        order = torch.randperm(16, generator=torch.Generator().manual_seed(i)).to(DEV)
        want = pkg.harness.draw_candidates(q.index_select(0, order), twins[0][2], twins[0][1].num_entity, NEG, SEED, 2 ** 32 - 2 + i,
                                           sampler=samplers[0])
        assert torch.equal(twins[0][0]._captured_cand_train_step.cand, want), i
    step = twins[0][0]._captured_cand_train_step
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 1, 2, False) and step.sampler is samplers[0]
    for m, dl, idx, opt in twins[1:]:
        _assert_same_state(twins[0][0], twins[0][3], m, opt)
    if which == 'weighted':
        plain = pkg.harness.draw_candidates(batches[0], twins[0][2], twins[0][1].num_entity, NEG, SEED, 0)
        assert not torch.equal(plain, pkg.harness.draw_candidates(batches[0], twins[0][2], twins[0][1].num_entity, NEG, SEED, 0, sampler=samplers[0]))


def test_another_sampler_recaptures_and_the_generator_route_refuses(pkg):
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    s1, s2 = _sampler(pkg, dl_a, idx_a, 'weighted'), _sampler(pkg, dl_a, idx_a, 'uniform')
    step = pkg.CapturedCandidateStep(a, dl_a.graph, idx_a, opt_a, NEG, SEED, loss='softmax', lbl_smooth=SMOOTH, clip=CLIP, sampler=s1)
    for i, q in enumerate(_repeating_batches(dl_a, 5)):
        s = s1 if i < 4 else s2
        step.sampler = s
        got = step(q[:, 0], q[:, 1]).clone()
        cand, labels = pkg.harness.draw_candidates(q, idx_b, dl_b.num_entity, NEG, SEED, i, labels=True, sampler=s)
        opt_b.zero_grad()
        want = b.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl_b.graph, labels=labels, lbl_smooth=SMOOTH, loss='softmax', logq=s.logq)
        want.backward()
        opt_b.clip_and_step(CLIP)
        assert torch.equal(got, want.detach()) and torch.equal(step.cand, cand), i
    assert (step.captures, step.replays, step.eager_steps) == (2, 3, 2)
    _assert_same_state(a, opt_a, b, opt_b)
    nat = pkg._native
    with pytest.raises(nat.NativeError, match='draw_seed'):
        pkg.harness.train_sampled_negatives(a, q, idx_a, dl_a.graph, opt_a, a.params, 16, NEG, sampler=s1)
    step.sampler = pkg.NegativeSampler.uniform(dl_a.num_entity)               # on the CPU
    with pytest.raises(nat.NativeError, match='sampler must hold'):
        step(q[:, 0], q[:, 1])


@pytest.mark.parametrize('which', ['weighted', 'uniform'])
def test_world1_sharded_step_equals_one_gpu_step(pkg, monkeypatch, which):
    """dist.train_step_sharded_candidates(loss='softmax', logq=...) with one rank against forward_loss_candidates + backward +
    ClipAdam.clip_and_step at counter dropout 0.3 with the HIP trunk and query path: 3 steps, every loss, parameter, BN statistic
    and Adam moment bit for bit. With the uniform sampler, the sharded step WITHOUT logq on lists drawn WITHOUT a table agrees."""
    monkeypatch.setenv('MGCN_DROPOUT', 'counter')
    monkeypatch.setenv('MGCN_TRUNK_TRAIN', 'hip')
    monkeypatch.setenv('MGCN_QUERY_TRAIN', 'hip')
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        built = [_models(pkg, 'syn_b', 1, dropout=0.3) for _ in range(3 if which == 'uniform' else 2)]
        for m, _, _ in built:
            m.conv1.drop.p = 0.3
            m.train()
        (ref, dl, _), (sm, dl_s, _) = built[:2]
        idx = dl.train_index().to(DEV)
        s = _sampler(pkg, dl, idx, which)
        opts = [pkg.optim.ClipAdam(m.parameters(), lr=1e-3) for m, _, _ in built]
        for step, q in enumerate(_batches(dl, 3)):
            cand, labels = pkg.harness.draw_candidates(q, idx, dl.num_entity, NEG, SEED, step, labels=True, sampler=s)
            opts[0].zero_grad()
            loss_r = ref.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, labels=labels, lbl_smooth=0.1, loss='softmax', logq=s.logq)
            loss_r.backward()
            opts[0].clip_and_step(0.5)
            loss_s = pkg.dist.train_step_sharded_candidates(sm, dl_s.graph, q[:, 0], q[:, 1], cand, idx, opts[1], labels=labels,
                                                            lbl_smooth=0.1, clip=0.5, loss='softmax', logq=s.logq)
            assert torch.equal(loss_s, loss_r.detach()) and bool(torch.isfinite(loss_s)) and float(loss_s) > 0
            if which == 'uniform':
                c2, l2 = pkg.harness.draw_candidates(q, idx, dl.num_entity, NEG, SEED, step, labels=True)
                assert torch.equal(c2, cand) and torch.equal(l2, labels)
                loss_p = pkg.dist.train_step_sharded_candidates(built[2][0], built[2][1].graph, q[:, 0], q[:, 1], c2, idx, opts[2], labels=l2,
                                                                lbl_smooth=0.1, clip=0.5, loss='softmax')
                assert torch.equal(loss_p, loss_s)
        with pytest.raises(pkg._native.NativeError, match='softmax only'):
            pkg.dist.train_step_sharded_candidates(sm, dl_s.graph, q[:, 0], q[:, 1], cand, idx, opts[1], labels=labels, loss='bce', logq=s.logq)
    finally:
        torch.use_deterministic_algorithms(False)
    for (m, _, _), opt in zip(built[1:], opts[1:]):
        _same_state(ref, m, 1, False, opts[0], opt)


# -- two processes on one GPU over gloo -------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, q):
    try:
        _gloo_worker_body(rank, world, port, q)
    except Exception:                                        # surface the failure in the parent instead of a timeout
        import traceback
        q.put((rank, {'error': traceback.format_exc()}))


def _gloo_worker_body(rank, world, port, q):
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    pkg = importlib.import_module('kgc-gcn_amd')
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    out = {}
    runs = {}
    for name in ('weighted', 'uniform', 'none'):
        sm, dl, params = _models(pkg, 'syn_b', 1, 0.0, shard=True, world=world, rank=rank)
        idx = dl.train_index().to(DEV)
        mine = None
        if rank == 0 and name != 'none':                     # only rank 0 builds a table; rank 1 takes what it is sent
            mine = pkg.NegativeSampler.from_degrees(index=idx, num_entities=dl.num_entity) if name == 'weighted' else \
                pkg.NegativeSampler.uniform(dl.num_entity)
        s = pkg.dist.broadcast_sampler(mine, device=torch.device(DEV)) if name != 'none' else None
        opt = torch.optim.Adam(sm.parameters(), lr=1e-3)
        b = _batches(dl, 1)[0]
        cand, labels = pkg.harness.draw_candidates(b, idx, dl.num_entity, 8, 77, 0, labels=True, sampler=s)     # this rank's own draw
        loss = float(pkg.dist.train_step_sharded_candidates(sm, dl.graph, b[:, 0], b[:, 1], cand, idx, opt, labels=labels, loss='softmax',
                                                            logq=None if s is None else s.logq))
        csr, n0, n1 = sm._edge_shard
        counts, sub = csr.shard_slot_counts(n0, n1), csr.shard_ee_sub(n0, n1)
        slots = (torch.arange(sum(counts)) + torch.tensor(sub).repeat_interleave(torch.tensor(counts))).to(DEV)
        tables = {n: p for n, p in sm._edge_tables()}
        runs[name] = dict(losses=[loss], cand=_np(cand), rows=(n0, n1), ref_ids=_np(csr.perm.index_select(0, slots)),
                          table=None if s is None else _np(s.table),
                          grads={n: _np(p.grad) for n, p in sm.named_parameters() if p.grad is not None},
                          state={k: _np(v) for k, v in sm.state_dict().items() if k not in tables},
                          tables={n: _np(t) for n, t in tables.items()})
    u, p = runs['uniform'], runs['none']                     # the uniform sampler against no sampler: this rank's bits
    differ = [k for k in ('losses',) if u[k] != p[k]] + [k for k in ('cand',) if not np.array_equal(u[k], p[k])]
    differ += ['%s.%s' % (k, n) for k in ('grads', 'state', 'tables') for n in set(u[k]) | set(p[k])
               if n not in u[k] or n not in p[k] or not np.array_equal(u[k][n], p[k][n])]
    out['uniform_differs_from_none'] = sorted(differ)
    out['weighted'] = runs['weighted']
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_draw_from_a_broadcast_sampler_and_match_the_single_step(pkg):
    """Two processes over gloo (both on one GPU), one softmax step of the 1-layer syn_b at dropout 0: rank 0 builds the sampler,
    broadcast_sampler hands rank 1 the table, each rank draws its own lists and subtracts its slice of logq. Held to the
    one-process step at the bars of tests/test_gpu_cand_sharded.py: loss 1e-5, gradients rtol 2e-3 / atol 2e-5 of the tensor's
    largest entry (+ floor), replicated gradients and state bit-identical on the two ranks, table rows after the step 1e-5. On
    each rank the step with the uniform sampler has the bits of the step without one."""
    import torch.multiprocessing as mp
    _PORTS[0] += 1
    world, port = 2, 31700 + (os.getpid() * 7 + 50 * _PORTS[0]) % 2000
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, queue)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(queue.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        assert 'error' not in got[r], got[r]['error']
        assert got[r]['uniform_differs_from_none'] == [], r
    name = 'weighted'
    ref, dl, params = _models(pkg, 'syn_b', 1)
    idx = dl.train_index().to(DEV)
    s = pkg.NegativeSampler.from_degrees(index=idx, num_entities=dl.num_entity).to(DEV)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    b = _batches(dl, 1)[0]
    cand, labels = pkg.harness.draw_candidates(b, idx, dl.num_entity, 8, 77, 0, labels=True, sampler=s)
    for r in (0, 1):
        assert np.array_equal(got[r][name]['table'], _np(s.table)), r
        assert np.array_equal(got[r][name]['cand'], _np(cand)), r
    n0, n1 = got[0][name]['rows']
    assert n0 == 0 and 0 < n1 < dl.num_entity and got[1][name]['rows'] == (n1, dl.num_entity)
    own = ((cand >= n0) & (cand < n1)).sum().item()
    assert 0 < own < cand.numel()
    opt.zero_grad()
    loss = ref.forward_loss_candidates(b[:, 0], b[:, 1], cand, dl.graph, labels=labels, lbl_smooth=0.0, loss='softmax', logq=s.logq)
    loss.backward()
    assert float(loss.detach()) > 0
    want_grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}
    opt.step()
    inv = ref._slot_csr.inv_perm
    for n in want_grads:
        if n.startswith('edge_embeddings'):
            want_grads[n] = want_grads[n].index_select(0, inv)   # slot order -> reference order
    for r in (0, 1):
        assert abs(got[r][name]['losses'][0] - float(loss.detach())) < 1e-5, r
    tgrads = _assemble(got, name, 'grads')
    for n, want in want_grads.items():
        gr = tgrads[n] if n.startswith('edge_embeddings') else got[0][name]['grads'][n]
        if not n.startswith('edge_embeddings'):
            assert np.array_equal(got[0][name]['grads'][n], got[1][name]['grads'][n]), n
        ref_g = want.cpu()
        scale = float(ref_g.abs().max()) + 1e-12
        floor = 2e-6 if n.startswith('conv2.') else 1e-9
        np.testing.assert_allclose(gr, ref_g.numpy(), rtol=2e-3, atol=2e-5 * scale + floor, err_msg=n)
    for k, v in got[0][name]['state'].items():
        assert np.array_equal(v, got[1][name]['state'][k]), k
    ref_sd = ref.state_dict()
    for tname, t in _assemble(got, name, 'tables').items():
        np.testing.assert_allclose(t, ref_sd[tname].cpu().numpy(), rtol=0, atol=1e-5, err_msg=tname)
