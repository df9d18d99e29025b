"""The list backward with split runs (include/mgcn_hip.h (18)) on a real MI355X: mgcn_cand_bce_bwd_ent_split against
the numpy-f32 emulation of tests/cand_split_ref.py bit for bit (no tolerance on the kernels) on lists built so that runs of one
piece, of exactly S, of S + 1 and of several pieces all occur, then through the model, the sharded step and the captured step.
No out-of-range plan entries and no foreign keys are handed to the GPU here: that part of the contract is held by reading."""
import pytest
import torch

from . import cand_ce_ref as E
from . import cand_split_ref as SP
from . import cand_train_ref as C
from . import dense_ref as R
from .test_gpu_cand_train import SWITCHES, _batch, _grads, _model, _recording

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPLITS, DIMS = (16, 24), (1, 200, 257)


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def inputs(cand, dim, seed):
    B, K = cand.shape
    gen = R.gen(seed)
    x = R.pm_uniform((B, dim), gen)
    g = R.randn_scaled((B, K), gen, 1.0)
    g[torch.rand((B, K), generator=gen) < 0.1] = 0.0
    g[0, 0] = -0.0
    return x, g


def reference(g, cand, x, n, S, row0=0, mixed=True, **kw):
    """The emulation on the loop-built plan; asserts that the case holds a run longer than S and one of at most S."""
    perm, n_live = C.loop_plan(cand, n, row0)
    lengths = [L for _, L, _ in SP.plan_runs(SP.plan_rows(cand, perm, n_live, n, row0))]
    assert max(lengths) > S and (not mixed or min(lengths) <= S), (S, lengths)
    return SP.emul_ent_split_f32(g, cand, x, perm, n_live, n, S, row0=row0, **kw)


def split_call(nat, g, cand, x, n, S, row0=0, count=True, **kw):
    cd = cand.to(DEV)
    perm, n_live, keys = nat.cand_plan(cd, n, row0, count=count, keys=True)
    return nat.cand_bce_bwd_ent(g.to(DEV), cd, x.to(DEV), perm, n_live, n, ent_row0=row0, run_split=S, keys=keys, **kw)


@pytest.mark.parametrize('dim', DIMS)
@pytest.mark.parametrize('S', SPLITS)
def test_split_sums_equal_the_emulation(pkg, S, dim):
    """Runs of 1, S - 1, S, S + 1, 2 S, 2 S + 1 and the neighbours S + 1, 2 S + 1 with heads in one window, -1 padding and another
    shard's ids in between; then the same call for one output alone, from the uncounted plan (its dead tail is skipped), twice,
    and on the window row0 = 5, n_local = 4."""
    nat = pkg._native
    cand = SP.split_lists(S)
    x, g = inputs(cand, dim, R.seed_of(71, S, dim))
    want = reference(g, cand, x, 12, S)
    got = split_call(nat, g, cand, x, 12, S)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    again = split_call(nat, g, cand, x, 12, S)
    assert same_bits(again[0], got[0]) and same_bits(again[1], got[1])
    only_b = split_call(nat, g, cand, x, 12, S, want=('bias',))
    only_e = split_call(nat, g, cand, x, 12, S, want=('ent',))
    assert only_b[0] is None and same_bits(only_b[1], want[1]) and only_e[1] is None and same_bits(only_e[0], want[0])
    whole = split_call(nat, g, cand, x, 12, S, count=False)
    assert same_bits(whole[0], want[0]) and same_bits(whole[1], want[1])
    want_w = reference(g, cand, x, 4, S, row0=5)
    got_w = split_call(nat, g, cand, x, 4, S, row0=5)
    assert same_bits(got_w[0], want_w[0]) and same_bits(got_w[1], want_w[1])
    assert same_bits(got_w[0], want[0][5:9]) and same_bits(got_w[1], want[1][5:9])      # a row does not see the shard it is in


@pytest.mark.parametrize('dim', [7, 257])
def test_column_window_keeps_its_sentinels(pkg, dim):
    """d_ent as a column window of a wider block and a d_bias to write into: the rows no live position names and every column
    outside the window keep the sentinel."""
    nat = pkg._native
    S = 16
    cand = SP.split_lists(S)
    x, g = inputs(cand, dim, R.seed_of(72, dim))
    wide = torch.full((12, dim + 9), 5.0, device=DEV)
    win, d_bias = wide[:, 4:4 + dim], torch.full((12,), 5.0, device=DEV)
    want = reference(g, cand, x, 12, S, d_ent=torch.full((12, dim), 5.0), d_bias=torch.full((12,), 5.0))
    got = split_call(nat, g, cand, x, 12, S, d_ent=win, d_bias=d_bias)
    assert got[0].data_ptr() == win.data_ptr() and same_bits(win, want[0]) and same_bits(d_bias, want[1])
    named = torch.zeros(12, dtype=torch.bool)
    named[list(SP.run_lengths(S))] = True
    assert bool((win.cpu()[~named] == 5.0).all()) and bool((d_bias.cpu()[~named] == 5.0).all()) and not bool((win.cpu()[named] == 5.0).any())
    probe = wide.clone()
    probe[:, 4:4 + dim] = 5.0
    assert bool((probe == 5.0).all())


def test_one_entity_named_by_every_position(pkg):
    """B = 128, K = 64, S = 16: ONE run of 8192 entries, 512 pieces folded by one wave (this case has no second run: it is the
    long fold, the built lists above hold the mixtures)."""
    nat = pkg._native
    B, K, dim, S = 128, 64, 200, 16
    cand = SP.one_id_lists(B, K, 3)
    x, g = inputs(cand, dim, 73)
    want = reference(g, cand, x, 12, S, mixed=False)
    got = split_call(nat, g, cand, x, 12, S)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert int((got[0] != 0).any(1).sum()) == 1
    unsplit = C.emul_ent_f32(g, cand, x, *C.loop_plan(cand, 12), 12)
    assert not same_bits(unsplit[0], want[0])                   # (the split order is another order)


@pytest.mark.parametrize('S', SPLITS)
def test_a_split_no_shorter_than_the_longest_run_changes_no_bit(pkg, S):
    nat = pkg._native
    cand = SP.split_lists(S)
    x, g = inputs(cand, 200, R.seed_of(74, S))
    cd = cand.to(DEV)
    perm, n_live, keys = nat.cand_plan(cd, 12, keys=True)
    plain = nat.cand_bce_bwd_ent(g.to(DEV), cd, x.to(DEV), perm, n_live, 12)
    for big in (2 * S + 1, 65536):
        got = nat.cand_bce_bwd_ent(g.to(DEV), cd, x.to(DEV), perm, n_live, 12, run_split=big, keys=keys)
        assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1])
    cut = nat.cand_bce_bwd_ent(g.to(DEV), cd, x.to(DEV), perm, n_live, 12, run_split=S, keys=keys)
    assert not same_bits(cut[0], plain[0])


@pytest.mark.parametrize('S', SPLITS)
def test_three_shards_give_the_rows_of_one(pkg, S):
    nat = pkg._native
    cand = SP.split_lists(S)
    x, g = inputs(cand, 36, R.seed_of(75, S))
    N = SP.N_SPLIT
    want = reference(g, cand, x, N, S)
    whole = split_call(nat, g, cand, x, N, S)
    assert same_bits(whole[0], want[0]) and same_bits(whole[1], want[1])
    parts = []
    for n0, n1 in SP.SHARDS:
        reference(g, cand, x, n1 - n0, S, row0=n0, mixed=False)         # (asserts a run of several pieces in this shard)
        parts.append(split_call(nat, g, cand, x, n1 - n0, S, row0=n0))
    assert same_bits(torch.cat([p[0] for p in parts]), whole[0]) and same_bits(torch.cat([p[1] for p in parts]), whole[1])


@pytest.mark.parametrize('bad', [15, 65537, 16.0])
def test_refusals_raise_before_any_launch(pkg, bad):
    nat = pkg._native
    model, dl, params = _model(pkg, 'toy_small')
    model.train()
    idx = dl.train_index().to(DEV)
    q = _batch(dl)
    cand = pkg.harness.sample_candidates(q, idx, dl.num_entity, 20, generator=torch.Generator(device=DEV).manual_seed(3))
    launched = lambda: (getattr(model, '_query_rows_count', 0), getattr(model.conv2, '_trunk_train_count', 0))
    counts = launched()
    with pytest.raises(nat.NativeError, match='run_split'):
        model.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, index=idx, run_split=bad)
    opt = pkg.ClipAdam(model.parameters(), lr=1e-3)
    with pytest.raises(nat.NativeError, match='run_split'):
        pkg.dist.train_step_sharded_candidates(model, dl.graph, q[:, 0], q[:, 1], cand, idx, opt, run_split=bad)
    with pytest.raises(nat.NativeError, match='run_split'):
        pkg.CapturedCandidateStep(model, dl.graph, idx, opt, 20, 1, run_split=bad)(q[:, 0], q[:, 1])
    assert launched() == counts and all(p.grad is None for p in model.parameters())
    x, g = inputs(cand.cpu(), 5, 76)
    perm, n_live, keys = nat.cand_plan(cand, dl.num_entity, keys=True)
    with pytest.raises(nat.NativeError, match='run_split'):
        nat.cand_bce_bwd_ent(g.to(DEV), cand, x.to(DEV), perm, n_live, dl.num_entity, run_split=bad, keys=keys)


# ---------------------------------------------------------------------------------------------------------------- the model
def bce_grad_bars(ref, x, logit_bar, inv):
    """(d_ent, d_bias) bars of the BCE list, composed as cand_ce_ref.grad_bars composes the softmax's: g's bar (dense_ref) carried
    through the sums' magnitudes, plus the f32 sums themselves, cand_train_ref.gamma of the longest run: a bound for ANY order."""
    gb = torch.where(ref['live'], R.bce_grad_bar(ref['g'], ref['p'], ref['y'], logit_bar, inv), torch.zeros_like(ref['g']))
    B, K = ref['g'].shape
    flat_row, n = ref['row'].reshape(-1), ref['d_bias'].numel()
    runs = int(torch.bincount(flat_row[ref['live'].reshape(-1)], minlength=1).max())
    per = gb.reshape(-1) + C.gamma(runs + 2) * ref['g'].abs().reshape(-1)
    xa = x.cpu().double().abs().repeat_interleave(K, 0)
    de = torch.zeros((n, x.size(1)), dtype=torch.float64).index_add_(0, flat_row, per[:, None] * xa)
    db = torch.zeros(n, dtype=torch.float64).index_add_(0, flat_row, per)
    return de, db


@pytest.mark.parametrize('kind', ['bce', 'softmax'])
def test_through_the_model(pkg, kind):
    """toy_small (7 entities, so 8 lists of 70 name every entity about 80 times: every run has several pieces at S = 16): the
    loss and d x of run_split=16 have the bits of run_split=None; every parameter gradient equals, bit for bit, the backward of
    the stage composed by hand with the split call; and that call's d ent / d bias (d bias IS conv2.bias's gradient) lie within
    the float64 bars of the list loss, which bound any summation order."""
    nat = pkg._native
    model, dl, params = _model(pkg, 'toy_small')
    model.train()
    N = dl.num_entity
    idx = dl.train_index().to(DEV)
    q = _batch(dl)
    B = q.size(0)
    src, rel = q[:, 0].contiguous(), q[:, 1].contiguous()
    cand = pkg.harness.sample_candidates(q, idx, N, 69, generator=torch.Generator(device=DEV).manual_seed(3))
    cand[0, 5], cand[1, 6], cand[2, 7] = -1, N, 2 ** 62
    assert int(torch.bincount(cand[(cand >= 0) & (cand < N)]).max()) > 16
    seen = {}
    _recording(model, seen)

    def run(split):
        model.zero_grad(set_to_none=True)
        loss = model.forward_loss_candidates(src, rel, cand, dl.graph, index=idx, lbl_smooth=0.1, loss=kind, run_split=split)
        loss.backward()
        return loss.detach().clone(), seen['x'].grad.clone(), _grads(model)

    loss0, dx0, plain = run(None)
    loss1, dx1, got = run(16)
    assert same_bits(loss0, loss1) and same_bits(dx0, dx1) and set(got) == set(plain)
    bias_name = next(n for n, p in model.named_parameters() if p is model.conv2.bias)
    assert not same_bits(got[bias_name], plain[bias_name])                    # (another order did run)
    # composed by hand
    model.zero_grad(set_to_none=True)
    all_ent, all_rel = model.encode(dl.graph)
    x = model.conv2.trunk(pkg.model.query_rows(model, all_ent, src), pkg.model.query_rows(model, all_rel, rel))
    xd, ent, bias = x.detach(), all_ent.detach().contiguous(), model.conv2.bias.detach()
    labels = nat.cand_labels(idx.query_keys(src, rel), idx.keys, idx.ptr, idx.tails, cand, N)
    if kind == 'bce':
        hot, cold = nat.smoothed_targets(0.1, N)
        loss2, g = nat.cand_bce_fwd(xd, ent, bias, cand, labels, hot, cold)
    else:
        z, units = nat.cand_ce_logits(xd, ent, bias, cand, labels)
        loss2, g, _ = nat.cand_ce_finish(z, cand, labels, nat.cand_ce_merge(units), 0.1, N)
    perm, n_live, keys = nat.cand_plan(cand, N, keys=True)
    dx = nat.cand_bce_bwd_x(g, cand, ent)
    d_ent, d_bias = nat.cand_bce_bwd_ent(g, cand, xd, perm, n_live, N, run_split=16, keys=keys)
    torch.autograd.backward([x, all_ent, model.conv2.bias], [dx, d_ent, d_bias])
    want = _grads(model)
    assert same_bits(loss1, loss2) and same_bits(dx1, dx) and set(got) == set(want)
    for name in got:
        assert same_bits(got[name], want[name]), name
    assert same_bits(got[bias_name], d_bias)
    # against float64 on the same x, ent, bias
    if kind == 'bce':
        inv = 1.0 / (B * cand.size(1))
        ref = C.ref_list_bce(xd.cpu(), ent.cpu(), bias.cpu(), cand.cpu(), labels.cpu(), hot, cold, inv)
        be, bb = bce_grad_bars(ref, xd, R.dot_bar(ref['mag'], ent.size(1)), inv)
    else:
        inv = 1.0 / B
        ref = E.ref_list_ce(xd.cpu(), ent.cpu(), bias.cpu(), cand.cpu(), labels.cpu(), 0.1, inv)
        _, rowbar = E.logit_bars(ref, ent.size(1))
        _, be, bb = E.grad_bars(ref, xd.cpu(), ent.cpu(), rowbar, inv)
    r_e = R.max_ratio(d_ent.cpu(), ref['d_ent'], be + E.F32_TINY)
    r_b = R.max_ratio(d_bias.cpu(), ref['d_bias'], bb + E.F32_TINY)
    print('RATIO cand_split_model %s d_ent %.4f d_bias %.4f' % (kind, r_e, r_b))
    assert r_e <= 1.0 and r_b <= 1.0


def test_one_rank_of_the_sharded_step_equals_the_one_gpu_step(pkg):
    """train_step_sharded_candidates with one rank against forward_loss_candidates + backward + clip + Adam, both with
    run_split=16, two steps from the same state on lists of 2049 over syn_b's 483 entities: losses and state bit for bit."""
    from .test_gpu_cand_sharded import _same_state
    from .test_gpu_train_sharded import _batches, _models
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the trunk's index_select backward: no float atomics)
    try:
        ref, dl, params = _models(pkg, 'syn_b', 1)
        sm, dl_s, _ = _models(pkg, 'syn_b', 1)
        idx = dl.train_index().to(DEV)
        opt_r, opt_s = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.optim.Adam(sm.parameters(), lr=1e-3)
        for step, q in enumerate(_batches(dl, 2)):
            cand, labels = pkg.harness.draw_candidates(q, idx, dl.num_entity, 2048, 77, step, labels=True)
            assert int(torch.bincount(cand.reshape(-1)).max()) > 16
            opt_r.zero_grad()
            loss_r = ref.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, index=idx, lbl_smooth=0.1, run_split=16)
            loss_r.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
            opt_r.step()
            loss_s = pkg.dist.train_step_sharded_candidates(sm, dl_s.graph, q[:, 0], q[:, 1], cand, idx, opt_s, labels=labels,
                                                            lbl_smooth=0.1, clip=0.5, run_split=16)
            assert torch.equal(loss_s, loss_r.detach()) and bool(torch.isfinite(loss_s))
    finally:
        torch.use_deterministic_algorithms(False)
    _same_state(ref, sm, 1, False)


@pytest.mark.parametrize('kind', ['bce', 'softmax'])
def test_captured_step_with_a_split_equals_the_eager_loop(pkg, kind):
    """CapturedCandidateStep(run_split=16), warmup=1: one eager step, the capture with its first replay, one more replay, against
    three eager steps of a twin on lists of 1025 (16 400 positions over syn_b's 483 entities): losses, parameters, Adam state. Changing run_split re-captures."""
    from .test_gpu_cand_captured import FIRST_STEP, SEED
    from .test_gpu_captured_step import CLIP, SMOOTH, _assert_same_state, _twin
    from .test_gpu_query_train import _repeating_batches
    a, dl_a, idx_a, opt_a = _twin(pkg, 1)
    b, dl_b, idx_b, opt_b = _twin(pkg, 1)
    step = pkg.CapturedCandidateStep(a, dl_a.graph, idx_a, opt_a, 1024, SEED, draw_step=FIRST_STEP, loss=kind, lbl_smooth=SMOOTH, clip=CLIP,
                                     warmup=1, run_split=16)
    batches = _repeating_batches(dl_a, 4)
    for i, q in enumerate(batches[:3]):
        got = step(q[:, 0], q[:, 1]).clone()
        cand, labels = pkg.harness.draw_candidates(q, idx_b, b.entity_embedding.size(0), 1024, SEED, FIRST_STEP + i, labels=True)
        assert int(torch.bincount(cand.reshape(-1)).max()) > 16
        opt_b.zero_grad()
        want = b.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl_b.graph, labels=labels, lbl_smooth=SMOOTH, loss=kind, run_split=16)
        want.backward()
        opt_b.clip_and_step(CLIP)
        assert torch.equal(got, want.detach()), (i, float(got), float(want))
        assert torch.equal(step.cand, cand)
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 2, 1, False)
    _assert_same_state(a, opt_a, b, opt_b)
    step.run_split = 32                                # held by value in the graph: another value is another capture
    step(batches[3][:, 0], batches[3][:, 1])
    assert step.captures == 2 and not step.disabled
