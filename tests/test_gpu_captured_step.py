"""The captured training step (kgc-gcn_amd/captured.py) on a real MI355X (`-m gpu`): the device-scalar forms of the
dropout and Adam kernels bit for bit against their by-value forms, and CapturedTrainStep against an eager twin built from the
same golden state (case syn_b, B = 16, the builders and switches of test_gpu_query_train): bit-identical where the eager step is
reproducible, within the eager step's own run-to-run spread where it is not."""
import copy

import pytest
import torch

from .conftest import golden
from .test_gpu_query_train import DEV, _fresh, _repeating_batches

pytestmark = pytest.mark.gpu
SWITCHES = ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN', 'MGCN_TRUNK', 'MGCN_DROPOUT', 'MGCN_TRAIN_TORCH')
M64 = (1 << 64) - 1
CLIP, SMOOTH = 0.5, 0.1
EAGER_RUNS = 6          # eager runs whose largest pairwise difference is the yardstick of the torch-trunk test


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _i32(t):
    """Bit patterns: equality of these tells +0.0 from -0.0."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _word(nat, seed, step):
    """The one-word int64 device tensor of (seed, step): the 64 bits of dropout_step_key, two's complement."""
    v = nat.dropout_step_key(seed, step)
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------- kernels: dropout
D_ROWS, D_COLS, D_ROW0S, D_PS = (1, 5, 64), (1, 3, 4, 203), (0, 2 ** 32 + 7), (0.1, 1.0)
SEED, STEP, SITE_A, SITE_B = 1234, 3, 4, 0x1001


def _window(vals, aligned, fill, dtype=torch.float32):
    """(whole buffer, view [rows, cols]): a 16-byte-aligned window with a leading dimension that is a multiple of four (the vector
    path), or the same window one column further in (the element path); the rest of the buffer holds `fill`."""
    rows, cols = vals.shape
    ld = (cols + 3) // 4 * 4 + 4
    full = torch.full((rows, ld), fill, dtype=dtype, device=DEV)
    view = full[:, :cols] if aligned else full[:, 1:1 + cols]
    view.copy_(vals)
    return full, view


def test_dropout_device_key_forms_equal_the_by_value_forms(pkg):
    """apply (out of place, in place), the pair from one shared input and the mask into a padded uint8 view, over the grid: every
    byte of every buffer, padding included, equals the by-value call with dropout_key(seed, step, site). Then the device word is
    overwritten with step + 1's through a copy and the SAME calls give the by-value results of step + 1."""
    nat = pkg._native
    g = torch.Generator().manual_seed(5)
    x_all = torch.randn(max(D_ROWS), max(D_COLS), generator=g).to(DEV)
    word = _word(nat, SEED, STEP)
    ka_dev, kb_dev = nat.DeviceKey(word, SITE_A), nat.DeviceKey(word, SITE_B)
    verdicts, labels = [], []

    def run(ka, kb, x, aligned, row0, p):
        """Every buffer the five calls write, under keys (ka, kb)."""
        rows, cols = x.shape
        _, xv = _window(x, aligned, 7.5)
        out = []
        full, ov = _window(torch.zeros_like(x), aligned, 7.5)
        nat.dropout_apply(xv, ka, row0, p, out=ov)
        out.append(full)
        full, iv = _window(x, aligned, 7.5)
        nat.dropout_apply(iv, ka, row0, p, out=iv)
        out.append(full)
        fa, oa = _window(torch.zeros_like(x), aligned, 7.5)
        fb, ob = _window(torch.zeros_like(x), aligned, 7.5)
        nat.dropout_apply_pair(xv, ka, xv, kb, row0, p, out_a=oa, out_b=ob)
        out += [fa, fb]
        fm, mv = _window(torch.zeros((rows, cols), dtype=torch.uint8), aligned, 9, dtype=torch.uint8)
        nat.dropout_mask(rows, cols, kb, row0, p, out=mv)
        out.append(fm)
        return out

    cases = [(rows, cols, aligned, row0, p) for rows in D_ROWS for cols in D_COLS for aligned in (True, False) for row0 in D_ROW0S
             for p in D_PS]
    for step in (STEP, STEP + 1):
        if step != STEP:
            word.copy_(_word(nat, SEED, step))                   # the device word changes; the calls' arguments do not
        ka, kb = nat.dropout_key(SEED, step, SITE_A), nat.dropout_key(SEED, step, SITE_B)
        for case in cases:
            rows, cols, aligned, row0, p = case
            x = x_all[:rows, :cols]
            want, got = run(ka, kb, x, aligned, row0, p), run(ka_dev, kb_dev, x, aligned, row0, p)
            for i, (w, gt) in enumerate(zip(want, got)):
                verdicts.append((_i32(w) == _i32(gt)).all().reshape(1))
                labels.append((step, i) + case)
    # the two steps' masks differ (the relaunch really followed the word)
    a = nat.dropout_mask(64, 203, nat.dropout_key(SEED, STEP, SITE_B), 0, 0.1, device=DEV)
    b = nat.dropout_mask(64, 203, kb_dev, 0, 0.1, device=DEV)
    assert not torch.equal(a, b)
    res = torch.cat(verdicts).cpu()
    bad = [labels[i] for i in torch.nonzero(~res).flatten().tolist()]
    assert len(labels) == 2 * 5 * len(cases) and not bad, '%d of %d checks failed, first: %s' % (len(bad), len(labels), bad[:8])


def test_dropout_device_key_wrapper_refusals(pkg):
    nat = pkg._native
    with pytest.raises(nat.NativeError):
        nat.DeviceKey(torch.zeros(1, dtype=torch.int64), 0)                       # a host tensor
    with pytest.raises(nat.NativeError):
        nat.DeviceKey(torch.zeros(2, dtype=torch.int64, device=DEV), 0)
    x = torch.ones(2, 4, device=DEV)
    w1, w2 = _word(nat, 1, 1), _word(nat, 1, 1)
    with pytest.raises(nat.NativeError):
        nat.dropout_apply_pair(x, nat.DeviceKey(w1, 0), x, nat.DeviceKey(w2, 1), 0, 0.5)   # two words in one pair
    with pytest.raises(nat.NativeError):
        nat.dropout_apply_pair(x, nat.DeviceKey(w1, 0), x, 5, 0, 0.5)


# ------------------------------------------------------------------------------------------------- kernels: Adam
A_LISTS = {'sizes': [1, 3, 8191, 8192, 8193], 'many': [5] * 65}


def _adam_tensors(sizes, offset):
    """g, p, m, v per size, each in its own buffer; `offset`: every base one element past a 16-byte boundary (the scalar path)."""
    g = torch.Generator().manual_seed(17)
    out = []
    for role in range(4):
        ts = []
        for n in sizes:
            raw = torch.randn(n + 8, generator=g).to(DEV)
            if role == 3:
                raw = raw.abs()                                    # second moments are not negative
            ts.append(raw[1:1 + n] if offset else raw[:n])
        out.append(ts)
    return out


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('with_coef', [False, True], ids=['no_coef', 'coef'])
@pytest.mark.parametrize('offset', [False, True], ids=['aligned', 'offset'])
@pytest.mark.parametrize('kind', sorted(A_LISTS))
def test_adam_step_through_device_hyper_equals_the_scalar_form(pkg, kind, offset, with_coef, wd):
    """One update with (step_size, bc2_sqrt) in device memory against the by-value call, p / m / v bit for bit; then the two
    floats are changed on the device and the same call equals the by-value call with the new values."""
    nat = pkg._native
    sizes = A_LISTS[kind]
    coef = torch.tensor([0.37], device=DEV) if with_coef else None
    a, b = _adam_tensors(sizes, offset), _adam_tensors(sizes, offset)
    hyper = torch.empty(2, dtype=torch.float32, device=DEV)
    group = {'betas': (0.9, 0.999), 'lr': 1e-2}
    for step in (1.0, 7.0):
        ss, bc = pkg.ClipAdam._step_hyper(group, step)
        hyper.copy_(torch.tensor([ss, bc], dtype=torch.float32))
        nat.adam_step(a[0], a[1], a[2], a[3], coef, ss, bc, 0.9, 0.999, 1e-8, wd)
        nat.adam_step(b[0], b[1], b[2], b[3], coef, 0.0, 1.0, 0.9, 0.999, 1e-8, wd, hyper_dev=hyper)
        ok = torch.stack([(_i32(x) == _i32(y)).all() for role in (0, 1, 2, 3) for x, y in zip(a[role], b[role])])
        assert bool(ok.all()), (step, torch.nonzero(~ok).flatten().tolist()[:8])
        assert all(bool(torch.isfinite(t).all()) for t in b[1])
    fresh = _adam_tensors(sizes, offset)
    assert not torch.equal(fresh[1][-1], b[1][-1])                 # the parameters did move


# ------------------------------------------------------------------------------------------------- the wrapper
def _twin(pkg, layers=1, lr=1e-3, **over):
    """(model, loader, train index, ClipAdam) from the golden state of syn_b with counter dropout 0.3 on all five sites; two calls
    give bit-identical twins (the extra layers of gcn_layers > 1 are seeded)."""
    torch.manual_seed(4321)
    model, dl = _fresh(pkg, 'syn_b', 0.3, gcn_layers=layers, **over)
    model.params.dropout = 'counter'
    for layer in [model.conv1] + list(model.conv1_extra):
        layer.drop.p = 0.3
    model.train()
    return model, dl, dl.train_index().to(DEV), pkg.ClipAdam(model.parameters(), lr=lr)


def _eager_step(model, dl, idx, opt, q, clip=CLIP):
    opt.zero_grad()
    loss = model.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=SMOOTH)
    loss.backward()
    opt.clip_and_step(clip)
    return loss.detach().clone()


def _captured(pkg, model, dl, idx, opt, **kw):
    return pkg.CapturedTrainStep(model, dl.graph, idx, opt, lbl_smooth=SMOOTH, clip=CLIP, **kw)


def _assert_same_state(a, opt_a, b, opt_b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    pa = [p for g in opt_a.param_groups for p in g['params']]
    pb = [p for g in opt_b.param_groups for p in g['params']]
    seen = 0
    for x, y in zip(pa, pb):
        st_a, st_b = opt_a.state.get(x), opt_b.state.get(y)
        assert bool(st_a) == bool(st_b)
        if st_a:
            seen += 1
            for k in ('exp_avg', 'exp_avg_sq', 'step'):
                assert torch.equal(st_a[k], st_b[k]), k
    assert seen > 10
    assert a.dropout_state() == b.dropout_state()


@pytest.mark.parametrize('layers', [1, 2])
def test_captured_run_is_the_eager_run_bit_for_bit(pkg, layers):
    """ALL_ON, counter dropout 0.3, ClipAdam, clip 0.5, StepLR halving the rate after every step; six calls with warmup=2: two
    eager steps, the capture with its first replay, three more replays. Losses, every state_dict entry, every Adam moment and step
    count and the dropout state equal the eager twin's."""
    a, dl_a, idx_a, opt_a = _twin(pkg, layers)
    b, dl_b, idx_b, opt_b = _twin(pkg, layers)
    sch_a = torch.optim.lr_scheduler.StepLR(opt_a, step_size=1, gamma=0.5)
    sch_b = torch.optim.lr_scheduler.StepLR(opt_b, step_size=1, gamma=0.5)
    step = _captured(pkg, a, dl_a, idx_a, opt_a, warmup=2)
    for i, q in enumerate(_repeating_batches(dl_a, 6)):
        got = step(q[:, 0], q[:, 1]).clone()
        want = _eager_step(b, dl_b, idx_b, opt_b, q)
        assert got.dim() == 0 and torch.equal(got, want), (i, float(got), float(want))
        sch_a.step()
        sch_b.step()
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 4, 2, False)
    assert opt_a._hip_step_count == opt_b._hip_step_count == 6 and opt_a._torch_step_count == 0
    _assert_same_state(a, opt_a, b, opt_b)
    # the Python-side launch counters count the eager steps and the capture, not the replays
    assert a.conv2._trunk_train_count == 3 and a.conv2._tail_train_count == 3 and a._query_rows_count == 6
    assert all(p.grad is not None for p in a.parameters() if opt_a.state.get(p))


def test_replays_do_not_leave_a_stale_encoder_cache(pkg):
    """An eval-mode encode before training fills the cache and captures the encoder's own graph; another one between replays
    refills it. After further replays the eval-mode encode equals the eager twin's: the replays bumped the version stamps."""
    runs = []
    for captured in (True, False):
        m, dl, idx, opt = _twin(pkg)
        step = _captured(pkg, m, dl, idx, opt) if captured else (lambda s, r: _eager_step(m, dl, idx, opt, torch.stack([s, r], 1)))
        batches = _repeating_batches(dl, 5)

        def frozen():
            m.eval()
            with torch.no_grad():
                out = [t.clone() for t in m.encode(dl.graph)]
            m.train()
            return out

        before = frozen()
        for q in batches[:3]:
            step(q[:, 0], q[:, 1])
        middle = frozen()
        assert m._enc_cache is not None and m._hip_graph is not None
        for q in batches[3:]:
            step(q[:, 0], q[:, 1])
        after = frozen()
        assert not torch.equal(middle[0], after[0]) and not torch.equal(before[0], middle[0])
        runs.append((middle, after))
        if captured:
            assert (step.captures, step.replays) == (1, 3)
    for got, want in zip(runs[0], runs[1]):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_changes_between_replays_take_effect_without_a_new_capture(pkg):
    """A written lr, load_dropout_state with another step, model.load_state_dict of the golden state: each acts on the next
    replay exactly as on the eager twin's next step, and `captures` stays 1. optimizer.load_state_dict replaces the state tensors:
    one re-capture, and equality still holds."""
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    step = _captured(pkg, a, dl_a, idx_a, opt_a)
    batches = iter(_repeating_batches(dl_a, 9))

    def both(n=1):
        for _ in range(n):
            q = next(batches)
            got, want = step(q[:, 0], q[:, 1]).clone(), _eager_step(b, dl_b, idx_b, opt_b, q)
            assert torch.equal(got, want)
        _assert_same_state(a, opt_a, b, opt_b)

    both(3)
    assert (step.captures, step.replays) == (1, 1)
    for opt in (opt_a, opt_b):
        opt.param_groups[0]['lr'] = 5e-4
    both()
    for m in (a, b):
        m.load_dropout_state({'dropout_seed': 77, 'dropout_step': 40})
    both()
    assert a.dropout_state() == {'dropout_seed': 77, 'dropout_step': 41}
    sd = golden('syn_b').state_dict()
    for m in (a, b):
        assert not m.load_state_dict(sd, strict=False).unexpected_keys
    both()
    assert (step.captures, step.replays, step.eager_steps) == (1, 4, 2)
    for opt in (opt_a, opt_b):
        opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    both(2)
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (2, 6, 2, False)
    step.clip = 0.25                                       # a plain attribute: held by value in the graph, so a third capture
    q = next(batches)
    got, want = step(q[:, 0], q[:, 1]).clone(), _eager_step(b, dl_b, idx_b, opt_b, q, clip=0.25)
    assert torch.equal(got, want) and step.captures == 3
    _assert_same_state(a, opt_a, b, opt_b)


def test_another_batch_size_runs_eagerly_and_is_counted(pkg):
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    step = _captured(pkg, a, dl_a, idx_a, opt_a)
    batches = _repeating_batches(dl_a, 5)
    batches[3] = batches[3][:12]
    for q in batches:
        assert torch.equal(step(q[:, 0], q[:, 1]).clone(), _eager_step(b, dl_b, idx_b, opt_b, q))
    assert (step.captures, step.replays, step.eager_steps) == (1, 2, 3)
    _assert_same_state(a, opt_a, b, opt_b)


def test_harness_epoch_with_a_captured_step(pkg):
    """harness.train_device_labels(captured=True) against the default loop on a twin: the same running loss (read once at the end
    of the epoch), the same state; a second epoch reuses the graph."""
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    for m in (a, b):
        m.params.lbl_smooth, m.params.clip_grad = SMOOTH, CLIP
    k = min(5, (dl_a.train_queries().size(0) - 8) // 16)
    assert k >= 3
    queries = dl_a.train_queries()[:16 * k + 8]                       # k batches of 16 and a last one of 8
    for epoch in range(2):
        got = pkg.harness.train_device_labels(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, generator=torch.Generator().manual_seed(epoch),
                                              captured=True)
        want = pkg.harness.train_device_labels(b, queries, idx_b, dl_b.graph, opt_b, b.params, 16, generator=torch.Generator().manual_seed(epoch))
        assert got == want
    step = a._captured_train_step
    assert (step.captures, step.replays, step.eager_steps) == (1, 2 * k - 2, 4)      # eager: two warm-up steps, two last batches
    _assert_same_state(a, opt_a, b, opt_b)


def test_refusals_raise_before_anything_is_captured(pkg):
    nat = pkg._native
    q = None

    def refused(model, dl, idx, opt, match, batch=None):
        step = _captured(pkg, model, dl, idx, opt)
        s = q if batch is None else batch
        with pytest.raises(nat.NativeError, match=match):
            step(s[:, 0], s[:, 1])
        assert step.captures == 0 and step.replays == 0 and not step.disabled

    m, dl, idx, opt = _twin(pkg)
    q = _repeating_batches(dl, 1)[0]
    refused(m, dl, idx, torch.optim.Adam(m.parameters(), lr=1e-3), 'clip_and_step')
    refused(m, dl, idx, pkg.ClipAdam(m.parameters(), lr=1e-3, amsgrad=True), "torch's own step")
    refused(m, dl, idx, opt, 'batch of 14', batch=q[:14])
    _eager_step(m, dl, idx, opt, q)                                  # one real step, then one parameter's count runs ahead
    first = next(p for p in m.parameters() if opt.state.get(p))
    opt.state[first]['step'] += 1
    refused(m, dl, idx, opt, 'disagree on the step count')
    opt.state[first]['step'] -= 1
    m._edge_shard = (None, 0, 1)
    refused(m, dl, idx, opt, 'shard')
    m._edge_shard = None
    m.eval()
    refused(m, dl, idx, opt, 'eval mode')
    m.train()
    torch.manual_seed(4321)
    t, dl_t = _fresh(pkg, 'syn_b', 0.3)                               # dropout 0.3 drawn by torch
    t.train()
    refused(t, dl_t, dl_t.train_index().to(DEV), pkg.ClipAdam(t.parameters(), lr=1e-3), "not 'counter'")
    c, dl_c, idx_c, _ = _twin(pkg)
    c.cpu()
    refused(c, dl_c, idx_c, pkg.ClipAdam(c.parameters(), lr=1e-3), 'CPU')


def test_torch_trunk_and_torch_query_path_within_the_eager_spread(pkg):
    """Counter dropout and ClipAdam with the torch trunk and the torch query path (index_add_'s float atomics: the eager step is not
    bit-reproducible). Four steps (two eager, the capture, one more replay): the captured run's losses and parameters lie within
    four times the largest difference between two eager runs of the same configuration, floor 1e-6. The eager spread is measured
    here over EAGER_RUNS runs (every pair): it is bimodal -- when the atomics happen to land in one order two runs agree to ~1e-8,
    when they do not, Adam's m / sqrt(v) turns the rounding of a near-zero gradient into a change of the order of lr, ~1e-4 after
    four steps -- so a single pair often sees only the lower mode.
    Measured on an MI355X (the SPREAD line this test prints under pytest -s), three processes, one eager pair each: eager spread
    1.49e-08 / 2.47e-04 / 3.31e-06, captured against the first eager run 1.49e-08 / 1.39e-04 / 1.48e-04. The third of these
    misses 4 x its own single-pair spread; the captured figures lie inside the eager step's upper mode (2.47e-04)."""
    over = dict(conve_trunk_train='torch', query_path_train='torch')
    runs = []
    for captured in (False,) * EAGER_RUNS + (True,):
        m, dl, idx, opt = _twin(pkg, **over)
        step = _captured(pkg, m, dl, idx, opt) if captured else None
        vals = []
        for q in _repeating_batches(dl, 4):
            loss = step(q[:, 0], q[:, 1]) if captured else _eager_step(m, dl, idx, opt, q)
            vals.append(loss.detach().reshape(1).clone())
        if captured:
            assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 2, 2, False)
        assert getattr(m.conv2, '_trunk_train_count', 0) == 0 and getattr(m, '_query_rows_count', 0) == 0
        vals += [v.detach().reshape(-1).float() for k, v in sorted(m.state_dict().items()) if v.is_floating_point()]
        runs.append(torch.cat(vals))
    eager, cap = runs[:-1], runs[-1]
    spread = max(float((a - b).abs().max()) for i, a in enumerate(eager) for b in eager[i + 1:])
    worst = float((cap - eager[0]).abs().max())
    bound = max(4.0 * spread, 1e-6)
    print('SPREAD eager-vs-eager (largest of %d pairs) %.3g, captured-vs-eager %.3g, bound %.3g'
          % (len(eager) * (len(eager) - 1) // 2, spread, worst, bound))
    assert worst <= bound
