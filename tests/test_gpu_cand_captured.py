"""The captured sampled-negative step (kgc-gcn_amd/captured.py CapturedCandidateStep) on a real MI355X (`-m gpu`):
mgcn_cand_draw_dev bit for bit against mgcn_cand_draw under the key of the word it reads, the word read when the kernel runs (a
rewritten word, a replayed graph), and the wrapper and harness.train_sampled_negatives(captured=True) against an eager twin built
from the same golden state (case syn_b, B = 16, the builders of test_gpu_captured_step). Everything is integers or a
reproducible float path (HIP trunk and query path, fixed-order list backward), so every comparison is torch.equal."""
import pytest
import torch

from . import cand_draw_ref as R
from .test_gpu_captured_step import CLIP, SMOOTH, SWITCHES, _assert_same_state, _twin, _word
from .test_gpu_query_train import DEV, _repeating_batches

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
EDGE = (0, 1, 7, 1234, 2 ** 32, 2 ** 63, M64)      # the (seed, step) edge values of test_captured_step_host
FIRST_STEP = 2 ** 32 - 3                            # the draw step crosses 2^32 during the six calls


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _on(dev, *ts):
    return [t.to(dev) for t in ts]


def _pairs(nat):
    """Three (seed, step) pairs of the edge values: the first whose word has its top bit set, the first whose word has not, and
    the all-ones pair."""
    words = [((s, t), nat.dropout_step_key(s, t)) for s in EDGE for t in EDGE]
    high = next(p for p, w in words if w >> 63)
    low = next(p for p, w in words if not w >> 63)
    return [high, low, (M64, M64)]


# ------------------------------------------------------------------------------------------------- the kernel
def test_device_key_draw_equals_the_by_value_draw_on_the_grid(pkg):
    """cand_draw_ref's grid (B x K x N x row0) under three words: both outputs written into padded windows of poisoned buffers;
    every byte of both buffers equals the by-value call's, the padding keeps its poison, and labels=False gives no label. ONE word
    tensor serves all keys: it is rewritten in place between the launches."""
    nat = pkg._native
    dkeys, dptr, dtails = _on(DEV, *R.grid_index())
    dq = R.grid_queries(max(R.GRID_B)).to(DEV)
    pairs = _pairs(nat)
    assert nat.dropout_step_key(*pairs[0]) >> 63 == 1 and nat.dropout_step_key(*pairs[1]) >> 63 == 0
    word = _word(nat, 0, 0)
    dk = nat.DeviceKey(word, nat.CAND_DRAW_SITE)
    verdicts, labels = [], []

    def run(key, B, K, N, row0):
        cbuf = torch.full((B + 1, K + 7), -77, dtype=torch.int64, device=DEV)
        lbuf = torch.full((B + 1, K + 11), 77, dtype=torch.uint8, device=DEV)
        c, l = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, key, row0=row0, out=(cbuf[:B, 3:3 + K], lbuf[:B, 5:5 + K]))
        assert c.data_ptr() == cbuf[:B, 3:3 + K].data_ptr() and l.data_ptr() == lbuf[:B, 5:5 + K].data_ptr()
        return cbuf, lbuf

    for seed, step in pairs:
        word.copy_(_word(nat, seed, step))
        k = nat.dropout_key(seed, step, nat.CAND_DRAW_SITE)
        for N in R.GRID_N:
            for row0 in R.GRID_ROW0:
                for B in R.GRID_B:
                    for K in R.GRID_K:
                        want_c, want_l = run(k, B, K, N, row0)
                        got_c, got_l = run(dk, B, K, N, row0)
                        only, none = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, dk, row0=row0, labels=False)
                        assert none is None
                        pad_c, pad_l = got_c.clone(), got_l.clone()
                        pad_c[:B, 3:3 + K], pad_l[:B, 5:5 + K] = -77, 77
                        verdicts.append(((got_c == want_c).all() & (got_l == want_l).all() & (only == want_c[:B, 3:3 + K]).all()
                                         & (pad_c == -77).all() & (pad_l == 77).all()).reshape(1))
                        labels.append((seed, step, N, row0, B, K))
    res = torch.cat(verdicts).cpu()
    bad = [labels[i] for i in torch.nonzero(~res).flatten().tolist()]
    assert len(labels) == 3 * len(R.GRID_N) * len(R.GRID_ROW0) * len(R.GRID_B) * len(R.GRID_K) and not bad, (len(bad), bad[:8])
    # the three words gave three different blocks (the relaunches followed the word)
    blocks = []
    for seed, step in pairs:
        word.copy_(_word(nat, seed, step))
        blocks.append(nat.cand_draw(dq, dkeys, dptr, dtails, 40943, 65, dk)[0])
    assert not torch.equal(blocks[0], blocks[1]) and not torch.equal(blocks[1], blocks[2]) and not torch.equal(blocks[0], blocks[2])


def test_device_key_more_than_one_workgroup_and_a_grid_stride(pkg):
    """B K / 2 above 2048 x 256 units, so that every workgroup strides: 1100 x 1001 positions (the by-value test's shape)."""
    nat = pkg._native
    keys, ptr, tails = _on(DEV, *R.grid_index())
    q = R.grid_queries(1100).to(DEV)
    seed, step = 5, 6
    want_c, want_l = nat.cand_draw(q, keys, ptr, tails, 40943, 1001, nat.dropout_key(seed, step, nat.CAND_DRAW_SITE), row0=2 ** 32 - 7)
    got_c, got_l = nat.cand_draw(q, keys, ptr, tails, 40943, 1001, nat.DeviceKey(_word(nat, seed, step), nat.CAND_DRAW_SITE), row0=2 ** 32 - 7)
    assert torch.equal(got_c, want_c) and torch.equal(got_l, want_l)
    assert int(got_c[:, 1:].min()) >= 0 and int(got_c[:, 1:].max()) < 40943


def test_the_word_is_read_when_the_kernel_runs(pkg):
    """The same word tensor rewritten in place between two launches: each gives the by-value block of its own key. Then ONE
    cand_draw with a DeviceKey captured in a torch.cuda.graph and replayed under three different words."""
    nat = pkg._native
    keys, ptr, tails = _on(DEV, *R.grid_index())
    q = R.grid_queries(67).to(DEV)
    N, K = 40943, 65
    pairs = _pairs(nat)

    def by_value(seed, step):
        return nat.cand_draw(q, keys, ptr, tails, N, K, nat.dropout_key(seed, step, nat.CAND_DRAW_SITE), row0=3)

    word = _word(nat, *pairs[0])
    dk = nat.DeviceKey(word, nat.CAND_DRAW_SITE)
    first = nat.cand_draw(q, keys, ptr, tails, N, K, dk, row0=3)
    word.copy_(_word(nat, *pairs[1]))
    second = nat.cand_draw(q, keys, ptr, tails, N, K, dk, row0=3)
    for got, pair in ((first, pairs[0]), (second, pairs[1])):
        want = by_value(*pair)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(first[0], second[0])
    cbuf = torch.full((67, K), -77, dtype=torch.int64, device=DEV)
    lbuf = torch.full((67, K), 77, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nat.cand_draw(q, keys, ptr, tails, N, K, dk, row0=3, out=(cbuf, lbuf))
    seen = []
    for pair in pairs:
        word.copy_(_word(nat, *pair))
        graph.replay()
        want = by_value(*pair)
        assert torch.equal(cbuf, want[0]) and torch.equal(lbuf, want[1]), pair
        seen.append(cbuf.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_device_key_wrapper_refusals_write_nothing(pkg):
    nat = pkg._native
    keys, ptr, tails = _on(DEV, *R.grid_index())
    q = R.grid_queries(4).to(DEV)
    cbuf = torch.full((4, 8), -77, dtype=torch.int64, device=DEV)
    lbuf = torch.full((4, 8), 77, dtype=torch.uint8, device=DEV)
    with pytest.raises(nat.NativeError):
        nat.cand_draw(q, keys, ptr, tails, 7, 8, nat.DeviceKey(torch.zeros(1, dtype=torch.int64), nat.CAND_DRAW_SITE), out=(cbuf, lbuf))
    with pytest.raises(nat.NativeError):
        nat.cand_draw(q, keys, ptr, tails, 7, 8, nat.DeviceKey(torch.zeros(2, dtype=torch.int64, device=DEV), nat.CAND_DRAW_SITE),
                      out=(cbuf, lbuf))
    with pytest.raises(nat.NativeError):                       # the host twin takes no device word
        nat.cand_draw_host(q.cpu(), keys.cpu(), ptr.cpu(), tails.cpu(), 7, 8, nat.DeviceKey(_word(nat, 1, 1), nat.CAND_DRAW_SITE))
    with pytest.raises(nat.NativeError):
        pkg.harness.draw_candidates(torch.zeros((4, 2), dtype=torch.int64, device=DEV), _Index(keys, ptr, tails), 7, 7, 1, 1,
                                    step_key_dev=torch.zeros(1, dtype=torch.int64))
    torch.cuda.synchronize()
    assert bool((cbuf == -77).all()) and bool((lbuf == 77).all())


class _Index(object):
    """The three arrays and the key rule draw_candidates asks of an index."""

    def __init__(self, keys, ptr, tails):
        self.keys, self.ptr, self.tails = keys, ptr, tails

    def query_keys(self, src, rel):
        return src * 2 + rel


def test_a_word_on_another_device_is_refused(pkg):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs a second GPU: the word and the tensors must be on different devices')
    nat = pkg._native
    keys, ptr, tails = _on(DEV, *R.grid_index())
    q = R.grid_queries(4).to(DEV)
    cbuf = torch.full((4, 8), -77, dtype=torch.int64, device=DEV)
    other = torch.zeros(1, dtype=torch.int64, device='cuda:1')
    with pytest.raises(nat.NativeError, match='different devices'):
        nat.cand_draw(q, keys, ptr, tails, 7, 8, nat.DeviceKey(other, nat.CAND_DRAW_SITE), out=cbuf, labels=False)
    torch.cuda.synchronize()
    assert bool((cbuf == -77).all())


# ------------------------------------------------------------------------------------------------- the wrapper
SEED = 99


def _eager_step(pkg, model, dl, idx, opt, q, num_neg, seed, step, loss, clip=CLIP):
    """One step of train_sampled_negatives(draw_seed=seed) at draw step `step`; (loss, cand)."""
    cand, labels = pkg.harness.draw_candidates(q, idx, model.entity_embedding.size(0), num_neg, seed, step, labels=True)
    opt.zero_grad()
    out = model.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, labels=labels, lbl_smooth=SMOOTH, loss=loss)
    out.backward()
    opt.clip_and_step(clip)
    return out.detach().clone(), cand


def _captured(pkg, model, dl, idx, opt, num_neg, loss, **kw):
    return pkg.CapturedCandidateStep(model, dl.graph, idx, opt, num_neg, SEED, draw_step=FIRST_STEP, loss=loss, lbl_smooth=SMOOTH, clip=CLIP, **kw)


@pytest.mark.parametrize('num_neg', [2, 64])
@pytest.mark.parametrize('layers', [1, 2])
@pytest.mark.parametrize('loss', ['bce', 'softmax'])
def test_captured_run_is_the_eager_run_bit_for_bit(pkg, loss, layers, num_neg):
    """Counter dropout 0.3 on all five sites, HIP trunk and query path, ClipAdam, clip 0.5, StepLR halving the rate after every
    step; six calls with warmup=2 from draw step 2^32 - 3: two eager steps, the capture with its first replay, three more
    replays. Losses, lists, every state_dict entry, every Adam moment and step count and the dropout state equal the eager
    twin's. num_neg = 64: K = 65 crosses the 64-position chunk of the softmax statistics; the table of syn_b is small, so ids
    repeat within and across lists (runs in the plan)."""
    a, dl_a, idx_a, opt_a = _twin(pkg, layers)
    b, dl_b, idx_b, opt_b = _twin(pkg, layers)
    sch_a = torch.optim.lr_scheduler.StepLR(opt_a, step_size=1, gamma=0.5)
    sch_b = torch.optim.lr_scheduler.StepLR(opt_b, step_size=1, gamma=0.5)
    step = _captured(pkg, a, dl_a, idx_a, opt_a, num_neg, loss, warmup=2)
    lists = []
    for i, q in enumerate(_repeating_batches(dl_a, 6)):
        assert step.draw_step == FIRST_STEP + i
        got = step(q[:, 0], q[:, 1]).clone()
        want, cand = _eager_step(pkg, b, dl_b, idx_b, opt_b, q, num_neg, SEED, FIRST_STEP + i, loss)
        assert got.dim() == 0 and torch.equal(got, want), (i, float(got), float(want))
        assert tuple(step.cand.shape) == (16, 1 + num_neg) and torch.equal(step.cand, cand), i
        lists.append((step.cand.data_ptr(), step.cand.clone()))
        sch_a.step()
        sch_b.step()
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 4, 2, False)
    assert step.draw_step == FIRST_STEP + 6
    # the replays write ONE static block, and consecutive replays leave different lists in it
    assert len({p for p, _ in lists[2:]}) == 1
    assert all(not torch.equal(x[1], y[1]) for x, y in zip(lists[2:], lists[3:]))
    assert opt_a._hip_step_count == opt_b._hip_step_count == 6 and opt_a._torch_step_count == 0
    _assert_same_state(a, opt_a, b, opt_b)
    assert all(p.grad is not None for p in a.parameters() if opt_a.state.get(p))


@pytest.mark.parametrize('change', ['num_neg', 'loss'])
def test_changes_between_replays_take_effect_without_a_new_capture(pkg, change):
    """A changed draw_seed, a set draw_step, load_dropout_state and a written lr: each acts on the next replay exactly as on the
    eager twin's next step and `captures` stays 1. num_neg / loss are held by value in the graph: one re-capture, still equal."""
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    step = _captured(pkg, a, dl_a, idx_a, opt_a, 7, 'bce')
    batches = iter(_repeating_batches(dl_a, 10))
    twin = dict(seed=SEED, step=FIRST_STEP, num_neg=7, loss='bce')

    def both(n=1):
        for _ in range(n):
            q = next(batches)
            got = step(q[:, 0], q[:, 1]).clone()
            want, cand = _eager_step(pkg, b, dl_b, idx_b, opt_b, q, twin['num_neg'], twin['seed'], twin['step'], twin['loss'])
            twin['step'] += 1
            assert torch.equal(got, want) and torch.equal(step.cand, cand)
        _assert_same_state(a, opt_a, b, opt_b)
        assert step.draw_step == twin['step']

    both(3)
    assert (step.captures, step.replays) == (1, 1)
    step.draw_seed = twin['seed'] = 2 ** 63 + 5
    both()
    step.draw_step = twin['step'] = 12
    both()
    for m in (a, b):
        m.load_dropout_state({'dropout_seed': 77, 'dropout_step': 40})
    both()
    for opt in (opt_a, opt_b):
        opt.param_groups[0]['lr'] = 5e-4
    both()
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 5, 2, False)
    if change == 'num_neg':
        step.num_neg = twin['num_neg'] = 3
    else:
        step.loss = twin['loss'] = 'softmax'
    both(2)
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (2, 7, 2, False)


def test_another_batch_size_runs_eagerly_and_is_counted(pkg):
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    step = _captured(pkg, a, dl_a, idx_a, opt_a, 5, 'softmax')
    batches = _repeating_batches(dl_a, 5)
    batches[3] = batches[3][:13]                               # (no multiple of four: the list stage takes any batch)
    for i, q in enumerate(batches):
        got = step(q[:, 0], q[:, 1]).clone()
        want, cand = _eager_step(pkg, b, dl_b, idx_b, opt_b, q, 5, SEED, FIRST_STEP + i, 'softmax')
        assert torch.equal(got, want) and torch.equal(step.cand, cand), i
    assert (step.captures, step.replays, step.eager_steps) == (1, 2, 3) and step.draw_step == FIRST_STEP + 5
    _assert_same_state(a, opt_a, b, opt_b)


@pytest.mark.parametrize('loss', ['bce', 'softmax'])
def test_harness_epoch_with_a_captured_step(pkg, loss):
    """harness.train_sampled_negatives(draw_seed=s, first_step=k, captured=True) against the default loop on a twin: the same
    running loss (read once at the end of the epoch), the same state; a second epoch reuses the graph."""
    a, dl_a, idx_a, opt_a = _twin(pkg)
    b, dl_b, idx_b, opt_b = _twin(pkg)
    for m in (a, b):
        m.params.lbl_smooth, m.params.clip_grad = SMOOTH, CLIP
    k = min(5, (dl_a.train_queries().size(0) - 8) // 16)
    assert k >= 3
    queries = dl_a.train_queries()[:16 * k + 8]                       # k batches of 16 and a last one of 8
    first = 2 ** 32 - 2
    for epoch in range(2):
        kw = dict(generator=None, draw_seed=SEED, first_step=first + epoch * (k + 1), loss=loss)
        kw['generator'] = torch.Generator().manual_seed(epoch)
        got = pkg.harness.train_sampled_negatives(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, 9, captured=True, **kw)
        kw['generator'] = torch.Generator().manual_seed(epoch)
        want = pkg.harness.train_sampled_negatives(b, queries, idx_b, dl_b.graph, opt_b, b.params, 16, 9, **kw)
        assert got == want
    step = a._captured_cand_train_step
    assert isinstance(step, pkg.CapturedCandidateStep)
    assert (step.captures, step.replays, step.eager_steps) == (1, 2 * k - 2, 4)      # eager: two warm-up steps, two last batches
    assert step.draw_step == first + 2 * (k + 1)
    _assert_same_state(a, opt_a, b, opt_b)
    with pytest.raises(pkg._native.NativeError, match='draw_seed'):
        pkg.harness.train_sampled_negatives(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, 9, captured=True)
    assert (step.captures, step.replays, step.eager_steps) == (1, 2 * k - 2, 4)


def test_refusals_raise_before_anything_is_captured(pkg):
    from .test_gpu_query_train import _fresh
    nat = pkg._native
    m, dl, idx, opt = _twin(pkg)
    q = _repeating_batches(dl, 1)[0]

    def refused(model, dl, idx, opt, match, num_neg=4, loss='bce'):
        step = _captured(pkg, model, dl, idx, opt, num_neg, loss)
        with pytest.raises(nat.NativeError, match=match):
            step(q[:, 0], q[:, 1])
        assert step.captures == 0 and step.replays == 0 and step.eager_steps == 0 and not step.disabled
        assert step.draw_step == FIRST_STEP and step.cand is None

    refused(m, dl, idx, torch.optim.Adam(m.parameters(), lr=1e-3), 'clip_and_step')
    refused(m, dl, idx, opt, 'num_neg', num_neg=-1)
    refused(m, dl, idx, opt, 'num_neg', num_neg=2.5)
    refused(m, dl, idx, opt, "'bce' or 'softmax'", loss='hinge')
    refused(m, dl, dl.train_index(), opt, "not on the model's device")
    m.eval()
    refused(m, dl, idx, opt, 'eval mode')
    m.train()
    torch.manual_seed(4321)
    t, dl_t = _fresh(pkg, 'syn_b', 0.3)                               # dropout 0.3 drawn by torch
    t.train()
    refused(t, dl_t, dl_t.train_index().to(DEV), pkg.ClipAdam(t.parameters(), lr=1e-3), "not 'counter'")
    # what the parent refuses of the batch belongs to the full-table launch: 14 rows are taken here
    step = _captured(pkg, m, dl, idx, opt, 4, 'bce')
    step(q[:14, 0], q[:14, 1])
    assert step.eager_steps == 1 and step.draw_step == FIRST_STEP + 1
