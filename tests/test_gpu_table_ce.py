"""The softmax cross-entropy over the full entity table (include/mgcn_hip.h (20)) on a real MI355X (`-m gpu`):
mgcn_score_ce_logits / mgcn_cand_ce_merge / mgcn_score_ce_finish and _ScoreCEFn against the float64 reference of
tests/table_ce_ref.py under its bars at every tile, mask-word and column-tile edge; the bit identities with the list logits;
one process playing three ranks of the scoring stage; the second form for batches the logits launch refuses; the four routes of
the step (forward_loss, train_device_labels, CapturedTrainStep, train_step_sharded) bit for bit; two processes over gloo."""
import os

import numpy as np
import pytest
import torch

from . import cand_train_ref as C
from . import dense_ref as R
from . import table_ce_ref as T
from .test_gpu_captured_step import CLIP, SMOOTH, _assert_same_state, _twin
from .test_gpu_query_train import _repeating_batches
from .test_gpu_train_sharded import _PORTS, _assemble, _batches, _models, _np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN', 'MGCN_TRUNK', 'MGCN_DROPOUT', 'MGCN_TRAIN_TORCH')
NS = (1, 31, 32, 33, 64, 95, 257, 2100)
# both sides of every column-tile width pick_nt can choose (32, 64, 128, 208 columns; above 208 strips of 128, strips of 208 at a
# multiple of 208 and above 1024: 1024 itself takes strips of 128), which also straddles the finish's groups of 64 queries; plus B = 4
BS = (4, 32, 36, 64, 68, 128, 132, 208, 212, 416, 1024, 1028)
DIMS, SCALES, EPS = (4, 20, 200), (1.0, 30.0, 100.0), (0.0, 0.1)


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _on_device(pkg, x, ent, bias, y, row0=0, n_local=None):
    """(x, this shard's ent and bias, its bit-packed positives) on the device: query b has the key b."""
    n_local = ent.size(0) - row0 if n_local is None else n_local
    keys, ptr, tails = (t.to(DEV) for t in T.index_of(y))
    mask = pkg._native.filter_mask(torch.arange(x.size(0), device=DEV), keys, ptr, tails, n_local, ent_row0=row0)
    return x.to(DEV), ent[row0:row0 + n_local].contiguous().to(DEV), bias[row0:row0 + n_local].contiguous().to(DEV), mask


def _apply(pkg, xd, ed, bd, mask, eps, total, ex=None):
    """(loss, g [n, B], dx, d_ent, d_bias) of _ScoreCEFn; xd keeps its layout."""
    xs, es, bs = xd.detach().requires_grad_(True), ed.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    loss = pkg.autograd._ScoreCEFn.apply(xs, es, bs, mask, eps, total, ex)
    g = loss.grad_fn.saved_tensors[2]
    loss.backward()
    return loss.detach(), g, xs.grad, es.grad, bs.grad


def _worst(got, want, bar):
    if want.numel() == 0:
        return 0.0
    return float(((got.detach().cpu().double() - want).abs() / bar).max())


def _hold(tag, ref, x, ent_shard, dim, out, n_partials):
    """Every element of g, the loss, dx, d_ent, d_bias of `out` against the float64 `ref` under the bars; the ratios."""
    inv = 1.0 / x.size(0)
    loss, g, dx, de, db = out
    _, rowbar = T.logit_bars(ref, dim)
    dxb, deb, dbb = T.grad_bars(ref, x, ent_shard, rowbar, inv)
    ratios = dict(g=_worst(g.t(), ref['g'], T.g_bar(ref, rowbar, inv)),
                  loss=abs(float(loss.double()) - ref['loss']) / T.loss_bar(ref, rowbar, inv, n_partials),
                  dx=_worst(dx, ref['dx'], dxb), d_ent=_worst(de, ref['d_ent'], deb), d_bias=_worst(db, ref['d_bias'], dbb))
    print('RATIO table_ce %s %s' % (tag, ' '.join('%s=%.4f' % kv for kv in sorted(ratios.items()))))
    assert max(ratios.values()) <= 1.0, (tag, ratios)
    return ratios


@pytest.mark.parametrize('n', NS)
def test_structural_grid_against_float64(pkg, n):
    """For this n every B of BS. NOT the full product with dim, logit scale and eps: those three cycle with (n, B), so that every
    value of each occurs at every n and with several B, and every (n, B) pair is run. Every element of z, the tiles' records, the
    rows' statistics, g, the loss, dx, d_ent and d_bias against float64 under the bars."""
    nat = pkg._native
    for j, B in enumerate(BS):
        i = NS.index(n)
        dim, scale, eps = DIMS[(i + j) % 3], SCALES[(i + 2 * j + j // 3) % 3], EPS[(i + j // 2) % 2]
        tag = 'n=%d B=%d dim=%d scale=%g eps=%g' % (n, B, dim, scale, eps)
        x, ent, bias, y = T.problem(B, n, dim, R.seed_of(91, n, B), scale=scale)
        ref = T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B)
        xd, ed, bd, mask = _on_device(pkg, x, ent, bias, y)
        assert nat.score_ce_supported(xd, ed)
        z, stat = nat.score_ce_logits(xd, ed, bd, mask)
        tiles, G, P = nat.score_ce_fold_shape(n)
        assert tiles == (n + 31) // 32 and G * P >= tiles and (G > 1) == (n == 2100)
        assert tuple(z.shape) == (n, B) and tuple(stat.shape) == (G * P, B, 4)
        zbar, rowbar = T.logit_bars(ref, dim)
        assert _worst(z.t(), ref['z'], zbar) <= 1.0, tag
        # a record is its own tile's: the maximum of the launch's own z (exact), the rows of the tile, the positives of the tile
        m_t, s_t, nl_t, np_t = nat.cand_ce_stat_fields(stat)
        for t in range(tiles):
            rows = slice(32 * t, min(32 * t + 32, n))
            assert torch.equal(m_t[t], z[rows].max(0).values), (tag, t)
            assert bool((nl_t[t] == rows.stop - rows.start).all()), (tag, t)
            assert torch.equal(np_t[t].cpu().long(), y[:, rows].sum(1)), (tag, t)
            want_s = torch.exp(z[rows].double() - m_t[t].double()).sum(0)
            assert float(((s_t[t].double() - want_s).abs() / want_s).max()) <= C.gamma(34) + 16 * R.U, (tag, t)   # 32 rounded exps of rounded arguments, 31 additions
        assert bool((m_t[tiles:] == float('-inf')).all()) and not bool(stat[tiles:, :, 1:].view(torch.int32).any()), tag
        merged = nat.score_ce_fold(stat, n)
        m, s, nl, npos = nat.cand_ce_stat_fields(merged)
        assert bool((nl == n).all()) and torch.equal(npos.cpu().long(), y.sum(1)), tag
        assert torch.equal(npos, nat.mask_popcount(mask)), tag
        assert _worst(m, ref['M'], rowbar) <= 1.0, tag
        lse = m.double().cpu() + torch.log(s.double().cpu())
        assert float(((lse - (ref['M'] + torch.log(ref['S']))).abs() / T.lse_bar(ref, rowbar)).max()) <= 1.0, tag
        out = _apply(pkg, xd, ed, bd, mask, eps, n)
        _hold(tag, ref, x, ent, dim, out, int(nat.lib().mgcn_score_ce_partials(B, n)))
        # the Function is these launches: the finish on the launch's z and merged records gives its loss and g, bit for bit
        loss2, g2, parts = nat.score_ce_finish(z.clone(), mask, merged, eps, n)
        assert torch.equal(g2, out[1]) and torch.equal(loss2, out[0]) and parts.numel() == tiles * ((B + 63) // 64), tag
        rows_without = (y.sum(1) == 0).to(DEV)
        assert bool((out[1][:, rows_without] == 0).all()), tag


@pytest.mark.parametrize('n', [2049, 2304, 4100])
def test_two_level_fold_of_the_tile_records(pkg, n):
    """Beyond 64 tiles the records fold in two levels through the merge kernel's strides: 65 tiles in 9 groups of 8 (7 padded
    records), 72 tiles in 9 groups of 8 (none), 129 tiles in 12 groups of 11 (3). The padding is the empty statistic, the counts
    are exact, M is the one-level fold's M bit for bit and M + log S of both folds meets the float64 bar; the Function's g, loss
    and gradients meet theirs."""
    nat = pkg._native
    B, dim, eps = 36, 20, 0.1
    x, ent, bias, y = T.problem(B, n, dim, R.seed_of(95, n), scale=30.0)
    ref = T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B)
    xd, ed, bd, mask = _on_device(pkg, x, ent, bias, y)
    z, stat = nat.score_ce_logits(xd, ed, bd, mask)
    tiles, G, P = nat.score_ce_fold_shape(n)
    assert (tiles, G, P) == T.fold_shape(n) == {2049: (65, 9, 8), 2304: (72, 9, 8), 4100: (129, 12, 11)}[n]
    assert tuple(stat.shape) == (G * P, B, 4)
    m_t = nat.cand_ce_stat_fields(stat)[0]
    assert bool(torch.isfinite(m_t[:tiles]).all()) and bool((m_t[tiles:] == float('-inf')).all())
    two, one = nat.score_ce_fold(stat, n), nat.cand_ce_merge(stat, part_dim=0)
    _, rowbar = T.logit_bars(ref, dim)
    want = ref['M'] + torch.log(ref['S'])
    for name, rec in (('two levels', two), ('one level', one)):
        m, s, nl, npos = nat.cand_ce_stat_fields(rec)
        assert bool((nl == n).all()) and torch.equal(npos.cpu().long(), y.sum(1)), name
        assert torch.equal(m, z.max(0).values), name
        lse = m.double().cpu() + torch.log(s.double().cpu())
        assert float(((lse - want).abs() / T.lse_bar(ref, rowbar)).max()) <= 1.0, name
    _hold('two-level fold n=%d' % n, ref, x, ent, dim, _apply(pkg, xd, ed, bd, mask, eps, n), int(nat.lib().mgcn_score_ce_partials(B, n)))


@pytest.mark.parametrize('n,B,dim', [(257, 36, 200), (95, 132, 20), (2100, 4, 4)])
def test_bit_identities(pkg, n, B, dim):
    """z equals the list logits of the list that names every entity, transposed; two runs give the same bits."""
    nat = pkg._native
    x, ent, bias, y = T.problem(B, n, dim, R.seed_of(92, n, B))
    xd, ed, bd, mask = _on_device(pkg, x, ent, bias, y)
    z, stat = nat.score_ce_logits(xd, ed, bd, mask)
    cand = torch.arange(n, device=DEV).repeat(B, 1)
    zl, _ = nat.cand_ce_logits(xd, ed, bd, cand, torch.zeros((B, n), dtype=torch.uint8, device=DEV))
    assert torch.equal(z, zl.t())
    a, b = _apply(pkg, xd, ed, bd, mask, 0.1, n), _apply(pkg, xd, ed, bd, mask, 0.1, n)
    z2, stat2 = nat.score_ce_logits(xd, ed, bd, mask)
    assert torch.equal(z, z2) and torch.equal(stat.view(torch.int32), stat2.view(torch.int32))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


class _Played(object):
    """The exchange of one rank among `world` played in one process: gather_stats hands back the block of all ranks' records and
    checks that this rank's own record is the one the block holds for it."""

    def __init__(self, rank, block):
        self.rank, self.block, self.world, self.calls = rank, block, block.size(0), 0

    def gather_stats(self, stat):
        self.calls += 1
        assert torch.equal(stat.view(torch.int32), self.block[self.rank].view(torch.int32))
        return self.block.clone()


@pytest.mark.parametrize('B,dim', [(36, 200), (5, 20)])
def test_three_ranks_of_the_scoring_stage(pkg, B, dim):
    """Bounds [0, 45, 45, 130] (no multiple of 32, an empty middle shard), through the logits launch (B = 36) and through the
    second form (B = 5): every rank's g, d_ent and d_bias rows against the float64 reference of its shard with GLOBAL statistics;
    the ranks' losses and dx add up to the whole table's within the shards' bars; every rank merges the same block."""
    nat = pkg._native
    N, eps, bounds = 130, 0.1, [0, 45, 45, 130]
    x, ent, bias, y = T.problem(B, N, dim, R.seed_of(93, B, dim))
    shards = [_on_device(pkg, x, ent, bias, y, a, e - a) for a, e in zip(bounds[:-1], bounds[1:])]
    block = []
    for xd, ed, bd, mask in shards:                       # what each rank hands to the all-gather
        if ed.size(0) == 0:
            block.append(nat.cand_ce_empty_stat(B, DEV))
        elif nat.score_ce_supported(xd, ed):
            block.append(nat.score_ce_fold(nat.score_ce_logits(xd, ed, bd, mask)[1], ed.size(0)))
        else:
            block.append(None)
    assert (block[0] is None) == (B % 4 != 0)
    if block[0] is None:      # the second form's records: taken from a first pass of the Function itself, so _Played's own-record
        # check only says that two passes give the same bits; the float64 bars on g, the loss and the gradients carry this case
        seen = {}

        class _Spy(_Played):
            def gather_stats(self, stat):
                seen[self.rank] = stat.clone()
                return torch.stack([stat] * self.world)
        for r, (xd, ed, bd, mask) in enumerate(shards):
            pkg.autograd._ScoreCEFn.apply(xd, ed, bd, mask, eps, N, _Spy(r, torch.zeros((3, B, 4), device=DEV)))
        block = [seen[r] for r in range(3)]
    block = torch.stack(block)
    glob = nat.cand_ce_merge(block, part_dim=0)
    m, s, nl, npos = nat.cand_ce_stat_fields(glob)
    assert bool((nl == N).all()) and torch.equal(npos.cpu().long(), y.sum(1))
    whole = T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B)
    loss_sum, dx_sum, loss_bar, dx_bar = 0.0, torch.zeros((B, dim), dtype=torch.float64), 0.0, torch.zeros((B, dim), dtype=torch.float64)
    for r, (xd, ed, bd, mask) in enumerate(shards):
        a, e = bounds[r], bounds[r + 1]
        ex = _Played(r, block)
        out = _apply(pkg, xd, ed, bd, mask, eps, N, ex)
        assert ex.calls == 1                              # a rank without rows joins the all-gather too
        ref = T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B, row0=a, n_local=e - a)
        n_partials = int(nat.lib().mgcn_score_ce_partials(B, e - a))
        if e > a:
            _hold('rank %d of 3, B=%d' % (r, B), ref, x, ent[a:e], dim, out, n_partials)
        else:
            assert float(out[0]) == 0.0 and out[1].numel() == 0 and not bool(out[2].any()) and out[3].numel() == 0
        _, rowbar = T.logit_bars(ref, dim)
        loss_sum, dx_sum = loss_sum + float(out[0].double()), dx_sum + out[2].cpu().double()
        loss_bar += T.loss_bar(ref, rowbar, 1.0 / B, n_partials)
        dx_bar += T.grad_bars(ref, x, ent[a:e], rowbar, 1.0 / B)[0]
    assert abs(loss_sum - whole['loss']) <= loss_bar + C.gamma(3) * abs(whole['loss'])
    assert float(((dx_sum - whole['dx']).abs() / (dx_bar + C.gamma(3) * whole['dx'].abs())).max()) <= 1.0


def test_batches_the_logits_launch_refuses_take_the_second_form(pkg):
    """B = 5, and a misaligned view of x at B = 8: the same bars."""
    nat = pkg._native
    n, dim, eps = 95, 20, 0.1
    for B, view in ((5, False), (8, True), (7, True)):
        x, ent, bias, y = T.problem(B, n, dim, R.seed_of(94, B))
        xd, ed, bd, mask = _on_device(pkg, x, ent, bias, y)
        if view:
            wide = torch.full((B, dim + 3), float('nan'), device=DEV)
            wide[:, 1:1 + dim] = xd
            xd = wide[:, 1:1 + dim]
        assert not nat.score_ce_supported(xd, ed)
        with pytest.raises(nat.NativeError, match='score_ce_logits'):
            nat.score_ce_logits(xd, ed, bd, mask)
        ref = T.ref_table_ce(x, ent, bias, y, eps, 1.0 / B)
        out = _apply(pkg, xd, ed, bd, mask, eps, n)
        _hold('second form B=%d view=%s' % (B, view), ref, x, ent, dim, out, int(nat.lib().mgcn_score_ce_partials(B, n)))


def _adam_state(opt):
    return [(st['exp_avg'], st['exp_avg_sq'], st['step']) for g in opt.param_groups for p in g['params'] for st in [opt.state.get(p)] if st]


@pytest.mark.parametrize('layers', [1, 2])
def test_four_routes_agree_bit_for_bit(pkg, layers):
    """Three steps at counter dropout 0.3 with ClipAdam from the same state through forward_loss(loss='softmax') + backward +
    clip_and_step, train_device_labels(loss='softmax'), CapturedTrainStep(loss='softmax') (a warm-up step, the capture with its
    first replay, a replay) and train_step_sharded(loss='softmax') at one rank: the losses, every state_dict entry and the Adam
    state have the same bits. Changing step.loss re-captures. The softmax is not the BCE."""
    twins = [_twin(pkg, layers) for _ in range(4)]
    for m, _, _, _ in twins:
        m.params.lbl_smooth, m.params.clip_grad = SMOOTH, CLIP
    (a, dl_a, idx_a, opt_a), (b, dl_b, idx_b, opt_b), (c, dl_c, idx_c, opt_c), (d, dl_d, idx_d, opt_d) = twins
    batches = _repeating_batches(dl_a, 3)
    queries = torch.cat(batches)
    order = torch.randperm(queries.size(0), generator=torch.Generator().manual_seed(11))
    shuffled = queries.new_empty(queries.shape)
    shuffled[order.to(DEV)] = queries                     # the epoch's shuffle then yields `batches` in order
    losses = []
    for q in batches:
        opt_a.zero_grad()
        loss = a.forward_loss(q[:, 0], q[:, 1], dl_a.graph, idx_a, lbl_smooth=SMOOTH, loss='softmax')
        loss.backward()
        opt_a.clip_and_step(CLIP)
        losses.append(loss.detach().clone())
    avg = pkg.utils.RunningAverage()
    for v in losses:
        avg.update(v.item())
    got_b = pkg.harness.train_device_labels(b, shuffled, idx_b, dl_b.graph, opt_b, b.params, 16, generator=torch.Generator().manual_seed(11),
                                            loss='softmax')
    assert got_b == avg()
    _assert_same_state(a, opt_a, b, opt_b)
    step = pkg.CapturedTrainStep(c, dl_c.graph, idx_c, opt_c, lbl_smooth=SMOOTH, clip=CLIP, warmup=1, loss='softmax')
    for q, want in zip(batches, losses):
        assert torch.equal(step(q[:, 0], q[:, 1]).clone(), want)
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 2, 1, False)
    _assert_same_state(a, opt_a, c, opt_c)
    for q, want in zip(batches, losses):
        got = pkg.dist.train_step_sharded(d, dl_d.graph, q[:, 0], q[:, 1], idx_d, opt_d, lbl_smooth=SMOOTH, clip=CLIP, loss='softmax')
        assert torch.equal(got, want)
    _assert_same_state(a, opt_a, d, opt_d)
    # `loss` is part of the capture key
    step.loss = 'bce'
    opt_a.zero_grad()
    want = a.forward_loss(batches[0][:, 0], batches[0][:, 1], dl_a.graph, idx_a, lbl_smooth=SMOOTH)
    want.backward()
    opt_a.clip_and_step(CLIP)
    assert torch.equal(step(batches[0][:, 0], batches[0][:, 1]).clone(), want.detach()) and step.captures == 2
    assert not torch.equal(want.detach(), losses[0])
    _assert_same_state(a, opt_a, c, opt_c)


def test_the_default_is_the_call_as_it_was(pkg):
    """loss='bce' given explicitly equals the call without the argument, bit for bit, on the eager, sharded and epoch routes (the
    captured step: test_captured_step_default_is_bce); other strings are refused before anything runs."""
    (a, dl_a, idx_a, opt_a), (b, dl_b, idx_b, opt_b) = _twin(pkg), _twin(pkg)
    for m in (a, b):
        m.params.lbl_smooth, m.params.clip_grad = SMOOTH, CLIP
    q = _repeating_batches(dl_a, 1)[0]
    queries = dl_a.train_queries()[:40]
    for _ in range(2):
        opt_a.zero_grad()
        la = a.forward_loss(q[:, 0], q[:, 1], dl_a.graph, idx_a, lbl_smooth=SMOOTH)
        la.backward()
        opt_a.clip_and_step(CLIP)
        opt_b.zero_grad()
        lb = b.forward_loss(q[:, 0], q[:, 1], dl_b.graph, idx_b, lbl_smooth=SMOOTH, loss='bce')
        lb.backward()
        opt_b.clip_and_step(CLIP)
        assert torch.equal(la.detach(), lb.detach())
        assert torch.equal(pkg.dist.train_step_sharded(a, dl_a.graph, q[:, 0], q[:, 1], idx_a, opt_a, lbl_smooth=SMOOTH, clip=CLIP),
                           pkg.dist.train_step_sharded(b, dl_b.graph, q[:, 0], q[:, 1], idx_b, opt_b, lbl_smooth=SMOOTH, clip=CLIP, loss='bce'))
    assert pkg.harness.train_device_labels(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, generator=torch.Generator().manual_seed(3)) == \
        pkg.harness.train_device_labels(b, queries, idx_b, dl_b.graph, opt_b, b.params, 16, generator=torch.Generator().manual_seed(3), loss='bce')
    assert pkg.dist.train_epoch_sharded(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, generator=torch.Generator().manual_seed(5)) == \
        pkg.dist.train_epoch_sharded(b, queries, idx_b, dl_b.graph, opt_b, b.params, 16, generator=torch.Generator().manual_seed(5), loss='bce')
    _assert_same_state(a, opt_a, b, opt_b)
    before = {k: v.clone() for k, v in a.state_dict().items()}
    for call in (lambda: a.forward_loss(q[:, 0], q[:, 1], dl_a.graph, idx_a, loss='ce'),
                 lambda: pkg.dist.train_step_sharded(a, dl_a.graph, q[:, 0], q[:, 1], idx_a, opt_a, loss='ce'),
                 lambda: pkg.harness.train_device_labels(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, loss='ce'),
                 lambda: pkg.harness.train_device_labels(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, loss='softmax', fused_loss=False),
                 lambda: pkg.CapturedTrainStep(a, dl_a.graph, idx_a, opt_a, loss='ce')(q[:, 0], q[:, 1])):
        with pytest.raises(pkg._native.NativeError):
            call()
    assert all(torch.equal(v, before[k]) for k, v in a.state_dict().items())


def test_captured_step_default_is_bce(pkg):
    """CapturedTrainStep(loss='bce') (a warm-up step, the capture with its first replay, a replay) against the eager step that
    names no loss, bit for bit; a step built without the argument holds 'bce'. One captured step is alive at a time, as in
    tests/test_gpu_captured_step.py."""
    (a, dl_a, idx_a, opt_a), (b, dl_b, idx_b, opt_b) = _twin(pkg), _twin(pkg)
    assert pkg.CapturedTrainStep(a, dl_a.graph, idx_a, opt_a).loss == 'bce'
    step = pkg.CapturedTrainStep(a, dl_a.graph, idx_a, opt_a, lbl_smooth=SMOOTH, clip=CLIP, warmup=1, loss='bce')
    for q in _repeating_batches(dl_a, 3):
        opt_b.zero_grad()
        want = b.forward_loss(q[:, 0], q[:, 1], dl_b.graph, idx_b, lbl_smooth=SMOOTH)
        want.backward()
        opt_b.clip_and_step(CLIP)
        assert torch.equal(step(q[:, 0], q[:, 1]).clone(), want.detach())
    assert (step.captures, step.replays, step.eager_steps, step.disabled) == (1, 2, 1, False)
    _assert_same_state(a, opt_a, b, opt_b)


def test_sharded_epoch_takes_its_last_batch(pkg):
    """An epoch of 40 queries in batches of 16 leaves a last batch of 8; one of 38 leaves 6 (B % 4 != 0): train_epoch_sharded at
    one rank equals train_device_labels bit for bit under the softmax, and neither fails on the last batch."""
    (a, dl_a, idx_a, opt_a), (b, dl_b, idx_b, opt_b) = _twin(pkg), _twin(pkg)
    for m in (a, b):
        m.params.lbl_smooth, m.params.clip_grad = SMOOTH, CLIP
    for count in (40, 38):
        queries = dl_a.train_queries()[:count]
        got = pkg.dist.train_epoch_sharded(a, queries, idx_a, dl_a.graph, opt_a, a.params, 16, generator=torch.Generator().manual_seed(5),
                                           loss='softmax')
        want = pkg.harness.train_device_labels(b, queries, idx_b, dl_b.graph, opt_b, b.params, 16, generator=torch.Generator().manual_seed(5),
                                               loss='softmax')
        assert got == want and np.isfinite(got)
    _assert_same_state(a, opt_a, b, opt_b)


# -- two processes on one GPU over gloo -------------------------------------------------------------------------------
JOBS = [('even', 8), ('odd', 6)]          # the logits launch; the second form (B % 4 != 0)


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
    out = {}
    for name, B in JOBS:
        sm, dl, params = _models(pkg, 'syn_b', 1, 0.0, shard=True, world=world, rank=rank)
        idx = dl.train_index().to(DEV)
        opt = torch.optim.Adam(sm.parameters(), lr=1e-3)
        b = _batches(dl, 1, B)[0]
        loss = float(pkg.dist.train_step_sharded(sm, dl.graph, b[:, 0], b[:, 1], idx, opt, lbl_smooth=0.1, loss='softmax'))
        csr, n0, n1 = sm._edge_shard
        counts, sub = csr.shard_slot_counts(n0, n1), csr.shard_ee_sub(n0, n1)
        slots = (torch.arange(sum(counts)) + torch.tensor(sub).repeat_interleave(torch.tensor(counts))).to(DEV)
        tables = {n: p for n, p in sm._edge_tables()}
        out[name] = dict(losses=[loss], rows=(n0, n1), ref_ids=_np(csr.perm.index_select(0, slots)),
                         grads={n: _np(p.grad) for n, p in sm.named_parameters() if p.grad is not None},
                         state={k: _np(v) for k, v in sm.state_dict().items() if k not in tables},
                         tables={n: _np(t) for n, t in tables.items()})
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_the_single_step(pkg):
    """Two processes over gloo, one softmax step of syn_b each at B = 8 and B = 6, dropout 0, lbl_smooth 0.1: the loss is the
    one-process forward_loss(loss='softmax') step's to 1e-5, every gradient matches it with
    test_two_ranks_one_gpu_match_golden_and_single_step's tolerances (the table gradient reassembled from both shards),
    replicated gradients and state are bit-identical on the two ranks, the table rows after the step match to 1e-5."""
    import torch.multiprocessing as mp
    _PORTS[0] += 1
    world, port = 2, 31700 + (os.getpid() * 7 + 50 * _PORTS[0] + 25) % 2000
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
    for name, B in JOBS:
        ref, dl, params = _models(pkg, 'syn_b', 1)
        idx = dl.train_index().to(DEV)
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
        b = _batches(dl, 1, B)[0]
        n0, n1 = got[0][name]['rows']
        assert 0 < n1 < dl.num_entity and got[1][name]['rows'] == (n1, dl.num_entity)
        opt.zero_grad()
        loss = ref.forward_loss(b[:, 0], b[:, 1], dl.graph, idx, lbl_smooth=0.1, loss='softmax')
        loss.backward()
        want_grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}
        opt.step()
        inv = ref._slot_csr.inv_perm
        for n in want_grads:
            if n.startswith('edge_embeddings'):
                want_grads[n] = want_grads[n].index_select(0, inv)   # slot order -> reference order
        for r in (0, 1):
            assert abs(got[r][name]['losses'][0] - float(loss.detach())) < 1e-5, (name, r)
        tgrads = _assemble(got, name, 'grads')
        for n, want in want_grads.items():
            gr = tgrads[n] if n.startswith('edge_embeddings') else got[0][name]['grads'][n]
            if not n.startswith('edge_embeddings'):
                assert np.array_equal(got[0][name]['grads'][n], got[1][name]['grads'][n]), (name, n)
            ref_g = want.cpu()
            scale = float(ref_g.abs().max()) + 1e-12
            floor = 2e-6 if n.startswith('conv2.') else 1e-9
            np.testing.assert_allclose(gr, ref_g.numpy(), rtol=2e-3, atol=2e-5 * scale + floor, err_msg='%s %s' % (name, n))
        for k, v in got[0][name]['state'].items():           # replicated state: the same bits on both ranks
            assert np.array_equal(v, got[1][name]['state'][k]), (name, k)
        ref_sd = ref.state_dict()
        for tname, t in _assemble(got, name, 'tables').items():
            np.testing.assert_allclose(t, ref_sd[tname].cpu().numpy(), rtol=0, atol=1e-5, err_msg=tname)
