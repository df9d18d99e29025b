"""Filtered top-k link prediction (section (7) of mgcn_hip.h) on a real MI355X. "Expected" is always: take
_native.score_fwd's block, drop the filtered columns, stable sort descending (ids ascending within a tie), first k, pad
with (-inf, -1). Ids and scores are compared with torch.equal."""
import os
import types

import pytest
import torch

from .conftest import FULL_CASES, GOLDEN, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def unpack(mask, n):
    """Bit-packed int32 filter rows -> bool [B, n]."""
    col = torch.arange(n, device=mask.device)
    words = mask.long().index_select(1, col >> 5) & 0xffffffff
    return ((words >> (col & 31)) & 1).bool()


def pack(dense):
    """bool [B, n] -> bit-packed int32 rows [B, ceil(n / 32)] (the layout of filter_mask)."""
    B, n = dense.shape
    words = (n + 31) // 32
    pad = torch.zeros((B, words * 32), dtype=torch.int64, device=dense.device)
    pad[:, :n] = dense.long()
    v = (pad.view(B, words, 32) << torch.arange(32, device=dense.device)).sum(2)
    return (((v + (1 << 31)) % (1 << 32)) - (1 << 31)).to(torch.int32).contiguous()


def expected(score, k, filtered=None, row0=0):
    B, n = score.shape
    s = score if filtered is None else torch.where(filtered, torch.full_like(score, float('-inf')), score)
    vals, idx = torch.sort(s, dim=1, descending=True, stable=True)
    live = torch.ones_like(score, dtype=torch.bool) if filtered is None else ~filtered
    nvalid = live.sum(1, keepdim=True)
    out_s = torch.full((B, k), float('-inf'), device=score.device)
    out_i = torch.full((B, k), -1, dtype=torch.int64, device=score.device)
    m = min(k, n)
    out_s[:, :m], out_i[:, :m] = vals[:, :m], idx[:, :m] + row0
    pos = torch.arange(k, device=score.device)[None, :]
    out_s[pos >= nvalid] = float('-inf')
    out_i[pos >= nvalid] = -1
    return out_s, out_i


def check(pkg, x, ent, bias, k, mask=None, row0=0):
    nat = pkg._native
    got_s, got_i = nat.score_topk(x, ent, bias, k, mask=mask, ent_row0=row0)
    score = nat.score_fwd(x, ent, bias)
    want_s, want_i = expected(score, k, unpack(mask, ent.size(0)) if mask is not None else None, row0)
    assert torch.equal(got_i, want_i)
    assert torch.equal(got_s, want_s)
    return got_s, got_i


@pytest.fixture(scope='module')
def wn():
    """WN18RR shape: N = 40 943 entities, O = 200."""
    g = torch.Generator(device=DEV).manual_seed(11)
    N, O = 40943, 200
    x = torch.randn(333, O, device=DEV, generator=g) * 0.3
    ent = torch.randn(N, O, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g) * 0.2
    filt = torch.rand(333, N, device=DEV, generator=g) < 0.3
    filt[5] = True                                               # a row with every entity filtered
    return x, ent, bias, pack(filt)


@pytest.mark.parametrize('B', [1, 63, 128, 333])
@pytest.mark.parametrize('k', [1, 10, 100, 1024])
@pytest.mark.parametrize('filtered', [False, True])
def test_topk_wn18rr_shape(pkg, wn, B, k, filtered):
    x, ent, bias, mask = wn
    s, i = check(pkg, x[:B], ent, bias, k, mask=mask[:B] if filtered else None)
    live = torch.ones(B, dtype=torch.bool, device=DEV)
    if filtered and B > 5:
        live[5] = False                                          # the all-filtered row: nothing but padding
        assert (i[5] == -1).all() and (s[5] == float('-inf')).all()
    assert (i[live] >= 0).all()


def test_topk_exact_f32_path(pkg):
    """Shapes the six-product split declines (dim % 4 != 0; an entity view with an odd leading dimension) take the
    exact-f32 tile kernel in score_fwd and in score_topk alike."""
    g = torch.Generator(device=DEV).manual_seed(12)
    N = 40943
    x = torch.randn(128, 198, device=DEV, generator=g) * 0.3
    ent = torch.randn(N, 198, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g) * 0.2
    mask = pack(torch.rand(128, N, device=DEV, generator=g) < 0.2)
    for k in (10, 100):
        check(pkg, x, ent, bias, k)
        check(pkg, x, ent, bias, k, mask=mask)
    # the same operands padded to O = 200 and aligned take the split: a different arithmetic, so the O = 198 block really
    # came from the other kernel
    x2 = torch.zeros(128, 200, device=DEV)
    e2 = torch.zeros(N, 200, device=DEV)
    x2[:, :198], e2[:, :198] = x, ent
    assert not torch.equal(pkg._native.score_fwd(x2, e2, bias), pkg._native.score_fwd(x, ent, bias))
    # an entity view with an odd leading dimension (201 floats): rows not 16-byte aligned
    big = torch.randn(N, 201, device=DEV, generator=g) * 0.1
    view = big[:, :200]
    assert view.stride(0) == 201
    xs = torch.randn(63, 200, device=DEV, generator=g) * 0.3
    for k in (1, 10, 1024):
        check(pkg, xs, view, bias, k)
    assert not torch.equal(pkg._native.score_fwd(xs, view, bias), pkg._native.score_fwd(xs, view.contiguous(), bias))


def test_topk_ties_in_id_order(pkg):
    g = torch.Generator(device=DEV).manual_seed(13)
    N, O = 40943, 200
    ent = torch.randn(N, O, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g) * 0.2
    ent[20000:30000], bias[20000:30000] = ent[0:10000], bias[0:10000]       # duplicated rows, equal bias
    x = torch.randn(64, O, device=DEV, generator=g) * 0.3
    x[:32] *= 60.0                                                           # logits far above 17: many exact 1.0f
    mask = pack(torch.rand(64, N, device=DEV, generator=g) < 0.1)
    for k in (10, 100, 1024):
        for m in (None, mask):
            s, i = check(pkg, x, ent, bias, k, mask=m)
            same = s[:, 1:] == s[:, :-1]
            assert bool(same.any())
            assert bool((i[:, 1:][same] > i[:, :-1][same]).all())          # ids ascend within every tie
    s, _ = pkg._native.score_topk(x[:32], ent, bias, 1024)
    assert int((s == 1.0).sum(1).min()) >= 100                               # the saturated rows do tie at 1.0f


def test_topk_chunked_shard(pkg):
    """600 k rows at O = 64: three chunks of at most 2^18 rows folded through the merge; equal to the single-pass
    expected result, and the same on every call."""
    g = torch.Generator(device=DEV).manual_seed(14)
    N, O, B = 600000, 64, 128
    ent = torch.randn(N, O, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g) * 0.2
    ent[500000:510000], bias[500000:510000] = ent[10:10010], bias[10:10010]   # ties across chunks
    x = torch.randn(B, O, device=DEV, generator=g) * 0.5
    mask = pack(torch.rand(B, N, device=DEV, generator=g) < 0.25)
    for k in (10, 1024):
        for m in (None, mask):
            s, i = check(pkg, x, ent, bias, k, mask=m)
            for _ in range(2):
                s2, i2 = pkg._native.score_topk(x, ent, bias, k, mask=m)
                assert torch.equal(s, s2) and torch.equal(i, i2)


def _known(N, keys, g, per_key=40):
    known = {}
    for key in keys:
        tails = torch.randint(0, N, (per_key,), generator=g).tolist()
        known[(key, 0)] = set(tails)
    return known


def test_topk_fb15k237_shards_merge(pkg):
    """configs[3]'s split: FB15k-237's 14 541 rows in 8 shards of 1 818 (1 815 in the last), played in one process
    through ent_row0; topk_merge of the eight local lists equals the unsharded call."""
    nat, d = pkg._native, pkg.dist
    gd = torch.Generator(device=DEV).manual_seed(15)
    N, O, B = 14541, 200, 128
    ent = torch.randn(N, O, device=DEV, generator=gd) * 0.1
    bias = torch.randn(N, device=DEV, generator=gd) * 0.2
    ent[9000:9100], bias[9000:9100] = ent[100:200], bias[100:200]       # ties across shards
    x = torch.randn(B, O, device=DEV, generator=gd) * 0.3
    g = torch.Generator().manual_seed(15)
    filt = d.FilterIndex.from_known(_known(N, range(B), g, per_key=600), 1).to(DEV)
    qkey = torch.arange(B, device=DEV, dtype=torch.int64)
    b = d.shard_bounds(N, 8)
    assert [b[r + 1] - b[r] for r in range(8)] == [1818] * 7 + [1815]
    for k in (10, 100, 1024):
        for use_filter in (False, True):
            full_mask = nat.filter_mask(qkey, filt.keys, filt.ptr, filt.tails, N) if use_filter else None
            want_s, want_i = check(pkg, x, ent, bias, k, mask=full_mask)
            lists_s, lists_i = [], []
            for r in range(8):
                n0, n1 = b[r], b[r + 1]
                m = nat.filter_mask(qkey, filt.keys, filt.ptr, filt.tails, n1 - n0, ent_row0=n0) if use_filter else None
                s, i = check(pkg, x, ent[n0:n1], bias[n0:n1], k, mask=m, row0=n0)
                lists_s.append(s)
                lists_i.append(i)
            s, i = nat.topk_merge(torch.cat(lists_s, 1), torch.cat(lists_i, 1), k)
            assert torch.equal(i, want_i) and torch.equal(s, want_s)
            # the lists in another order merge to the same result (the order is total)
            s, i = nat.topk_merge(torch.cat(lists_s[::-1], 1), torch.cat(lists_i[::-1], 1), k)
            assert torch.equal(i, want_i) and torch.equal(s, want_s)


def test_topk_agrees_with_rank_counts(pkg):
    """With the target's own bit cleared, its 0-based position in the list is gt + ties_lower of score_rank, and it is
    absent exactly when gt + ties_lower >= k."""
    nat, d = pkg._native, pkg.dist
    gd = torch.Generator(device=DEV).manual_seed(16)
    N, O, B = 40943, 200, 256
    ent = torch.randn(N, O, device=DEV, generator=gd) * 0.1
    bias = torch.randn(N, device=DEV, generator=gd) * 0.2
    ent[30000:30500], bias[30000:30500] = ent[0:500], bias[0:500]
    x = torch.randn(B, O, device=DEV, generator=gd) * 0.3
    x[:16] *= 60.0                                                      # saturated rows: the rank's tie rule matters
    g = torch.Generator().manual_seed(16)
    filt = d.FilterIndex.from_known(_known(N, range(B), g, per_key=200), 1).to(DEV)
    qkey = torch.arange(B, device=DEV, dtype=torch.int64)
    score = nat.score_fwd(x, ent, bias)
    place = torch.randint(0, 3000, (B,), generator=g)
    place[16:80] = torch.randint(0, 8, (64,), generator=g)             # near the top: present in every list
    obj = score.argsort(1, descending=True)[torch.arange(B, device=DEV), place.to(DEV)].contiguous()
    obj[:16] = torch.randint(0, 500, (16,), generator=g).to(DEV)          # targets inside the duplicated rows
    mask = nat.filter_mask(qkey, filt.keys, filt.ptr, filt.tails, N)
    word, bit = obj >> 5, obj & 31
    rows = torch.arange(B, device=DEV)
    w = mask.long()[rows, word] & ~(1 << bit)
    mask[rows, word] = (((w + (1 << 31)) % (1 << 32)) - (1 << 31)).to(torch.int32)
    target = nat.score_target(x, ent, bias, obj)
    counts = nat.score_rank(x, ent, bias, obj, target, mask=mask)
    pos = counts[:, 0] + counts[:, 1]
    for k in (10, 100, 1024):
        s, i = check(pkg, x, ent, bias, k, mask=mask)
        hit = i == obj[:, None]
        present = hit.any(1)
        assert torch.equal(present, pos < k)
        assert torch.equal(hit.float().argmax(1)[present], pos[present])
        assert bool(present.any()) and (k == 1024 or bool((~present).any()))


def test_topk_padding(pkg):
    g = torch.Generator(device=DEV).manual_seed(17)
    nat = pkg._native
    x = torch.randn(9, 200, device=DEV, generator=g)
    ent = torch.randn(50, 200, device=DEV, generator=g) * 0.1
    bias = torch.randn(50, device=DEV, generator=g)
    for k in (1, 10, 100, 1024):                                         # n_local = 50 < k for the last three
        s, i = check(pkg, x, ent, bias, k, row0=7)
        assert (i[:, :min(k, 50)] >= 7).all() and (i[:, 50:] == -1).all() and torch.isinf(s[:, 50:]).all()
        every = torch.full((9, 2), -1, dtype=torch.int32, device=DEV)    # every entity filtered
        s, i = check(pkg, x, ent, bias, k, mask=every)
        assert (i == -1).all() and (s == float('-inf')).all()
    # an empty shard and an empty merge pad every row
    s, i = nat.score_topk(x, ent[:0], bias[:0], 5)
    assert (i == -1).all() and (s == float('-inf')).all()
    s, i = nat.topk_merge(torch.empty((9, 0), device=DEV), torch.empty((9, 0), dtype=torch.int64, device=DEV), 5)
    assert (i == -1).all() and (s == float('-inf')).all()


def _model(pkg, g):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**g.hp)
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    missing = model.load_state_dict(g.state_dict(), strict=False)
    assert not missing.unexpected_keys
    return model.to(DEV), dl


@pytest.mark.parametrize('case', FULL_CASES)
def test_model_predict_topk_vs_forward_and_reference(pkg, case):
    g = golden(case)
    model, dl = _model(pkg, g)
    model.eval()
    N = dl.num_entity
    filt = dl.filter_index().to(DEV)
    tol = 2e-5                                             # the parity tolerance of the forward scores
    for split in ('valid_tail', 'valid_head', 'test_tail', 'test_head'):
        trip = g.t('dl_q_%s_triple' % split).to(DEV)
        src, rel = trip[:, 0], trip[:, 1]
        with torch.no_grad():
            score = model(src, rel, dl.graph)
        mask = pkg._native.filter_mask(filt.query_keys(src, rel), filt.keys, filt.ptr, filt.tails, N)
        for k in (1, 10, N):
            ids, s = model.predict_topk(src, rel, dl.graph, k=k)
            want_s, want_i = expected(score, k)
            assert torch.equal(ids, want_i) and torch.equal(s, want_s), (split, k)
            ids_f, s_f = model.predict_topk(src, rel, dl.graph, k=k, filter_index=filt)
            want_s, want_i = expected(score, k, unpack(mask, N))
            assert torch.equal(ids_f, want_i) and torch.equal(s_f, want_s), (split, k)
            assert not model.training
            # the reference's own ranking wherever its consecutive scores are further apart than the parity tolerance
            ref = torch.from_numpy(g['eval_%s_score' % split])
            maxdiff = float((score.cpu() - ref).abs().max())
            assert maxdiff <= tol
            rv, ri = torch.sort(ref, dim=1, descending=True, stable=True)
            gap = rv[:, :-1] - rv[:, 1:]
            big = torch.ones((ref.size(0), N + 1), dtype=torch.bool)
            big[:, 1:N] = gap > max(tol, 2 * maxdiff)
            decided = (big[:, :-1] & big[:, 1:])[:, :min(k, N)]    # position j: apart from both neighbours
            assert torch.equal(ids.cpu()[:, :min(k, N)][decided], ri[:, :min(k, N)][decided])
            if k == 1:
                assert int(decided.sum()) > 0
    if case == 'toy_small':                                # 7 entities: k = 10 pads through the public API
        assert N == 7
        ids, s = model.predict_topk(src, rel, dl.graph, k=10)
        assert (ids[:, :7] >= 0).all() and (ids[:, 7:] == -1).all() and torch.isinf(s[:, 7:]).all()


@pytest.mark.parametrize('case', FULL_CASES)
def test_predict_topk_sharded_world1_equals_predict_topk(pkg, case):
    g = golden(case)
    model, dl = _model(pkg, g)
    model.eval()
    filt = dl.filter_index().to(DEV)
    q = dl.eval_queries('test')[:, :2]
    src, rel = q[:, 0].to(DEV), q[:, 1].to(DEV)
    for k in (3, 10):
        for f in (None, filt):
            ids, s = pkg.dist.predict_topk_sharded(model, dl.graph, q, k, filt=f)
            want_i, want_s = model.predict_topk(src, rel, dl.graph, k=k, filter_index=f)
            assert torch.equal(ids, want_i) and torch.equal(s, want_s)
            ids2, s2 = pkg.dist.predict_topk_sharded(model, dl.graph, q, k, filt=f, trunk_chunk=5)
            assert ids2.shape == (q.size(0), k) and s2.shape == (q.size(0), k)
