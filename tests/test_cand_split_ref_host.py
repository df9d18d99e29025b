"""The list backward with split runs (include/mgcn_hip.h (18)) without a GPU: the numpy-f32 emulation of tests/cand_split_ref.py
against the unsplit emulation, against itself on a partition of the table and against float64 within the summation bound; the
workspace slot formula by brute force; _native.cand_plan(keys=True) on CPU tensors; the refusals that precede the first HIP call."""
import itertools

import pytest
import torch

from . import cand_split_ref as S_
from . import cand_train_ref as C
from . import dense_ref as R


def inputs(cand, dim, seed):
    B, K = cand.shape
    gen = R.gen(seed)
    x = R.pm_uniform((B, dim), gen)
    g = R.randn_scaled((B, K), gen, 1.0)
    g[0, 0] = -0.0
    return x, g


def cases():
    yield 'uniform', C.lists(33, 6, 37, 61), 33
    yield 'hub', torch.where(torch.rand((9, 40), generator=R.gen(62)) < 0.5, torch.tensor(3), C.lists(12, 9, 40, 63)), 12
    for S in (16, 24):
        yield 'built-%d' % S, S_.split_lists(S), S_.N_SPLIT


CASES = list(cases())


@pytest.mark.parametrize('name,cand,N', CASES, ids=[c[0] for c in CASES])
def test_a_split_no_shorter_than_the_longest_run_is_the_unsplit_order(name, cand, N):
    x, g = inputs(cand, 5, 64)
    perm, n_live = C.loop_plan(cand, N)
    longest = max(L for _, L, _ in S_.plan_runs(S_.plan_rows(cand, perm, n_live, N)))
    want = C.emul_ent_f32(g, cand, x, perm, n_live, N)
    for S in (longest, longest + 1, 65536):
        got = S_.emul_ent_split_f32(g, cand, x, perm, n_live, N, S)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    if longest > 17:                                   # and a shorter one is another order: the emulation does cut
        cut = S_.emul_ent_split_f32(g, cand, x, perm, n_live, N, 16)
        assert not torch.equal(cut[0], want[0])


@pytest.mark.parametrize('name,cand,N', CASES, ids=[c[0] for c in CASES])
def test_rows_of_a_three_way_partition_equal_the_one_shard_rows(name, cand, N):
    x, g = inputs(cand, 5, 65)
    perm, n_live = C.loop_plan(cand, N)
    bounds = (0, N // 3, N // 3 + 1 + N // 4, N)
    for S in (16, 24):
        whole = S_.emul_ent_split_f32(g, cand, x, perm, n_live, N, S)
        parts = []
        for n0, n1 in zip(bounds, bounds[1:]):
            p, l = C.loop_plan(cand, n1 - n0, n0)
            parts.append(S_.emul_ent_split_f32(g, cand, x, p, l, n1 - n0, S, row0=n0))
        assert torch.equal(torch.cat([p[0] for p in parts]), whole[0]) and torch.equal(torch.cat([p[1] for p in parts]), whole[1])


@pytest.mark.parametrize('name,cand,N', CASES, ids=[c[0] for c in CASES])
def test_split_sums_within_the_summation_bound(name, cand, N):
    """|f32 sum - float64 sum| <= gamma_L sum |addends| for a row named L times: the bound holds for ANY order in which L rounded
    products are added (cand_train_ref.gamma), the split order included: derived, not measured."""
    B, K = cand.shape
    dim = 5
    x, g = inputs(cand, dim, 66)
    perm, n_live = C.loop_plan(cand, N)
    live, row = C.live_rows(cand, 0, N)
    fr, fg = row.reshape(-1), torch.where(live, g.double(), torch.zeros((), dtype=torch.float64)).reshape(-1)
    xr = x.double().repeat_interleave(K, 0)
    de64 = torch.zeros((N, dim), dtype=torch.float64).index_add_(0, fr, fg[:, None] * xr)
    dem = torch.zeros((N, dim), dtype=torch.float64).index_add_(0, fr, fg.abs()[:, None] * xr.abs())
    db64 = torch.zeros(N, dtype=torch.float64).index_add_(0, fr, fg)
    dbm = torch.zeros(N, dtype=torch.float64).index_add_(0, fr, fg.abs())
    cnt = torch.zeros(N, dtype=torch.float64).index_add_(0, fr, live.reshape(-1).double()).clamp(min=1)
    for S in (16, 24):
        de, db = S_.emul_ent_split_f32(g, cand, x, perm, n_live, N, S)
        assert bool(((de.double() - de64).abs() <= C.gamma(cnt)[:, None] * dem).all())
        assert bool(((db.double() - db64).abs() <= C.gamma(cnt) * dbm).all())


def test_built_lists_have_the_runs_they_promise():
    for S in (16, 24):
        cand = S_.split_lists(S)
        perm, n_live = C.loop_plan(cand, 12)
        runs = S_.plan_runs(S_.plan_rows(cand, perm, n_live, 12))
        assert {r: L for _, L, r in runs} == S_.run_lengths(S)
        assert sorted(L for _, L, _ in runs) == sorted([1, S - 1, S, S + 1, 2 * S, 2 * S + 1, S + 1, 2 * S + 1])
        assert bool((cand == -1).any()) and bool((cand == 13).any())
        for _, L, r in runs:                           # a run's entries come from several queries
            assert L == 1 or len(set((cand == r).nonzero()[:, 0].tolist())) > 1
        heads = [(i, first) for i, first, multi in S_.piece_heads(S_.plan_rows(cand, perm, n_live, 12), S) if multi]
        windows = [i // S for i, _ in heads]
        assert len(set(windows)) < len(windows)        # some window holds a head of two runs


def check_slots(rows, S):
    heads = [(i, first) for i, first, multi in S_.piece_heads(rows, S) if multi]
    slots = [S_.slot_of(i, first, S) for i, first in heads]
    assert len(set(slots)) == len(slots), (rows, S)
    assert all(0 <= s < 2 * -(-len(rows) // S) for s in slots)
    firsts = S_.window_first(rows, S)                  # (asserts one per window)
    for w, s in firsts.items():                        # the run holds entry (w + 1) S, whose thread reports it
        assert s < (w + 1) * S < len(rows) and rows[(w + 1) * S] == rows[s]
    return len(heads)


@pytest.mark.parametrize('S', [3, 4])
def test_slots_never_collide_on_every_short_sorted_sequence(S):
    seen = 0
    for n in range(1, 3 * S + 1):
        for cuts in itertools.combinations_with_replacement(range(n + 1), 3):      # where rows 1, 2, 3 begin
            rows = [sum(i >= c for c in cuts) for i in range(n)]
            seen += check_slots(rows, S)
    assert seen > 0


def test_slots_never_collide_on_random_sequences_at_16():
    gen = R.gen(67)
    seen = 0
    for _ in range(300):
        lengths = torch.randint(1, 70, (12,), generator=gen).tolist()
        rows = [r for r, L in enumerate(lengths) for _ in range(L)]
        rows = [r if r % 5 else -1 for r in rows] if len(rows) % 2 else rows     # dead stretches between runs in half of them
        seen += check_slots(rows, 16)
    assert seen > 0


def test_cand_plan_returns_its_sorted_keys_on_request(pkg):
    nat = pkg._native
    cand = S_.split_lists(16)
    for row0, n in ((0, 12), (5, 4), (0, 16)):
        perm, n_live = nat.cand_plan(cand, n, row0)
        p2, l2, keys = nat.cand_plan(cand, n, row0, keys=True)
        assert l2 == n_live and torch.equal(p2, perm) and keys.dtype == torch.int64 and keys.shape == perm.shape
        live, row = C.live_rows(cand, row0, n)
        want = torch.where(live, row, torch.tensor(n)).reshape(-1) * cand.numel() + torch.arange(cand.numel())
        assert torch.equal(keys, want[perm]) and bool((keys[1:] > keys[:-1]).all())
        assert len(nat.cand_plan(cand, n, row0, count=False, keys=True)) == 3


@pytest.mark.parametrize('bad', [15, 65537, 16.0, True, '16', 0, -16])
def test_a_run_split_outside_its_domain_is_refused_before_any_launch(pkg, bad):
    """CPU tensors throughout: a call that got as far as a launch would fail on them with another message."""
    nat = pkg._native
    cand = S_.split_lists(16)
    x, g = inputs(cand, 5, 68)
    perm, n_live, keys = nat.cand_plan(cand, 12, keys=True)
    with pytest.raises(nat.NativeError, match='run_split'):
        nat.cand_bce_bwd_ent(g, cand, x, perm, n_live, 12, run_split=bad, keys=keys)
    with pytest.raises(nat.NativeError, match='run_split'):
        pkg.model._CandBCEFn.apply(x, torch.zeros(12, 5), torch.zeros(12), cand, cand >= 0, 0.9, 0.1, 0, bad)


def test_run_split_needs_the_keys(pkg):
    nat = pkg._native
    cand = S_.split_lists(16)
    x, g = inputs(cand, 5, 69)
    perm, n_live, keys = nat.cand_plan(cand, 12, keys=True)
    with pytest.raises(nat.NativeError, match='keys'):
        nat.cand_bce_bwd_ent(g, cand, x, perm, n_live, 12, run_split=16)
    with pytest.raises(nat.NativeError, match='keys'):
        nat.cand_bce_bwd_ent(g, cand, x, perm, n_live, 12, run_split=16, keys=keys[:-1])


def test_entry_points_refuse_bad_arguments_without_a_gpu(pkg):
    import ctypes
    lib = pkg._native.lib()
    assert lib.mgcn_cand_bwd_ent_split_workspace(16, 16, 200, 15) == 0 and lib.mgcn_cand_bwd_ent_split_workspace(16, 16, 200, 65537) == 0
    assert lib.mgcn_cand_bwd_ent_split_workspace(16, 16, 0, 16) == 0 and lib.mgcn_cand_bwd_ent_split_workspace(-1, 16, 200, 16) == 0
    need = lib.mgcn_cand_bwd_ent_split_workspace(128, 4096, 200, 64)
    assert need % 16 == 0 and 2 * (128 * 4096 // 64) * 201 * 4 <= need <= 2 * (128 * 4096 // 64) * 201 * 4 + 128 * 4096 + 8 * 8192 + 64
    P = 64                                              # a non-null, 16-byte aligned address that no refused call follows

    def call(keys=P, S=16, ws=P, ws_bytes=None):
        nb = lib.mgcn_cand_bwd_ent_split_workspace(4, 8, 5, 16) if ws_bytes is None else ws_bytes
        return lib.mgcn_cand_bce_bwd_ent_split(4, 8, 12, 0, 5, P, 8, P, 8, P, 32, P, 5, P, 5, P, keys, S, ws, nb, None)

    for kw in (dict(keys=None), dict(S=15), dict(S=65537), dict(ws=None), dict(ws=P + 4), dict(ws_bytes=16)):
        assert call(**kw) != 0, kw
        assert lib.mgcn_last_error()
