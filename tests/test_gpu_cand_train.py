"""Training on per-query candidate lists (include/mgcn_hip.h (14)) on a real MI355X.

  * g against mgcn_score_bce_fwd's grad_logit gathered at the candidates: torch.equal, no tolerance (the header's contract);
  * g on the shapes that entry point refuses, and the loss everywhere, against float64 with dense_ref's own bars for this formula;
  * the two backward sums against the numpy-f32 emulations of tests/cand_train_ref.py, bit for bit;
  * labels against the bits of _native.filter_mask; poison in everything a launch must not write; refusals; bad plans;
  * MGCN.forward_loss_candidates against a composition of the same calls (bits) and against forward_loss (its tolerances);
    two seeded runs of harness.train_sampled_negatives; the bf16 model's refusal.
"""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from . import cand_train_ref as C
from . import dense_ref as R
from .conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = ctypes.c_float


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


# ---------------------------------------------------------------------------------------------------------------- g, bit for bit
# (B, N, dim, K, entities of the mean): the shapes mgcn_score_bce_fwd takes. dim = 200 is the case that matters: score_fwd takes
# the six-product split there and the BCE launch does not.
BIT_CASES = [(4, 33, 4, 17, None), (36, 1000, 36, 65, None), (4, 100, 200, 130, None), (132, 1000, 36, 63, 4099)]


@pytest.mark.parametrize('scale', [None, 40.0], ids=['plain', 'logits40'])
@pytest.mark.parametrize('B,N,dim,K,total', BIT_CASES, ids=['%d-%d-%d-%d' % c[:4] for c in BIT_CASES])
def test_g_has_the_bits_of_score_bce_fwd(pkg, B, N, dim, K, total, scale):
    nat = pkg._native
    x, ent, bias, hit = (t.to(DEV) for t in R.bce_inputs(B, N, dim, scale))
    hot, cold = nat.smoothed_targets(0.1, N if total is None else total)
    inv = 1.0 / (float(B) * float(N if total is None else total))
    loss_full, G = nat.score_bce_fwd(x, ent, bias, R.pack_bits(hit), hot, cold, num_entities=total)
    cand = C.lists(N, B, K, R.seed_of(41, B, N, dim, K)).to(DEV)
    label = hit.gather(1, cand)
    assert bool(label.any()) and not bool(label.all())
    loss, g = nat.cand_bce_fwd(x, ent, bias, cand, label, hot, cold, inv_count=inv)
    assert g.shape == (B, K) and torch.equal(g, G.t().gather(1, cand))
    loss2, g2 = nat.cand_bce_fwd(x, ent, bias, cand, label.to(torch.uint8), hot, cold, inv_count=inv)
    assert torch.equal(g2, g) and torch.equal(loss2, loss)                       # the same launch twice: the same bits


def test_whole_table_as_the_list_gives_score_bce_fwd(pkg):
    """cand[b] = arange(N): every g, and the loss up to the order of its partial sums."""
    nat = pkg._native
    B, N, dim = 36, 1000, 36
    x, ent, bias, hit = (t.to(DEV) for t in R.bce_inputs(B, N, dim))
    hot, cold = nat.smoothed_targets(0.1, N)
    loss_full, G = nat.score_bce_fwd(x, ent, bias, R.pack_bits(hit), hot, cold)
    cand = torch.arange(N, device=DEV).expand(B, N).contiguous()
    loss, g = nat.cand_bce_fwd(x, ent, bias, cand, hit, hot, cold)
    assert torch.equal(g, G.t())
    assert abs(float(loss) - float(loss_full)) <= 1e-6 * max(1.0, abs(float(loss_full)))


# ---------------------------------------------------------------------------------------------------------------- g and loss, float64
DEAD = (-1, None, 2 ** 62, -2 ** 62)                  # None: N itself


def with_dead(cand, N):
    B, K = cand.shape
    if B * K > 4:
        for i, v in enumerate(DEAD):
            cand[i % B, (3 * i + 1) % K] = N if v is None else v
    return cand


# (B, K, N, dim, layout of x / ent): dim 4 7 36 200, B 1 4 5 36, K around the 16-row tile and the 64-position chunk, N 33 1000; every
# value of an axis at least twice. B % 4 != 0, dim % 4 != 0 and offset-by-one-float operands are shapes the parent refuses.
GRID = [
    (1, 1, 33, 4, 'contiguous'), (4, 15, 1000, 7, 'contiguous'), (5, 16, 33, 36, 'contiguous'), (36, 17, 1000, 200, 'contiguous'),
    (1, 63, 1000, 7, 'contiguous'), (4, 64, 33, 36, 'offset1'), (5, 65, 1000, 200, 'contiguous'), (36, 130, 33, 4, 'contiguous'),
    (1, 130, 33, 200, 'offset1'), (4, 1, 1000, 36, 'contiguous'), (5, 15, 33, 4, 'offset1'), (36, 16, 1000, 7, 'contiguous'),
    (1, 17, 1000, 36, 'window'), (4, 63, 33, 200, 'contiguous'), (5, 64, 1000, 4, 'contiguous'), (36, 65, 33, 7, 'oddstride'),
    (5, 130, 1000, 36, 'contiguous'), (36, 64, 1000, 200, 'window'),
]


def grid_inputs(B, K, N, dim, seed, scale=None):
    g = R.gen(seed)
    x, ent, bias = R.pm_uniform((B, dim), g), R.pm_uniform((N, dim), g), R.pm_uniform((N,), g)
    if scale is not None:
        s = (scale / float(R.ref_logits(x, ent, bias)[0].abs().max())) ** 0.5
        x, ent, bias = x * s, ent * s, bias * (s * s)
    cand = with_dead(C.lists(N, B, K, seed + 1), N)
    label = torch.rand((B, K), generator=g) < 0.3
    return x, ent, bias, cand, label


def check_against_float64(nat, x, ent, bias, cand, label, hot, cold, inv, cid, row0=0, lay='contiguous'):
    xd, ed = R.layout(x.to(DEV), lay), R.layout(ent.to(DEV), lay)
    loss, g = nat.cand_bce_fwd(xd, ed, bias.to(DEV), cand.to(DEV), label.to(DEV), hot, cold, inv_count=inv, ent_row0=row0)
    ref = C.ref_list_bce(x, ent, bias, cand, label, hot, cold, inv, row0=row0)
    sat = C.ref_list_bce(x, ent, bias, cand, label, hot, cold, inv, row0=row0, saturate_f32=True)
    live = ref['live']
    got = g.cpu()
    assert bool((got[~live] == 0).all()) and bool(torch.isfinite(got).all())
    loss_bar = R.bce_loss_bar(sat['loss'], R.emul_bce_loss_f32(ref['z'][live], ref['y'][live], inv)) if bool(live.any()) else 0.0
    print('RATIO cand_bce_loss %s %.4f' % (cid, abs(float(loss) - sat['loss']) / loss_bar if loss_bar else 0.0))
    assert abs(float(loss) - sat['loss']) <= loss_bar, (cid, float(loss), sat['loss'], ref['loss'])
    logit_bar = R.dot_bar(ref['mag'], x.size(1))
    bar = R.bce_grad_bar(ref['g'], ref['p'], ref['y'], logit_bar, inv)
    # as test_gpu_dense_edges holds mgcn_score_bce_fwd: saturated entries to torch's f32 value, at the edge of saturation either side
    q64 = torch.sigmoid(-ref['z'])
    edge = (q64 >= R.U / 4 * torch.exp(-logit_bar)) & (q64 <= 4 * R.U * torch.exp(logit_bar))
    err = (got.double() - sat['g']).abs() / bar
    either = torch.minimum((got.double() - ref['g']).abs(), got.double().abs()) / bar
    ratio = float(torch.where(edge, either, err)[live].max()) if bool(live.any()) else 0.0
    print('RATIO cand_bce_grad %s %.4f' % (cid, ratio))
    assert ratio <= 1.0, (cid, ratio)
    return g


@pytest.mark.parametrize('B,K,N,dim,lay', GRID, ids=['%d-%d-%d-%d-%s' % c for c in GRID])
def test_g_and_loss_against_float64(pkg, B, K, N, dim, lay):
    nat = pkg._native
    x, ent, bias, cand, label = grid_inputs(B, K, N, dim, R.seed_of(42, B, K, N, dim))
    hot, cold = nat.smoothed_targets(0.1, N)
    check_against_float64(nat, x, ent, bias, cand, label, hot, cold, 1.0 / (B * K), 'grid-%d-%d-%d-%d-%s' % (B, K, N, dim, lay), lay=lay)


@pytest.mark.parametrize('B,K,N,dim', [(5, 65, 1000, 36), (36, 17, 33, 7), (4, 130, 100, 200)])
def test_saturated_logits_against_float64(pkg, B, K, N, dim):
    """Logits up to 40 (f32 p saturates at 1) and unsmoothed targets 1 / 0: the -100 clamp and the 1e-12 floor."""
    nat = pkg._native
    x, ent, bias, cand, label = grid_inputs(B, K, N, dim, R.seed_of(43, B, K, N, dim), scale=40.0)
    check_against_float64(nat, x, ent, bias, cand, label, 1.0, 0.0, 1.0 / (B * K), 'sat-%d-%d-%d-%d' % (B, K, N, dim))


@pytest.mark.parametrize('dim', [36, 7])
def test_shard_window_of_the_table(pkg, dim):
    """ent_row0 = 500, n_local = 300 of N = 1000: ids of the other 700 rows are dead."""
    nat = pkg._native
    B, K, N, row0, n = 5, 65, 1000, 500, 300
    x, ent, bias, cand, label = grid_inputs(B, K, N, dim, R.seed_of(44, dim))
    cand[0, :3] = torch.tensor([499, 500, 799])
    cand[1, :2] = torch.tensor([800, 0])
    live, _ = C.live_rows(cand, row0, n)
    assert bool(live.any()) and not bool(live.all()) and live[0, :3].tolist() == [False, True, True] and live[1, :2].tolist() == [False, False]
    g = check_against_float64(nat, x, ent[row0:row0 + n], bias[row0:row0 + n], cand, label, 0.9, 0.001, 1.0 / (B * K), 'shard-%d' % dim,
                              row0=row0)
    whole = nat.cand_bce_fwd(x.to(DEV), ent.to(DEV), bias.to(DEV), cand.to(DEV), label.to(DEV), 0.9, 0.001)[1]
    assert torch.equal(g.cpu()[live], whole.cpu()[live])                         # a row's g does not depend on the shard it is read from


# ---------------------------------------------------------------------------------------------------------------- labels
def _loader(pkg, g, **over):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**dict(g.hp, **over))
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    return dl, params


@pytest.mark.parametrize('case', ['toy_small', 'syn_a'])
def test_labels_equal_the_filter_mask_bits(pkg, case):
    nat = pkg._native
    dl, _ = _loader(pkg, golden(case))
    N = dl.num_entity
    idx = dl.train_index().to(DEV)
    q = dl.train_queries().to(DEV)
    q = torch.cat([q[:35], torch.tensor([[N + 5, 0]], device=DEV)])             # the last query has no key in the index
    keys = idx.query_keys(q[:, 0], q[:, 1])
    B, K = q.size(0), 70
    cand = torch.randint(-2, N + 2, (B, K), generator=R.gen(45)).to(DEV)
    cand[:, :N] = torch.arange(N, device=DEV)                                   # every entity, so every known tail occurs
    cand[0, K - 1], cand[1, K - 1] = 2 ** 62, -2 ** 62
    for row0, n in ((0, N), (N // 3, N - N // 3 - 1)):
        mask = nat.filter_mask(keys, idx.keys, idx.ptr, idx.tails, n, ent_row0=row0)
        o = cand - row0
        live = (o >= 0) & (o < n)
        col = o.clamp(0, n - 1)
        want = (((mask.long().gather(1, col >> 5) >> (col & 31)) & 1).bool() & live).to(torch.uint8)
        wide = torch.full((B + 1, K + 9), 0xAB, dtype=torch.uint8, device=DEV)
        out = wide[:B, 4:4 + K]
        got = nat.cand_labels(keys, idx.keys, idx.ptr, idx.tails, cand, n, ent_row0=row0, out=out)
        assert got.data_ptr() == out.data_ptr() and got.dtype == torch.uint8 and torch.equal(got, want)
        assert bool(want.any()) and not bool(want[B - 1].any()) and not bool(want[~live].any())
        probe = wide.clone()
        probe[:B, 4:4 + K] = 0xAB
        assert bool((probe == 0xAB).all())
        assert torch.equal(nat.cand_labels(keys, idx.keys, idx.ptr, idx.tails, cand, n, ent_row0=row0), want)
        assert torch.equal(want.cpu(), C.loop_labels(keys, idx.keys, idx.ptr, idx.tails, cand, row0, n))


# ---------------------------------------------------------------------------------------------------------------- the backward sums
def arbitrary_g(B, K, seed):
    g = R.randn_scaled((B, K), R.gen(seed), 1.0)
    g[torch.rand((B, K), generator=R.gen(seed + 1)) < 0.1] = 0.0
    g[0, 0] = -0.0
    return g


BWD = [(1, 1, 33, 4), (4, 15, 33, 7), (5, 16, 1000, 36), (36, 17, 33, 200), (1, 63, 1000, 200), (4, 64, 1000, 4), (5, 65, 33, 7),
       (36, 130, 1000, 36), (4, 130, 33, 200), (36, 65, 1000, 7), (5, 64, 33, 36), (1, 130, 33, 4), (5, 300, 1000, 260)]


@pytest.mark.parametrize('B,K,N,dim', BWD, ids=['%d-%d-%d-%d' % c for c in BWD])
def test_backward_sums_equal_the_f32_emulations(pkg, B, K, N, dim):
    nat = pkg._native
    gen = R.gen(R.seed_of(46, B, K, N, dim))
    x, ent = R.pm_uniform((B, dim), gen), R.pm_uniform((N, dim), gen)
    cand = with_dead(C.lists(N, B, K, R.seed_of(47, B, K, N)), N)
    g = arbitrary_g(B, K, R.seed_of(48, B, K))
    gd, cd, xd, ed = g.to(DEV), cand.to(DEV), x.to(DEV), ent.to(DEV)
    dx = nat.cand_bce_bwd_x(gd, cd, ed)
    assert same_bits(dx, C.emul_dx_f32(g, cand, ent))
    assert same_bits(nat.cand_bce_bwd_x(gd, cd, ed), dx)
    perm, n_live = nat.cand_plan(cd, N)
    want_perm, want_live = C.loop_plan(cand, N)
    assert n_live == want_live and torch.equal(perm.cpu(), want_perm)
    d_ent, d_bias = nat.cand_bce_bwd_ent(gd, cd, xd, perm, n_live, N)
    we, wb = C.emul_ent_f32(g, cand, x, want_perm, want_live, N)
    assert same_bits(d_ent, we) and same_bits(d_bias, wb)
    e2, b2 = nat.cand_bce_bwd_ent(gd, cd, xd, perm, n_live, N)
    assert same_bits(e2, d_ent) and same_bits(b2, d_bias)
    only_b = nat.cand_bce_bwd_ent(gd, cd, xd, perm, n_live, N, want=('bias',))
    only_e = nat.cand_bce_bwd_ent(gd, cd, xd, perm, n_live, N, want=('ent',))
    assert only_b[0] is None and same_bits(only_b[1], d_bias) and only_e[1] is None and same_bits(only_e[0], d_ent)


def test_one_entity_named_by_every_position_is_one_run(pkg):
    """A run of 36 * 65 = 2340 plan entries walked by one wave; and a shard window in which it is the only live row."""
    nat = pkg._native
    B, K, N, dim = 36, 65, 33, 36
    gen = R.gen(49)
    x, ent = R.pm_uniform((B, dim), gen), R.pm_uniform((N, dim), gen)
    cand = torch.full((B, K), 20, dtype=torch.int64)
    g = arbitrary_g(B, K, 50)
    gd, cd, xd, ed = g.to(DEV), cand.to(DEV), x.to(DEV), ent.to(DEV)
    for row0, n in ((0, N), (17, 5)):
        perm, n_live = nat.cand_plan(cd, n, row0)
        assert n_live == B * K and torch.equal(perm.cpu(), torch.arange(B * K))
        d_ent, d_bias = nat.cand_bce_bwd_ent(gd, cd, xd, perm, n_live, n, ent_row0=row0)
        we, wb = C.emul_ent_f32(g, cand, x, perm, n_live, n, row0=row0)
        assert same_bits(d_ent, we) and same_bits(d_bias, wb)
        assert int((d_ent != 0).any(1).sum()) == 1
        assert same_bits(nat.cand_bce_bwd_x(gd, cd, ed[row0:row0 + n], ent_row0=row0), C.emul_dx_f32(g, cand, ent[row0:row0 + n], row0=row0))


# ---------------------------------------------------------------------------------------------------------------- windows and poison
class Launch(object):
    """The operands of one (B, K, dim) problem on a shard window [500, 800) of N = 1000, every one of them a window of a wider
    block whose guard columns are poisoned (NaN operands, ids 2^40 in cand, guard patterns in the outputs)."""

    def __init__(self, pkg, B=5, K=65, dim=36, row0=500, n=300, N=1000):
        self.lib = pkg._native.lib()
        self.B, self.K, self.dim, self.row0, self.n = B, K, dim, row0, n
        gen = R.gen(R.seed_of(51, B, K, dim))
        self.x, self.ent, self.bias = R.pm_uniform((B, dim), gen), R.pm_uniform((n, dim), gen), R.pm_uniform((n,), gen)
        self.cand = with_dead(C.lists(N, B, K, 52), N)
        self.cand[:, 1] = row0 + 7                                              # a row every query names
        self.label = torch.rand((B, K), generator=gen) < 0.3
        self.xw, self.ew = R.layout(self.x.to(DEV), 'window'), R.layout(self.ent.to(DEV), 'window')
        self.bd = self.bias.to(DEV)
        wide = torch.full((B, K + 5), 2 ** 40, dtype=torch.int64, device=DEV)
        self.cw = wide[:, 3:3 + K]
        self.cw.copy_(self.cand)
        lw = torch.full((B, K + 7), 1, dtype=torch.uint8, device=DEV)
        self.lw = lw[:, 2:2 + K]
        self.lw.copy_(self.label)
        self.parts_n = int(self.lib.mgcn_cand_bce_partials(B, K))
        self.fresh()

    def fresh(self):
        B, K, dim, n = self.B, self.K, self.dim, self.n
        self.g = R.Guarded(B, K, K + 3, DEV)
        self.parts = R.Guarded(1, self.parts_n, self.parts_n + 8, DEV)
        self.dx = R.Guarded(B, dim, dim + 4, DEV)
        self.d_ent = R.Guarded(n, dim, dim + 4, DEV)
        self.d_bias = R.Guarded(1, n, n + 8, DEV)

    def fwd(self, **kw):
        a = dict(x=self.xw.data_ptr(), ent=self.ew.data_ptr(), bias=self.bd.data_ptr(), cand=self.cw.data_ptr(), label=self.lw.data_ptr(),
                 g=self.g.ptr(), parts=self.parts.ptr(), ldg=self.g.ld, ldc=self.cw.stride(0), ldl=self.lw.stride(0))
        a.update(kw)
        rc = self.lib.mgcn_cand_bce_fwd(self.B, self.K, self.n, self.row0, self.dim, a['x'], self.xw.stride(0), a['ent'], self.ew.stride(0),
                                        a['bias'], a['cand'], a['ldc'], a['label'], a['ldl'], F(0.9), F(0.001), F(1.0 / (self.B * self.K)),
                                        a['g'], a['ldg'], a['parts'], _stream())
        torch.cuda.synchronize()
        return rc

    def bwd_x(self, g, **kw):
        a = dict(g=g.data_ptr(), ldg=g.stride(0), cand=self.cw.data_ptr(), ent=self.ew.data_ptr(), dx=self.dx.ptr(), ldx=self.dx.ld)
        a.update(kw)
        rc = self.lib.mgcn_cand_bce_bwd_x(self.B, self.K, self.n, self.row0, self.dim, a['g'], a['ldg'], a['cand'], self.cw.stride(0),
                                          a['ent'], self.ew.stride(0), a['dx'], a['ldx'], _stream())
        torch.cuda.synchronize()
        return rc

    def bwd_ent(self, g, plan, n_live, **kw):
        a = dict(g=g.data_ptr(), ldg=g.stride(0), cand=self.cw.data_ptr(), perm=plan.data_ptr(), x=self.xw.data_ptr(),
                 d_ent=self.d_ent.ptr(), lde=self.d_ent.ld, d_bias=self.d_bias.ptr(), n_live=n_live)
        a.update(kw)
        rc = self.lib.mgcn_cand_bce_bwd_ent(self.B, self.K, self.n, self.row0, self.dim, a['g'], a['ldg'], a['cand'], self.cw.stride(0),
                                            a['perm'], a['n_live'], a['x'], self.xw.stride(0), a['d_ent'], a['lde'], a['d_bias'], _stream())
        torch.cuda.synchronize()
        return rc

    def outputs_untouched(self):
        return all(o.untouched() for o in (self.g, self.parts, self.dx, self.d_ent, self.d_bias))


@pytest.mark.parametrize('dim', [36, 7])
def test_windows_keep_their_guards_and_unnamed_rows_their_poison(pkg, dim):
    nat = pkg._native
    L = Launch(pkg, dim=dim)
    assert L.fwd() == 0, L.lib.mgcn_last_error()
    L.g.check('g')
    L.parts.check('loss_partial')
    live, _ = C.live_rows(L.cand, L.row0, L.n)
    g = L.g.view.clone()
    assert bool((g.cpu()[~live] == 0).all()) and not bool(live.all())           # a dead position's g is exactly 0
    plain_loss, plain_g = nat.cand_bce_fwd(L.x.to(DEV), L.ent.to(DEV), L.bd, L.cand.to(DEV), L.label.to(DEV), 0.9, 0.001, ent_row0=L.row0)
    assert torch.equal(g, plain_g)                                               # windows: the same arithmetic on the same values
    assert float(L.parts.view.double().sum()) / (L.B * L.K) == pytest.approx(float(plain_loss), rel=1e-6)
    # backward on arbitrary g, read through a window as well
    ga = arbitrary_g(L.B, L.K, 53)
    gw = R.layout(ga.to(DEV), 'offset1')
    assert L.bwd_x(gw) == 0
    L.dx.check('dx')
    assert same_bits(L.dx.view, C.emul_dx_f32(ga, L.cand, L.ent, row0=L.row0))
    perm, n_live = nat.cand_plan(L.cw, L.n, L.row0)
    assert L.bwd_ent(gw, perm, n_live) == 0
    L.d_ent.check('d_ent')
    L.d_bias.check('d_bias')
    init_e, init_b = R.Guarded(L.n, dim, dim + 4, 'cpu').view, R.Guarded(1, L.n, L.n + 8, 'cpu').view[0]
    we, wb = C.emul_ent_f32(ga, L.cand, L.x, perm, n_live, L.n, row0=L.row0, d_ent=init_e, d_bias=init_b)
    assert same_bits(L.d_ent.view, we) and same_bits(L.d_bias.view[0], wb)
    named = torch.zeros(L.n, dtype=torch.bool)
    named[(L.cand - L.row0)[live]] = True
    assert not bool(named.all())
    assert bool((bits(L.d_ent.view.cpu())[~named] == R.GUARD_F32).all()) and bool((bits(L.d_bias.view[0].cpu())[~named] == R.GUARD_F32).all())
    assert bool(torch.isfinite(L.d_ent.view.cpu()[named]).all())
    # either output alone
    L.fresh()
    assert L.bwd_ent(gw, perm, n_live, d_ent=None) == 0 and L.d_ent.untouched() and same_bits(L.d_bias.view[0], wb)
    L.fresh()
    assert L.bwd_ent(gw, perm, n_live, d_bias=None) == 0 and L.d_bias.untouched() and same_bits(L.d_ent.view, we)


def test_refused_calls_write_nothing(pkg):
    L = Launch(pkg)
    ga = arbitrary_g(L.B, L.K, 54).to(DEV)
    perm, n_live = pkg._native.cand_plan(L.cw, L.n, L.row0)
    refused = [lambda: L.fwd(x=None), lambda: L.fwd(label=None), lambda: L.fwd(parts=None), lambda: L.fwd(ldg=L.K - 1),
               lambda: L.fwd(ldc=L.K - 1), lambda: L.fwd(ldl=L.K - 1),
               lambda: L.bwd_x(ga, ent=None), lambda: L.bwd_x(ga, ldg=L.K - 1), lambda: L.bwd_x(ga, ldx=L.dim - 1),
               lambda: L.bwd_ent(ga, perm, n_live, perm=None), lambda: L.bwd_ent(ga, perm, n_live, x=None),
               lambda: L.bwd_ent(ga, perm, n_live, ldg=L.K - 1), lambda: L.bwd_ent(ga, perm, n_live, lde=L.dim - 1),
               lambda: L.bwd_ent(ga, perm, L.B * L.K + 1), lambda: L.bwd_ent(ga, perm, -1)]
    for i, call in enumerate(refused):
        assert call() == 1, (i, L.lib.mgcn_last_error())
        assert L.outputs_untouched(), i
    assert L.bwd_ent(ga, perm, 0) == 0 and L.bwd_ent(ga, perm, n_live, d_ent=None, d_bias=None) == 0 and L.outputs_untouched()


def test_a_bad_plan_changes_nothing_outside_the_checked_rows(pkg):
    """Out-of-range and dead entries inside the prefix (at the boundaries of runs) are skipped: the result is that of the emulation
    following the same plan, and rows no live position names keep their poison. Nothing here is expected to fault: the kernel
    re-checks every entry before it forms an address."""
    nat = pkg._native
    L = Launch(pkg)
    ga = arbitrary_g(L.B, L.K, 55)
    perm, n_live = C.loop_plan(L.cand, L.n, L.row0)
    dead_pos = int(perm[n_live])                                                # a dead position of the list
    _, rows = C.live_rows(L.cand, L.row0, L.n)
    flat_rows = rows.reshape(-1)[perm[:n_live]]
    cut = int((flat_rows[1:] != flat_rows[:-1]).nonzero()[n_live // 200, 0]) + 1   # a boundary between two runs
    junk = torch.tensor([L.B * L.K, -1, dead_pos, 2 ** 62, -2 ** 62])
    bad = torch.cat([junk, perm[:cut], junk, perm[cut:n_live], junk]).to(DEV)
    assert L.bwd_ent(ga.to(DEV), bad, bad.numel() - 2) == 0                     # (the prefix ends inside the trailing junk)
    L.d_ent.check('d_ent')
    L.d_bias.check('d_bias')
    init_e, init_b = R.Guarded(L.n, L.dim, L.dim + 4, 'cpu').view, R.Guarded(1, L.n, L.n + 8, 'cpu').view[0]
    we, wb = C.emul_ent_f32(ga, L.cand, L.x, bad.cpu(), bad.numel() - 2, L.n, row0=L.row0, d_ent=init_e, d_bias=init_b)
    good_e, good_b = C.emul_ent_f32(ga, L.cand, L.x, perm, n_live, L.n, row0=L.row0, d_ent=init_e, d_bias=init_b)
    assert same_bits(we, good_e) and same_bits(wb, good_b)                       # (junk between runs changes no sum)
    assert same_bits(L.d_ent.view, we) and same_bits(L.d_bias.view[0], wb)


# ---------------------------------------------------------------------------------------------------------------- the model
ALL_ON = dict(conve_trunk_train='hip', query_path_train='hip')
SWITCHES = ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN', 'MGCN_TRUNK', 'MGCN_DROPOUT', 'MGCN_EE', 'MGCN_TRAIN_TORCH')


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _model(pkg, case, dropout=0.0, **over):
    g = golden(case)
    dl, params = _loader(pkg, g, **dict(dict(gcn_drop=dropout, hidden_drop=dropout, feat_drop=dropout, **ALL_ON), **over))
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    assert not model.load_state_dict(g.state_dict(), strict=False).unexpected_keys
    model.conv1.drop.p = dropout / 3
    return model.to(DEV), dl, params


def _batch(dl, B=8):
    q = dl.train_queries()
    pick = torch.randperm(q.size(0), generator=R.gen(5))[:B - 3]
    return torch.cat([q[pick], q[pick[:1]].repeat(3, 1)]).to(DEV)              # one (source, relation) four times


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_forward_loss_candidates_equals_its_composition_bit_for_bit(pkg):
    nat = pkg._native
    model, dl, params = _model(pkg, 'toy_small')
    model.train()
    N = dl.num_entity
    idx = dl.train_index().to(DEV)
    q = _batch(dl)
    src, rel = q[:, 0].contiguous(), q[:, 1].contiguous()
    cand = pkg.harness.sample_candidates(q, idx, N, 69, generator=torch.Generator(device=DEV).manual_seed(3))
    cand[0, 5], cand[1, 6], cand[2, 7] = -1, N, 2 ** 62
    loss = model.forward_loss_candidates(src, rel, cand, dl.graph, index=idx, lbl_smooth=0.1)
    loss.backward()
    got = _grads(model)
    assert model._query_rows_count == 2 and model.conv2._trunk_train_count == 1
    assert got and all(bool(torch.isfinite(v).all()) for v in got.values())
    model.zero_grad(set_to_none=True)
    all_ent, all_rel = model.encode(dl.graph)
    x = model.conv2.trunk(pkg.model.query_rows(model, all_ent, src), pkg.model.query_rows(model, all_rel, rel))
    xd, ent, bias = x.detach(), all_ent.detach().contiguous(), model.conv2.bias.detach()
    labels = nat.cand_labels(idx.query_keys(src, rel), idx.keys, idx.ptr, idx.tails, cand, N)
    assert bool((labels[:, 0] == 1).all())
    hot, cold = nat.smoothed_targets(0.1, N)
    loss2, g = nat.cand_bce_fwd(xd, ent, bias, cand, labels, hot, cold)
    perm, n_live = nat.cand_plan(cand, N)
    dx = nat.cand_bce_bwd_x(g, cand, ent)
    d_ent, d_bias = nat.cand_bce_bwd_ent(g, cand, xd, perm, n_live, N)
    torch.autograd.backward([x, all_ent, model.conv2.bias], [dx, d_ent, d_bias])
    want = _grads(model)
    assert same_bits(loss.detach(), loss2)
    assert set(got) == set(want)
    for name in got:
        assert same_bits(got[name], want[name]), name
    # labels given instead of the index: the same loss
    again = model.forward_loss_candidates(src, rel, cand, dl.graph, labels=labels.bool(), lbl_smooth=0.1)
    assert same_bits(again.detach(), loss2)
    with pytest.raises(nat.NativeError, match='exactly one'):
        model.forward_loss_candidates(src, rel, cand, dl.graph)
    with pytest.raises(nat.NativeError, match='exactly one'):
        model.forward_loss_candidates(src, rel, cand, dl.graph, index=idx, labels=labels)


INVARIANT = ('conv2.bn0.weight', 'conv2.bn0.bias', 'conv2.fc.bias')      # parameters whose exact gradient is 0: see the test below


def _recording(model, seen):
    """model.encode and model.conv2.trunk wrapped so that all_ent and x of the next call keep their gradients in `seen`."""
    encode, trunk = model.encode, model.conv2.trunk

    def rec_encode(data):
        ae, ar = encode(data)
        ae.retain_grad()
        seen['all_ent'] = ae
        return ae, ar

    def rec_trunk(*a, **kw):
        x = trunk(*a, **kw)
        x.retain_grad()
        seen['x'] = x
        return x

    model.encode, model.conv2.trunk = rec_encode, rec_trunk


def test_every_entity_as_the_list_agrees_with_forward_loss(pkg):
    """cand[b] = arange(N): the loss and every gradient of forward_loss; only the summation order differs. Held to the tolerances of
    test_fused_bce_equals_two_step_loss as that test applies them: loss 1e-6; for every gradient (the stage's leaves x, all_ent
    and every parameter) rtol 1e-4, atol 1e-5 of THAT tensor's largest entry. Three parameters are named apart (INVARIANT), because in
    this configuration (no convolution bias, every dropout 0, batch statistics) the loss does not depend on them and their exact
    gradient is 0:
      conv2.bn0.weight   bn0 has one channel, so its weight scales the whole stacked image; conv_e is linear without a bias and bn1
                         normalises each of its channels with batch statistics: the scale cancels;
      conv2.bn0.bias     adds one constant to the image; conv_e (padding 0, no bias) turns it into one constant per channel, which
                         bn1's batch mean removes;
      conv2.fc.bias      adds one constant per output column of fc; with hidden_drop 0 bn2's batch mean removes it.
    What either route holds there is the rounding noise of a cancelling sum (1e-7 against a largest gradient entry of 2), which
    has no scale of its own: it is asserted to be below 1e-5 of the model's largest gradient entry on BOTH routes instead."""
    model, dl, params = _model(pkg, 'toy_small')
    model.train()
    N = dl.num_entity
    idx = dl.train_index().to(DEV)
    q = _batch(dl)
    src, rel = q[:, 0].contiguous(), q[:, 1].contiguous()
    seen = {}
    _recording(model, seen)

    def run(call):
        model.zero_grad(set_to_none=True)
        loss = call()
        loss.backward()
        out = _grads(model)
        out['x'], out['all_ent'] = seen['x'].grad.clone(), seen['all_ent'].grad.clone()
        return float(loss.detach()), out

    ref, want = run(lambda: model.forward_loss(src, rel, dl.graph, idx, lbl_smooth=0.1))
    cand = torch.arange(N, device=DEV).expand(q.size(0), N).contiguous()
    loss, got = run(lambda: model.forward_loss_candidates(src, rel, cand, dl.graph, index=idx, lbl_smooth=0.1))
    assert abs(loss - ref) < 1e-6 * max(1.0, abs(ref))
    assert set(got) == set(want)
    assert params.bias is False and model.conv2.conv_e.bias is None and model.conv2.conv_e.padding == (0, 0)   # (what the argument needs)
    assert model.conv2.hidden_drop.p == 0 and model.conv2.feature_drop.p == 0
    whole = max(float(v.abs().max()) for k, v in want.items() if k not in ('x', 'all_ent'))
    for name in want:
        scale = float(want[name].abs().max())
        print('GRAD %s max |diff| %.3g, own scale %.3g, model scale %.3g' % (name, float((got[name] - want[name]).abs().max()), scale, whole))
    for name in want:
        if name in INVARIANT:
            assert float(want[name].abs().max()) < 1e-5 * whole and float(got[name].abs().max()) < 1e-5 * whole, name
            continue
        scale = float(want[name].abs().max())
        np.testing.assert_allclose(got[name].cpu().numpy(), want[name].cpu().numpy(), rtol=1e-4, atol=1e-5 * scale, err_msg=name)


def test_two_seeded_runs_of_train_sampled_negatives_give_the_same_bits(pkg):
    """Three steps at dropout 0.3, twice from the same seeds: every parameter, buffer and Adam moment has the same bits."""
    states = []
    for _ in range(2):
        model, dl, params = _model(pkg, 'toy_small', dropout=0.3)
        idx = dl.train_index().to(DEV)
        opt = pkg.ClipAdam(model.parameters(), lr=1e-3)
        torch.manual_seed(9)
        loss = pkg.harness.train_sampled_negatives(model, dl.train_queries()[:12], idx, dl.graph, opt, params, 4, 40,
                                                   generator=torch.Generator().manual_seed(3))
        assert model.training and np.isfinite(loss) and opt._hip_step_count == 3
        moments = [copy.deepcopy({k: v for k, v in opt.state[p].items() if torch.is_tensor(v)}) for p in model.parameters()]
        states.append((loss, copy.deepcopy(model.state_dict()), moments))
    assert states[0][0] == states[1][0]
    for k, v in states[0][1].items():
        assert torch.equal(v, states[1][1][k]), k
    assert any(len(m) for m in states[0][2])
    for a, b in zip(states[0][2], states[1][2]):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_bf16_table_model_refuses_and_keeps_its_mode(pkg):
    model, dl, params = _model(pkg, 'toy_small', edge_table_dtype='bf16')
    assert model.edge_embeddings.dtype == torch.bfloat16
    idx = dl.train_index().to(DEV)
    q = _batch(dl)
    cand = pkg.harness.sample_candidates(q, idx, dl.num_entity, 5)
    model.train()
    with pytest.raises(pkg._native.NativeError, match='inference-only'):
        model.forward_loss_candidates(q[:, 0], q[:, 1], cand, dl.graph, index=idx)
    assert model.training
