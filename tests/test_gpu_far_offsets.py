"""Row addressing past 2^32 elements of a table (`-m gpu`; LAB_NOTES.md "Address products past 2^32").

One module-scoped allocation of tests/far_offsets.py's TOTAL f32 (28 GiB), poisoned with all-ones words (a NaN as f32 and as
bf16, 0xFF as a byte); its first HEAD = 2^31 elements stay poison and every operand a kernel receives starts at element HEAD,
so the rows it touches lie >= 2^32 elements from the pointer it is handed and a truncated offset reads or writes poison or
another row INSIDE the allocation (proved on the CPU by tests/test_far_offsets_host.py for the very operands used here).

THE CONTRACT: a launch on far operands returns, bit for bit, what the same entry point returns on the compact twin -- the same
data with a small leading dimension of the same residue mod 4 and the same base alignment (L), or the project's own shard forms
(ent_row0 with the sliced table, node_range with edge_table_shard / ee_sub) (R). No tolerance. One compact result per family is
also held to that family's float64 reference under its existing bar, so the far launch is pinned to float64 and a wrong
renumbering in this file cannot hide. After every far launch the operand windows are wiped and the whole allocation must be
poison again; the fused status word is zero and the hub arrival counters are back at zero.

The module prints `FAR wall <s> peak <GiB>` at teardown (pytest -s). It skips only when the device reports under 36 GiB free."""
import time

import numpy as np
import pytest
import torch

from . import aggregate_ref as A
from . import cand_train_ref as CT
from . import dense_ref as R
from . import dropout_ref as DR
from . import far_offsets as F
from . import fused_cases as FC
from . import fused_ref
from . import query_train_ref as Q
from . import trunk_ref as T
from .test_gpu_aggregate_edges import _hub_counters_zero
from .test_gpu_trunk import pack_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = F.by_name()
EUNSUPPORTED = 3
ODD = pytest.mark.parametrize('odd', [False, True], ids=['ld%4=0', 'ld%4=1'])
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class FarBuffer(object):
    def __init__(self):
        self.raw = torch.empty(F.TOTAL, dtype=torch.int32, device=DEV)

    def poison(self):
        self.raw.fill_(-1)

    def view(self, op, dtype=torch.float32):
        """The operand as a [rows, cols] view whose data pointer is HEAD (+ the operand's band) elements into the allocation."""
        flat = self.raw.view(dtype)
        assert flat.element_size() == op.itemsize
        return torch.as_strided(flat, (op.rows, op.cols), (op.ld, 1), F.HEAD + op.col0)

    def wipe(self, *ops):
        for op in ops:
            self.view(op, _INT[op.itemsize]).fill_(-1 if op.itemsize > 1 else 255)

    def clean(self):
        step = 1 << 28
        return bool(torch.stack([(self.raw[i:i + step] == -1).all() for i in range(0, F.TOTAL, step)]).all())


@pytest.fixture(scope='module')
def far(pkg):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < 36 << 30:
        pytest.skip('the far-offset buffer needs 36 GiB free, the device reports %.1f GiB' % (free / 2.0 ** 30))
    torch.cuda.reset_peak_memory_stats(torch.device(DEV))
    t0 = time.time()
    buf = FarBuffer()
    buf.poison()
    torch.cuda.synchronize()
    print('FAR allocation and first fill %.2f s' % (time.time() - t0))
    yield buf
    torch.cuda.synchronize()
    print('FAR wall %.1f s peak %.2f GiB' % (time.time() - t0, torch.cuda.max_memory_allocated(torch.device(DEV)) / 2.0 ** 30))
    del buf.raw
    del buf
    torch.cuda.empty_cache()


def _bits(t):
    t = t.contiguous()
    return t.view(_INT[t.element_size()]) if t.dtype in (torch.float32, torch.bfloat16, torch.bool) else t


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and torch.equal(_bits(a), _bits(b))


class Compact(object):
    """[rows, cols] window of a small poisoned buffer: leading dimension and base alignment of the far operand's class (odd:
    ld % 4 == 1 and a base one element off a 16-byte boundary), everything around the window must stay poison."""

    def __init__(self, rows, cols, odd, dtype=torch.float32, values=None):
        ld = (cols + 3) // 4 * 4 + 4 + (1 if odd else 0)
        off = 4 + (1 if odd else 0)
        es = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((off + rows * ld + 4,), -1 if es > 1 else 255, dtype=_INT[es], device=DEV)
        self.args = ((rows, cols), (ld, 1), off)
        self.view = torch.as_strided(self.raw.view(dtype), *self.args)
        if values is not None:
            self.view.copy_(values)

    def guards_ok(self):
        outside = torch.ones_like(self.raw, dtype=torch.bool)
        torch.as_strided(outside, *self.args).fill_(False)
        return bool((self.raw[outside] == (-1 if self.raw.dtype != torch.uint8 else 255)).all())


def _ops(name, odd=False):
    case = CASES[name + ('-odd' if odd else '')]
    return case, {op.name: op for op in case.operands}


def _place(far, ops, **values):
    """Far views of the named operands; a value is copied in, None leaves the window poisoned (an output)."""
    out = {}
    for k, v in values.items():
        out[k] = far.view(ops[k])
        assert out[k].data_ptr() - far.raw.data_ptr() >= F.HEAD * 4
        if v is not None:
            out[k].copy_(v)
    return out


def _done(far, case):
    """After the far launches of a case: nothing but the operand windows was written."""
    torch.cuda.synchronize()
    far.wipe(*case.operands)
    assert far.clean(), '%s: poison outside the operand windows was overwritten' % case.name


def _report(what, ratio):
    print('RATIO %s %.4f' % (what, ratio))
    assert ratio <= 1.0, '%s: worst |got - float64| is %.3f x its bar' % (what, ratio)


# ----------------------------------------------------------------------------------------------------------------
# (12) dropout
KEY_A, KEY_B = DR.key(77, 5, 4), DR.key(77, 5, 5)
ROW0, P_DROP = 2 ** 32 - 7, 0.3


@ODD
def test_dropout_apply_pair_and_mask(pkg, far, odd):
    nat = pkg._native
    far.poison()
    g = torch.Generator().manual_seed(5)
    xa, xb = torch.randn(F.ROWS20, 200, generator=g), torch.randn(F.ROWS20, 200, generator=g)
    want_a = torch.from_numpy(DR.apply(xa.numpy(), KEY_A, ROW0, P_DROP)).to(DEV)
    want_b = torch.from_numpy(DR.apply(xb.numpy(), KEY_B, ROW0, P_DROP)).to(DEV)
    want_m = torch.from_numpy(DR.mask(KEY_A, F.ROWS20, 200, ROW0, DR.threshold(P_DROP))).to(DEV)

    case, ops = _ops('dropout_apply', odd)
    v = _place(far, ops, x=xa, out=None)
    nat.dropout_apply(v['x'], KEY_A, ROW0, P_DROP, out=v['out'])
    got = v['out'].contiguous()
    nat.dropout_apply(v['x'], KEY_A, ROW0, P_DROP, out=v['x'])              # in place
    got_in_place = v['x'].contiguous()
    _done(far, case)
    cx, co = Compact(F.ROWS20, 200, odd, values=xa.to(DEV)), Compact(F.ROWS20, 200, odd)
    nat.dropout_apply(cx.view, KEY_A, ROW0, P_DROP, out=co.view)
    assert co.guards_ok() and _same(co.view, want_a), 'compact dropout_apply differs from the reference'
    assert _same(got, co.view) and _same(got_in_place, co.view), 'far dropout_apply differs from its compact twin'

    case, ops = _ops('dropout_apply_pair', odd)
    v = _place(far, ops, xa=xa, xb=xb, outa=None, outb=None)
    nat.dropout_apply_pair(v['xa'], KEY_A, v['xb'], KEY_B, ROW0, P_DROP, out_a=v['outa'], out_b=v['outb'])
    got = v['outa'].contiguous(), v['outb'].contiguous()
    _done(far, case)
    ca, cb = Compact(F.ROWS20, 200, odd, values=xa.to(DEV)), Compact(F.ROWS20, 200, odd, values=xb.to(DEV))
    oa, ob = Compact(F.ROWS20, 200, odd), Compact(F.ROWS20, 200, odd)
    nat.dropout_apply_pair(ca.view, KEY_A, cb.view, KEY_B, ROW0, P_DROP, out_a=oa.view, out_b=ob.view)
    assert oa.guards_ok() and ob.guards_ok() and _same(oa.view, want_a) and _same(ob.view, want_b)
    assert _same(got[0], oa.view) and _same(got[1], ob.view), 'far dropout_apply_pair differs from its compact twin'

    case, ops = _ops('dropout_mask', odd)
    mv = far.view(ops['mask'], torch.uint8)
    assert mv.data_ptr() - far.raw.data_ptr() >= F.HEAD
    nat.dropout_mask(F.ROWS20, 200, KEY_A, ROW0, P_DROP, out=mv)
    got = mv.contiguous()
    _done(far, case)
    cm = Compact(F.ROWS20, 200, odd, dtype=torch.uint8)
    nat.dropout_mask(F.ROWS20, 200, KEY_A, ROW0, P_DROP, out=cm.view)
    assert cm.guards_ok() and torch.equal(cm.view, want_m)
    assert torch.equal(got, cm.view), 'far dropout_mask differs from its compact twin'


# ----------------------------------------------------------------------------------------------------------------
# (2) / (3) aggregation, (L): x / ldx, a / lda, g / ldg on a 20-node graph with hubs among the far rows
def _small_graph():
    """20 nodes, every one a source and a destination of both halves; nodes 17 and 19 are entered by 23 edges (hubs at
    hub_threshold = 5, chunks of 4 slots: six chunks, the last one short)."""
    N, Rn = F.ROWS20, 3
    s, o, r = [], [], []
    for d in range(N):
        for k in range(23 if d in (17, 19) else 1 + d % 4):
            s.append((d + 1 + 3 * k) % N); o.append(d); r.append((k + d) % Rn)
    return A._mirrored(N, Rn, s, o, r)


_small = {}


def _small_csr(pkg):
    if 'csr' not in _small:
        N, Rn, ei, et = _small_graph()
        csr = pkg.GraphCSR(N, 2 * Rn + 1, ei, et, DEV, hub_threshold=5, hub_chunk=4)
        assert csr.num_chunks >= 12
        _small.update(N=N, R=Rn, ei=ei.to(DEV), et=et.to(DEV), csr=csr)
    return _small


@ODD
def test_aggregate_fwd_far_x_and_output(pkg, far, odd):
    nat = pkg._native
    far.poison()
    G = _small_csr(pkg)
    N, csr, D = G['N'], G['csr'], 100
    inp = A.Inputs(*(t.to(DEV) for t in A.make_inputs('far-fwd-%s' % odd, N, 2 * G['R'] + 1, G['ei'].size(1), D)))
    ee_slot = inp.ee.index_select(0, csr.perm).contiguous()
    case, ops = _ops('aggregate_fwd', odd)
    for name, ee, slot_order, ee_ref, loop in (('slot order', ee_slot, True, inp.ee, True), ('edge order', inp.ee, False, inp.ee, True),
                                               ('no table', None, True, None, False)):
        cols = (3 if loop else 2) * D
        v = _place(far, ops, x=inp.x, a=None)
        nat.aggregate_fwd(csr, v['x'], inp.rel, ee, slot_order, inp.loop_edge if loop else None, v['a'][:, :cols])
        got = v['a'][:, :cols].contiguous()
        _done(far, case)
        _hub_counters_zero(csr, D)
        cx, ca = Compact(N, D, odd, values=inp.x), Compact(N, cols, odd)
        nat.aggregate_fwd(csr, cx.view, inp.rel, ee, slot_order, inp.loop_edge if loop else None, ca.view)
        torch.cuda.synchronize()
        assert ca.guards_ok()
        _hub_counters_zero(csr, D)
        what = 'aggregate_fwd %s %s' % (name, 'odd' if odd else 'aligned')
        ratio = A.check(ca.view[:, :2 * D].contiguous(), A.ref_forward(N, G['ei'], G['et'], inp.x, inp.rel, ee_ref), what)
        print('RATIO %s %.4f' % (what, ratio))
        if loop:
            A.check_loop(ca.view[:, 2 * D:].contiguous(), A.ref_loop(inp.x, inp.rel, inp.loop_edge), what)
        assert _same(got, ca.view), '%s: the far launch differs from its compact twin' % what


@ODD
def test_aggregate_bwd_far_x_and_g(pkg, far, odd):
    nat = pkg._native
    far.poison()
    G = _small_csr(pkg)
    N, csr, D = G['N'], G['csr'], 100
    inp = A.Inputs(*(t.to(DEV) for t in A.make_inputs('far-bwd-%s' % odd, N, 2 * G['R'] + 1, G['ei'].size(1), D)))
    ee_slot = inp.ee.index_select(0, csr.perm).contiguous()
    case, ops = _ops('aggregate_bwd', odd)
    v = _place(far, ops, x=inp.x, g=inp.g)
    got = nat.aggregate_bwd(csr, v['x'], inp.rel, ee_slot, v['g'])
    got_s = nat.aggregate_bwd_shard(csr, v['x'], inp.rel, ee_slot, v['g'], (0, N))
    torch.cuda.synchronize()
    assert _same(v['x'], inp.x) and _same(v['g'], inp.g)                      # inputs are read only
    _done(far, case)
    cx, cg = Compact(N, D, odd, values=inp.x), Compact(N, 2 * D, odd, values=inp.g)
    want = nat.aggregate_bwd(csr, cx.view, inp.rel, ee_slot, cg.view)
    want_s = nat.aggregate_bwd_shard(csr, cx.view, inp.rel, ee_slot, cg.view, (0, N))
    gx64, gee64, grel64 = A.ref_grads(N, G['ei'], G['et'], inp.x, inp.rel, inp.ee, inp.g)
    gee64 = A.select_rows(gee64, csr.perm)
    for name, w, r in zip(('gx', 'gee', 'grel'), want, (gx64, gee64, grel64)):
        print('RATIO aggregate_bwd %s %.4f' % (name, A.check(w, r, 'aggregate_bwd ' + name)))
    for name, a, b, c, d in zip(('gx', 'gee', 'grel'), got, want, got_s, want_s):
        assert _same(a, b), 'aggregate_bwd %s: the far launch differs from its compact twin' % name
        assert _same(c, d) and _same(c, a), 'aggregate_bwd_shard %s: far / compact / whole-graph differ' % name


# ----------------------------------------------------------------------------------------------------------------
# (4) dense step, split-K product, (4s) stage sum: (L)
@ODD
def test_dense_bn_tanh_fwd_far_rows(pkg, far, odd):
    nat = pkg._native
    far.poison()
    n, d, o = F.ROWS20, 100, 100
    a, w, bias, mean, var, gamma, beta = [t.to(DEV) if t is not None else None for t in R.bn_tanh_inputs(n, d, o, True)]
    case, ops = _ops('dense_bn_tanh_fwd', odd)
    v = _place(far, ops, a=a, out=None)
    nat.dense_bn_tanh_fwd(v['a'], w, bias, mean, var, gamma, beta, R.BN_EPS, v['out'])
    got = v['out'].contiguous()
    _done(far, case)
    ca, co = Compact(n, 3 * d, odd, values=a), Compact(n, o, odd)
    nat.dense_bn_tanh_fwd(ca.view, w, bias, mean, var, gamma, beta, R.BN_EPS, co.view)
    assert co.guards_ok()
    want, bar = R.ref_dense_bn_tanh(a, w, bias, mean, var, gamma, beta, R.BN_EPS)
    _report('dense_bn_tanh_fwd compact', R.max_ratio(co.view, want, bar))
    assert _same(got, co.view), 'dense_bn_tanh_fwd: the far launch differs from its compact twin'


@ODD
def test_matmul_tn_far_rows(pkg, far, odd):
    nat = pkg._native
    far.poison()
    k, m, n = F.ROWS20, 100, 200
    a, b = [t.to(DEV) for t in R.matmul_tn_inputs(k, m, n)]
    case, ops = _ops('matmul_tn', odd)
    v = _place(far, ops, a=a, b=b)
    got = nat.matmul_tn(v['a'], v['b'])
    _done(far, case)
    ca, cb = Compact(k, m, odd, values=a), Compact(k, n, odd, values=b)
    twin = nat.matmul_tn(ca.view, cb.view)
    want, mag = R.ref_matmul_tn(a, b)
    _report('matmul_tn compact', R.max_ratio(twin, want, R.dot_bar(mag, k)))
    assert _same(got, twin), 'matmul_tn: the far launch differs from its compact twin'


@ODD
def test_bn_train_far_rows_by_ldu(pkg, far, odd):
    """The two BN training entry points with a leading dimension (ldu): (4s) stage 1 and the (4t) forward. Every other operand
    of (4t) / (4s) is a contiguous [rows, O] block (test_bn_stage_center_whole_block_past_2_32 runs the one that fits)."""
    nat = pkg._native
    far.poison()
    n, o = F.ROWS20, 100
    u, bias, gamma, beta, rm, rv, gy = R.train_inputs(n, o, True, True)
    u, bias, gamma, beta, rm, rv = [t.to(DEV) for t in u], bias.to(DEV), gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    case, ops = _ops('bn_train_stage_sum', odd)
    v = _place(far, ops, u_in=u[0], u_out=u[1], u_loop=u[2])
    z, part = nat.bn_train_stage_sum(v['u_in'], v['u_out'], v['u_loop'], bias)
    _done(far, case)
    cu = [Compact(n, o, odd, values=t) for t in u]
    z_c, part_c = nat.bn_train_stage_sum(cu[0].view, cu[1].view, cu[2].view, bias)
    # the compact stage against (4t), whose z the split stages promise bit for bit with one rank (tests/test_gpu_train_edges.py
    # holds (4t) to float64 under dense_ref.train_bars)
    rm_c, rv_c = rm.clone(), rv.clone()
    full_c = nat.bn_tanh_train_fwd(cu[0].view, cu[1].view, cu[2].view, bias, gamma, beta, rm_c, rv_c, R.BN_MOMENTUM, R.BN_EPS)
    assert _same(z_c, full_c[1])
    y_c, z_t, mean_c, rstd_c = full_c
    gz_c, gu_c, gg_c, gb_c = nat.bn_tanh_train_bwd(z_t, y_c, gy.to(DEV), mean_c, rstd_c, gamma)
    _, r64, bars = R.train_reference(n, o, True, True)
    got = dict(z=z_t, y=y_c, mean=mean_c, rstd=rstd_c, rm=rm_c, rv=rv_c, gz=gz_c, gu=gu_c, ggamma=gg_c, gbeta=gb_c)
    for name, ratio in R.train_ratios(got, r64, bars).items():
        _report('bn_tanh_train compact ' + name, ratio)
    assert _same(z, z_c) and _same(part, part_c), 'bn_train_stage_sum: the far launch differs from its compact twin'
    # (4t) forward on the same far rows (ldu): z, y, statistics and running statistics
    v = _place(far, ops, u_in=u[0], u_out=u[1], u_loop=u[2])
    rm_f, rv_f = rm.clone(), rv.clone()
    full_f = nat.bn_tanh_train_fwd(v['u_in'], v['u_out'], v['u_loop'], bias, gamma, beta, rm_f, rv_f, R.BN_MOMENTUM, R.BN_EPS)
    _done(far, case)
    for name, a, b in zip(('y', 'z', 'mean', 'rstd', 'rm', 'rv'), tuple(full_f) + (rm_f, rv_f), tuple(full_c) + (rm_c, rv_c)):
        assert _same(a, b), 'bn_tanh_train_fwd %s: the far launch differs from its compact twin' % name


# ----------------------------------------------------------------------------------------------------------------
# (5) / (7) scoring
def _score_suite(nat, x, ent, bias, obj, target, label, mask, k):
    """The four entry points of (5) / (7) on one (x, ent, bias): everything they return."""
    score = nat.score_fwd(x, ent, bias)
    tgt = nat.score_target(x, ent, bias, obj)
    cnt_l = nat.score_rank(x, ent, bias, obj, target, label=label)
    cnt_m = nat.score_rank(x, ent, bias, obj, target, mask=mask)
    top = nat.score_topk(x, ent, bias, k, mask=mask)
    return [score, tgt, cnt_l, cnt_m, top[0], top[1]]


@ODD
def test_scoring_far_entity_rows_by_lde(pkg, far, odd):
    """ent [20, 200] with lde past 2^28: score_fwd, score_target, score_rank (both filter forms) and score_topk."""
    nat = pkg._native
    far.poison()
    B, n, dim, k = 3, F.ROWS20, 200, 5
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim, 91))]
    g = R.gen(R.seed_of(92, B, n))
    obj = torch.tensor([n - 1, 16, 3], device=DEV)
    hit = (torch.rand((B, n), generator=g) < 0.2).to(DEV)
    mask = R.pack_bits(hit, 1)
    case, ops = _ops('score_fwd_ent', odd)
    cx = Compact(B, dim, odd, values=x)
    ce = Compact(n, dim, odd, values=ent)
    score = nat.score_fwd(cx.view, ce.view, bias)
    target = score[torch.arange(B, device=DEV), obj].contiguous()
    twin = _score_suite(nat, cx.view, ce.view, bias, obj, target, hit.float(), mask, k)
    v = _place(far, ops, ent=ent)
    got = _score_suite(nat, cx.view, v['ent'], bias, obj, target, hit.float(), mask, k)
    _done(far, case)
    p64, z64, mag = R.ref_scores(x, ent, bias)
    logit_bar = R.dot_bar(mag, dim) if odd else R.split_logit_bar(mag)
    _report('score_fwd compact', R.max_ratio(twin[0], p64, R.sigmoid_bar(p64, logit_bar)))
    assert _same(twin[1], target)
    for name, a, b in zip(('score_fwd', 'score_target', 'score_rank label', 'score_rank mask', 'topk scores', 'topk ids'), got, twin):
        assert _same(a, b), '%s: the far launch differs from its compact twin' % name


@ODD
def test_score_block_and_queries_far_by_ldx_lds(pkg, far, odd):
    """x [3, 200] with ldx past 2^31 and the score block [3, 33] with lds past 2^31 (row 2 of each is past 2^32); dense label
    rows far through ldl in score_rank."""
    nat, lib = pkg._native, pkg._native.lib()
    far.poison()
    B, n, dim = F.ROWS3, 33, 200
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim, 93))]
    case, ops = _ops('score_fwd_block', odd)
    v = _place(far, ops, x=x, score=None)
    rc = lib.mgcn_score_fwd(B, n, dim, v['x'].data_ptr(), v['x'].stride(0), ent.data_ptr(), ent.stride(0), bias.data_ptr(),
                            v['score'].data_ptr(), v['score'].stride(0), _stream())
    assert rc == 0, lib.mgcn_last_error()
    got = v['score'].contiguous()
    # label rows of score_rank in the band of the score block (f32 [B, n], ldl = the far leading dimension)
    hit = (torch.rand((B, n), generator=R.gen(5)) < 0.2).to(DEV)
    obj = torch.tensor([n - 1, 0, 7], device=DEV)
    target = got[torch.arange(B, device=DEV), obj].contiguous()
    v['score'].copy_(hit.float())
    cnt = nat.score_rank(v['x'], ent, bias, obj, target, label=v['score'])
    _done(far, case)
    cx = Compact(B, dim, odd, values=x)
    cs = Compact(B, n, odd)
    rc = lib.mgcn_score_fwd(B, n, dim, cx.view.data_ptr(), cx.view.stride(0), ent.data_ptr(), ent.stride(0), bias.data_ptr(),
                            cs.view.data_ptr(), cs.view.stride(0), _stream())
    assert rc == 0, lib.mgcn_last_error()
    torch.cuda.synchronize()
    assert cs.guards_ok()
    p64, z64, mag = R.ref_scores(x, ent, bias)
    logit_bar = R.dot_bar(mag, dim) if odd else R.split_logit_bar(mag)
    _report('score_fwd block compact', R.max_ratio(cs.view, p64, R.sigmoid_bar(p64, logit_bar)))
    assert _same(got, cs.view), 'score_fwd: the far launch differs from its compact twin'
    cl = Compact(B, n, odd, values=hit.float())
    assert torch.equal(cnt, nat.score_rank(cx.view, ent, bias, obj, target, label=cl.view)), 'score_rank: far label rows'


@ODD
def test_score_candidates_far_queries_and_output(pkg, far, odd):
    nat = pkg._native
    far.poison()
    B, n, dim, K = F.ROWS3, 57, 200, 130
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim, 94))]
    cand = CT.lists(n + 6, B, K, 95).to(DEV) - 3                              # ids below, inside and above the shard
    case, ops = _ops('score_candidates_block', odd)
    v = _place(far, ops, x=x, out=None)
    nat.score_candidates(v['x'], ent, bias, cand, out=v['out'])
    got = v['out'].contiguous()
    _done(far, case)
    cx, co = Compact(B, dim, odd, values=x), Compact(B, K, odd)
    nat.score_candidates(cx.view, ent, bias, cand, out=co.view)
    torch.cuda.synchronize()
    assert co.guards_ok()
    live = (cand >= 0) & (cand < n)
    assert bool(live.any()) and bool((~live).any())
    p64, z64, mag = R.ref_scores(x, ent, bias)
    logit_bar = R.dot_bar(mag, dim) if odd else R.split_logit_bar(mag)
    bar = R.sigmoid_bar(p64, logit_bar)
    rows = torch.arange(B, device=DEV).unsqueeze(1).expand(B, K)[live]
    _report('score_candidates compact', R.max_ratio(co.view[live], p64[rows, cand[live]], bar[rows, cand[live]]))
    assert bool((_bits(co.view)[~live] == -1).all())                           # dead positions are left as they are
    assert _same(got, co.view), 'score_candidates: the far launch differs from its compact twin'


# ----------------------------------------------------------------------------------------------------------------
# (R) the entity table [ENT_N, 200], N * dim a little over 2^32: rows named by candidate, target, source and scatter ids
def _entity_table(far, fill=True):
    case = CASES['entity_rows']
    ent = far.view(case.operands[0])
    assert ent.is_contiguous() and tuple(ent.shape) == (F.ENT_N, F.ENT_DIM)
    if fill:
        live = ent[F.ENT_FIRST_FAR:]
        live.copy_(R.pm_uniform((F.ENT_LIVE, F.ENT_DIM), R.gen(96)))
    return case, ent


def _far_ids(shape, seed):
    """int64 ids of rows past 2^32 elements, with repeats; the first and the last such row among them."""
    ids = torch.randint(F.ENT_FIRST_FAR, F.ENT_N, shape, generator=R.gen(seed))
    ids.view(-1)[0], ids.view(-1)[-1] = F.ENT_FIRST_FAR, F.ENT_N - 1
    return ids


def test_entity_rows_by_candidate_and_target_id(pkg, far):
    """score_candidates, score_target, cand_bce_fwd, cand_bce_bwd_x on the whole table with far ids, against the sliced table
    with ent_row0 (the shard form); the shard results against float64 / the f32 loop."""
    nat = pkg._native
    far.poison()
    case, ent = _entity_table(far)
    r0, n, dim, B, K = F.ENT_FIRST_FAR, F.ENT_LIVE, F.ENT_DIM, 4, 130
    shard = ent[r0:].clone()
    bias = torch.full((F.ENT_N,), float('nan'), device=DEV)
    bias[r0:] = R.pm_uniform((n,), R.gen(97)).to(DEV)
    x = R.pm_uniform((B, dim), R.gen(98)).to(DEV) * 0.2
    cand = _far_ids((B, K), 99)
    cand[1, 5], cand[2, 9] = -1, 2 ** 40                                       # padding and a huge id: dead in both forms
    cand = cand.to(DEV)
    obj = _far_ids((B,), 100).to(DEV)
    label = (torch.rand((B, K), generator=R.gen(101)) < 0.1).to(DEV)
    hot, cold = 0.9, 0.001

    def run(e, b, row0, cd):
        out = nat.score_candidates(x, e, b, cd, ent_row0=row0)
        tgt = nat.score_target(x, e, b, obj, ent_row0=row0)
        loss, g = nat.cand_bce_fwd(x, e, b, cd, label, hot, cold, ent_row0=row0)
        dx = nat.cand_bce_bwd_x(g, cd, e, ent_row0=row0)
        return [out, tgt, loss.reshape(1), g, dx]

    live_only = cand
    got = run(ent, bias, 0, live_only)
    twin = run(shard, bias[r0:].contiguous(), r0, live_only)
    torch.cuda.synchronize()
    assert _same(ent[r0:], shard)
    far.wipe(*case.operands)
    assert far.clean()
    for name, a, b in zip(('score_candidates', 'score_target', 'cand_bce_fwd loss', 'cand_bce_fwd g', 'cand_bce_bwd_x'), got, twin):
        assert _same(a, b), '%s: the launch on the whole table differs from the shard form' % name
    # the shard form against float64 (scores, g) and the f32 loop (dx)
    ref = CT.ref_list_bce(x, shard, bias[r0:], live_only, label, hot, cold, 1.0 / (B * K), row0=r0)
    lv = ref['live'].to(DEV)
    p64 = ref['p'].to(DEV)
    logit_bar = R.split_logit_bar(ref['mag'].to(DEV))
    _report('score_candidates shard', R.max_ratio(twin[0][lv], p64[lv], R.sigmoid_bar(p64, logit_bar)[lv]))
    gbar = R.bce_grad_bar(ref['g'].to(DEV), p64, ref['y'].to(DEV), R.dot_bar(ref['mag'].to(DEV), dim), 1.0 / (B * K))
    _report('cand_bce_fwd g shard', R.max_ratio(twin[3][lv], ref['g'].to(DEV)[lv], gbar[lv]))
    assert bool((twin[3][~lv] == 0).all())
    assert _same(twin[4], CT.emul_dx_f32(twin[3], live_only, shard, row0=r0).to(DEV)), 'cand_bce_bwd_x shard: not the f32 loop'


@pytest.mark.parametrize('run_split', [None, 16], ids=['one-wave-runs', 'run_split=16'])
def test_entity_rows_written_by_candidate_id(pkg, far, run_split):
    """cand_bce_bwd_ent writes d_ent rows past 2^32 elements of the table it is handed and leaves every other row alone."""
    nat = pkg._native
    far.poison()
    case, d_ent = _entity_table(far, fill=False)
    r0, n, dim, B, K = F.ENT_FIRST_FAR, F.ENT_LIVE, F.ENT_DIM, 4, 130
    cand = _far_ids((B, K), 102)
    cand[:, 64:100] = F.ENT_N - 2                                              # one run of 144 entries: cut into pieces of 16
    cand[0, 3] = -1
    cand = cand.to(DEV)
    g = (R.pm_uniform((B, K), R.gen(103)) * 0.01).to(DEV)
    x = R.pm_uniform((B, dim), R.gen(104)).to(DEV)
    kw = dict(run_split=run_split)
    perm, n_live, keys = nat.cand_plan(cand, F.ENT_N, 0, keys=True)
    d_bias = torch.full((F.ENT_N,), float('nan'), device=DEV)
    nat.cand_bce_bwd_ent(g, cand, x, perm, n_live, F.ENT_N, 0, d_ent=d_ent, d_bias=d_bias, keys=keys if run_split else None, **kw)
    torch.cuda.synchronize()
    named = torch.unique(cand[cand >= 0])
    got_rows, got_bias = d_ent[named].clone(), d_bias[named].clone()
    d_ent.view(torch.int32)[named] = -1
    assert far.clean(), 'cand_bce_bwd_ent wrote a row that no live position names'
    d_bias[named] = float('nan')
    assert bool(torch.isnan(d_bias).all())
    perm_s, n_live_s, keys_s = nat.cand_plan(cand, n, r0, keys=True)
    te, tb = nat.cand_bce_bwd_ent(g, cand, x, perm_s, n_live_s, n, r0, keys=keys_s if run_split else None, **kw)
    assert _same(got_rows, te[named - r0]) and _same(got_bias, tb[named - r0]), 'cand_bce_bwd_ent: whole table differs from the shard form'
    if run_split is None:
        we, wb = CT.emul_ent_f32(g, cand, x, perm_s, n_live_s, n, row0=r0)
        assert _same(te, we.to(DEV)) and _same(tb, wb.to(DEV)), 'cand_bce_bwd_ent shard: not the f32 loop'


def test_entity_rows_gathered_by_the_trunk_and_scattered_by_query_rows_bwd(pkg, far):
    nat = pkg._native
    far.poison()
    case, ent = _entity_table(far)
    r0, dim, B = F.ENT_FIRST_FAR, F.ENT_DIM, 37
    tc = T.PRODUCTION
    geom = T.geometry(tc)
    assert geom[4] == dim
    sd = T.weights(tc)
    pack = pack_of(nat, tc, sd)
    rel = R.pm_uniform((23, dim), R.gen(105)).to(DEV)
    src, ri = _far_ids((B,), 106).to(DEV), torch.randint(0, 23, (B,), generator=R.gen(107)).to(DEV)
    got = nat.conve_trunk(geom, pack, ent, src, rel, ri)
    shard = ent[r0:].clone()
    twin = nat.conve_trunk(geom, pack, shard, src - r0, rel, ri)
    want, bar = T.ref_trunk(tc, sd, shard[src - r0], rel[ri])
    _report('conve_trunk shard', R.max_ratio(twin, want, bar))
    assert _same(got, twin), 'conve_trunk: rows gathered by far ids differ from the sliced table'

    # query_rows_bwd writes the whole [ENT_N, 200] block: zeros, and the fixed-order sums in the rows the batch names
    idx = _far_ids((B,), 108)
    idx[5] = idx[7] = idx[30]                                                   # a run of three addends
    d = Q.scatter_addends(B, dim)
    nat.query_rows_bwd(idx.to(DEV), d.to(DEV), F.ENT_N, out=ent)
    torch.cuda.synchronize()
    want = Q.scatter_loop(idx - r0, d, F.ENT_LIVE).to(DEV)
    assert _same(ent[r0:], want), 'query_rows_bwd: rows past 2^32 elements are not the sequential loop'
    step = 1 << 21
    low = torch.stack([(ent[i:min(i + step, r0)].view(torch.int32) == 0).all() for i in range(0, r0, step)])
    assert bool(low.all()), 'query_rows_bwd: a row no index names is not +0.0'
    assert _same(nat.query_rows_bwd((idx - r0).to(DEV), d.to(DEV), F.ENT_LIVE), want)
    ent.view(torch.int32).fill_(-1)
    assert far.clean()


@ODD
def test_trunk_and_scatter_far_by_leading_dimension(pkg, far, odd):
    """conve_trunk with ent / rel rows lde / ldr apart, query_rows_bwd into a window with ldo past 2^28."""
    nat = pkg._native
    far.poison()
    tc = T.PRODUCTION
    geom, dim, n, B = T.geometry(tc), 200, F.ROWS20, 37
    sd = T.weights(tc)
    pack = pack_of(nat, tc, sd)
    ent, rel = R.pm_uniform((n, dim), R.gen(109)).to(DEV), R.pm_uniform((n, dim), R.gen(110)).to(DEV)
    src, ri = torch.randint(0, n, (B,), generator=R.gen(111)).to(DEV), torch.randint(0, n, (B,), generator=R.gen(112)).to(DEV)
    src[0], ri[0], src[1], ri[1] = n - 1, n - 1, 16, 17
    case, ops = _ops('conve_trunk_rows', odd)
    v = _place(far, ops, ent=ent, rel=rel)
    got = nat.conve_trunk(geom, pack, v['ent'], src, v['rel'], ri)
    _done(far, case)
    ce, cr = Compact(n, dim, odd, values=ent), Compact(n, dim, odd, values=rel)
    twin = nat.conve_trunk(geom, pack, ce.view, src, cr.view, ri)
    want, bar = T.ref_trunk(tc, sd, ent[src], rel[ri])
    _report('conve_trunk compact', R.max_ratio(twin, want, bar))
    assert _same(got, twin), 'conve_trunk: the far launch differs from its compact twin'

    case, ops = _ops('query_rows_bwd_ld', odd)
    idx = torch.randint(0, n, (B,), generator=R.gen(113))
    idx[0], idx[1], idx[2] = n - 1, 16, n - 1
    d = Q.scatter_addends(B, dim)
    v = _place(far, ops, out=None)
    nat.query_rows_bwd(idx.to(DEV), d.to(DEV), n, out=v['out'])
    got = v['out'].contiguous()
    _done(far, case)
    co = Compact(n, dim, odd)
    nat.query_rows_bwd(idx.to(DEV), d.to(DEV), n, out=co.view)
    torch.cuda.synchronize()
    assert co.guards_ok() and _same(co.view, Q.scatter_loop(idx, d, n).to(DEV))
    assert _same(got, co.view), 'query_rows_bwd: the far launch differs from its compact twin'


@ODD
def test_conve_tail_far_rows(pkg, far, odd):
    nat = pkg._native
    far.poison()
    B, O, p = F.ROWS3, 200, 0.3
    z, keep, inv_keep, gamma, beta, rm, rv, gx = [t.to(DEV) if torch.is_tensor(t) else t for t in Q.tail_inputs(B, O, p)]
    case, ops = _ops('conve_tail', odd)
    cz = Compact(B, O, odd, values=z)
    rm_c, rv_c = rm.clone(), rv.clone()
    x_c, saved_c = nat.conve_tail_fwd(cz.view, keep, inv_keep, gamma, beta, rm_c, rv_c, Q.BN_MOMENTUM, Q.BN_EPS)
    cxo = Compact(B, O, odd, values=x_c)
    bw_c = nat.conve_tail_bwd(cz.view, keep, inv_keep, cxo.view, saved_c, gamma, gx)
    v = _place(far, ops, z=z, x=x_c)
    case_k, ops_k = _ops('conve_tail_keep', odd)
    keep_f = far.view(ops_k['keep'], torch.uint8)                               # the keep bytes, rows ldk = 2^31 bytes apart
    keep_f.copy_(keep.view(torch.uint8))
    rm_f, rv_f = rm.clone(), rv.clone()
    x_f, saved_f = nat.conve_tail_fwd(v['z'], keep_f, inv_keep, gamma, beta, rm_f, rv_f, Q.BN_MOMENTUM, Q.BN_EPS)
    bw_f = nat.conve_tail_bwd(v['z'], keep_f, inv_keep, v['x'], saved_f, gamma, gx)
    far.wipe(*case_k.operands)
    _done(far, case)
    for name, a, b in zip(('x', 'saved', 'running_mean', 'running_var', 'gz', 'd_gamma', 'd_beta'),
                          (x_f, saved_f, rm_f, rv_f) + tuple(bw_f), (x_c, saved_c, rm_c, rv_c) + tuple(bw_c)):
        assert _same(a, b), 'conve_tail %s: the far launch differs from its compact twin' % name
    ref = Q.tail_reference(B, O, p)
    got = dict(x=x_c, mean=saved_c[0], rstd=saved_c[1], rm=rm_c, rv=rv_c, gz=bw_c[0], d_gamma=bw_c[1], d_beta=bw_c[2])
    for name in Q.OUTPUTS:
        _report('conve_tail compact %s' % name, ref.ratio(name, got[name]))


# ----------------------------------------------------------------------------------------------------------------
# index look-ups and list losses whose rows are a batch: (L) at 2^31
def _index():
    """keys / ptr / tails of three known (subject, relation) keys, tails ascending within a key, and three queries (one unknown)."""
    keys = torch.tensor([5, 9, 12], dtype=torch.int64)
    ptr = torch.tensor([0, 3, 4, 9], dtype=torch.int64)
    tails = torch.tensor([1, 40, 99, 7, 0, 3, 50, 98, 99], dtype=torch.int32)
    return torch.tensor([12, 7, 5], dtype=torch.int64), keys, ptr, tails


@ODD
def test_label_rows_and_cand_labels_far_rows(pkg, far, odd):
    nat = pkg._native
    far.poison()
    qkey, keys, ptr, tails = _index()
    dq, dk, dp, dt = (t.to(DEV) for t in (qkey, keys, ptr, tails))
    B, n, row0 = F.ROWS3, 100, 0
    hit = R.ref_filter(qkey, keys, ptr, tails, row0, n)
    hot, cold = nat.smoothed_targets(0.1, n)
    want_rows = torch.where(hit, torch.tensor(hot), torch.tensor(cold)).to(DEV)
    case, ops = _ops('label_rows', odd)
    out = far.view(ops['out'])
    nat.label_rows(dq, dk, dp, dt, n, lbl_smooth=0.1, out=out)
    got_rows = out.contiguous()
    _done(far, case)
    co = Compact(B, n, odd)
    nat.label_rows(dq, dk, dp, dt, n, lbl_smooth=0.1, out=co.view)
    torch.cuda.synchronize()
    assert co.guards_ok() and _same(co.view, want_rows)
    assert _same(got_rows, co.view), 'label_rows: far rows differ from the compact twin'
    # (mgcn_filter_mask zeroes batch x ldm words in one memset: its mask block is contiguous by contract, there is no far form;
    # the bits it sets are the label rows' hits)
    assert torch.equal(nat.filter_mask(dq, dk, dp, dt, n), R.pack_bits(hit.to(DEV)))

    K = 130
    cand = CT.lists(n + 6, B, K, 131) - 3
    want_l = CT.loop_labels(qkey, keys, ptr, tails, cand, row0, n).to(DEV)
    case, ops = _ops('cand_labels', odd)
    lab = far.view(ops['label'], torch.uint8)
    nat.cand_labels(dq, dk, dp, dt, cand.to(DEV), n, out=lab)
    got = lab.contiguous()
    _done(far, case)
    cl = Compact(B, K, odd, dtype=torch.uint8)
    nat.cand_labels(dq, dk, dp, dt, cand.to(DEV), n, out=cl.view)
    torch.cuda.synchronize()
    assert cl.guards_ok() and torch.equal(cl.view.contiguous(), want_l) and bool(want_l.any())
    assert torch.equal(got, cl.view.contiguous()), 'cand_labels: far rows differ from the compact twin'

    # the drawn lists of (15): cand is int64 (no far form under the cap), the label bytes are rows 2^31 bytes apart
    key = nat.dropout_key(5, 3, nat.CAND_DRAW_SITE)
    lab.fill_(255)
    cand_f, _ = nat.cand_draw(dq, dk, dp, dt, n, K, key, row0=2 ** 32 - 1, out=(None, lab))
    got = lab.contiguous()
    _done(far, case)
    cd = Compact(B, K, odd, dtype=torch.uint8)
    cand_c, _ = nat.cand_draw(dq, dk, dp, dt, n, K, key, row0=2 ** 32 - 1, out=(None, cd.view))
    want_c, want_l = nat.cand_draw_host(qkey, keys, ptr, tails, n, K, key, row0=2 ** 32 - 1)
    torch.cuda.synchronize()
    assert cd.guards_ok() and torch.equal(cand_c.cpu(), want_c) and torch.equal(cd.view.contiguous().cpu(), want_l) and bool(want_l.any())
    assert torch.equal(cand_f, cand_c) and torch.equal(got, cd.view.contiguous()), 'cand_draw: far label rows differ from the compact twin'


@ODD
def test_cand_ce_far_queries_and_logits(pkg, far, odd):
    """cand_ce_logits with x rows 2^31 apart, cand_ce_finish with the logits z rows 2^31 apart."""
    from . import cand_ce_ref as CE
    nat = pkg._native
    far.poison()
    B, K, N, dim, eps = F.ROWS3, 130, 57, 200, 0.1
    x, ent, bias, cand, label = CE.problem(B, K, N, dim, 133, edges=False)
    dx, de, db, dc, dl = (t.to(DEV) for t in (x, ent, bias, cand, label))

    def run(xv, zbuf):
        z, stat = nat.cand_ce_logits(xv, de, db, dc, dl)
        zbuf.copy_(z)
        row = nat.cand_ce_merge(stat)
        loss, g, parts = nat.cand_ce_finish(zbuf, dc, dl, row, eps, N)
        return [z, stat, row, loss.reshape(1), g, parts]

    case, ops = _ops('cand_ce', odd)
    v = _place(far, ops, x=dx, z=None)
    got = run(v['x'], v['z'])
    _done(far, case)
    cx, cz = Compact(B, dim, odd, values=dx), Compact(B, K, odd)
    twin = run(cx.view, cz.view)
    for name, a, b in zip(('z', 'stat', 'row stat', 'loss', 'g', 'loss partials'), got, twin):
        assert _same(a, b), 'cand_ce %s: the far launch differs from its compact twin' % name
    ref = CE.ref_list_ce(x, ent, bias, cand, label, eps, 1.0 / B)
    zbar, rowbar = CE.logit_bars(ref, dim)
    live = ref['live']
    _report('cand_ce_logits z compact', R.max_ratio(twin[0].cpu()[live], ref['z'][live], zbar[live]))
    _report('cand_ce_finish g compact', R.max_ratio(twin[4].cpu(), ref['g'], CE.g_bar(ref, rowbar, 1.0 / B)))


# ----------------------------------------------------------------------------------------------------------------
# (4s) on a contiguous [rows, O] block past 2^32 elements: stage_center is the one stage with a single such operand (z); the
# others read or write two or three (z, y, gy, gz, gu), which with the poison is over the 32 GiB of tests/far_offsets.py
def test_bn_stage_center_whole_block_past_2_32(pkg, far):
    nat = pkg._native
    far.poison()
    case = CASES['bn_stage_center_rows']
    z = far.view(case.operands[0])
    n, O = F.ENT_N, F.ENT_DIM
    gen = torch.Generator(device=DEV).manual_seed(9)
    step = 1 << 21
    for i in range(0, n, step):
        z[i:i + step].normal_(0.0, 1.0, generator=gen)
    sums = (torch.randn((3, O), generator=R.gen(140)) * 1000.0).to(DEV)      # any three blocks of column sums
    mean, part = nat.bn_train_stage_center(z, sums, n)
    cuts = [((n * j // 16) // 128) * 128 for j in range(16)] + [n]
    assert all((b - a) * O < 2 ** 29 for a, b in zip(cuts, cuts[1:]))
    twin = [nat.bn_train_stage_center(z[a:b], sums, n) for a, b in zip(cuts, cuts[1:])]
    assert all(_same(m, mean) for m, _ in twin)
    assert _same(part, torch.cat([p for _, p in twin])), 'bn_train_stage_center: the whole block differs from its row shards'
    a = (F.ENT_FIRST_FAR // 128 + 1) * 128                                    # the whole 128-row blocks past 2^32 elements
    d = (z[a:].double() - mean.double()) ** 2
    pad = torch.zeros(((-d.size(0)) % 128, O), dtype=torch.float64, device=DEV)
    want = torch.cat([d, pad]).view(-1, 128, O).sum(1)
    got = part[a // 128:]
    assert got.size(0) == want.size(0) >= 30
    _report('bn_train_stage_center last blocks', R.max_ratio(got, want, R.colsum_bar(want, 128)))
    torch.cuda.synchronize()
    z.view(torch.int32).fill_(-1)
    assert far.clean()


# ----------------------------------------------------------------------------------------------------------------
# (9) the training trunk: s / lds, r / ldr, z / ldz, gz / ldg, ds / ldds, dr / lddr at 2^31
class _Win(object):
    """A window in the place of a dense_ref.Guarded output of test_gpu_trunk_train.Call."""

    def __init__(self, view):
        self.view, self.ld = view, view.stride(0)

    def ptr(self):
        return self.view.data_ptr()


@ODD
def test_conve_train_far_rows(pkg, far, odd):
    from . import trunk_train_ref as TT
    from .test_gpu_trunk_train import Call
    nat = pkg._native
    far.poison()
    tc, B, p = TT.SMALL, F.ROWS3, 0.2
    O = tc[0] * tc[1]
    case, ops = _ops('conve_train', odd)

    def run(window):
        c = Call(nat, tc, B, p)
        c.s, c.r, c.gz = window('s', c.s), window('r', c.r), window('gz', c.gz)
        for k in ('z', 'ds', 'dr'):
            c.out[k] = _Win(window(k, None))
        assert c.fwd() == 0, c.lib.mgcn_last_error()
        assert c.bwd() == 0, c.lib.mgcn_last_error()
        torch.cuda.synchronize()
        for k, gd in c.out.items():
            if k not in ('z', 'ds', 'dr'):
                gd.check('conve_train %s' % k)
        return {k: t.contiguous().clone() for k, t in c.results().items()}

    def far_window(name, values):
        v = far.view(ops[name])
        if values is not None:
            v.copy_(values)
        return v

    got = run(far_window)
    _done(far, case)
    wins = []

    def compact_window(name, values):
        wins.append(Compact(B, O, odd, values=values))
        return wins[-1].view

    twin = run(compact_window)
    assert all(w.guards_ok() for w in wins)
    ref = TT.reference(tc, B, p)
    for name in sorted(twin):
        _report('conve_train compact %s' % name, ref.ratio(name, twin[name]))
        assert _same(got[name], twin[name]), 'conve_train %s: the far launch differs from its compact twin' % name


# ----------------------------------------------------------------------------------------------------------------
# list blocks and masks with rows 2^31 apart: g / ldg, label / ldl (bytes), mask / ldm
@ODD
def test_list_blocks_and_masks_far_rows(pkg, far, odd):
    from . import cand_ce_ref as CE
    nat, lib = pkg._native, pkg._native.lib()
    far.poison()
    B, K, N, dim, eps = F.ROWS3, 130, 57, 200, 0.1
    x, ent, bias, cand, label = CE.problem(B, K, N, dim, 141, edges=False)
    dx, de, db, dc = (t.to(DEV) for t in (x, ent, bias, cand))
    dl = label.to(DEV).to(torch.uint8)
    hit = (torch.rand((B, N), generator=R.gen(142)) < 0.2).to(DEV)
    mask2 = R.pack_bits(hit)
    obj = torch.tensor([N - 1, 0, 7], device=DEV)
    hot, cold, inv = 0.9, 0.001, 1.0 / (B * K)
    case, ops = _ops('cand_blocks', odd)
    case_b, ops_b = _ops('cand_label_bytes', odd)
    st = _stream()

    def run(g, lab, mask):
        """Every entry point that takes a g, label or mask block, with these three as its blocks."""
        out = {}
        parts = torch.zeros(int(lib.mgcn_cand_bce_partials(B, K)), device=DEV)
        rc = lib.mgcn_cand_bce_fwd(B, K, N, 0, dim, dx.data_ptr(), dim, de.data_ptr(), dim, db.data_ptr(), dc.data_ptr(), K, lab.data_ptr(),
                                   lab.stride(0), hot, cold, inv, g.data_ptr(), g.stride(0), parts.data_ptr(), st)
        assert rc == 0, lib.mgcn_last_error()
        out['bce g'], out['bce partials'] = g.contiguous().clone(), parts
        out['bce dx'] = nat.cand_bce_bwd_x(g, dc, de)
        perm, n_live = nat.cand_plan(dc, N)
        out['bce d_ent'], out['bce d_bias'] = nat.cand_bce_bwd_ent(g, dc, dx, perm, n_live, N)
        z, stat = nat.cand_ce_logits(dx, de, db, dc, lab)
        row = nat.cand_ce_merge(stat)
        parts2 = torch.zeros(int(lib.mgcn_cand_ce_partials(B, K)), device=DEV)
        rc = lib.mgcn_cand_ce_finish(B, K, N, 0, z.data_ptr(), K, dc.data_ptr(), K, lab.data_ptr(), lab.stride(0), row.data_ptr(), eps,
                                     1.0 / B, g.data_ptr(), g.stride(0), parts2.data_ptr(), st)
        assert rc == 0, lib.mgcn_last_error()
        out['ce stat'], out['ce g'], out['ce partials'] = stat, g.contiguous().clone(), parts2
        sc = torch.full((B, K), float('-inf'), device=DEV)
        rc = lib.mgcn_score_candidates(B, K, N, 0, dim, dx.data_ptr(), dim, de.data_ptr(), dim, db.data_ptr(), dc.data_ptr(), K,
                                       mask.data_ptr(), mask.stride(0), sc.data_ptr(), K, st)
        assert rc == 0, lib.mgcn_last_error()
        out['score_candidates masked'] = sc
        score = nat.score_fwd(dx, de, db)
        target = score[torch.arange(B, device=DEV), obj].contiguous()
        cnt = torch.zeros((B, 3), dtype=torch.int64, device=DEV)
        rc = lib.mgcn_score_rank(B, N, 0, dim, dx.data_ptr(), dim, de.data_ptr(), dim, db.data_ptr(), obj.data_ptr(), target.data_ptr(), None, 0,
                                 mask.data_ptr(), mask.stride(0), cnt.data_ptr(), st)
        assert rc == 0, lib.mgcn_last_error()
        out['score_rank masked'] = cnt
        torch.cuda.synchronize()
        return out

    g_f = far.view(ops['g'])
    m_f = far.view(ops['mask'], torch.int32)
    m_f.copy_(mask2)
    l_f = far.view(ops_b['label'], torch.uint8)
    l_f.copy_(dl)
    got = run(g_f, l_f, m_f)
    far.wipe(*case_b.operands)
    _done(far, case)
    cg, cm, cl = Compact(B, K, odd), Compact(B, 2, odd, dtype=torch.int32, values=mask2), Compact(B, K, odd, dtype=torch.uint8, values=dl)
    twin = run(cg.view, cl.view, cm.view)
    assert cg.guards_ok() and cm.guards_ok() and cl.guards_ok()
    for name in twin:
        assert _same(got[name], twin[name]), '%s: far g / label / mask blocks differ from the compact twin' % name
    # the compact results against float64: the list loss gradients, and the masked scores against the unmasked reference
    ref = CT.ref_list_bce(x, ent, bias, cand, label, hot, cold, inv)
    lv, p64 = ref['live'].to(DEV), ref['p'].to(DEV)
    gbar = R.bce_grad_bar(ref['g'].to(DEV), p64, ref['y'].to(DEV), R.dot_bar(ref['mag'].to(DEV), dim), inv)
    _report('cand_bce_fwd g compact', R.max_ratio(twin['bce g'][lv], ref['g'].to(DEV)[lv], gbar[lv]))
    rce = CE.ref_list_ce(x, ent, bias, cand, label, eps, 1.0 / B)
    zbar, rowbar = CE.logit_bars(rce, dim)
    _report('cand_ce_finish g compact', R.max_ratio(twin['ce g'].cpu(), rce['g'], CE.g_bar(rce, rowbar, 1.0 / B)))
    filtered = lv & hit[torch.arange(B, device=DEV).unsqueeze(1), cand.to(DEV).clamp(0, N - 1)]
    assert bool(filtered.any()) and bool((twin['score_candidates masked'][filtered] == float('-inf')).all())
    keep = lv & ~filtered
    sbar = R.sigmoid_bar(p64, R.split_logit_bar(ref['mag'].to(DEV)))
    _report('score_candidates masked compact', R.max_ratio(twin['score_candidates masked'][keep], p64[keep], sbar[keep]))


# ----------------------------------------------------------------------------------------------------------------
# (6) the fused BCE pass: ent / lde and the entity-major gradient block grad_logit / ldg with rows past 2^28
def test_score_bce_fwd_far_entity_and_gradient_rows(pkg, far):
    nat, lib = pkg._native, pkg._native.lib()
    far.poison()
    B, n, dim = 4, F.ROWS20, 200
    x, ent, bias = [t.to(DEV) for t in R.score_inputs(B, n, dim, R.seed_of(B, n, dim, 150), 0.1)]
    hit = (torch.rand((B, n), generator=R.gen(151)) < 0.2).to(DEV)
    mask = R.pack_bits(hit)
    hot, cold, inv = 0.9, 0.001, 1.0 / (B * n)
    case, ops = _ops('score_bce')

    def run(e, g):
        parts = torch.zeros(int(lib.mgcn_score_bce_partials(B, n)), device=DEV)
        rc = lib.mgcn_score_bce_fwd(B, n, dim, x.data_ptr(), dim, e.data_ptr(), e.stride(0), bias.data_ptr(), mask.data_ptr(), mask.size(1),
                                    hot, cold, inv, g.data_ptr(), g.stride(0), parts.data_ptr(), _stream())
        assert rc == 0, lib.mgcn_last_error()
        torch.cuda.synchronize()
        return g.contiguous().clone(), parts

    v = _place(far, ops, ent=ent, g=None)
    got = run(v['ent'], v['g'])
    _done(far, case)
    ce, cg = Compact(n, dim, False, values=ent), Compact(n, B, False)
    twin = run(ce.view, cg.view)
    assert cg.guards_ok()
    z64, mag = R.ref_logits(x, ent, bias)
    y = torch.where(hit, torch.tensor(hot, dtype=torch.float64, device=DEV), torch.tensor(cold, dtype=torch.float64, device=DEV))
    loss64, g64, p64 = R.ref_bce(z64, y, inv)
    _report('score_bce_fwd G compact', R.max_ratio(twin[0].t(), g64, R.bce_grad_bar(g64, p64, y, R.dot_bar(mag, dim), inv)))
    assert _same(got[0], twin[0]) and _same(got[1], twin[1]), 'score_bce_fwd: the far launch differs from its compact twin'


# ----------------------------------------------------------------------------------------------------------------
# (5) / (7) on the WHOLE table: every row is read, so the table is filled with device randoms
def test_scoring_whole_table_past_2_32_elements(pkg, far):
    """score_fwd, score_rank and score_topk over [ENT_N, 200] against sixteen row shards (each under 2^29 elements from its own
    pointer) launched with ent_row0: scores concatenated, counts summed, top-k lists merged."""
    nat = pkg._native
    far.poison()
    case, ent = _entity_table(far, fill=False)
    step = 1 << 21
    gen = torch.Generator(device=DEV).manual_seed(7)
    for i in range(0, F.ENT_N, step):
        ent[i:i + step].uniform_(-1.0, 1.0, generator=gen)
    B, dim, k, n = 3, F.ENT_DIM, 10, F.ENT_N
    x = (R.pm_uniform((B, dim), R.gen(120)) * 0.15).to(DEV)
    bias = (torch.rand(n, generator=R.gen(121)) * 0.2 - 0.1).to(DEV)
    obj = torch.tensor([F.ENT_N - 1, F.ENT_FIRST_FAR + 11, 12345], device=DEV)
    words = (n + 31) // 32
    mask = torch.zeros((B, words), dtype=torch.int32, device=DEV)
    mask[:, ::7] = 0x10010001
    mask[:, -40:] = 0x00f0f00f
    score = nat.score_fwd(x, ent, bias)
    target = nat.score_target(x, ent, bias, obj)
    assert _same(target, score[torch.arange(B, device=DEV), obj])
    counts = nat.score_rank(x, ent, bias, obj, target, mask=mask)
    top_s, top_i = nat.score_topk(x, ent, bias, k, mask=mask)
    cuts = [((n * j // 16) // 32) * 32 for j in range(16)] + [n]
    assert all((b - a) * dim < 2 ** 29 for a, b in zip(cuts, cuts[1:]))
    cnt = torch.zeros((B, 3), dtype=torch.int64, device=DEV)
    parts_s, parts_i = [], []
    for a, b in zip(cuts, cuts[1:]):
        e, bs, m = ent[a:b], bias[a:b], mask[:, a // 32:(b + 31) // 32].contiguous()
        assert _same(score[:, a:b], nat.score_fwd(x, e, bs)), 'score_fwd: rows [%d, %d) of the whole table differ from the shard' % (a, b)
        nat.score_rank(x, e, bs, obj, target, mask=m, ent_row0=a, counts=cnt)
        s, i = nat.score_topk(x, e, bs, k, mask=m, ent_row0=a)
        parts_s.append(s); parts_i.append(i)
    assert torch.equal(counts, cnt), 'score_rank: the whole table differs from the sum over its shards'
    ms, mi = nat.topk_merge(torch.cat(parts_s, 1), torch.cat(parts_i, 1), k)
    assert torch.equal(top_i, mi) and _same(top_s, ms), 'score_topk: the whole table differs from the merge of its shards'
    # the last shard against float64
    a = cuts[-2]
    p64, z64, mag = R.ref_scores(x, ent[a:], bias[a:])
    _report('score_fwd last shard', R.max_ratio(score[:, a:], p64, R.sigmoid_bar(p64, R.split_logit_bar(mag))))
    torch.cuda.synchronize()
    ent.view(torch.int32).fill_(-1)
    assert far.clean()


# ----------------------------------------------------------------------------------------------------------------
# (2b) fused layer: refusal, (L) through ldx / ldo, (R) through the per-edge table
def _layer_params(D, O):
    import importlib
    oracle = importlib.import_module('oracle.mgcn_oracle')
    sd = oracle.init_layer_state('', D, O, torch.Generator().manual_seed(1), bias=True)
    p = dict(in_weight=sd['in_weight'].numpy(), out_weight=sd['out_weight'].numpy(), loop_weight=sd['loop_weight'].numpy(),
             rels_weight=sd['rels_weight'].numpy(), loop_rel=sd['loop_rel'].numpy().reshape(-1),
             loop_edge=sd['loop_edge'].numpy().reshape(-1), bias=sd['bias'].numpy(), bn_mean=sd['ent_bn.running_mean'].numpy(),
             bn_var=sd['ent_bn.running_var'].numpy(), bn_gamma=sd['ent_bn.weight'].numpy(), bn_beta=sd['ent_bn.bias'].numpy(),
             eps=1e-5)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in p.items() if k != 'eps'}
    dev['w_cat'] = torch.cat([dev['in_weight'], dev['out_weight'], dev['loop_weight']], 0).contiguous()
    return p, dev


def _fused(nat, csr, x, rel, ee, dv, wp, O, out, tune, **kw):
    nat.layer_fwd_fused(csr, x, rel, dv['loop_rel'], ee, True, dv['loop_edge'], wp, O, dv['bias'], dv['bn_mean'], dv['bn_var'],
                        dv['bn_gamma'], dv['bn_beta'], 1e-5, out, tune=tune, **kw)
    torch.cuda.synchronize()
    assert int(nat.fused_status(torch.device(DEV)).item()) == 0, 'the fused status word is set'
    return out


def test_fused_refuses_ldx_past_int32_and_writes_nothing(pkg, far):
    nat = pkg._native
    far.poison()
    N, Rn, D, O = F.ROWS3, 3, 200, 200
    _, _, ei, et = A._mirrored(N, Rn, [0, 1, 2, 0], [1, 2, 0, 2], [0, 1, 2, 0])
    csr = pkg.GraphCSR(N, 2 * Rn + 1, ei, et, DEV, hub_threshold=0)
    p, dv = _layer_params(D, O)
    wp = nat.pack_weights(dv['w_cat'])
    case, ops = _ops('fused_refusal')
    g = torch.Generator().manual_seed(3)
    v = _place(far, ops, x=torch.randn(N, D, generator=g), out=None)             # ldx = ldo = 2^31 + 2^16
    rel = torch.randn(2 * Rn, D, generator=g).to(DEV)
    ee = torch.randn(2 * csr.num_edges_half, D, generator=g).to(DEV)
    with pytest.raises(nat.FusedUnsupported):
        _fused(nat, csr, v['x'], rel, ee, dv, wp, O, v['out'], 0)
    torch.cuda.synchronize()
    far.wipe(ops['x'])
    assert far.clean(), 'a refused fused launch wrote its output'
    # the module's fall-back for such an input, (2) then (4), takes the same rows
    agg = torch.empty((N, 3 * D), device=DEV)
    nat.aggregate_fwd(csr, v['x'].copy_(torch.randn(N, D, generator=g)), torch.cat([rel, dv['loop_rel'].reshape(1, D)]), ee, True,
                      dv['loop_edge'], agg)
    nat.dense_bn_tanh_fwd(agg, dv['w_cat'], dv['bias'], dv['bn_mean'], dv['bn_var'], dv['bn_gamma'], dv['bn_beta'], 1e-5, v['out'])
    got = v['out'].contiguous()
    cx, co = Compact(N, D, False, values=v['x']), Compact(N, O, False)
    _done(far, case)
    nat.aggregate_fwd(csr, cx.view, torch.cat([rel, dv['loop_rel'].reshape(1, D)]), ee, True, dv['loop_edge'], agg)
    nat.dense_bn_tanh_fwd(agg, dv['w_cat'], dv['bias'], dv['bn_mean'], dv['bn_var'], dv['bn_gamma'], dv['bn_beta'], 1e-5, co.view)
    assert _same(got, co.view), 'aggregate_fwd + dense_bn_tanh_fwd on rows 2^31 apart differ from the compact twin'


@pytest.mark.parametrize('tune', [FC.GEN2, FC.GEN3], ids=['generation-2', 'generation-3'])
def test_fused_far_input_rows_and_output_rows(pkg, far, tune):
    """x with ldx past 2^28 (the fused kernels carry ldx as uint32 and widen at the multiply) and out with ldo past 2^28."""
    nat = pkg._native
    far.poison()
    G = _small_csr(pkg)
    N, csr, D, O = G['N'], G['csr'], 200, 200
    p, dv = _layer_params(D, O)
    wp = nat.pack_weights(dv['w_cat'], generation=nat.tune_generation(tune))
    g = torch.Generator().manual_seed(6)
    x, rel = torch.randn(N, D, generator=g) * 0.4, torch.randn(2 * G['R'], D, generator=g) * 0.5
    ee = torch.randn(2 * csr.num_edges_half, D, generator=g) * 0.5
    ee_slot = ee.to(DEV).index_select(0, csr.perm).contiguous()
    case, ops = _ops('fused_rows')
    v = _place(far, ops, x=x, out=None)
    _fused(nat, csr, v['x'], rel.to(DEV), ee_slot, dv, wp, O, v['out'], tune)
    got = v['out'].contiguous()
    _done(far, case)
    _hub_counters_zero(csr, D)
    cx, co = Compact(N, D, False, values=x.to(DEV)), Compact(N, O, False)
    _fused(nat, csr, cx.view, rel.to(DEV), ee_slot, dv, wp, O, co.view, tune)
    assert co.guards_ok()
    _hub_counters_zero(csr, D)
    want, _, Bc, _ = fused_ref.layer_f64(p, x.numpy(), rel.numpy(), ee.numpy(), G['ei'].cpu().numpy(), G['et'].cpu().numpy())
    ratio = float(np.max(np.abs(co.view.cpu().double().numpy() - want) / fused_ref.bar(Bc)))
    _report('fused compact tune=%#x' % tune, ratio)
    assert _same(got, co.view), 'fused layer: the far launch differs from its compact twin'


_per_edge = {}


def _per_edge_graph(pkg, D):
    if D not in _per_edge:
        N, Rn, ei, et, n0, n1 = F.per_edge_graph(D)
        csr = pkg.GraphCSR(N, 2 * Rn + 1, ei, et, DEV, with_backward=False)
        assert csr.num_chunks > 0 and csr.live_rowptr is not None
        _per_edge.clear()                                                        # one graph resident at a time
        _per_edge[D] = dict(N=N, R=Rn, ei=ei, et=et, n0=n0, n1=n1, csr=csr)
    return _per_edge[D]


def _range_ref(G, x, rel, table, n0, n1, D):
    """float64 sums of destinations [n0, n1) from the edge list alone: (A.Ref of [rows, 2D], messages' magnitudes likewise);
    `table` is the slot-ordered table on the device (only the range's rows are read), norms from the whole graph's degrees."""
    ei, et, csr, N = G['ei'], G['et'], G['csr'], G['N']
    E = ei.size(1) // 2
    inv = csr.inv_perm.cpu()
    rows = n1 - n0
    val = torch.zeros((rows, 2 * D), dtype=torch.float64)
    mag, cnt = torch.zeros_like(val), torch.zeros_like(val)
    for h in range(2):
        src, dst, typ = ei[0, h * E:(h + 1) * E], ei[1, h * E:(h + 1) * E], et[h * E:(h + 1) * E]
        deg = torch.bincount(src, minlength=N).double()
        dinv = deg.pow(-0.5)
        dinv[torch.isinf(dinv)] = 0
        sel = torch.nonzero((dst >= n0) & (dst < n1)).flatten()
        s, d, t = src[sel], dst[sel], typ[sel]
        eer = table.index_select(0, inv[sel + h * E].to(table.device)).float().cpu().double()
        m = x.index_select(0, s.to(x.device)).cpu().double() * rel.cpu().double()[t] * eer * (dinv[s] * dinv[d]).unsqueeze(1)
        val[:, h * D:(h + 1) * D].index_add_(0, d - n0, m)
        mag[:, h * D:(h + 1) * D].index_add_(0, d - n0, m.abs())
        cnt[:, h * D:(h + 1) * D] += torch.bincount(d - n0, minlength=rows).double().unsqueeze(1)
    return A.Ref(val, cnt, mag)


def _fill_range_rows(G, table, D, bf16):
    """Device randoms in the rows of the slot-ordered table that the range reads; everything else stays poison."""
    csr = G['csr']
    gen = torch.Generator(device=DEV).manual_seed(31)
    for a, b in csr._shard_bounds(G['n0'], G['n1']):
        vals = torch.randn((b - a, D), generator=gen, device=DEV) * 0.5
        table[a:b] = vals.to(torch.bfloat16) if bf16 else vals
    return csr._shard_bounds(G['n0'], G['n1'])


@pytest.mark.parametrize('bf16', [False, True], ids=['f32-table', 'bf16-table'])
def test_aggregate_fwd_per_edge_table_past_2_32(pkg, far, bf16):
    """aggregate_fwd on the last 64 destinations of a graph whose slot-ordered table [2E, 200] is over 2^32 elements: the
    in-half rows lie past 2^31, the out-half and hub rows past 2^32 elements from ee_dev. Twin: the range's own shard."""
    nat = pkg._native
    far.poison()
    D = 200
    G = _per_edge_graph(pkg, D)
    csr, N, n0, n1 = G['csr'], G['N'], G['n0'], G['n1']
    E2 = 2 * csr.num_edges_half
    dtype = torch.bfloat16 if bf16 else torch.float32
    table = far.view(F.per_edge_table(D, [], 2 if bf16 else 4, E2), dtype)
    runs = _fill_range_rows(G, table, D, bf16)
    assert runs[1][0] * D >= F.FAR and runs[2][0] * D >= F.FAR and runs[0][1] * D > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(32)
    x = torch.randn((N, D), generator=g, device=DEV) * 0.4
    rel = torch.randn((2 * G['R'] + 1, D), generator=g, device=DEV) * 0.5
    loop_edge = torch.randn((D,), generator=g, device=DEV)
    got = Compact(n1 - n0, 3 * D, False)
    nat.aggregate_fwd(csr, x, rel, table, True, loop_edge, got.view, node_range=(n0, n1), out_row0=n0)
    torch.cuda.synchronize()
    _hub_counters_zero(csr, D)
    shard = csr.edge_table_shard(table, n0, n1)
    twin = Compact(n1 - n0, 3 * D, False)
    nat.aggregate_fwd(csr, x, rel, shard, True, loop_edge, twin.view, node_range=(n0, n1), ee_sub=csr.shard_ee_sub(n0, n1), out_row0=n0)
    torch.cuda.synchronize()
    _hub_counters_zero(csr, D)
    assert got.guards_ok() and twin.guards_ok()
    what = 'aggregate_fwd per-edge table %s' % ('bf16' if bf16 else 'f32')
    print('RATIO %s %.4f' % (what, A.check(twin.view[:, :2 * D].contiguous().cpu(), _range_ref(G, x, rel[:-1], table, n0, n1, D), what)))
    assert _same(got.view, twin.view), '%s: the whole table differs from the range\'s shard' % what
    for a, b in runs:
        table[a:b].view(torch.int16 if bf16 else torch.int32).fill_(-1)
    assert far.clean()
    # the same table in EDGE-ID order (gathered through rec.eid, `int64_t(r.w) * p.d`): the rows of the range's edge ids, the
    # out-half hub's past 2^32 elements; the launch has no shard form (edge ids are global), its twin is the slot-order shard
    slots = torch.cat([torch.arange(a, b) for a, b in runs]).to(DEV)
    eids = csr.rec.index_select(0, slots)[:, 3].to(torch.int64)
    assert int((eids * D >= F.FAR).sum()) >= 32 and int(((eids * D >= 2 ** 31) & (eids * D < F.FAR)).sum()) >= 32
    table.index_copy_(0, eids, shard)
    by_id = Compact(n1 - n0, 3 * D, False)
    nat.aggregate_fwd(csr, x, rel, table, False, loop_edge, by_id.view, node_range=(n0, n1), out_row0=n0)
    torch.cuda.synchronize()
    _hub_counters_zero(csr, D)
    assert by_id.guards_ok()
    assert _same(by_id.view, twin.view), '%s: the table in edge-id order differs from the slot-order shard' % what
    table.view(torch.int16 if bf16 else torch.int32).index_fill_(0, eids, -1)
    assert far.clean()


FUSED_R = [(200, 200, FC.GEN2), (200, 200, FC.GEN3), (1024, 512, FC.GEN3)]


@pytest.mark.parametrize('D,O,tune', FUSED_R, ids=['%dx%d-gen%d' % (d, o, 2 if t == FC.GEN2 else 3) for d, o, t in FUSED_R])
def test_fused_per_edge_table_past_2_32(pkg, far, D, O, tune):
    """The fused layer on the last 64 destinations, per-edge rows past 2^32 elements: canonical and live view, f32 and bf16
    table, the whole table against the range's shard (ee_sub); the shard launch against float64."""
    nat = pkg._native
    G = _per_edge_graph(pkg, D)
    csr, N, n0, n1 = G['csr'], G['N'], G['n0'], G['n1']
    E2 = 2 * csr.num_edges_half
    p, dv = _layer_params(D, O)
    wp = nat.pack_weights(dv['w_cat'], generation=nat.tune_generation(tune))
    g = torch.Generator(device=DEV).manual_seed(33)
    x = torch.randn((N, D), generator=g, device=DEV) * 0.4
    rel = torch.randn((2 * G['R'], D), generator=g, device=DEV) * 0.5
    rows = n1 - n0
    for bf16 in (False, True):
        far.poison()
        dtype = torch.bfloat16 if bf16 else torch.float32
        table = far.view(F.per_edge_table(D, [], 2 if bf16 else 4, E2), dtype)
        runs = _fill_range_rows(G, table, D, bf16)
        assert runs[1][0] * D >= F.FAR and runs[2][0] * D >= F.FAR
        shard, sub = csr.edge_table_shard(table, n0, n1), csr.shard_ee_sub(n0, n1)
        first = None
        for live in (False, True):
            got, twin = Compact(rows, O, False), Compact(rows, O, False)
            _fused(nat, csr, x, rel, table, dv, wp, O, got.view, tune, node_range=(n0, n1), live=live)
            _hub_counters_zero(csr, D)
            _fused(nat, csr, x, rel, shard, dv, wp, O, twin.view, tune, node_range=(n0, n1), ee_sub=sub, live=live)
            _hub_counters_zero(csr, D)
            what = 'fused %dx%d tune=%#x %s %s' % (D, O, tune, 'bf16' if bf16 else 'f32', 'live' if live else 'canonical')
            assert got.guards_ok() and twin.guards_ok()
            assert _same(got.view, twin.view), '%s: the whole table differs from the range\'s shard' % what
            first = twin.view.clone() if first is None else first
            assert _same(twin.view, first), '%s: the live view differs from the canonical launch' % what
        # the shard launch against float64, rows of the range only
        agg = _range_ref(G, x, rel, table, n0, n1, D)
        w64 = {k: torch.from_numpy(np.asarray(p[k], dtype=np.float64)) for k in p if k != 'eps'}
        loop = x[n0:n1].cpu().double() * w64['loop_rel'] * w64['loop_edge']
        z = (agg.value[:, :D] @ w64['in_weight'] + agg.value[:, D:] @ w64['out_weight'] + loop @ w64['loop_weight']) / 3 + w64['bias']
        Bc = agg.mag[:, :D] @ w64['in_weight'].abs() + agg.mag[:, D:] @ w64['out_weight'].abs() + loop.abs() @ w64['loop_weight'].abs()
        inv = w64['bn_gamma'] / torch.sqrt(w64['bn_var'] + 1e-5)
        want = torch.tanh((z - w64['bn_mean']) * inv + w64['bn_beta'])
        ratio = float(((first.cpu().double() - want).abs() / fused_ref.bar(Bc * inv.abs() / 3)).max())
        _report('fused %dx%d tune=%#x %s shard' % (D, O, tune, 'bf16' if bf16 else 'f32'), ratio)
        for a, b in runs:
            table[a:b].view(torch.int16 if bf16 else torch.int32).fill_(-1)
        assert far.clean()
