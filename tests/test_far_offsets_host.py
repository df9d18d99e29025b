"""The far-offset geometry (tests/far_offsets.py) restated in Python integers, no GPU: every case reaches past 2^32 elements,
every truncation of a far offset stays inside the allocation and reads poison or another element's data, a gather that
truncates is rejected by the bit comparison the GPU module makes, no case needs more than 32 GiB; and the refusals the
inventory (LAB_NOTES.md "Address products past 2^32") lists under (b) are returned, with a NULL stream and nothing launched."""
import math

import numpy as np
import pytest

from . import far_offsets as F

CASES = F.cases()
_ids = [c.name for c in CASES]


def _far_elements(case):
    """(operand index, operand, row, column, offset) of the probed elements of every far row."""
    for k, op in enumerate(case.operands):
        rows = F.far_rows(op)
        for r in (rows if len(rows) <= 8 else rows[:3] + rows[len(rows) // 2:len(rows) // 2 + 2] + rows[-3:]):
            for c in F.probe_columns(op):
                yield k, op, r, c, F.row_offset(op, r) + c


def test_the_constants_are_what_the_layout_needs():
    assert F.HEAD == 2 ** 31 and F.TOTAL * 4 <= F.CAP_BYTES
    assert F.LD20 % 4 == 0 and F.LD20_ODD % 4 == 1 and F.LD3 % 4 == 0 and F.LD3_ODD % 4 == 1
    assert 16 * F.BAND <= 16 * F.SKEW and F.BAND % 4 == 0         # a truncated far row lands past every band of a low row
    assert (F.ENT_FIRST_FAR - 1) * F.ENT_DIM < F.FAR <= F.ENT_FIRST_FAR * F.ENT_DIM
    assert F.ENT_N * F.ENT_DIM - F.FAR <= 2 ** 20 + F.ENT_DIM      # "rows of the last 2^20 elements"
    assert F.ENT_N < 2 ** 31 - 64
    assert len(set(_ids)) == len(_ids)


def test_truncate_is_two_complement():
    assert F.truncate(2 ** 32 + 5, 4, 'uint32_element') == 5 and F.truncate(2 ** 32 + 5, 4, 'int32_element') == 5
    assert F.truncate(2 ** 31 + 5, 4, 'int32_element') == -2 ** 31 + 5 and F.truncate(2 ** 31 + 5, 4, 'uint32_element') == 2 ** 31 + 5
    assert F.truncate(2 ** 30 + 5, 4, 'uint32_byte') == 5 and F.truncate(2 ** 29 + 5, 4, 'int32_byte') == -2 ** 29 + 5
    assert F.truncate(2 ** 31 + 7, 1, 'int32_byte') == -2 ** 31 + 7 and F.truncate(2 ** 32 + 7, 2, 'uint32_byte') == 7


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_case_is_far_and_fits(case):
    for op in case.operands:
        assert F.far_rows(op), '%s.%s touches no offset >= 2^32 elements' % (case.name, op.name)
        assert F.span(op) <= F.TOTAL * 4 // op.itemsize - F.HEAD
        assert (F.HEAD + F.span(op)) * op.itemsize <= F.CAP_BYTES
        for r in op.live:                                              # rows in [2^31, 2^32): the HEAD covers their negative wrap
            for off in (F.row_offset(op, r), F.row_offset(op, r) + op.cols - 1):
                if 2 ** 31 <= off < 2 ** 32:
                    assert -F.HEAD <= F.truncate(off, op.itemsize, 'int32_element') < 0
    assert F.allocation_elements(case) * case.operands[0].itemsize <= F.CAP_BYTES
    # operands of one case do not overlap
    spans = sorted((F.row_offset(op, r), F.row_offset(op, r) + op.cols) for op in case.operands
                   for r in (op.live if len(op.live) <= 64 else op.live[:32] + op.live[-32:]))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_every_truncation_lands_in_the_allocation_on_other_data(case):
    buf = F.SparseBuffer(case)
    seen = 0
    for k, op, r, c, off in _far_elements(case):
        want = buf.read(off)
        assert want == buf.value(k, r, c)
        for kind in F.TRUNCATIONS:
            t = F.truncate(off, op.itemsize, kind)
            assert t != off, (case.name, op.name, r, c, kind)
            assert buf.inside(t), '%s.%s row %d col %d: %s lands at %d, outside [-HEAD, %d)' % (case.name, op.name, r, c, kind, t, buf.size)
            got = buf.read(t)
            assert math.isnan(got) or got != want
            seen += 1
    assert seen >= 4 * len(case.operands)


@pytest.mark.parametrize('case', CASES, ids=_ids)
@pytest.mark.parametrize('kind', F.TRUNCATIONS)
def test_a_truncating_gather_is_rejected(case, kind):
    """The GPU module compares bit patterns of whole results: a gather that truncates must differ in every far element."""
    buf = F.SparseBuffer(case)
    for k, op in enumerate(case.operands):
        elems = [(r, c, off) for kk, _, r, c, off in _far_elements(case) if kk == k]
        want = np.array([buf.value(k, r, c) for r, c, _ in elems], dtype=np.float64)
        honest = np.array([buf.read(off) for _, _, off in elems], dtype=np.float64)
        wrong = np.array([buf.read(F.truncate(off, op.itemsize, kind)) for _, _, off in elems], dtype=np.float64)
        assert np.array_equal(honest.view(np.int64), want.view(np.int64))
        assert not (wrong.view(np.int64) == want.view(np.int64)).any()


# ----------------------------------------------------------------------------------------------------------------
# (R) the per-edge table: the rows a launch on the last destinations reads, from the feeder's own layout
@pytest.mark.parametrize('D', sorted(F.PER_EDGE))
def test_per_edge_table_cases(pkg, D):
    N, R, ei, et, n0, n1 = F.per_edge_graph(D)
    host = pkg._native.csr_build_host(N, 2 * R + 1, ei, et, with_backward=False)
    E2 = ei.size(1)
    assert E2 * D > F.FAR and E2 * D - F.FAR <= 2 ** 21
    runs = F.shard_runs(host, n0, n1)
    assert len(runs) == 3 and all(b > a for a, b in runs), 'the range needs in-half, out-half and hub slots'
    assert host['num_chunks'] > 0
    norms = host['rec'][:, 2].contiguous().view(__import__('torch').float32)
    assert bool((norms[runs[0][0]:runs[0][1]] == 0).any()) and bool((norms[runs[0][0]:runs[0][1]] != 0).any())   # a live view exists
    for itemsize in (4, 2):
        case = F.Case('per_edge_%d_%d' % (D, itemsize), (F.per_edge_table(D, runs, itemsize, E2),))
        test_case_is_far_and_fits(case)
        test_every_truncation_lands_in_the_allocation_on_other_data(case)
        for kind in F.TRUNCATIONS:
            test_a_truncating_gather_is_rejected(case, kind)
        op = case.operands[0]
        far = F.far_rows(op)
        assert set(range(*runs[2])) <= set(far) and len(far) >= 256       # the hub slots and most of the out-half slots are far
        assert any(2 ** 31 <= F.row_offset(op, r) < 2 ** 32 for r in range(*runs[0]))   # in-half slots: the negative wrap


# ----------------------------------------------------------------------------------------------------------------
# refusals of kind (b): returned before anything is launched (NULL stream, pointers that are never followed)
EINVAL, EUNSUPPORTED = 1, 3
P = 1 << 12              # a non-null, 16-byte aligned "device pointer" for calls that must refuse before any launch


def test_fused_refuses_a_leading_dimension_past_int32(pkg):
    """The fused kernels narrow ldx to uint32: the dispatcher refuses ldx >= 2^31 (callers fall back to (2) + (4))."""
    lib = pkg._native.lib()
    args = lambda ldx, sub_in=0, sub_out=0: (8, 8, 200, 200, 3, P, P, P, ldx, P, P, P, 1, P, P, None, P, P, P, P, 1e-5, P, 200, 0, 8,
                                             sub_in, sub_out, 0, None, None, 0, 0, None, None, None, None, 0, 0, None, None)
    assert lib.mgcn_layer_fwd_fused(*args(2 ** 31)) == EUNSUPPORTED
    assert lib.mgcn_layer_fwd_fused(*args(F.LD3)) == EUNSUPPORTED
    assert lib.mgcn_layer_fwd_fused_ee16(*args(F.LD3)) == EUNSUPPORTED
    # ... and the two shard offsets as int32: a value outside int32 used to be cut silently
    for sub in ((2 ** 31, 0), (0, 2 ** 32 + 5), (-2 ** 31 - 1, 0)):
        assert lib.mgcn_layer_fwd_fused(*args(200, *sub)) == EINVAL and b'exceed int32' in lib.mgcn_last_error()
        assert lib.mgcn_layer_fwd_fused_ee16(*args(200, *sub)) == EINVAL
    live = lambda sub_in: (8, 8, 200, 200, 3, P, P, P, P, 200, P, P, P, 1, P, P, None, P, P, P, P, 1e-5, P, 200, 0, 8, sub_in, 0, 0, None,
                           None, 0, 0, None, None, None, None, 0, 0, None, None)
    assert lib.mgcn_layer_fwd_fused_live(*live(2 ** 31)) == EINVAL


def test_int32_sized_arguments_are_refused(pkg):
    lib = pkg._native.lib()
    big = 2 ** 31
    # (2): node and slot counts are int32 on the device
    rc = lib.mgcn_aggregate_fwd(big, 8, 4, 3, P, P, P, 4, P, P, None, 1, None, P, 8, 0, 1, None, None, 0, 0, None, 0, 0, 0, None)
    assert rc == EINVAL and b'int32' in lib.mgcn_last_error()
    rc = lib.mgcn_aggregate_fwd(8, big // 2, 4, 3, P, P, P, 4, P, P, None, 1, None, P, 8, 0, 1, None, None, 0, 0, None, 0, 0, 0, None)
    assert rc == EINVAL
    # (13): list lengths are int32
    rc = lib.mgcn_score_candidates(2, big, 8, 0, 4, P, 4, P, 4, P, P, big, None, 0, P, big, None)
    assert rc == EINVAL and b'int32' in lib.mgcn_last_error()
    # (7): global ids are int32 in the selection
    assert lib.mgcn_score_topk_workspace(2, 8, 1) > 0
    rc = lib.mgcn_score_topk(2, 8, big - 4, 4, P, 4, P, 4, P, None, 0, 1, P, 1, P, 1, P, 1 << 20, None)
    assert rc == EINVAL and b'2^31' in lib.mgcn_last_error()
    # (11): num_rows above 2^50
    rc = lib.mgcn_query_rows_bwd(2, 2 ** 50 + 1, 4, P, P, 4, P, 4, P, 1 << 20, None)
    assert rc == EUNSUPPORTED
    # (4t) / (4s): grids are sized by rows / 128 and rows * O / 256 in 32 bits; more than 2^37 elements is refused
    rows = 2 ** 36 + 1
    rc = lib.mgcn_bn_train_stage_sum(rows, 2, P, P, P, 2, None, P, P, None)
    assert rc == EINVAL and b'2^37' in lib.mgcn_last_error()
    assert lib.mgcn_bn_tanh_train_fwd(rows, 2, P, P, P, 2, None, P, P, None, None, 0.1, 1e-5, P, P, P, P, P, 0, None) == EINVAL
    assert lib.mgcn_bn_tanh_train_bwd(rows, 2, P, P, P, P, P, P, P, P, P, P, P, 0, None) == EINVAL
    assert lib.mgcn_bn_train_stage_center(rows, 2, P, P, 1, rows, P, P, None) == EINVAL
    assert lib.mgcn_bn_train_stage_finish(rows, 2, P, P, 1, rows, P, P, P, None, None, 0.1, 1e-5, P, P, None) == EINVAL
    assert lib.mgcn_bn_train_bwd_stage_sums(rows, 2, P, P, P, P, P, P, P, None) == EINVAL
    assert lib.mgcn_bn_train_bwd_stage_apply(rows, 2, P, P, P, P, P, P, P, P, 1, rows, P, P, P, P, None) == EINVAL
    assert b'2^37' in lib.mgcn_last_error()
    # (12): rows x ld above 2^60
    rc = lib.mgcn_dropout_apply(2 ** 31, 4, P, 2 ** 30, P, 2 ** 30, 1, 0, 1 << 31, 2.0, None)
    assert rc == EINVAL and b'2^60' in lib.mgcn_last_error()


def test_the_other_limits_of_the_inventory_are_refused(pkg):
    """Every other (b) of the inventory, one call each, NULL stream, pointers never followed."""
    import ctypes
    lib = pkg._native.lib()
    big, lim = 2 ** 31, 2 ** 31 - 64
    err = lambda: lib.mgcn_last_error()
    # (4) and mgcn_matmul_f32: rows of the tile kernel are int32 in the launch geometry
    assert lib.mgcn_matmul_f32(lim, 4, 4, P, 4, P, 4, P, 4, None) == EINVAL and b'int32' in err()
    assert lib.mgcn_dense_bn_tanh_fwd(lim, 4, 4, P, 12, P, None, P, P, P, P, 1e-5, P, 4, None) == EINVAL and b'int32' in err()
    # mgcn_matmul_tn_f32: M <= 208, N <= 256
    assert lib.mgcn_matmul_tn_f32(8, 209, 4, P, 209, P, 4, P, 4, P, 1 << 20, None) == EUNSUPPORTED
    assert lib.mgcn_matmul_tn_f32(8, 4, 257, P, 4, P, 257, P, 257, P, 1 << 20, None) == EUNSUPPORTED
    # (5): n_local
    assert lib.mgcn_score_fwd(2, lim, 4, P, 4, P, 4, P, P, lim, None) == EINVAL and b'int32' in err()
    assert lib.mgcn_score_target(2, lim, 0, 4, P, 4, P, 4, P, P, P, None) == EINVAL and b'int32' in err()
    assert lib.mgcn_score_rank(2, lim, 0, 4, P, 4, P, 4, P, P, P, P, lim, None, 0, P, None) == EINVAL and b'int32' in err()
    assert lib.mgcn_score_bce_fwd(4, lim, 4, P, 4, P, 4, P, P, lim // 32 + 1, 1.0, 0.0, 1.0, P, 4, P, None) == EINVAL and b'int32' in err()
    # hub chunks are int32: (2) and (2b)
    rc = lib.mgcn_aggregate_fwd(8, 8, 4, 3, P, P, P, 4, P, P, None, 1, None, P, 8, 0, 1, None, None, big, big, None, 0, 0, 0, None)
    assert rc == EINVAL and b'hub chunks' in err()
    rc = lib.mgcn_layer_fwd_fused(8, 8, 200, 200, 3, P, P, P, 200, P, P, P, 1, P, P, None, P, P, P, P, 1e-5, P, 200, 0, 8, 0, 0, 0, None,
                                  None, big, big, None, None, None, None, 0, 0, None, None)
    assert rc == EINVAL and b'hub chunks' in err()
    # the fused shapes and their packing: D <= 1024, O <= 512
    assert lib.mgcn_pack_weights(1028, 512, P, P, 1 << 30, None) == EINVAL and lib.mgcn_pack_weights(1024, 516, P, P, 1 << 30, None) == EINVAL
    shape = lambda D, O: lib.mgcn_layer_fwd_fused(8, 8, D, O, 3, P, P, P, D, P, P, P, 1, P, P, None, P, P, P, P, 1e-5, P, O, 0, 8, 0, 0, 0,
                                                  None, None, 0, 0, None, None, None, None, 0, 0, None, None)
    assert shape(1028, 512) == EUNSUPPORTED and shape(1024, 516) == EUNSUPPORTED
    # (13), (14), (16): list sizes
    assert lib.mgcn_cand_bce_fwd(2, lim, 8, 0, 4, P, 4, P, 4, P, P, lim, P, lim, 1.0, 0.0, 1.0, P, lim, P, None) == EINVAL and b'int32' in err()
    assert lib.mgcn_cand_bce_bwd_x(2, lim, 8, 0, 4, P, lim, P, lim, P, 4, P, 4, None) == EINVAL
    assert lib.mgcn_cand_bce_bwd_ent(2, lim, 8, 0, 4, P, lim, P, lim, P, 1, P, 4, P, 4, P, None) == EINVAL
    assert lib.mgcn_cand_ce_logits(2, lim, 8, 0, 4, P, 4, P, 4, P, P, lim, P, lim, P, lim, P, None) == EINVAL and b'int32' in err()
    assert lib.mgcn_cand_ce_finish(2, lim, 8, 0, P, lim, P, lim, P, lim, P, 0.1, 0.5, P, lim, P, None) == EINVAL
    assert lib.mgcn_cand_ce_merge(2, 2, P, 2 ** 40, 1, P, None) == EINVAL and b'stride' in err()
    assert lib.mgcn_cand_labels(2, lim, P, 1, P, P, P, 0, 8, P, lim, P, lim, None) == EINVAL
    # (8), (9): the pack below 2^31 floats; 1 <= B <= 4096 and B K < 2^31
    assert lib.mgcn_conve_packed_bytes(16, 32, 1, 5000, 512) == 0 and lib.mgcn_conve_packed_bytes(16, 32, 1, 8, 512) > 0
    assert lib.mgcn_conve_trunk_fwd(2, 16, 32, 1, 5000, 512, P, 512, 8, None, P, 512, 8, None, P, P, 512, None, 0, None) == EUNSUPPORTED
    assert lib.mgcn_conve_train_workspace(4097, 4, 8, 3, 8, 32) == 0 and lib.mgcn_conve_train_workspace(4096, 4, 8, 3, 8, 32) > 0
    assert lib.mgcn_conve_train_workspace(4096, 16, 32, 1, 512, 512) == 0            # B K = 2^31
    tr = lambda B, geom, O: lib.mgcn_conve_train_fwd(B, *geom, P, O, P, O, P, None, P, geom[3] * 1024, None, P, P, P, P, 0.1, 1e-5, P, P, P, P,
                                                     0.1, 1e-5, None, 1.0, P, O, P, P, 1 << 40, None)
    assert tr(4096, (16, 32, 1, 512, 512), 512) == EUNSUPPORTED
    # (15), (17): the drawn lists
    draw = lambda batch, n_cand: lib.mgcn_cand_draw(batch, n_cand, 100, P, 1, P, P, P, 1, 7, 0, P, max(n_cand, 1), None, 0, None)
    assert draw(lim, 4) == EINVAL and b'int32' in err()
    assert draw(4, lim) == EINVAL and b'int32' in err()
    assert lib.mgcn_cand_draw(2 ** 40, 4, 100, P, 1, P, P, P, 1, 7, 0, P, 2 ** 30, None, 0, None) == EINVAL
    assert lib.mgcn_cand_draw_alias(4, 4, big, P, 1, P, P, P, 1, P, 7, 0, P, 4, None, 0, None) == EINVAL and b'31 bits' in err()
    # (19): this step's records
    drop = lambda N, E, chunks: lib.mgcn_edge_drop_records(N, E, P, P, P, P, P, chunks, P, 1 << 20, 4, None, 7, 1 << 31, P, P << 1, None)
    for args in ((big - 1, 8, 0), (8, big // 2, 0), (8, 8, big - 1)):
        assert drop(*args) == EINVAL and b'int32' in err()
    # (10): chunk counts of one launch
    numel = (ctypes.c_int64 * 1)(2 ** 31 * 8192 + 1)
    ptrs = (ctypes.c_void_p * 1)(P)
    assert lib.mgcn_adam_sq_norms(1, ptrs, numel, P, P, 1 << 62, None) == EUNSUPPORTED
    assert lib.mgcn_adam_step(1, ptrs, ptrs, ptrs, ptrs, numel, None, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, None) == EUNSUPPORTED


def test_what_the_cap_leaves_out():
    """The forms no case runs, and the arithmetic behind each: they need more than the 32 GiB one case may allocate."""
    one_f32 = (F.HEAD + F.FAR) * 4                      # one f32 block past 2^32 elements behind its poison
    assert one_f32 <= F.CAP_BYTES < one_f32 + F.FAR * 4
    # ... so nothing with TWO such blocks live: (4s) stage_finish (z, y), the (4t) / (4s) backward (z, y, gy, gz, gu), the (4t)
    # forward's z and y, whole-graph aggregate_bwd (ee, gee), mgcn_adam_step (p, g, m, v)
    assert (F.HEAD + F.FAR) * 8 > F.CAP_BYTES           # an int64 block (cand / ldc, out_id / ldi, drawn lists) 2^32 elements out
    # mgcn_edge_drop_records: its largest index is (h N + n) 2 + 1 <= 4 N - 1 into hubinfo [2, N, 2] (then 2 N + 1 into rowptr
    # [2, N + 1], 2 N - 1 into cinv [2, N]), N < 2^31 - 1. It passes 2^32 elements only above N = 2^30 nodes, where the three
    # arrays, all read for every node, are over the cap by themselves; it passes 2^31 from N = 2^29, where they are 16 GiB that
    # the host feeder must first build for 5 * 10^8 nodes (12 GB of host arrays): not a test of a few seconds
    N = 2 ** 30
    assert 4 * N - 1 < F.FAR <= 4 * (N + 1) - 1 and 4 * (2 * (N + 1) + 4 * N + 2 * N) > F.CAP_BYTES
    N = 2 ** 29
    assert 4 * N - 1 < 2 ** 31 <= 4 * (N + 1) - 1 and 4 * (2 * (N + 1) + 4 * N + 2 * N) > 16 << 30
