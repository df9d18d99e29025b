"""Geometry of the far-offset tests (LAB_NOTES.md "Address products past 2^32"), in Python integers, no GPU.

One flat device allocation serves a case. Its first HEAD = 2^31 elements are poison (NaN for floats, 0xFF bytes for byte
tables); the tensor a kernel receives starts at element HEAD, so the rows it touches lie at element offsets >= 2^32 from the
pointer the kernel is handed, and every truncation of such an offset -- int32 / uint32 on the element index, signed / unsigned
32 bits on the byte offset -- lands INSIDE the allocation, on poison or on another row's different data. A kernel that drops
the high bits of an address product returns wrong values; it cannot fault. tests/test_far_offsets_host.py proves that on a
numpy model of the sparse buffer for every operand below, and tests/test_gpu_far_offsets.py builds its views from the same
numbers.

Two ways of being far:
  (L) a few rows with a huge leading dimension: LD20 (up to 20 rows, ld a little over 2^28: rows 16.. are far, rows 8..15 lie
      in [2^31, 2^32) and wrap negative under int32) and LD3 (up to 3 rows, ld a little over 2^31: row 2 is far) for operands
      whose row count is a batch of <= 4. Operands of one case share the allocation as column BANDS of the same rows.
  (R) a whole table whose row stride is its width: the entity table [ENT_N, ENT_DIM] with ENT_N * ENT_DIM a little over 2^32,
      of which only the rows past 2^32 elements hold data and are named by the launch.
"""
import collections

import numpy as np

HEAD = 1 << 31                      # poison elements before the base pointer
TAIL = 5 << 30                      # elements from the base pointer on
TOTAL = HEAD + TAIL                 # 7 Gi elements: 28 GiB of f32
CAP_BYTES = 32 << 30                # no case may allocate more
FAR = 1 << 32

SKEW = 1 << 16                      # what a leading dimension adds to its power of two: 16 * SKEW columns clear every band
LD20 = (1 << 28) + SKEW             # ld % 4 == 0: the 16-byte paths
LD20_ODD = LD20 + 1                 # ld % 4 == 1: the element-wise paths
ROWS20 = 20
LD3 = (1 << 31) + SKEW
LD3_ODD = LD3 + 1
ROWS3 = 3
BAND = 4096                         # columns between the operands of one case (a multiple of 4); at most 16 bands

ENT_DIM = 200
ENT_N = 21480000                    # ENT_N * ENT_DIM = 2^32 + 1 032 704
ENT_FIRST_FAR = -(-FAR // ENT_DIM)  # 21474837: the first row that starts past 2^32 elements
ENT_LIVE = ENT_N - ENT_FIRST_FAR    # 5163 rows hold data

TRUNCATIONS = ('int32_element', 'uint32_element', 'int32_byte', 'uint32_byte')


def _wrap(v, bits, signed):
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def truncate(offset, itemsize, kind):
    """Element offset a kernel would address if it formed `offset` (elements from its base pointer) with `kind` arithmetic."""
    if kind == 'int32_element':
        return _wrap(offset, 32, True)
    if kind == 'uint32_element':
        return _wrap(offset, 32, False)
    byte = _wrap(offset * itemsize, 32, kind == 'int32_byte')
    assert byte % itemsize == 0
    return byte // itemsize


# An operand of a case: `rows` rows of `cols` elements, row r at element r * ld + col0 from the base pointer (HEAD elements into
# the allocation); `live` = the rows that hold data (the others are poison and no launch names them).
Operand = collections.namedtuple('Operand', 'name itemsize ld col0 cols rows live')


def strided(name, rows, cols, ld, band, itemsize=4, shift=0):
    """(L) operand: band `band` of the case's rows; `shift` elements off the band's start (1 = a misaligned base pointer)."""
    assert rows <= (ROWS3 if ld >= LD3 else ROWS20) and cols + shift <= BAND and 0 <= band < 16
    return Operand(name, itemsize, ld, band * BAND + shift, cols, rows, tuple(range(rows)))


def entity_table(name='ent', itemsize=4):
    """(R) operand: the whole [ENT_N, ENT_DIM] table, data in its last ENT_LIVE rows only."""
    return Operand(name, itemsize, ENT_DIM, 0, ENT_DIM, ENT_N, tuple(range(ENT_FIRST_FAR, ENT_N)))


def row_offset(op, r):
    return r * op.ld + op.col0


def far_rows(op):
    return [r for r in op.live if row_offset(op, r) >= FAR]


def span(op):
    """Elements from the base pointer to the end of the operand's last row."""
    return row_offset(op, op.rows - 1) + op.cols


# A case = the operands that live in ONE allocation during one launch (same itemsize), by family.
Case = collections.namedtuple('Case', 'name operands')


def _case(name, *ops):
    assert len({o.itemsize for o in ops}) == 1
    return Case(name, ops)


def _ld20(odd):
    return (LD20_ODD, 1) if odd else (LD20, 0)


def _ld3(odd):
    return (LD3_ODD, 1) if odd else (LD3, 0)


def cases():
    """Every planned case. The GPU module builds its views from these very operands (by case name and operand name)."""
    out = []
    for odd in (False, True):
        tag = '-odd' if odd else ''
        ld, sh = _ld20(odd)
        out += [
            _case('dropout_apply' + tag, strided('x', ROWS20, 200, ld, 0, shift=sh), strided('out', ROWS20, 200, ld, 1, shift=sh)),
            _case('dropout_apply_pair' + tag, strided('xa', ROWS20, 200, ld, 0, shift=sh), strided('xb', ROWS20, 200, ld, 1, shift=sh),
                  strided('outa', ROWS20, 200, ld, 2, shift=sh), strided('outb', ROWS20, 200, ld, 3, shift=sh)),
            _case('dropout_mask' + tag, strided('mask', ROWS20, 200, ld, 0, itemsize=1, shift=sh)),
            _case('aggregate_fwd' + tag, strided('x', ROWS20, 100, ld, 0, shift=sh), strided('a', ROWS20, 300, ld, 1, shift=sh)),
            _case('aggregate_bwd' + tag, strided('x', ROWS20, 100, ld, 0, shift=sh), strided('g', ROWS20, 200, ld, 1, shift=sh)),
            _case('dense_bn_tanh_fwd' + tag, strided('a', ROWS20, 300, ld, 0, shift=sh), strided('out', ROWS20, 100, ld, 1, shift=sh)),
            _case('matmul_tn' + tag, strided('a', ROWS20, 100, ld, 0, shift=sh), strided('b', ROWS20, 200, ld, 1, shift=sh)),
            _case('bn_train_stage_sum' + tag, strided('u_in', ROWS20, 100, ld, 0, shift=sh), strided('u_out', ROWS20, 100, ld, 1, shift=sh),
                  strided('u_loop', ROWS20, 100, ld, 2, shift=sh)),
            _case('score_fwd_ent' + tag, strided('ent', ROWS20, 200, ld, 0, shift=sh)),
            _case('conve_trunk_rows' + tag, strided('ent', ROWS20, 200, ld, 0, shift=sh), strided('rel', ROWS20, 200, ld, 1, shift=sh)),
            _case('query_rows_bwd_ld' + tag, strided('out', ROWS20, 200, ld, 0, shift=sh)),
            _case('score_bce' + tag, strided('ent', ROWS20, 200, ld, 0, shift=sh), strided('g', ROWS20, 4, ld, 1, shift=sh)),
        ]
        ld, sh = _ld3(odd)
        out += [
            _case('score_fwd_block' + tag, strided('x', ROWS3, 200, ld, 0, shift=sh), strided('score', ROWS3, 33, ld, 1, shift=sh)),
            _case('score_candidates_block' + tag, strided('x', ROWS3, 200, ld, 0, shift=sh), strided('out', ROWS3, 130, ld, 1, shift=sh)),
            _case('conve_tail' + tag, strided('z', ROWS3, 200, ld, 0, shift=sh), strided('x', ROWS3, 200, ld, 1, shift=sh)),
            _case('conve_tail_keep' + tag, strided('keep', ROWS3, 200, ld, 2, itemsize=1, shift=sh)),
            _case('label_rows' + tag, strided('out', ROWS3, 100, ld, 0, shift=sh)),
            _case('cand_labels' + tag, strided('label', ROWS3, 130, ld, 0, itemsize=1, shift=sh)),
            _case('cand_ce' + tag, strided('x', ROWS3, 200, ld, 0, shift=sh), strided('z', ROWS3, 130, ld, 1, shift=sh)),
            _case('cand_blocks' + tag, strided('g', ROWS3, 130, ld, 0, shift=sh), strided('mask', ROWS3, 2, ld, 1, shift=sh)),
            _case('cand_label_bytes' + tag, strided('label', ROWS3, 130, ld, 2, itemsize=1, shift=sh)),
            _case('conve_train' + tag, *[strided(nm, ROWS3, 32, ld, k, shift=sh) for k, nm in enumerate(('s', 'r', 'z', 'gz', 'ds', 'dr'))]),
        ]
    out += [
        _case('fused_refusal', strided('x', ROWS3, 200, LD3, 0), strided('out', ROWS3, 200, LD3, 1)),
        _case('fused_rows', strided('x', ROWS20, 200, LD20, 0), strided('out', ROWS20, 200, LD20, 1)),
        _case('entity_rows', entity_table()),           # score_candidates, score_target, cand_bce_*, conve_trunk by far ids
        _case('query_rows_bwd_rows', entity_table('out')),
        _case('bn_stage_center_rows', entity_table('z')),
    ]
    return out


def by_name():
    return {c.name: c for c in cases()}


def allocation_elements(case):
    """Elements the case's allocation needs: every case uses the module's one buffer of TOTAL f32 (reinterpreted per itemsize:
    the same BYTES hold TOTAL * 4 / itemsize elements); this is what the case itself reaches."""
    return HEAD + max(span(o) for o in case.operands)


# ----------------------------------------------------------------------------------------------------------------
# numpy model of the sparse buffer
class SparseBuffer(object):
    """The allocation of a case as {element offset from the base pointer: value} for the elements that hold data; every other
    element of [-HEAD, size) is poison (NaN). Data of element (operand, row, col) is a function of all three, so two different
    elements never hold equal values."""

    def __init__(self, case):
        self.case = case
        self.size = allocation_elements(case) - HEAD
        self.starts = {}
        for k, op in enumerate(case.operands):
            for r in op.live:
                self.starts[row_offset(op, r)] = (k, r, op.cols)
        self.sorted = np.array(sorted(self.starts), dtype=np.int64)

    @staticmethod
    def value(k, r, c):
        return float((k + 1) * 1000003 + r * 4099 + c + 0.5)

    def inside(self, offset):
        return -HEAD <= offset < self.size

    def read(self, offset):
        """The value at an element offset from the base pointer (NaN = poison)."""
        assert self.inside(offset)
        i = int(np.searchsorted(self.sorted, offset, side='right')) - 1
        if i < 0:
            return float('nan')
        start = int(self.sorted[i])
        k, r, cols = self.starts[start]
        return self.value(k, r, offset - start) if offset - start < cols else float('nan')


# ----------------------------------------------------------------------------------------------------------------
# (R) for the per-edge table [2E, D]: a near-uniform graph whose table is a little over 2^32 elements
PER_EDGE = {200: 1342240, 1024: 262208}     # D -> nodes: 16 N D = 2^32 + 200 704 / + 1 048 576 (8 slots per node and half)
PER_EDGE_RANGE = 64                         # the launch covers the last 64 destinations
PER_EDGE_LEAVES = 8                         # the last 8 nodes are never a source in the in-half: their in-half runs are dead
PER_EDGE_DEG = 8
PER_EDGE_HUB_EXTRA = 40


def per_edge_graph(D):
    """(N, R, edge_index [2, 2E], edge_type [2E], n0, n1): every node is entered by 8 edges in the in-half, from sources spread
    over the nodes [0, N - 8); nodes N - 20 and N - 40 are entered by 40 more (hubs of the in-half), node N - 30 leaves 40 more
    (a hub of the out-half). The second half is the first reversed (types r + R), as the loader builds it."""
    import torch
    N, R = PER_EDGE[D], 3
    M = N - PER_EDGE_LEAVES
    o = torch.arange(N, dtype=torch.int64).repeat_interleave(PER_EDGE_DEG)
    k = torch.arange(PER_EDGE_DEG, dtype=torch.int64).repeat(N)
    s = (o + 1 + k * 104729) % M
    j = torch.arange(PER_EDGE_HUB_EXTRA, dtype=torch.int64)
    extra_s = torch.cat([(7 * j + 3) % M, (11 * j + 5) % M, torch.full_like(j, N - 30)])
    extra_o = torch.cat([torch.full_like(j, N - 20), torch.full_like(j, N - 40), (j * 1001 + 17) % N])
    s, o = torch.cat([s, extra_s]), torch.cat([o, extra_o])
    r = (s + o) % R
    ei = torch.stack((torch.cat((s, o)), torch.cat((o, s))))
    return N, R, ei, torch.cat((r, r + R)), N - PER_EDGE_RANGE, N


def shard_runs(host, n0, n1):
    """[(first slot, end slot)] of the in-half, out-half and hub slots of destinations [n0, n1), from the host arrays of
    mgcn_csr_build_host (GraphCSR.edge_table_shard takes the same three runs)."""
    rp = host['rowptr']
    runs = [(int(rp[h, n0]), int(rp[h, n1])) for h in (0, 1)]
    info = host['hubinfo'][:, n0:n1].reshape(-1, 2)
    hubs = info[info[:, 1] > 0]
    if hubs.numel():
        c0, c1 = int(hubs[:, 0].min()), int((hubs[:, 0] + hubs[:, 1]).max())
        runs.append((int(host['chunks'][c0, 0]), int(host['chunks'][c1 - 1, 1])))
    return runs


def per_edge_table(D, runs, itemsize=4, num_slots=None):
    """(R) operand: the slot-ordered table, data in the rows of `runs` only."""
    live = tuple(s for a, b in runs for s in range(a, b))
    return Operand('ee', itemsize, D, 0, D, num_slots, live)


def probe_columns(op):
    """Columns of a row the host proof visits: both ends and one inside."""
    return sorted({0, op.cols // 2, op.cols - 1})
