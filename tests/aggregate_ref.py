"""What csrc/aggregate.hip is held to: float64 references of the aggregation forward and of its three gradients built from
the edge list alone, deterministic graphs that put run lengths, hub chunk counts and relation runs on the kernels' internal
boundaries, the width grid with the geometry each width is meant to take, and the error bar. Plain torch, any device.

The bar is derived, not measured. A term of any of the four sums is a product of f32 values rounded at most three times
that carries the f32 norm of csr_build.cpp, (1 / sqrt(float(deg_s))) * (1 / sqrt(float(deg_d))), at most 2.5 u off the
float64 norm; the n terms of an element are added with n - 1 roundings in some order. To first order

    |got - ref64| <= (n + 6) u mag,    u = 2^-24, mag = sum of |term|

for ANY summation tree (slot order, hub chunk sums, the two fold levels, the by-type partial rows). BAR_SLACK = 1.01 pays
for the higher-order terms. The bar is per element and never scaled by a tensor's maximum; an element without terms
(isolated node, relation without edges, a shard's gx of a node none of its slots leaves) must be exactly 0.0.

Every input entry has magnitude in [0.5, 2] and a random sign, so one dropped, doubled or mis-indexed term moves an
element by at least 2^-4 times its norm: orders above the bar at these sizes. Seeds come from the case label.

EMUL_WORST_RATIO_MEASURED is a record (tests/test_aggregate_ref_host.py recomputes it): how close the CPU f32 emulation
of the same sums comes to the bar on the grids. It is not the bar's source."""
import collections
import zlib

import torch

U = 2.0 ** -24
BAR_SLACK = 1.01
TERM_ROUNDINGS = 6          # three product roundings + 2.5 u of the f32 norm, rounded up
LOOP_BAR_U = 3.0            # (x * rel[-1]) * loop_edge: two roundings
NORM_F32_MAX_U = 2.5        # f32 norm against the float64 norm (checked on every grid graph by the host test)
EMUL_WORST_RATIO_MEASURED = 0.725  # worst |emulation - ref64| / bar over the grids (host test: stale beyond a factor 2)

K_FOLD_SPAN = 16            # aggregate.hip kFoldSpan
K_TYPE_CHUNK = 16           # aggregate.hip kTypeChunk

Ref = collections.namedtuple('Ref', 'value n mag')


# ----------------------------------------------------------------------------------------------------------------
# geometry (aggregate.hip pick_geometry, restated)
def pick_geometry(d, aligned):
    """-> (vec, cpl, gs) or None when the width is refused."""
    vec = 4 if (d % 4 == 0 and aligned) else 1
    nchunk = d // vec
    gl = 2
    while (1 << gl) < nchunk and gl < 6:
        gl += 1
    cpl = (nchunk + (1 << gl) - 1) >> gl
    cpl = 1 if cpl <= 1 else 2 if cpl <= 2 else 4 if cpl <= 4 else 8 if cpl <= 8 else 0
    return (vec, cpl, 1 << gl) if cpl else None


# layouts: which operand is off the 16-byte grid (all leave the VALUES alone)
PLAIN, XCOL, XSTRIDE, OUTWIN, GLD = 'plain', 'xcol', 'xstride', 'outwin', 'gld'

Case = collections.namedtuple('Case', 'd layout label')      # label: the geometry the width is MEANT to take, by hand


def _c(d, label, layout=PLAIN):
    return Case(d, layout, label)


ALIGNED_CASES = [
    _c(4, 'v4c1g4'), _c(20, 'v4c1g8'), _c(36, 'v4c1g16'), _c(68, 'v4c1g32'), _c(100, 'v4c1g32'), _c(132, 'v4c1g64'),
    _c(256, 'v4c1g64'), _c(260, 'v4c2g64'), _c(512, 'v4c2g64'), _c(516, 'v4c4g64'), _c(1024, 'v4c4g64'),
    _c(1028, 'v4c8g64'), _c(2048, 'v4c8g64'),
]
UNALIGNED_WIDTH_CASES = [
    _c(1, 'v1c1g4'), _c(2, 'v1c1g4'), _c(3, 'v1c1g4'), _c(5, 'v1c1g8'), _c(63, 'v1c1g64'), _c(65, 'v1c2g64'),
    _c(129, 'v1c4g64'), _c(257, 'v1c8g64'), _c(511, 'v1c8g64'),
]
# D % 4 == 0 sent down the VEC = 1 path by an operand's layout: 100 floats = 2 x 64 lanes, 256 = 4 x 64, 512 = 8 x 64
FWD_LAYOUT_CASES = [_c(d, lab, lay) for d, lab in ((100, 'v1c2g64'), (256, 'v1c4g64'), (512, 'v1c8g64'))
                    for lay in (XCOL, XSTRIDE, OUTWIN)]
BWD_LAYOUT_CASES = [_c(d, lab, lay) for d, lab in ((100, 'v1c2g64'), (256, 'v1c4g64'), (512, 'v1c8g64'))
                    for lay in (XCOL, XSTRIDE, GLD)]
# refused: more than 8 column chunks per lane of a 64-lane group. 2048 floats = 512 dwordx4 = 8 x 64 is the widest aligned
# row and 512 the widest unaligned one; 516 through a misaligned view is 516 single floats = 9 x 64 (its aligned geometry,
# 129 dwordx4 -> CPL 4, does not carry over).
REFUSED_CASES = [_c(2052, 'refused'), _c(513, 'refused'), _c(516, 'refused', XCOL), _c(516, 'refused', OUTWIN),
                 _c(1024, 'refused', XSTRIDE)]
# ... and what is still accepted right below: 2048 aligned (ALIGNED_CASES), 511 / 512 unaligned (above)

FWD_CASES = ALIGNED_CASES + UNALIGNED_WIDTH_CASES + FWD_LAYOUT_CASES
BWD_CASES = ALIGNED_CASES + UNALIGNED_WIDTH_CASES + BWD_LAYOUT_CASES
# one width per (vec, cpl) for the graphs that are too big to run at every width
GEOM_CASES = [_c(100, 'v4c1g32'), _c(260, 'v4c2g64'), _c(516, 'v4c4g64'), _c(1028, 'v4c8g64'),
              _c(63, 'v1c1g64'), _c(65, 'v1c2g64'), _c(129, 'v1c4g64'), _c(257, 'v1c8g64')]
FWD_GEOM_CASES = GEOM_CASES + [_c(100, 'v1c2g64', XCOL), _c(256, 'v1c4g64', OUTWIN)]
BWD_GEOM_CASES = GEOM_CASES + [_c(100, 'v1c2g64', GLD), _c(256, 'v1c4g64', XSTRIDE)]


def case_id(c):
    return 'D%d-%s-%s' % (c.d, c.layout, c.label)


def case_geometry(c):
    return pick_geometry(c.d, c.layout == PLAIN)


def geometry_label(geom):
    return 'refused' if geom is None else 'v%dc%dg%d' % geom


# kernel family -> the cases its GPU tests run (tests/test_gpu_aggregate_edges.py parametrises from this table, the host test
# checks that every family keeps all eight (vec, cpl) instances)
FAMILY_CASES = collections.OrderedDict([
    ('fwd', FWD_CASES),                       # agg_fwd_kernel, degree_profile
    ('hub_prepass', FWD_GEOM_CASES),          # agg_hub_kernel + in-launch fold, hub_profile
    ('gee_grel_fused', BWD_CASES),            # agg_bwd_gee_grel_kernel
    ('gee_alone', BWD_CASES),                 # agg_bwd_gee_kernel
    ('grel_partial_ee', BWD_CASES),           # agg_bwd_grel_partial_kernel with the per-edge table
    ('grel_partial_noee', BWD_CASES),         # ... without
    ('grel_final', BWD_CASES),                # agg_bwd_grel_final_kernel
    ('gx_long', BWD_CASES),                   # agg_bwd_gx_kernel (E >= 4N: type_profile; degree_profile, hub_profile, switch_pair)
    ('gx_short', BWD_CASES),                  # agg_bwd_gx_short_kernel (E < 4N: type_profile(small); switch_pair)
    ('gx_hub_fold', BWD_GEOM_CASES),          # agg_bwd_gx_hub_kernel + agg_hub_fold_kernel launches
    ('shard_gee_grel', GEOM_CASES),           # agg_bwd_shard_gee_grel_kernel
    ('shard_gx', GEOM_CASES),                 # agg_bwd_shard_gx_kernel
    ('shard_gx_hub', GEOM_CASES),             # agg_bwd_shard_gx_hub_kernel
])


def all_labels():
    """'family:v<vec>c<cpl>' of every case the GPU tests run, from the geometry each case really takes."""
    have = set()
    for fam, cases in FAMILY_CASES.items():
        for c in cases:
            g = case_geometry(c)
            if g is not None:
                have.add('%s:v%dc%d' % (fam, g[0], g[1]))
    # the E < 4N switch of the forward (VEC 4, CPL 1 only): both sides come from switch_pair, run at a v4c1 width
    if any(case_geometry(c)[:2] == (4, 1) for c in SWITCH_CASES):
        have.update(('agg_fwd_kernel<4,1,2>', 'agg_fwd_kernel<4,1,4>'))
    return have


# ----------------------------------------------------------------------------------------------------------------
# inputs
def seed_of(label):
    return zlib.crc32(str(label).encode()) & 0x7fffffff


def rand_unit(shape, gen):
    """Magnitude in [0.5, 2] (log-uniform), random sign: no entry is ignorable next to another."""
    mag = torch.exp2(torch.rand(shape, generator=gen) * 2.0 - 1.0)
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2.0 - 1.0
    return (mag * sign).float()


Inputs = collections.namedtuple('Inputs', 'x rel ee g loop_edge')


def make_inputs(label, N, rel_rows, E2, D):
    """CPU f32 tensors: x [N, D], rel [rel_rows, D] (last row = self-loop row), ee [2E, D] in EDGE-ID order, g [N, 2D],
    loop_edge [D]."""
    gen = torch.Generator().manual_seed(seed_of(label))
    return Inputs(rand_unit((N, D), gen), rand_unit((rel_rows, D), gen), rand_unit((E2, D), gen), rand_unit((N, 2 * D), gen),
                  rand_unit((D,), gen))


# ----------------------------------------------------------------------------------------------------------------
# norms
def _degrees(N, src):
    return torch.zeros(N, dtype=torch.float64, device=src.device).index_add_(
        0, src, torch.ones(src.numel(), dtype=torch.float64, device=src.device))


def norm64(N, edge_index, half):
    """deg(src)^-1/2 * deg(dst)^-1/2 in float64, deg = the half's count by SOURCE, 0 where the degree is 0."""
    E = edge_index.size(1) // 2
    src, dst = edge_index[0, half * E:(half + 1) * E], edge_index[1, half * E:(half + 1) * E]
    deg = _degrees(N, src)
    c = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
    return c[src] * c[dst]


def norm32(N, edge_index, half):
    """The f32 norm as csr_build.cpp forms it: (1 / sqrt(float(deg_s))) * (1 / sqrt(float(deg_d)))."""
    E = edge_index.size(1) // 2
    src, dst = edge_index[0, half * E:(half + 1) * E], edge_index[1, half * E:(half + 1) * E]
    deg = _degrees(N, src).float()
    c = torch.where(deg > 0, 1.0 / torch.sqrt(deg.clamp(min=1)), torch.zeros_like(deg))
    return c[src] * c[dst]


def _halves(N, edge_index, edge_type, norms, norm_fn):
    E = edge_index.size(1) // 2
    for h in range(2):
        sl = slice(h * E, (h + 1) * E)
        nrm = norms[h] if norms is not None else norm_fn(N, edge_index, h)
        yield h, sl, edge_index[0, sl], edge_index[1, sl], edge_type[sl], nrm


def _count(rows, idx, device):
    return torch.zeros(rows, dtype=torch.float64, device=device).index_add_(
        0, idx, torch.ones(idx.numel(), dtype=torch.float64, device=device))


# ----------------------------------------------------------------------------------------------------------------
# float64 references (value, n = number of terms, mag = sum of |term|), all per element
def forward64(N, edge_index, edge_type, x, rel, ee, norms=None):
    """The differentiable float64 forward, [N, 2D]: out[dst, half] += x[src] * rel[type] (* ee[edge]) * norm."""
    outs = []
    for h, sl, src, dst, typ, nrm in _halves(N, edge_index, edge_type, norms, norm64):
        m = x[src] * rel[typ]
        if ee is not None:
            m = m * ee[sl]
        m = m * nrm.to(m.dtype).unsqueeze(1)
        outs.append(torch.zeros((N, x.size(1)), dtype=m.dtype, device=m.device).index_add(0, dst, m))
    return torch.cat(outs, 1)


def ref_forward(N, edge_index, edge_type, x, rel, ee, norms=None):
    """x [N, D], rel [rows, D], ee [2E, D] in edge-id order or None -> Ref of [N, 2D]."""
    x, rel = x.double(), rel.double()
    ee = None if ee is None else ee.double()
    D, dev = x.size(1), x.device
    val = torch.zeros((N, 2 * D), dtype=torch.float64, device=dev)
    mag, n = torch.zeros_like(val), torch.zeros_like(val)
    for h, sl, src, dst, typ, nrm in _halves(N, edge_index, edge_type, norms, norm64):
        m = x[src] * rel[typ]
        if ee is not None:
            m = m * ee[sl]
        m = m * nrm.double().unsqueeze(1)
        val[:, h * D:(h + 1) * D].index_add_(0, dst, m)
        mag[:, h * D:(h + 1) * D].index_add_(0, dst, m.abs())
        n[:, h * D:(h + 1) * D] += _count(N, dst, dev).unsqueeze(1)
    return Ref(val, n, mag)


def ref_loop(x, rel, loop_edge):
    """Self-loop block (x * rel[-1]) * loop_edge in float64, [N, D]."""
    return x.double() * rel[-1].double() * loop_edge.double()


def ref_grads(N, edge_index, edge_type, x, rel, ee, g, norms=None, edge_mask=None):
    """Explicit gradient sums for g [N, 2D] -> (gx Ref [N, D], gee Ref [2E, D] in EDGE-ID order, grel Ref [rows, D]).
    `ee` None: the forward had no per-edge table (gee is then the gradient w.r.t. a table of ones). `edge_mask` [2E] bool:
    only those edges contribute to gx / grel (a destination range's share)."""
    x, rel, g = x.double(), rel.double(), g.double()
    ee = None if ee is None else ee.double()
    D, dev, E2 = x.size(1), x.device, edge_index.size(1)
    rows = rel.size(0)
    z = lambda r: torch.zeros((r, D), dtype=torch.float64, device=dev)
    gx, gx_mag, gx_n = z(N), z(N), z(N)
    gr, gr_mag, gr_n = z(rows), z(rows), z(rows)
    gee = z(E2)
    for h, sl, src, dst, typ, nrm in _halves(N, edge_index, edge_type, norms, norm64):
        gn = g[dst, h * D:(h + 1) * D] * nrm.double().unsqueeze(1)
        gee[sl] = gn * x[src] * rel[typ]
        tx, tr = gn * rel[typ], gn * x[src]
        if ee is not None:
            tx, tr = tx * ee[sl], tr * ee[sl]
        if edge_mask is not None:
            keep = edge_mask[sl]
            src, typ, tx, tr = src[keep], typ[keep], tx[keep], tr[keep]
        gx.index_add_(0, src, tx); gx_mag.index_add_(0, src, tx.abs()); gx_n += _count(N, src, dev).unsqueeze(1)
        gr.index_add_(0, typ, tr); gr_mag.index_add_(0, typ, tr.abs()); gr_n += _count(rows, typ, dev).unsqueeze(1)
    return Ref(gx, gx_n, gx_mag), Ref(gee, torch.ones_like(gee), gee.abs()), Ref(gr, gr_n, gr_mag)


def select_rows(ref, idx):
    return Ref(ref.value.index_select(0, idx), ref.n.index_select(0, idx), ref.mag.index_select(0, idx))


def slice_ref(ref, rows=slice(None), cols=slice(None)):
    return Ref(ref.value[rows, cols], ref.n[rows, cols], ref.mag[rows, cols])


# ----------------------------------------------------------------------------------------------------------------
# the bar
def bar_of(ref):
    return BAR_SLACK * (ref.n + TERM_ROUNDINGS) * U * ref.mag


def loop_bar(value):
    return LOOP_BAR_U * U * value.abs()


def worst_ratio(got, ref):
    """-> (worst |got - ref| / bar over the elements with terms, number of term-less elements that are not exactly 0.0,
    flat index of the worst element). Non-finite `got` counts as an infinite ratio."""
    got = got.double()
    live = ref.n > 0
    err = (got - ref.value).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    ratio = torch.where(live, err / bar_of(ref).clamp(min=1e-300), torch.zeros_like(err))
    bad_zero = int(((got != 0) & ~live).sum())
    if ratio.numel() == 0:
        return 0.0, bad_zero, -1
    flat = ratio.reshape(-1)
    k = int(flat.argmax())
    return float(flat[k]), bad_zero, k


def check(got, ref, what):
    """Per-element assertion; returns the worst ratio (for the RATIO line)."""
    assert tuple(got.shape) == tuple(ref.value.shape), '%s: shape %s, reference %s' % (what, tuple(got.shape), tuple(ref.value.shape))
    ratio, bad_zero, k = worst_ratio(got, ref)
    assert bad_zero == 0, '%s: %d elements without a single term are not exactly 0.0' % (what, bad_zero)
    if ratio > 1.0:
        cols = ref.value.size(1)
        raise AssertionError('%s: element (%d, %d) is %.3g x its bar: got %r, float64 %r, n = %d'
                             % (what, k // cols, k % cols, ratio, float(got.reshape(-1)[k]), float(ref.value.reshape(-1)[k]),
                                int(ref.n.reshape(-1)[k])))
    return ratio


def check_loop(got, value, what):
    got = got.double()
    assert bool(torch.isfinite(got).all()), '%s: non-finite' % what
    if got.numel() == 0:
        return 0.0
    ratio = float(((got - value).abs() / loop_bar(value).clamp(min=1e-300)).max())
    assert ratio <= 1.0, '%s: self-loop block is %.3g x its bar' % (what, ratio)
    return ratio


# ----------------------------------------------------------------------------------------------------------------
# f32 emulation (host test only): the same sums in f32 on the CPU, edge order, csr_build.cpp's f32 norm
def emul_forward_f32(N, edge_index, edge_type, x, rel, ee):
    D = x.size(1)
    out = torch.zeros((N, 2 * D), dtype=torch.float32)
    for h, sl, src, dst, typ, nrm in _halves(N, edge_index, edge_type, None, norm32):
        m = x[src] * rel[typ]
        if ee is not None:
            m = m * ee[sl]
        out[:, h * D:(h + 1) * D].index_add_(0, dst, m * nrm.unsqueeze(1))
    return out


def emul_grads_f32(N, edge_index, edge_type, x, rel, ee, g):
    """-> (gx, gee in edge-id order, grel), each product in the kernels' order of factors."""
    D, E2 = x.size(1), edge_index.size(1)
    gx = torch.zeros((N, D), dtype=torch.float32)
    gr = torch.zeros((rel.size(0), D), dtype=torch.float32)
    gee = torch.zeros((E2, D), dtype=torch.float32)
    for h, sl, src, dst, typ, nrm in _halves(N, edge_index, edge_type, None, norm32):
        gn = g[dst, h * D:(h + 1) * D] * nrm.unsqueeze(1)
        gee[sl] = (gn * x[src]) * rel[typ]
        tx, tr = gn * rel[typ], gn * x[src]
        if ee is not None:
            tx, tr = tx * ee[sl], tr * ee[sl]
        gx.index_add_(0, src, tx)
        gr.index_add_(0, typ, tr)
    return gx, gee, gr


# ----------------------------------------------------------------------------------------------------------------
# graphs: each -> (N, R, edge_index [2, 2E], edge_type [2E]) with the mirrored second half (types r + R); the relation
# table has 2R + 1 rows
def _mirrored(N, R, s, o, r):
    s, o, r = (torch.tensor(v, dtype=torch.int64) for v in (s, o, r))
    ei = torch.stack((torch.cat((s, o)), torch.cat((o, s))))
    return N, R, ei, torch.cat((r, r + R))


def degree_runs(gs):
    """Run lengths at the edges of the slot walk: every batch size U in {1, 2, 4} at U - 1 / U / U + 1, the record window
    of 2 gs slots at -1 / 0 / +1, and a third window's first slot."""
    return [0, 1, 2, 3, 4, 5, 2 * gs - 1, 2 * gs, 2 * gs + 1, 4 * gs + 1]


def degree_profile(gs):
    """Destinations 0..9 have the in-degrees degree_runs(gs) in half 0; nodes 10..18 have the first nine of them in half 1
    (they are sources there). Sources come from a pool of 20 nodes, so long runs repeat edges; two pool nodes carry self
    edges (one twice); nodes 0, 10 (the runs of length 0), 19, 30 and N - 1 are isolated. The norm counts BOTH endpoints' degrees by source, so every
    destination also leaves an edge in the same half (else all its terms would be zero and nothing would be tested)."""
    runs = degree_runs(gs)
    pool = [n for n in range(20, 41) if n != 30]
    N, R = 42, 3
    s, o, r = [], [], []
    for d, L in enumerate(runs):
        for k in range(L):
            s.append(pool[(7 * k + d) % len(pool)]); o.append(d); r.append((k + d) % R)
    for d, L in enumerate(runs[:-1]):
        for k in range(L):
            s.append(10 + d); o.append(pool[(3 * k + 2 * d) % len(pool)]); r.append((k + 2 * d) % R)
    for j, p in enumerate(pool):                 # destinations 0..9 as sources of half 0 (and every pool node entered in it)
        s.append(1 + j % 9); o.append(p); r.append(j % R)
    for d in range(1, len(runs) - 1):             # nodes 10..18 entered in half 0 = sources of half 1
        s.append(pool[d]); o.append(10 + d); r.append(d % R)
    for p, times in ((pool[0], 1), (pool[5], 2)):
        for _ in range(times):
            s.append(p); o.append(p); r.append(1)
    return _mirrored(N, R, s, o, r)


HUB_CHUNK_COUNTS = (17, 1, 2, 15, 16, 32, 33, 16 * 16 + 1)


def hub_profile(thr=1, chunk=2):
    """Hubs (in-degree > thr) whose chunk counts in half 0 are HUB_CHUNK_COUNTS: node 0 has 17 (two fold levels, a last
    span of one row), nodes 1..6 one to 33, the LAST node 257 (17 spans: the level-2 fold has 17 rows). Every other count
    has a ragged last chunk. Each of them leaves ONE edge (so its norm is not zero) and is a hub in half 0 only; the 30 pool
    nodes that feed them are entered once in half 0 (ordinary runs of one slot) and are hubs in half 1 only. Four feeder
    nodes enter every pool node."""
    assert thr >= 1 and chunk >= 2
    P = 30
    pool = list(range(7, 7 + P))
    feeders = list(range(7 + P, 11 + P))
    N, R = 12 + P, 2
    hubs = list(range(7)) + [N - 1]
    s, o, r = [], [], []
    for i, (hub, cnt) in enumerate(zip(hubs, HUB_CHUNK_COUNTS)):
        L = max(cnt * chunk - (1 if (i % 2 and cnt > 1) else 0), thr + 1)
        for k in range(L):
            s.append(pool[(11 * k + 3 * i) % P]); o.append(hub); r.append((k + i) % R)
        s.append(hub); o.append(feeders[i % 4]); r.append(i % R)
    for j, p in enumerate(pool):
        s.append(feeders[j % 4]); o.append(p); r.append(j % R)
    return _mirrored(N, R, s, o, r)


TYPE_RUNS = (16, 0, 1, 15, 17, 33)


def type_profile(small=False):
    """Relation slot runs TYPE_RUNS (each twice: types r and r + R): type 0 fills chunk 0 exactly, type 2 starts on slot 16
    (a chunk boundary) and shares chunk 1 with type 3, which starts on 17; 33 slots span three chunks; 2E = 164 is no
    multiple of 16. `small`: 2E = 10 < 16, one chunk holding four types and one empty relation."""
    runs = (2, 0, 3) if small else TYPE_RUNS
    N, R = (5, 3) if small else (12, len(TYPE_RUNS))
    s, o, r = [], [], []
    k = 0
    for t, cnt in enumerate(runs):
        for _ in range(cnt):
            s.append(k % N); o.append(((2 * k + 1) if small else (5 * k + 2)) % N); r.append(t); k += 1
    return _mirrored(N, R, s, o, r)


LONG_TYPE_SLOTS = 64 * 16 * 16 + 116


def long_type():
    """One relation with more than 64 * 16 * 16 slots: at D = 4 (4 lanes per group, 64 groups, 16 rows in flight) the
    stage-2 loop of the by-type reduction runs more than once. Run at D = 4 only."""
    N, R = 64, 2
    s, o, r = [], [], []
    for k in range(LONG_TYPE_SLOTS + 37):
        s.append((13 * k + k // 64) % N); o.append((29 * k + 7) % N); r.append(0 if k < LONG_TYPE_SLOTS else 1)
    return _mirrored(N, R, s, o, r)


def switch_pair(N=24):
    """The same node set with E = 4N - 1 and E = 4N: the two sides of the `E < 4N` switch."""
    out = []
    for E in (4 * N - 1, 4 * N):
        s = [(5 * k + 1) % N for k in range(E)]
        o = [(7 * k + 3 + k // N) % N for k in range(E)]
        r = [k % 2 for k in range(E)]
        out.append(_mirrored(N, 2, s, o, r))
    return out


SWITCH_CASES = [_c(100, 'v4c1g32'), _c(4, 'v4c1g4'), _c(65, 'v1c2g64')]


def host_grid():
    """(label, graph) of every graph / width family the GPU tests run, for the host test's emulation sweep."""
    yield 'type', type_profile(), [c.d for c in BWD_CASES]
    yield 'type_small', type_profile(small=True), [c.d for c in GEOM_CASES]
    for gs in (4, 8, 16, 32, 64):
        yield 'degree%d' % gs, degree_profile(gs), sorted({c.d for c in FWD_CASES if case_geometry(c)[2] == gs})
    yield 'hub', hub_profile(), [c.d for c in GEOM_CASES]
    for i, gr in enumerate(switch_pair()):
        yield 'switch%d' % i, gr, [c.d for c in SWITCH_CASES]
    yield 'long_type', long_type(), [4]
