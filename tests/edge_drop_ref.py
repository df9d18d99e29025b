"""Restatement of include/mgcn_hip.h (19) in Python integers and numpy, from the edge list alone: the keep bits
of tests/dropout_ref.py, integer degrees of the kept list, the table T as the host entry point returns it, one f32 multiply per
kept edge. Nothing here walks slots, runs or chunks: the records are formed per directed edge and laid out through `perm`.
Also the cases that the host and GPU tests share."""
import numpy as np
import torch

from . import aggregate_ref as ar
from . import dropout_ref as dr

SITE = 0x3000


def keep_bits(seed, step, p, E):
    """keep(u), u = 0 .. E - 1: column 0 of the [E, 1] mask under key(seed, step, SITE) and T(p) (T = 0 for p >= 1)."""
    thr = 0 if p >= 1 else dr.threshold(max(p, 0.0))
    if E == 0:
        return np.zeros(0, dtype=bool)
    return dr.mask(dr.key(seed, step, SITE), E, 1, 0, thr)[:, 0].astype(bool)


def kept_edges(seed, step, p, E, forced=None):
    k = keep_bits(seed, step, p, E)
    return k if forced is None else k & ~np.asarray(forced, dtype=bool)


def edge_norms(N, edge_index, kept, table):
    """f32 norm of every directed edge d in [0, 2E): T[deg_h[src]] * T[deg_h[dst]] for a kept edge, +0.0 else; deg_h[n] = the
    kept edges of half 1 - h that ENTER n (the definition's destination run, counted without a layout)."""
    ei = np.asarray(edge_index)
    E = ei.shape[1] // 2
    table = np.asarray(table, dtype=np.float32)
    out = np.zeros(2 * E, dtype=np.float32)
    for h in range(2):
        o = 1 - h
        deg = [0] * N
        for d in range(o * E, (o + 1) * E):
            if kept[d - o * E]:
                deg[int(ei[1, d])] += 1
        for d in range(h * E, (h + 1) * E):
            if kept[d - h * E]:
                out[d] = np.float32(table[deg[int(ei[0, d])]]) * np.float32(table[deg[int(ei[1, d])]])
    return out


def records(host, norms):
    """rec' [2E, 4] int32 from the canonical layout `host` (csr_build_host's dict) and the per-edge norms: src, type and eid as
    they are, the norm bits of the slot's edge."""
    rec = host['rec'].numpy().copy()
    rec[:, 2] = norms[host['perm'].numpy()].view(np.int32)
    return rec


def kept_list(edge_index, edge_type, kept):
    """The kept edge list alone, mirrored halves, and the original edge id of each of its entries."""
    E = edge_index.size(1) // 2
    idx = torch.from_numpy(np.nonzero(kept)[0].astype(np.int64))
    ids = torch.cat((idx, idx + E))
    return edge_index[:, ids].contiguous(), edge_type[ids].contiguous(), ids


def norm64_kept(N, edge_index, kept):
    """[norm of half 0, norm of half 1] in float64 of the kept sub-graph, 0 on dropped edges: `norms=` of aggregate_ref."""
    E = edge_index.size(1) // 2
    k = torch.from_numpy(np.asarray(kept, dtype=bool))
    out = []
    for h in range(2):
        src, dst = edge_index[0, h * E:(h + 1) * E], edge_index[1, h * E:(h + 1) * E]
        deg = torch.zeros(N, dtype=torch.float64).index_add_(0, src[k], torch.ones(int(k.sum()), dtype=torch.float64))
        c = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
        out.append(torch.where(k, c[src] * c[dst], torch.zeros(E, dtype=torch.float64)))
    return out


# -- the flags -------------------------------------------------------------------------------------
def edge_keys(edge_index, edge_type, R):
    return (edge_index[0].to(torch.int64) * (2 * R) + edge_type.to(torch.int64)).tolist()


def flags(edge_index, edge_type, R, qkeys):
    """forced [E] uint8 by definition: u is marked iff one of its two directions has a key among the queries'."""
    E = edge_index.size(1) // 2
    want = set(int(q) for q in qkeys)
    out = np.zeros(E, dtype=np.uint8)
    for d, k in enumerate(edge_keys(edge_index, edge_type, R)):
        if k in want:
            out[d % E] = 1
    return out


def flags_by_bisect(ekeys, eund, E, qkeys):
    """What the kernel does with the sorted arrays: lower bound, then the run of equal keys."""
    ekeys, eund = [int(v) for v in ekeys], [int(v) for v in eund]
    out = np.zeros(E, dtype=np.uint8)
    for q in qkeys:
        lo, hi = 0, len(ekeys)
        while lo < hi:
            mid = (lo + hi) >> 1
            if ekeys[mid] < int(q):
                lo = mid + 1
            else:
                hi = mid
        while lo < len(ekeys) and ekeys[lo] == int(q):
            if 0 <= eund[lo] < E:
                out[eund[lo]] = 1
            lo += 1
    return out


def query_cases(edge_index, edge_type, R, N):
    """{label: list of query keys}: a query with no edge, an inverse-relation query, two queries sharing edges (one undirected
    edge named from both ends, and one query twice), keys below the first and above the last edge key, and a mix."""
    keys = edge_keys(edge_index, edge_type, R)
    E = len(keys) // 2
    have = set(keys)
    none = next(s * 2 * R + r for s in range(N) for r in range(2 * R) if s * 2 * R + r not in have)
    inverse = keys[E + 1]                  # a direction of the second half: relation r + R
    both_ends = [keys[2], keys[E + 2]]     # the two directions of undirected edge 2
    below, above = min(keys) - 1, max(keys) + 1
    return {'none': [none], 'inverse': [inverse], 'shared': both_ends + [keys[2]], 'below_above': [below, above, -5, N * 2 * R + 7],
            'mix': [keys[0], none, inverse, above, keys[E - 1], keys[7], keys[7]], 'empty': []}


# -- the shared cases ------------------------------------------------------------------------------
def graphs():
    """label -> (N, R, edge_index, edge_type, hub_threshold, hub_chunk): degree_profile (self edges, duplicate triples, isolated
    nodes), hub_profile with its chunk counts (hubs in both halves), type_profile. No E is a multiple of 64."""
    return {'degree': ar.degree_profile(8) + (0, 64), 'hub': ar.hub_profile(1, 2) + (1, 2), 'type': ar.type_profile() + (0, 64)}


def node_edges(edge_index, n):
    """forced [E] uint8 marking every undirected edge that touches node n."""
    E = edge_index.size(1) // 2
    s, o = edge_index[0, :E], edge_index[1, :E]
    return ((s == n) | (o == n)).numpy().astype(np.uint8)


def every_third(E):
    f = np.zeros(E, dtype=np.uint8)
    f[::3] = 1
    return f


SEED, STEP = 11, 4
# (label, p, forced maker or None): p = 0 with and without forced, forced alone, 0 < p < 1, p >= 1
DROP_CASES = [('p0', 0.0, None), ('p0_forced', 0.0, 'third'), ('p0_node', 0.0, 'node'), ('p02', 0.2, None), ('p05_forced', 0.5, 'third'),
              ('p05', 0.5, None), ('p1', 1.0, None), ('p15_forced', 1.5, 'third')]


def forced_of(kind, edge_index, node):
    E = edge_index.size(1) // 2
    return None if kind is None else every_third(E) if kind == 'third' else node_edges(edge_index, node)
