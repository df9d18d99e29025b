"""Graphs for the live-view tests (test_live_view_host.py, test_gpu_live_slots.py): edge lists given per half as
(src, dst, type) rows, so that a destination can be dead (norm exactly 0: it never occurs as a source in the same half,
include/mgcn_hip.h (1v)) in one half and live in the other — the feeder takes any [2, 2E] list split in halves by position."""
import numpy as np
import torch


def edge_list(half_in, half_out):
    """Two equally long lists of (src, dst, type) -> (edge_index [2, 2E] int64, edge_type [2E] int64)."""
    assert len(half_in) == len(half_out)
    rows = np.asarray(list(half_in) + list(half_out), dtype=np.int64).reshape(-1, 3)
    return torch.from_numpy(np.ascontiguousarray(rows[:, :2].T)), torch.from_numpy(np.ascontiguousarray(rows[:, 2]))


def host_norms(host):
    return host['rec'][:, 2].contiguous().view(torch.float32).numpy()


def run_states(host, half):
    """Per destination of the half's canonical layout: 'e' empty run, 'd' all slots dead, 'l' all live (a run is never
    mixed: a source has degree >= 1, so a slot is dead exactly when its destination has no degree)."""
    rp, nrm = host['rowptr'][half].numpy(), host_norms(host)
    out = []
    for n in range(len(rp) - 1):
        seg = nrm[rp[n]:rp[n + 1]]
        assert len(seg) == 0 or (seg == 0).all() or (seg != 0).all()
        out.append('e' if len(seg) == 0 else ('d' if (seg == 0).all() else 'l'))
    return ''.join(out)


def random_halves(N, R, share, seed, big=None, dead_block=None, dead_hub=None, max_in=5):
    """Seeded lists for both halves. Per half a source set S is drawn (a node is left out with probability `share`); every
    edge's source is in S, so a destination's run is dead exactly when the destination is not in S. share = 0: every node is a
    source (no dead slot); share = 1: destinations are drawn from outside S only (every slot dead).
    big = (node, slots): that destination is live with `slots` slots and its two neighbours are dead with slots;
    dead_block = (a, b): destinations a .. b - 1 are all dead, each with slots; dead_hub = (node, slots): a dead destination
    with that many slots."""
    rng = np.random.default_rng(seed)
    halves = []
    for h in range(2):
        if share >= 1.0:
            in_s = np.zeros(N, dtype=bool)
            in_s[rng.choice(N, size=max(1, N // 8), replace=False)] = True
        else:
            in_s = rng.random(N) >= share
            in_s[rng.integers(0, N)] = True
        forced_dead = []
        if big is not None:
            in_s[big[0]] = True
            forced_dead += [big[0] - 1, big[0] + 1]
        if dead_block is not None:
            forced_dead += list(range(dead_block[0], dead_block[1]))
        if dead_hub is not None:
            forced_dead.append(dead_hub[0])
        if share > 0:
            in_s[forced_dead] = False
        S = np.flatnonzero(in_s)
        edges = []
        if share < 1.0:
            edges += [(S[i], S[(i + 1) % len(S)], rng.integers(0, 2 * R)) for i in range(len(S))]   # every source has a degree
        for n in range(N):
            k = int(rng.integers(0, max_in + 1))
            if n in forced_dead:
                k = max(k, 1)
            if big is not None and n == big[0]:
                k = big[1] - 1                                                                       # (+ 1 from the ring)
            if dead_hub is not None and n == dead_hub[0]:
                k = dead_hub[1]
            if share >= 1.0 and in_s[n]:
                k = 0
            edges += [(S[rng.integers(0, len(S))], n, rng.integers(0, 2 * R)) for _ in range(k)]
        order = rng.permutation(len(edges))
        halves.append([edges[i] for i in order])
    E = max(len(halves[0]), len(halves[1]))
    for h in range(2):                       # equal halves: pad with copies of the half's first edge (same dead / live state)
        halves[h] += [halves[h][0]] * (E - len(halves[h]))
    return halves[0], halves[1]
