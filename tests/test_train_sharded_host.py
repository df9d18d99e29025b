"""CPU-only tests of the per-shard index lists of the destination-partitioned training step (GraphCSR.shard_backward_index,
include/mgcn_hip.h (3s)): over the ranks of a partition every slot is listed exactly once, each list run is in the order the
backward sums it, and the lists of one rank owning the whole graph are the whole graph's."""
import types

import numpy as np
import pytest
import torch

from .conftest import golden


def random_graph(num_nodes, num_rel, num_edges, zipf=0.0, seed=0):
    """A mirror-symmetric edge list as the loader builds it (data_loader.py:143-149): edges (s, r, o), then (o, r + R, s).
    zipf > 0 draws subjects and objects from a Zipf-like law (heavy destinations: hubs)."""
    g = torch.Generator().manual_seed(seed)
    if zipf > 0:
        w = 1.0 / torch.arange(1, num_nodes + 1, dtype=torch.float64) ** zipf
        s = torch.multinomial(w, num_edges, replacement=True, generator=g)
        o = torch.multinomial(w, num_edges, replacement=True, generator=g)
        perm = torch.randperm(num_nodes, generator=g)
        s, o = perm[s], perm[o]
    else:
        s = torch.randint(0, num_nodes, (num_edges,), generator=g)
        o = torch.randint(0, num_nodes, (num_edges,), generator=g)
    r = torch.randint(0, num_rel, (num_edges,), generator=g)
    edge_index = torch.stack([torch.cat([s, o]), torch.cat([o, s])])
    edge_type = torch.cat([r, r + num_rel])
    return edge_index, edge_type


def _golden_csr(pkg, case, **kw):
    g = golden(case)
    ei, et = g.t('dl_edge_index'), g.t('dl_edge_attr')[0]
    N, R = int(g['dl_num_entity']), int(g['dl_num_relation'])
    return pkg.GraphCSR(N, 2 * R + 1, ei, et, 'cpu', **kw)


def _check_lists(pkg, csr, world):
    E2, N = 2 * csr.num_edges_half, csr.num_nodes
    src_all, half_all = csr.rec[:, 0].long(), (csr.slot_dst.long() >> 31) & 1
    typ_all, mirror = csr.rec[:, 1].long(), csr.mirror.long()
    b = csr.balanced_bounds(world)
    seen_type, seen_src = [], []
    chunk_slots = [[] for _ in range(csr.num_chunks)]
    for r in range(world):
        n0, n1 = b[r], b[r + 1]
        counts, sub = csr.shard_slot_counts(n0, n1), csr.shard_ee_sub(n0, n1)
        rows = sum(counts)
        row_slot = torch.arange(rows) + torch.tensor(sub).repeat_interleave(torch.tensor(counts))
        idx = csr.shard_backward_index(n0, n1)
        assert idx is csr.shard_backward_index(n0, n1)                     # built once per range
        tp, tr = idx['type_ptr'].long(), idx['type_rows'].long()
        sp, sr = idx['src_ptr'].long(), idx['src_rows'].long()
        assert tp.numel() == csr.num_rel_rows + 1 and int(tp[-1]) == rows and tr.numel() == rows
        assert sp.numel() == 2 * N + 1 and int(sp[-1]) == rows and sr.numel() == rows
        ts, ss = row_slot[tr], row_slot[sr]
        seen_type.append(ts)
        seen_src.append(ss)
        for t in range(csr.num_rel_rows):                                  # by relation row, ascending slot order
            run = ts[tp[t]:tp[t + 1]]
            assert bool((typ_all[run] == t).all()) and bool((run[1:] > run[:-1]).all())
        grp = src_all[ss] * 2 + half_all[ss]                               # by (source, half) ...
        assert bool((grp[1:] >= grp[:-1]).all())
        assert torch.equal(sp[grp + 1] - sp[grp], torch.bincount(grp, minlength=2 * N)[grp])
        rev = mirror[ss]                                                   # ... each run in reverse-slot order
        same = grp[1:] == grp[:-1]
        assert bool((rev[1:][same] > rev[:-1][same]).all())
        if csr.num_chunks:
            ch = idx['src_chunks'].long()
            assert tuple(ch.shape) == (csr.num_chunks, 4) and torch.equal(ch[:, 2:], csr.chunks[:csr.num_chunks, 2:].long())
            for c in range(csr.num_chunks):
                beg, end = csr.chunks[c, 0].item(), csr.chunks[c, 1].item()
                part = rev[ch[c, 0]:ch[c, 1]]
                assert bool(((part >= beg) & (part < end)).all())
                chunk_slots[c].append(part)
    for lists in (seen_type, seen_src):                                    # every slot exactly once over the ranks
        assert torch.equal(torch.sort(torch.cat(lists)).values, torch.arange(E2))
    for c in range(csr.num_chunks):                                        # every hub chunk's reverses, split over the ranks
        beg, end = csr.chunks[c, 0].item(), csr.chunks[c, 1].item()
        assert torch.equal(torch.sort(torch.cat(chunk_slots[c])).values, torch.arange(beg, end))
    if world == 1:                                                         # one rank: the whole graph's by-type list
        idx = csr.shard_backward_index(0, N)
        assert torch.equal(idx['type_rows'], csr.typeslots) and torch.equal(idx['type_ptr'], csr.typeptr)


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('case,hubs', [('syn_a', False), ('syn_b', True), ('syn_c', False), ('syn_c', True)])
def test_shard_lists_on_goldens(pkg, case, hubs, world):
    csr = _golden_csr(pkg, case, **(dict(hub_threshold=3, hub_chunk=2) if hubs else dict(hub_threshold=0)))
    assert bool(csr.num_chunks) == hubs
    _check_lists(pkg, csr, world)


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('seed', [0, 1])
def test_shard_lists_on_random_graphs_with_hubs(pkg, world, seed):
    ei, et = random_graph(3000, 7, 20000, zipf=1.1, seed=seed)
    csr = pkg.GraphCSR(3000, 15, ei, et, 'cpu', hub_threshold=16, hub_chunk=8)
    assert csr.num_chunks > 0
    _check_lists(pkg, csr, world)


def test_shard_lists_of_an_empty_range(pkg):
    csr = _golden_csr(pkg, 'syn_b', hub_threshold=3, hub_chunk=2)
    idx = csr.shard_backward_index(5, 5)
    assert idx['type_rows'].numel() == 0 and idx['src_rows'].numel() == 0
    assert int(idx['src_ptr'][-1]) == 0 and bool((idx['src_chunks'][:, :2] == 0).all())


def test_shard_backward_binding_refuses_cpu_tensors(pkg):
    """No CPU path: the shard backward's binding raises before any launch."""
    csr = _golden_csr(pkg, 'syn_a')
    N, D = csr.num_nodes, 8
    rows = sum(csr.shard_slot_counts(0, N))
    with pytest.raises(pkg._native.NativeError, match='must live on a GPU'):
        pkg._native.aggregate_bwd_shard(csr, torch.zeros(N, D), torch.zeros(csr.num_rel_rows, D), torch.zeros(rows, D),
                                        torch.zeros(N, 2 * D), (0, N))


def test_epoch_order_is_new_every_epoch_and_follows_the_generator(pkg, monkeypatch):
    """train_epoch_sharded's batches (the step itself replaced by a recorder): without a generator every epoch takes a new
    order, as harness.train_device_labels does; with one, the order is torch.randperm's under that generator."""
    seen = []

    def record(model, graph, src, rel, index, optimizer, lbl_smooth=0.0, clip=None, group=None, generator=None):
        seen.append(torch.stack([src, rel], 1).clone())
        return torch.tensor(0.5)
    monkeypatch.setattr(pkg.dist, 'train_step_sharded', record)
    model = types.SimpleNamespace(entity_embedding=torch.zeros(1), train=lambda: None)
    params = types.SimpleNamespace(lbl_smooth=0.0, clip_grad=1.0)
    Q = 40
    queries = torch.stack([torch.arange(Q), torch.arange(Q) % 3], 1)

    def epoch(generator=None):
        seen.clear()
        assert pkg.dist.train_epoch_sharded(model, queries, None, None, None, params, 8, generator=generator) == 0.5
        return torch.cat(seen)
    first, second = epoch(), epoch()
    assert torch.equal(torch.sort(first[:, 0]).values, torch.arange(Q))         # every query once per epoch
    assert not torch.equal(first, second)
    given = epoch(torch.Generator().manual_seed(3))
    assert torch.equal(given[:, 0], torch.randperm(Q, generator=torch.Generator().manual_seed(3)))


def _subgroup_worker(rank, world, port, q):
    import importlib
    import os
    import sys

    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        d = importlib.import_module('kgc-gcn_amd').dist
        sub = dist.new_group([0, 1])
        t = torch.full((2, 3), float(rank))
        first = d._gather(t, sub, 2).sum(1).tolist() if rank < 2 else None     # ranks 0, 1 exchange on their sub-group first
        second = d._gather(t, None, world).sum(1).tolist()                      # then every rank on WORLD: each group probes
        q.put((rank, first, second))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:                                                          # surface the failure in the parent
        import traceback
        q.put((rank, 'error', traceback.format_exc()))


def test_gather_capability_is_probed_per_group():
    """A sub-group's exchange before the first WORLD exchange: the members of the sub-group must still take part in WORLD's
    capability probe (one probe per group), or the ranks would sit in different collectives."""
    import os

    import torch.multiprocessing as mp
    world, port = 3, 30500 + (os.getpid() * 3) % 2000
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_subgroup_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {r: (a, b) for r, a, b in [q.get(timeout=120) for _ in range(world)]}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        assert got[r][0] != 'error', got[r][1]
        assert got[r][1] == [0.0, 0.0, 3.0, 3.0, 6.0, 6.0]
    assert got[0][0] == got[1][0] == [0.0, 0.0, 3.0, 3.0] and got[2][0] is None
