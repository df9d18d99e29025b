"""Filtered top-k (section (7) of mgcn_hip.h) without a GPU: argument validation of the C ABI, the workspace formula,
the Python surface's refusal of CPU tensors, and gloo world-2 / world-3 rehearsals of dist.sharded_topk with torch
stand-ins for the two kernels: the sharded lists must equal the unsharded ones exactly."""
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from .conftest import ROOT, load_pkg


def _ws_formula(B, n, k):
    """mgcn_score_topk_workspace as the header states it."""
    a256 = lambda v: (v + 255) // 256 * 256
    C = min(n, 1 << 18)
    S = (C + 4095) // 4096
    return a256(4 * B * ((C + 3) // 4 * 4)) + a256(4 * B * (S + 1) * k) + 8 * B * (S + 1) * k


def test_topk_abi_argument_validation_without_a_gpu(pkg):
    """Every bad argument comes back as MGCN_EINVAL (1) with a message before any HIP call. The fake pointers are never
    dereferenced: every case below fails validation."""
    lib = pkg._native.lib()
    N, P = None, 256                               # null / a fake, 16-byte aligned address
    ws = lib.mgcn_score_topk_workspace(4, 100, 10)
    assert ws == _ws_formula(4, 100, 10)

    def topk(batch=4, n=100, row0=0, dim=8, x=P, ldx=8, ent=P, lde=8, bias=P, mask=N, ldm=0, k=10, os_=P, ldo=10,
             oi=P, ldi=10, w=P, wb=ws):
        return lib.mgcn_score_topk(batch, n, row0, dim, x, ldx, ent, lde, bias, mask, ldm, k, os_, ldo, oi, ldi, w, wb, N)

    cases = [
        (dict(x=N), 'null pointer'), (dict(ent=N), 'null pointer'), (dict(bias=N), 'null pointer'),
        (dict(os_=N), 'null pointer'), (dict(oi=N), 'null pointer'), (dict(w=N), 'null pointer'),
        (dict(k=0), r'k = 0 outside \[1, 1024\]'), (dict(k=1025), r'k = 1025 outside \[1, 1024\]'),
        (dict(ldx=7), 'leading dimension'), (dict(lde=7), 'leading dimension'),
        (dict(ldo=9), 'leading dimension'), (dict(ldi=9), 'leading dimension'),
        (dict(mask=P, ldm=3), 'mask rows too short'),                      # ceil(100 / 32) = 4 words
        (dict(wb=ws - 1), 'workspace of %d bytes, needs %d' % (ws - 1, ws)),
        (dict(w=P + 8), '16-byte aligned'),
        (dict(batch=-1), 'bad sizes'), (dict(n=-1), 'bad sizes'), (dict(dim=0), 'bad sizes'), (dict(row0=-1), 'bad sizes'),
        (dict(row0=(1 << 31) - 50), 'below 2\\^31'),
    ]
    for kw, pattern in cases:
        rc = topk(**kw)
        msg = lib.mgcn_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert re.search(pattern, msg), (kw, msg)
    assert topk(batch=0) == 0                      # nothing to do: returns before any launch

    merge_cases = [
        ((4, 2, N, P, 20, 10, P, P, N), 'null pointer'),
        ((4, 2, P, N, 20, 10, P, P, N), 'null pointer'),
        ((4, 2, P, P, 20, 10, N, P, N), 'null pointer'),
        ((4, 2, P, P, 20, 10, P, N, N), 'null pointer'),
        ((4, 2, P, P, 20, 0, P, P, N), r'k = 0 outside'),
        ((4, 2, P, P, 20 * 103, 1025, P, P, N), r'k = 1025 outside'),
        ((4, 2, P, P, 19, 10, P, P, N), 'leading dimension too small'),
        ((4, -1, P, P, 20, 10, P, P, N), 'bad sizes'),
    ]
    for args, pattern in merge_cases:
        rc = lib.mgcn_topk_merge(*args)
        msg = lib.mgcn_last_error().decode()
        assert rc == 1, (args, rc, msg)
        assert re.search(pattern, msg), (args, msg)
    assert lib.mgcn_topk_merge(0, 2, P, P, 20, 10, P, P, N) == 0


def test_topk_workspace_formula_and_bound(pkg):
    lib = pkg._native.lib()
    for B, n, k in [(1, 1, 1), (128, 40943, 10), (128, 40943, 100), (333, 40943, 1024), (128, 14541, 10), (3, 4095, 7),
                    (3, 4096, 7), (3, 4097, 7), (128, 1 << 18, 10), (128, 600000, 100), (5, 0, 3)]:
        assert lib.mgcn_score_topk_workspace(B, n, k) == _ws_formula(B, n, k), (B, n, k)
    # scored in chunks of 2^18 rows: the workspace stops growing there (configs[4]: 1.25 M rows per rank)
    cap = lib.mgcn_score_topk_workspace(128, 1 << 18, 100)
    for n in (1 << 18, 600000, 1250000, 10 ** 8, (1 << 31) - 100):
        assert lib.mgcn_score_topk_workspace(128, n, 100) == cap
    assert cap <= 4 * 128 * (1 << 18) + 12 * 128 * 65 * 100 + 512      # the score block + 65 lists of k per query
    assert lib.mgcn_score_topk_workspace(4, 100, 0) == 0 and lib.mgcn_score_topk_workspace(4, 100, 1025) == 0
    assert lib.mgcn_score_topk_workspace(-1, 100, 5) == 0


def test_topk_python_surface_needs_a_gpu(pkg):
    nat = pkg._native
    x, ent, bias = torch.zeros(2, 8), torch.zeros(5, 8), torch.zeros(5)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.score_topk(x, ent, bias, 3)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.topk_merge(torch.zeros(2, 6), torch.zeros(2, 6, dtype=torch.int64), 3)
    with pytest.raises(nat.NativeError, match='outside'):
        nat.score_topk(x, ent, bias, 0)
    with pytest.raises(nat.NativeError, match='lists'):
        nat.topk_merge(torch.zeros(2, 7), torch.zeros(2, 7, dtype=torch.int64), 3)


# ---------------------------------------------------------------------------------------------------------------------
# gloo rehearsal of dist.sharded_topk

def contract_topk(scores, ids, valid, k):
    """The contract by plain torch: drop the invalid entries, stable sort by score descending over ids in ascending
    order, first k, padded with (-inf, -1)."""
    B = scores.size(0)
    out_s = torch.full((B, k), float('-inf'))
    out_i = torch.full((B, k), -1, dtype=torch.int64)
    for b in range(B):
        s, i = scores[b][valid[b]], ids[b][valid[b]]
        o = torch.argsort(i, stable=True)
        s, i = s[o], i[o]
        o = torch.argsort(s, descending=True, stable=True)[:k]
        out_s[b, :o.numel()], out_i[b, :o.numel()] = s[o], i[o]
    return out_s, out_i


class TorchTopkKernels(object):
    """Same interface as kgc-gcn_amd._native for filter_mask / score_topk / topk_merge (test stand-in, CPU; the mask is
    a dense bool block here)."""

    @staticmethod
    def filter_mask(qkey, keys, ptr, tails, n_local, ent_row0=0, out=None):
        dense = torch.zeros((qkey.numel(), n_local), dtype=torch.bool)
        for b, k in enumerate(qkey.tolist()):
            i = int(torch.searchsorted(keys, torch.tensor(k)))
            if i < keys.numel() and int(keys[i]) == k:
                t = tails[ptr[i]:ptr[i + 1]].long() - ent_row0
                t = t[(t >= 0) & (t < n_local)]
                dense[b, t] = True
        return dense

    @staticmethod
    def score(x, ent, bias):
        """sigmoid(x . ent[n] + bias[n]) summed in a fixed order, one elementwise step per column: a BLAS matmul may round
        a shard's rows differently from the same rows of the whole table (its blocking depends on the shape and the CPU),
        which would make shards disagree with the whole for reasons that have nothing to do with the exchange."""
        acc = x[:, None, 0] * ent[None, :, 0]
        for j in range(1, x.size(1)):
            acc = acc + x[:, None, j] * ent[None, :, j]
        return torch.sigmoid(acc + bias)

    @staticmethod
    def score_topk(x, ent, bias, k, mask=None, ent_row0=0):
        s = TorchTopkKernels.score(x, ent, bias)
        ids = (torch.arange(ent.size(0)) + ent_row0).expand(x.size(0), -1)
        valid = ~mask if mask is not None else torch.ones_like(s, dtype=torch.bool)
        return contract_topk(s, ids, valid, k)

    @staticmethod
    def topk_merge(scores, ids, k):
        return contract_topk(scores, ids, ids >= 0, k)


def _problem(seed=0, B=6, N=101, O=8, world=2):
    g = torch.Generator().manual_seed(seed)
    x = [torch.randn(B, O, generator=g) for _ in range(world)]
    ent, bias = torch.randn(N, O, generator=g) * 0.5, torch.randn(N, generator=g) * 0.1
    ent[60:70], bias[60:70] = ent[10:20], bias[10:20]      # equal scores in different shards: ties across the merge
    x[0][0] *= 40.0                                          # a query whose best scores saturate to 1.0f: long ties
    sub = [torch.randint(0, N, (B,), generator=g) for _ in range(world)]
    rel = [torch.randint(0, 4, (B,), generator=g) for _ in range(world)]
    known = {}
    for r in range(world):
        for b in range(B):
            known.setdefault((int(sub[r][b]), int(rel[r][b])), set()).update(
                int(v) for v in torch.randint(0, N, (3,), generator=g))
    # the second query of every rank has all but 5 entities filtered: fewer than k left, overall and in every shard
    for r in range(world):
        keep = set(torch.randperm(N, generator=g)[:5].tolist())
        known[(int(sub[r][1]), int(rel[r][1]))] = set(range(N)) - keep
    return x, ent, bias, sub, rel, known


KS = (10, 40)          # 40 > the 34 rows of a world-3 shard: local lists padded even unfiltered


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    pkg = load_pkg()
    x, ent, bias, sub, rel, known = _problem(world=world)
    filt = pkg.dist.FilterIndex.from_known(known, 4)
    b = pkg.dist.shard_bounds(ent.size(0), world)
    out = []
    for k in KS:
        for f in (filt, None):
            s, i = pkg.dist.sharded_topk(x[rank], filt.query_keys(sub[rank], rel[rank]), ent[b[rank]:b[rank + 1]],
                                         bias[b[rank]:b[rank + 1]], b[rank], k, filt=f, kernels=TorchTopkKernels)
            out.append((s.numpy().copy(), i.numpy().copy()))
    q.put((rank, out))      # arrays travel by value: a tensor's shared-memory handle dies with this process
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])   # 3: uneven entity shards (101 rows: 34 + 34 + 33), three query blocks
def test_sharded_topk_equals_unsharded_gloo(world):
    port = 29500 + (os.getpid() + 13 * world + 501) % 2000
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    pkg = load_pkg()
    x, ent, bias, sub, rel, known = _problem(world=world)
    filt = pkg.dist.FilterIndex.from_known(known, 4)
    for r in range(world):
        j = 0
        for k in KS:
            for f in (filt, None):
                want_s, want_i = pkg.dist.sharded_topk(x[r], filt.query_keys(sub[r], rel[r]), ent, bias, 0, k, filt=f,
                                                       kernels=TorchTopkKernels)
                got_s, got_i = (torch.from_numpy(v) for v in got[r][j])
                j += 1
                assert torch.equal(got_i, want_i), (r, k, f is None)
                assert torch.equal(got_s, want_s), (r, k, f is None)
                if f is not None:      # the nearly all-filtered query: 5 entities, then padding
                    assert (want_i[1, :5] >= 0).all() and (want_i[1, 5:] == -1).all()
                    assert torch.isinf(want_s[1, 5:]).all()
                else:
                    assert (want_i >= 0).all() if k <= ent.size(0) else True
    # the saturated query really has ties at 1.0 that come back in id order
    s, i = pkg.dist.sharded_topk(x[0], None, ent, bias, 0, 40, kernels=TorchTopkKernels)
    ones = i[0][s[0] == 1.0]
    assert ones.numel() >= 2 and torch.equal(ones, ones.sort().values)
