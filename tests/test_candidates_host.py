"""Candidate-list scoring (section (13) of mgcn_hip.h) without a GPU: the header and the export, argument validation of the
C ABI, the count rule of MGCN.rank_candidates against a plain loop, and gloo world-2 / world-3 rehearsals of
dist.sharded_score_candidates with a torch stand-in that keeps the kernel's rule "write only my shard's ids"."""
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from .conftest import ROOT, load_pkg


def test_header_declares_and_library_exports_score_candidates(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    assert re.search(r'\bint mgcn_score_candidates\(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim,', header)
    assert re.search(r'#define MGCN_ABI_VERSION 4\b', header)
    lib = pkg._native.lib()
    assert hasattr(lib, 'mgcn_score_candidates') and 'mgcn_score_candidates' in pkg._native.EXPORTS
    assert lib.mgcn_abi_version() == 4 == pkg._native.ABI_VERSION


def test_score_candidates_abi_argument_validation_without_a_gpu(pkg):
    """Every bad argument comes back as MGCN_EINVAL (1) with a message before any HIP call. The fake pointers are never
    dereferenced: every case below fails validation or has nothing to do."""
    lib = pkg._native.lib()
    N, P = None, 256                               # null / a fake, 16-byte aligned address

    def call(batch=4, n_cand=10, n=100, row0=0, dim=8, x=P, ldx=8, ent=P, lde=8, bias=P, cand=P, ldc=10, mask=N, ldm=0,
             out=P, ldo=10):
        return lib.mgcn_score_candidates(batch, n_cand, n, row0, dim, x, ldx, ent, lde, bias, cand, ldc, mask, ldm, out, ldo, N)

    cases = [
        (dict(x=N), 'null pointer'), (dict(ent=N), 'null pointer'), (dict(bias=N), 'null pointer'),
        (dict(cand=N), 'null pointer'), (dict(out=N), 'null pointer'),
        (dict(ldc=9), 'leading dimension'), (dict(ldo=9), 'leading dimension'),
        (dict(ldx=7), 'leading dimension'), (dict(lde=7), 'leading dimension'),
        (dict(row0=-1), 'bad sizes'), (dict(batch=-1), 'bad sizes'), (dict(n_cand=-1), 'bad sizes'), (dict(n=-1), 'bad sizes'),
        (dict(dim=0), 'bad sizes'), (dict(dim=-4), 'bad sizes'),
        (dict(n=(1 << 31) - 64), 'exceed int32'), (dict(batch=(1 << 31) - 64), 'exceed int32'),
        (dict(n_cand=(1 << 31) - 64, ldc=1 << 31, ldo=1 << 31), 'exceed int32'),
        (dict(mask=P, ldm=3), 'mask rows too short'),                      # ceil(100 / 32) = 4 words
    ]
    for kw, pattern in cases:
        rc = call(**kw)
        msg = lib.mgcn_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert msg.startswith('score_candidates') and re.search(pattern, msg), (kw, msg)
    assert call(batch=0) == 0                      # nothing to do: returns before any launch
    assert call(n_cand=0) == 0
    assert call(n=0) == 0
    assert call(mask=P, ldm=4, batch=0) == 0


def test_score_candidates_python_surface_needs_a_gpu(pkg):
    nat = pkg._native
    x, ent, bias = torch.zeros(2, 8), torch.zeros(5, 8), torch.zeros(5)
    cand = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(nat.NativeError, match='GPU'):
        nat.score_candidates(x, ent, bias, cand)
    with pytest.raises(nat.NativeError, match='cand'):
        nat.score_candidates(x, ent, bias, cand[:1])
    with pytest.raises(nat.NativeError, match='out'):
        nat.score_candidates(x, ent, bias, cand, out=torch.zeros(2, 4))


# ---------------------------------------------------------------------------------------------------------------------
# the count rule of MGCN.rank_candidates

def loop_counts(scores, cand, obj, target):
    out = torch.zeros((len(obj), 3), dtype=torch.int64)
    for b in range(len(obj)):
        for s, c in zip(scores[b].tolist(), cand[b].tolist()):
            if s == float('-inf') or c == int(obj[b]):
                continue
            t = float(target[b])
            out[b, 0] += s > t
            out[b, 1] += s == t and c < int(obj[b])
            out[b, 2] += s == t
    return out


def test_candidate_count_rule_against_a_loop(pkg):
    ninf = float('-inf')
    #            above  tie<obj tie>obj  dup of tie<obj  target  below  padding  filtered  above-dup
    cand = torch.tensor([[9, 3, 12, 3, 7, 5, -1, 4, 9],
                         [7, 7, 7, 1, 2, 3, 4, 5, 6],            # the target three times: never counted
                         [0, 1, 2, 3, 4, 5, 6, 8, 9],            # target not in the list
                         [-1, -1, -1, -1, -1, -1, -1, -1, -1]])  # nothing but padding
    scores = torch.tensor([[0.9, 0.5, 0.5, 0.5, 0.5, 0.1, ninf, ninf, 0.9],
                           [0.25, 0.25, 0.25, 0.25, 0.75, 0.125, 0.25, ninf, 1.0],
                           [0.5, 0.5, 1.0, 0.0, 0.5, 0.25, 0.75, 0.5, ninf],
                           [ninf] * 9])
    obj = torch.tensor([7, 7, 7, 7])
    target = torch.tensor([0.5, 0.25, 0.5, 0.5])
    got = pkg.model.candidate_counts(scores, cand, obj, target)
    want = loop_counts(scores, cand, obj, target)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    # the hand count of the first rows: gt = two occurrences of 9; ties = 3, 12, 3 (7 itself is skipped); lower = 3 twice
    assert got.tolist() == [[2, 2, 3], [2, 2, 2], [2, 3, 4], [0, 0, 0]]
    # seeded rows with many exact ties
    g = torch.Generator().manual_seed(5)
    cand = torch.randint(-1, 12, (16, 40), generator=g)
    scores = torch.randint(0, 4, (16, 40), generator=g).float() / 4
    scores[cand < 0] = ninf
    scores[torch.rand(16, 40, generator=g) < 0.1] = ninf
    obj = torch.randint(0, 12, (16,), generator=g)
    target = torch.randint(0, 4, (16,), generator=g).float() / 4
    assert torch.equal(pkg.model.candidate_counts(scores, cand, obj, target), loop_counts(scores, cand, obj, target))


# ---------------------------------------------------------------------------------------------------------------------
# gloo rehearsal of dist.sharded_score_candidates

class TorchCandidateKernels(object):
    """Same interface as kgc-gcn_amd._native for filter_mask / score_candidates (test stand-in, CPU; the mask is a dense bool
    block here)."""
    calls = 0

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

    @classmethod
    def score_candidates(cls, x, ent, bias, cand, mask=None, ent_row0=0, out=None):
        """The rule of mgcn_score_candidates: only ids in [ent_row0, ent_row0 + n) are written, everything else keeps the
        block's -inf. One fixed-order sum per element, so a row's score does not depend on the shard it is read from."""
        cls.calls += 1
        n = ent.size(0)
        if out is None:
            out = torch.full(cand.shape, float('-inf'))
        o = cand - ent_row0
        mine = (o >= 0) & (o < n)
        rows = ent[o.clamp(0, max(n - 1, 0))] if n else torch.zeros(cand.shape + (x.size(1),))
        acc = x[:, None, 0] * rows[:, :, 0]
        for j in range(1, x.size(1)):
            acc = acc + x[:, None, j] * rows[:, :, j]
        s = torch.sigmoid(acc + (bias[o.clamp(0, max(n - 1, 0))] if n else 0.0))
        if mask is not None and n:
            s = torch.where(mask.gather(1, o.clamp(0, n - 1)), torch.full_like(s, float('-inf')), s)
        out[mine] = s[mine]
        return out


def _problem(seed=0, B=5, K=23, N=101, O=8, world=2):
    g = torch.Generator().manual_seed(seed)
    x = [torch.randn(B, O, generator=g) for _ in range(world)]
    ent, bias = torch.randn(N, O, generator=g) * 0.5, torch.randn(N, generator=g) * 0.1
    cand = [torch.randint(0, N, (B, K), generator=g) for _ in range(world)]
    sub = [torch.randint(0, N, (B,), generator=g) for _ in range(world)]
    rel = [torch.randint(0, 4, (B,), generator=g) for _ in range(world)]
    known = {}
    for r in range(world):
        cand[r][0, 5:9] = -1                                    # padding
        cand[r][1, 0], cand[r][1, 1] = N, N + 1000               # ids no shard owns
        cand[r][2, 3] = cand[r][2, 4]                            # a duplicate
        for b in range(B):
            known.setdefault((int(sub[r][b]), int(rel[r][b])), set()).update(int(v) for v in cand[r][b, 10:14] if v >= 0)
    return x, ent, bias, cand, sub, rel, known


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    pkg = load_pkg()
    x, ent, bias, cand, sub, rel, known = _problem(world=world)
    filt = pkg.dist.FilterIndex.from_known(known, 4)
    b = pkg.dist.shard_bounds(ent.size(0), world)
    out = []
    for f in (filt, None):
        s = pkg.dist.sharded_score_candidates(x[rank], filt.query_keys(sub[rank], rel[rank]), cand[rank], ent[b[rank]:b[rank + 1]],
                                              bias[b[rank]:b[rank + 1]], b[rank], filt=f, kernels=TorchCandidateKernels)
        out.append(s.numpy().copy())
    q.put((rank, out))      # arrays travel by value: a tensor's shared-memory handle dies with this process
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])   # 3: uneven entity shards (101 rows: 34 + 34 + 33)
def test_sharded_score_candidates_equals_unsharded_gloo(world):
    port = 29500 + (os.getpid() + 13 * world + 977) % 2000
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
    x, ent, bias, cand, sub, rel, known = _problem(world=world)
    filt = pkg.dist.FilterIndex.from_known(known, 4)
    ninf = float('-inf')
    for r in range(world):
        for j, f in enumerate((filt, None)):
            want = pkg.dist.sharded_score_candidates(x[r], filt.query_keys(sub[r], rel[r]), cand[r], ent, bias, 0, filt=f,
                                                     kernels=TorchCandidateKernels)
            g = torch.from_numpy(got[r][j])
            assert g.shape == cand[r].shape and torch.equal(g, want), (r, f is None)
            assert (g[0, 5:9] == ninf).all() and (g[1, :2] == ninf).all()          # padding and unowned ids
            assert g[2, 3] == g[2, 4]                                                # each occurrence of a duplicate
            if f is not None:
                assert (g[:, 10:14] == ninf).all()                                   # the known tails of every query
            else:
                inside = (cand[r] >= 0) & (cand[r] < ent.size(0))
                assert (g[inside] > 0).all() and (g[~inside] == ninf).all()
