"""Entity-sharded scoring and ranking across the GPUs of one node: one process per GPU,
torch.distributed ("nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU rehearsal tests).

Every rank keeps rows [row0, row0 + n_local) of the encoder output (its shard of the entity table), the matching
slice of the decoder bias and a replica of the (small) filter index. Per step each rank brings its own block of B
queries; the exchange is
    all-gather   x [B, O], obj [B], key [B]          (query embeddings, 100 KB per rank: latency-bound)
    all-reduce   target [W*B] f32  (sum; exactly one rank — the owner of obj — contributes a non-zero, so exact)
    all-reduce   counts [W*B, 3] int64 (sum; integers, so sharded ranks are bit-identical to 1-GPU ranks)
and the three local kernels (target, filter bits, score+filter+count) run on the shard. There is no collective
in the aggregation itself when every rank holds the whole graph (FB15k-237: 12 MB of encoder output).
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _native
from .autograd import _AggregateFn, _LayerTrainFn
from .model import _drawn_dropout, counter_dropout, list_loss_stage, query_rows, refuse_list_step, refuse_table_loss, step_csr, table_bce_stage, table_ce_stage


def shard_bounds(n, world):
    """Contiguous row ranges of equal length ceil(n / world) (the last ones shorter or empty): rank r owns
    [b[r], b[r+1]). Equal chunks let a layer output be exchanged with one all-gather."""
    chunk = (n + world - 1) // world
    return [min(r * chunk, n) for r in range(world + 1)]


class FilterIndex(object):
    """Known (subject, relation) -> tails as a sorted key array + CSR (the loader's sr2o over train+valid+test,
    data_loader.py:80-96), for building the evaluation filter on the device instead of dense [B, N] label rows."""

    def __init__(self, keys, ptr, tails, num_rel_ids):
        self.keys, self.ptr, self.tails, self.num_rel_ids = keys, ptr, tails, int(num_rel_ids)

    @classmethod
    def from_known(cls, known, num_rel_ids):
        items = sorted(((s * num_rel_ids + r), sorted(ts)) for (s, r), ts in known.items())
        keys = torch.tensor([k for k, _ in items], dtype=torch.int64)
        lens = torch.tensor([len(t) for _, t in items], dtype=torch.int64)
        ptr = torch.zeros(len(items) + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(lens, 0)
        tails = torch.tensor([t for _, ts in items for t in ts], dtype=torch.int32)
        return cls(keys, ptr, tails, num_rel_ids)

    def to(self, device):
        self.keys, self.ptr, self.tails = self.keys.to(device), self.ptr.to(device), self.tails.to(device)
        return self

    def query_keys(self, sub, rel):
        return sub.to(torch.int64) * self.num_rel_ids + rel.to(torch.int64)


_INTO_TENSOR = {}      # (backend, device type) -> the probe's answer
_PROBED = set()        # (group name, its global ranks, device type) whose members have run the probe (a name and a member list,
                       # not the object: holding a group would keep it from being destroyed with its process group)


def _into_tensor_ok(group, like):
    """Whether the group's backend has all_gather_into_tensor — decided by a one-element probe that EVERY process group runs
    once per device type, at its first exchange (all its members reach that point together), never by catching an error of a
    real collective: a rank whose collective fails for its own reasons (an RCCL error, a size mismatch) must raise, not
    quietly switch to another collective than its peers are in. Per group, not per backend: members of a sub-group that probed
    first would otherwise skip the probe that the other ranks run on a larger group, and the ranks would be in different
    collectives."""
    group = dist.group.WORLD if group is None else group
    key = (dist.get_backend(group), like.device.type)
    ident = (getattr(group, 'group_name', ''), tuple(dist.get_process_group_ranks(group)), key[1])
    if ident not in _PROBED:
        ok = hasattr(dist, 'all_gather_into_tensor')
        if ok:
            world = dist.get_world_size(group)
            try:
                dist.all_gather_into_tensor(like.new_zeros(world), like.new_zeros(1), group=group)
            except (RuntimeError, NotImplementedError):   # a capability of the backend: the same answer on every rank
                ok = False
        _INTO_TENSOR[key] = ok
        _PROBED.add(ident)
    return _INTO_TENSOR[key]


def _gather_into(out, t, group):
    """out [world * n, ...] <- every rank's t [n, ...], in rank order: ONE collective writing straight into `out`
    (all_gather_into_tensor; the list form costs a staging copy per rank on RCCL — 20.5 GB per layer at BASELINE
    configs[4]). Backends without it take the list form over views of `out`. Every rank passes the same n; n = 0 is no
    collective at all (nothing to exchange, on any rank). Errors of the collective propagate."""
    t = t.contiguous()
    if t.size(0) == 0:
        return out
    if _into_tensor_ok(group, t):
        dist.all_gather_into_tensor(out, t, group=group)
    else:
        dist.all_gather(list(out.chunk(out.size(0) // t.size(0), dim=0)), t, group=group)
    return out


def _gather(t, group, world):
    return _gather_into(t.new_empty((world * t.size(0),) + tuple(t.shape[1:])), t, group)


def sharded_rank_counts(x, qkey, obj, ent_shard, bias_shard, row0, filt, group=None, kernels=_native):
    """Filtered-rank counts of this rank's B queries against the WHOLE entity table, which is sharded by rows.
    x [B, O] query embeddings (ConvE trunk output), qkey [B] filter keys, obj [B] target entity (global id).
    Returns (counts [B, 3] int64 = gt / ties_lower / ties, target [B] f32). All ranks must pass the same B."""
    world = dist.get_world_size(group) if (group is not None or dist.is_initialized()) else 1
    rank = dist.get_rank(group) if world > 1 else 0
    B = x.size(0)
    if world > 1:
        x_all, key_all, obj_all = _gather(x, group, world), _gather(qkey, group, world), _gather(obj, group, world)
    else:
        x_all, key_all, obj_all = x.contiguous(), qkey, obj
    n_local = ent_shard.size(0)
    target = torch.zeros(x_all.size(0), dtype=torch.float32, device=x.device)
    kernels.score_target(x_all, ent_shard, bias_shard, obj_all, ent_row0=row0, out=target)
    if world > 1:
        dist.all_reduce(target, op=dist.ReduceOp.SUM, group=group)
    mask = kernels.filter_mask(key_all, filt.keys, filt.ptr, filt.tails, n_local, ent_row0=row0)
    counts = kernels.score_rank(x_all, ent_shard, bias_shard, obj_all, target, mask=mask, ent_row0=row0)
    if world > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    return counts[rank * B:(rank + 1) * B], target[rank * B:(rank + 1) * B]


def _topk_all(x, qkey, ent_shard, bias_shard, row0, k, filt, group, kernels):
    """sharded_topk for every rank's queries: (scores [W*B, k], ids [W*B, k]) in rank order, the same on every rank."""
    world = dist.get_world_size(group) if (group is not None or dist.is_initialized()) else 1
    if world > 1:
        x_all = _gather(x, group, world)
        key_all = _gather(qkey, group, world) if filt is not None else None
    else:
        x_all, key_all = x.contiguous(), qkey
    mask = kernels.filter_mask(key_all, filt.keys, filt.ptr, filt.tails, ent_shard.size(0), ent_row0=row0) \
        if filt is not None else None
    scores, ids = kernels.score_topk(x_all, ent_shard, bias_shard, k, mask=mask, ent_row0=row0)
    if world == 1:
        return scores, ids
    total = x_all.size(0)
    # every rank's [W*B, k] lists -> [W*B, W*k]: query b's candidates from every shard side by side, then one merge
    s_all, i_all = _gather(scores, group, world), _gather(ids, group, world)
    s_all = s_all.view(world, total, k).transpose(0, 1).reshape(total, world * k)
    i_all = i_all.view(world, total, k).transpose(0, 1).reshape(total, world * k)
    return kernels.topk_merge(s_all, i_all, k)


def sharded_topk(x, qkey, ent_shard, bias_shard, row0, k, filt=None, group=None, kernels=_native):
    """Filtered top-k of this rank's B queries against the WHOLE entity table, which is sharded by rows (the counterpart
    of sharded_rank_counts): x [B, O] query embeddings (ConvE trunk output), qkey [B] filter keys (filt.query_keys;
    ignored without `filt`), ent_shard / bias_shard the rows [row0, row0 + n_local). The exchange: one all-gather of x
    and the keys, the local top-k over the shard with global ids, one all-gather of the [W*B, k] candidate lists, and
    a merge. Returns (scores [B, k], ids [B, k]) equal to the unsharded result (the order is total). All ranks pass the
    same B and k, and all or none pass `filt`."""
    world = dist.get_world_size(group) if (group is not None or dist.is_initialized()) else 1
    rank = dist.get_rank(group) if world > 1 else 0
    B = x.size(0)
    scores, ids = _topk_all(x, qkey, ent_shard, bias_shard, row0, k, filt, group, kernels)
    return scores[rank * B:(rank + 1) * B], ids[rank * B:(rank + 1) * B]


def sharded_score_candidates(x, qkey, cand, ent_shard, bias_shard, row0, filt=None, group=None, kernels=_native):
    """Scores of this rank's per-query candidate lists against the WHOLE entity table, which is sharded by rows (the
    counterpart of sharded_topk for _native.score_candidates): x [B, O] query embeddings, qkey [B] filter keys (ignored
    without `filt`), cand [B, K] int64 global ids, ent_shard / bias_shard the rows [row0, row0 + n_local). The exchange: one
    all-gather of x, of the keys (only with `filt`) and of cand, the local launch into a -inf block (a rank writes only the
    ids of its shard), one all_reduce(MAX): at most one rank writes an element and a score is above -inf, so the result is
    exact in any order. Returns this rank's [B, K] rows, equal to the unsharded result (-inf at padding, at ids no shard
    owns and at filtered candidates). All ranks pass the same B and K, and all or none pass `filt`."""
    world = dist.get_world_size(group) if (group is not None or dist.is_initialized()) else 1
    rank = dist.get_rank(group) if world > 1 else 0
    B = x.size(0)
    if world > 1:
        x_all, cand_all = _gather(x, group, world), _gather(cand, group, world)
        key_all = _gather(qkey, group, world) if filt is not None else None
    else:
        x_all, key_all, cand_all = x.contiguous(), qkey, cand
    mask = kernels.filter_mask(key_all, filt.keys, filt.ptr, filt.tails, ent_shard.size(0), ent_row0=row0) \
        if filt is not None else None
    scores = kernels.score_candidates(x_all, ent_shard, bias_shard, cand_all, mask=mask, ent_row0=row0)
    if world > 1 and scores.numel() > 0:
        dist.all_reduce(scores, op=dist.ReduceOp.MAX, group=group)
    return scores[rank * B:(rank + 1) * B]


def xavier_rows(edge_ids, num_rows, dim, seed, device, chunk=1 << 16):
    """Rows `edge_ids` (reference edge ids, int64) of a [num_rows, dim] xavier-uniform table (utils.get_param's
    initialiser, utils.py:113-118) that is DEFINED chunk-wise: rows [c * chunk, (c + 1) * chunk) come from a generator
    seeded with (seed, c). Any rank can therefore materialise exactly the rows it owns, in any order, with one chunk
    of scratch — the whole table (410 GB at configs[4]) never exists anywhere."""
    bound = (6.0 / (num_rows + dim)) ** 0.5
    edge_ids = edge_ids.to(device)
    out = torch.empty((edge_ids.numel(), dim), dtype=torch.float32, device=device)
    which = torch.div(edge_ids, chunk, rounding_mode='floor')
    for c in torch.unique(which).tolist():
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed) * 1000003 + int(c))
        block = (torch.rand((chunk, dim), generator=gen, device=device) * 2 - 1) * bound
        sel = (which == c).nonzero(as_tuple=True)[0]
        out[sel] = block.index_select(0, edge_ids.index_select(0, sel) - c * chunk)
    return out


@torch.no_grad()
def shard_model_tables(model, csr, n0, n1, source):
    """Fill a model built with params.edge_table_rows = sum(csr.shard_slot_counts(n0, n1)) with the rows of destinations
    [n0, n1): in-half slots, out-half slots, hub slots (slot order). `source(layer, edge_ids) -> rows [len, D]` returns
    table rows by reference edge id — e.g. lambda l, ids: xavier_rows(ids, 2E, D_l, seed + l, device), or a slice of
    a state dict that is streamed from disk. Nothing of size [2E, D] is allocated. A model with bf16 tables
    (params.edge_table_dtype) rounds f32 rows to nearest even on the copy into the shard."""
    (i0, i1), (o0, o1), (h0, h1) = csr._shard_bounds(n0, n1)
    ids = torch.cat([csr.perm[i0:i1], csr.perm[o0:o1], csr.perm[h0:h1]])
    tables = [model.edge_embeddings] + list(model.edge_embeddings_extra)
    for li, t in enumerate(tables):
        if t.size(0) != ids.numel():
            raise _native.NativeError('shard_model_tables: table %d has %d rows, destinations [%d, %d) need %d'
                                      % (li, t.size(0), n0, n1, ids.numel()))
        t.data.copy_(source(li, ids).to(t.device))
    model._edge_shard = (csr, int(n0), int(n1))
    model._slot_csr = None
    model._enc_cache = None
    return model


def encode_layer_rows(layer, csr, x, rel, table_shard, n0, n1, ee_sub, out=None):
    """Rows [n0, n1) of one layer's eval output (model.py:82-106) from this rank's table shard: the fused launch where
    the shape allows, else the aggregation + dense launches on the range. `out` [n1 - n0, O] optional."""
    O, bn = layer.out_channels, layer.ent_bn
    if out is None:
        out = torch.empty((n1 - n0, O), dtype=torch.float32, device=x.device)
    wcat, wpack = layer.derived_weights()
    x, rel = x.contiguous(), rel.contiguous()
    fused = wpack is not None
    if fused:
        try:
            _native.layer_fwd_fused(csr, x, rel, layer.loop_rel.reshape(-1), table_shard, True, layer.loop_edge.reshape(-1),
                                    wpack, O, layer.bias, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out,
                                    node_range=(n0, n1), ee_sub=ee_sub)
        except _native.FusedUnsupported:      # e.g. a misaligned operand: the two launches on the range, as MGCNConv.forward
            fused = False
    if not fused and n1 > n0:
        # the aggregate of the range only ([n1 - n0, 3D]); the kernel writes rows by global node id, hence the offset view
        agg = torch.empty((n1 - n0, 3 * layer.in_channels), dtype=torch.float32, device=x.device)
        _native.aggregate_fwd(csr, x, rel, table_shard, True, layer.loop_edge.reshape(-1), agg, loop_rel=layer.loop_rel.reshape(-1),
                              node_range=(n0, n1), ee_sub=ee_sub, out_row0=n0)
        _native.dense_bn_tanh_fwd(agg, wcat, layer.bias, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, out)
    return out


@torch.no_grad()
def encode_sharded(model, graph, group=None):
    """Destination-partitioned encoder: rank r computes rows [b_r, b_{r+1}) of every layer's output,
    reading only ITS shard of the slot-ordered per-edge tables (1/W of their bytes — the table is what does not fit one
    GPU at 10^8 triples); every destination's sum is formed wholly on one rank, so the rows are bit-identical to the
    single-GPU ones. Sources are arbitrary, so each layer output is all-gathered (RCCL) before the next layer / the
    scorer reads it. Returns (all_ent [N, O], all_rel [2R, O]) complete on every rank.
    A model built with params.edge_table_rows (dist.shard_model_tables) holds nothing but its shard; a model with
    whole tables is sliced once per table version (a convenience for small graphs: no memory is saved then)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    model.eval()
    edge_type, edge_ids = graph.edge_attr
    layers = [model.conv1] + list(model.conv1_extra)
    tables = [model.edge_embeddings] + list(model.edge_embeddings_extra)
    csr = graph.csr(model.relation_embedding.size(0) + 1)
    N = csr.num_nodes
    b = csr.balanced_bounds(world)          # equal work (slots + nodes) per rank, not equal node counts (degree skew)
    n0, n1, chunk = b[rank], b[rank + 1], max(b[r + 1] - b[r] for r in range(world))
    if model._edge_shard is not None:
        ent_identity, edge_identity = model._graph_facts(graph)
        if not (ent_identity and edge_identity):
            # shard_model_tables filled the shard by csr.perm = edge-list POSITIONS: only right when edge k has id k
            raise _native.NativeError('encode_sharded: a model that holds a table shard needs a graph whose entity and edge ids '
                                      'are the identity (data_loader.py:113,147-149 builds them so)')
        if model._edge_shard[0] is not csr or model._edge_shard[1:] != (n0, n1):
            raise _native.NativeError('encode_sharded: the model holds the table shard of destinations %s, this rank owns (%d, %d)'
                                      % (model._edge_shard[1:], n0, n1))
        shards = [t.detach() for t in tables]
    else:
        ent_identity, edge_identity = model._graph_facts(graph)
        if world == 1 or not (ent_identity and edge_identity):
            return model.encode(graph)                          # nothing to partition / ids that need gathers: replicated
        model._use_slot_order(csr)
        cache = model.__dict__.setdefault('_ee_shard_cache', {})
        shards = []
        for li, table in enumerate(tables):
            key = (li, n0, n1, id(csr))
            hit = cache.get(key)
            if hit is None or hit[0] != table._version or hit[1].device != table.device:
                hit = (table._version, csr.edge_table_shard(table.detach(), n0, n1))
                cache[key] = hit
            shards.append(hit[1])
    x, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
    ee_sub = csr.shard_ee_sub(n0, n1)
    for layer, shard in zip(layers, shards):
        local = torch.zeros((chunk, layer.out_channels), dtype=torch.float32, device=x.device)
        encode_layer_rows(layer, csr, x, rel, shard, n0, n1, ee_sub, out=local[:n1 - n0])
        if world > 1:
            full = torch.empty((world * chunk, layer.out_channels), dtype=torch.float32, device=x.device)
            _gather_into(full, local, group)                                    # equal (padded) chunks, gathered in place
            if all(b[r + 1] - b[r] == chunk for r in range(world - 1)):
                x = full[:N]
            else:                                                              # drop each rank's padding rows
                x = torch.cat([full[r * chunk:r * chunk + b[r + 1] - b[r]] for r in range(world)], dim=0)
        else:
            x = local[:N]
        rel = _native.matmul(rel.contiguous(), layer.rels_weight)
    return x, rel


@torch.no_grad()
def evaluate_sharded(model, graph, queries, filt, batch_size=None, group=None, trunk_chunk=2048, shard_encoder=False,
                     parts=None):
    """Filtered MR / MRR / hits@{1,3,10} of `queries` ([Q, 3] int64: subject, relation id, object; both directions
    already expanded, as the loader's *_tail + *_head lists) with the entity table sharded over the group.

    Rank r owns the contiguous query range [c_r, c_{r+1}) (padded to a common length so every rank runs the same
    collectives). The queries go to the device once, the ConvE trunk runs over them in chunks of `trunk_chunk`, and the
    exchange happens ONCE for the whole evaluation: one all-gather of the query embeddings / keys / objects, one
    all-reduce of the target scores, one all-reduce of the integer counts. The score + filter + count kernel takes ALL
    queries in one launch whenever their filter bits fit 512 MB (one launch of 6 268 queries costs 0.8 ms, 49 launches
    of 128 cost 1.6 ms; the result does not depend on the split); `batch_size` forces blocks of that many queries (the
    reference's 128, main.py:117, for like-for-like timing). `shard_encoder=True` also partitions the encoder by
    destination (encode_sharded). `parts`: a dict that receives the wall-clock seconds of the encoder, the ConvE trunk
    (stock torch, out of scope), the exchange and the HIP kernels — it adds a device synchronisation per part, so the
    evaluation's total is NOT to be timed with it."""
    import time
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    model.eval()
    clock = [None]

    def lap(name):
        if parts is not None:
            torch.cuda.synchronize() if torch.cuda.is_available() else None
            now = time.perf_counter()
            if clock[0] is not None and name is not None:
                parts[name] = parts.get(name, 0.0) + now - clock[0]
            clock[0] = now
    lap(None)
    # encoder: replicated (default; 12-33 MB of output at FB15k-237 / WN18RR) or destination-partitioned
    all_ent, all_rel = encode_sharded(model, graph, group) if shard_encoder else model.encode(graph)
    lap('encoder_s')
    N = all_ent.size(0)
    b = shard_bounds(N, world)
    ent_shard = all_ent[b[rank]:b[rank + 1]].contiguous()
    bias_shard = model.conv2.bias[b[rank]:b[rank + 1]].contiguous()
    dev = all_ent.device
    Q = queries.size(0)
    per = (Q + world - 1) // world
    lo, hi = min(rank * per, Q), min((rank + 1) * per, Q)
    real = hi - lo
    q = torch.zeros((per, 3), dtype=torch.int64, device=dev)   # padding rows are harmless queries, dropped below
    q[:real] = queries[lo:hi].to(dev)
    sub, rel, obj = q[:, 0], q[:, 1], q[:, 2].contiguous()
    x = torch.cat([model.conv2.trunk_indexed(all_ent, sub[i:i + trunk_chunk], all_rel, rel[i:i + trunk_chunk])
                   for i in range(0, per, trunk_chunk)], dim=0) if per > 0 else all_ent.new_zeros((0, all_ent.size(1)))
    keys = filt.query_keys(sub, rel)
    lap('trunk_s')
    if world > 1:       # every rank's (padded) queries to every rank, once
        x_all, key_all, obj_all = _gather(x, group, world), _gather(keys, group, world), _gather(obj, group, world)
    else:
        x_all, key_all, obj_all = x.contiguous(), keys, obj
    lap('exchange_s')
    total, n_local = x_all.size(0), ent_shard.size(0)
    target = torch.zeros(total, dtype=torch.float32, device=dev)
    counts = torch.zeros((total, 3), dtype=torch.int64, device=dev)
    if total > 0 and n_local > 0:
        _native.score_target(x_all, ent_shard, bias_shard, obj_all, ent_row0=b[rank], out=target)
    lap('kernels_s')
    if world > 1:
        dist.all_reduce(target, op=dist.ReduceOp.SUM, group=group)   # exactly one rank holds each target entity
    lap('exchange_s')
    words = (n_local + 31) // 32
    fit = max(1, (512 << 20) // max(words * 4, 1))             # queries whose filter bits fit the budget at once
    step = min(total, fit) if not batch_size else int(batch_size)
    mask_all = _native.filter_mask(key_all, filt.keys, filt.ptr, filt.tails, n_local, ent_row0=b[rank]) \
        if (total <= fit and total > 0 and n_local > 0) else None
    for i in range(0, total, max(step, 1)):
        if n_local == 0:
            break
        mask = mask_all[i:i + step] if mask_all is not None else _native.filter_mask(
            key_all[i:i + step], filt.keys, filt.ptr, filt.tails, n_local, ent_row0=b[rank])
        _native.score_rank(x_all[i:i + step], ent_shard, bias_shard, obj_all[i:i + step], target[i:i + step], mask=mask,
                           ent_row0=b[rank], counts=counts[i:i + step])
    lap('kernels_s')
    if world > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    lap('exchange_s')
    mine = counts[rank * per:(rank + 1) * per]
    ranks = (1 + mine[:, 0] + mine[:, 1]).double()[:real]
    sums = torch.zeros(13, dtype=torch.float64, device=dev)    # count, sum rank, sum 1/rank, hits@1..10
    sums[0] = real
    if real > 0:
        sums[1] = ranks.sum()
        sums[2] = (1.0 / ranks).sum()
        sums[3:] = (ranks.view(-1, 1) <= torch.arange(1, 11, device=dev, dtype=torch.float64)).sum(0)
    if world > 1:
        dist.all_reduce(sums, group=group)
    sums = sums.tolist()
    lap('metrics_s')
    if dev.type == 'cuda':
        _native.check_fused_status(dev)         # (the host has just waited for the results: the fused launches' status word)
    count = sums[0]
    res = {'count': count, 'mr': sums[1] / count, 'mrr': sums[2] / count}
    for k in (1, 3, 10):
        res['hits@%d' % k] = sums[2 + k] / count
    return res


@torch.no_grad()
def predict_topk_sharded(model, graph, queries, k, filt=None, group=None, trunk_chunk=2048, shard_encoder=False):
    """Filtered top-k tails of `queries` ([Q, 2] int64: subject, relation id; heads through the inverse relation r + R)
    with the entity table sharded over the group, batched as evaluate_sharded: rank r takes the query range
    [c_r, c_{r+1}) padded to a common length, the ConvE trunk runs over it in chunks of `trunk_chunk`, and the exchange
    happens once (sharded_topk). `filt`: a FilterIndex on the device, or None for unfiltered lists. Returns
    (ids [Q, k] int64, scores [Q, k] f32) for ALL queries on every rank, equal to model.predict_topk at world size 1."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    model.eval()
    all_ent, all_rel = encode_sharded(model, graph, group) if shard_encoder else model.encode(graph)
    N = all_ent.size(0)
    b = shard_bounds(N, world)
    ent_shard = all_ent[b[rank]:b[rank + 1]].contiguous()
    bias_shard = model.conv2.bias[b[rank]:b[rank + 1]].contiguous()
    dev = all_ent.device
    Q = queries.size(0)
    per = (Q + world - 1) // world
    lo, hi = min(rank * per, Q), min((rank + 1) * per, Q)
    q = torch.zeros((per, 2), dtype=torch.int64, device=dev)   # padding rows are harmless queries, dropped below
    q[:hi - lo] = queries[lo:hi, :2].to(dev)
    sub, rel = q[:, 0], q[:, 1]
    x = torch.cat([model.conv2.trunk_indexed(all_ent, sub[i:i + trunk_chunk], all_rel, rel[i:i + trunk_chunk])
                   for i in range(0, per, trunk_chunk)], dim=0) if per > 0 else all_ent.new_zeros((0, all_ent.size(1)))
    keys = filt.query_keys(sub, rel) if filt is not None else sub
    if per == 0:
        return (torch.empty((0, k), dtype=torch.int64, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev))
    scores, ids = _topk_all(x, keys, ent_shard, bias_shard, b[rank], k, filt, group, _native)
    return ids[:Q], scores[:Q]


# ------------------------------------------------------------------------------------------------
# Training step of the destination partition: rank r owns destinations [n0, n1) = balanced_bounds(W)[r:r + 2], their
# shard of every per-edge table and the matching entity rows of the scorer; everything else is replicated.
# ------------------------------------------------------------------------------------------------
class _Exchange(object):
    """The collectives of one sharded step: bounds, this rank's rows, and the group (None = one rank, no collective)."""

    def __init__(self, bounds, rank, group, world):
        self.b, self.rank, self.group, self.world = bounds, rank, group, world
        self.n0, self.n1 = bounds[rank], bounds[rank + 1]
        self.rows = [bounds[r + 1] - bounds[r] for r in range(world)]
        self.chunk = max(self.rows)
        self.total = bounds[-1]

    def gather_rows(self, y):
        """[N, O]: every rank's rows in rank order (equal padded chunks, one all-gather)."""
        if self.world == 1:
            return y
        pad = y.new_zeros((self.chunk, y.size(1)))
        pad[:y.size(0)] = y
        full = y.new_empty((self.world * self.chunk, y.size(1)))
        _gather_into(full, pad, self.group)
        if all(n == self.chunk for n in self.rows[:-1]):
            return full[:self.total]
        return torch.cat([full[r * self.chunk:r * self.chunk + self.rows[r]] for r in range(self.world)], dim=0)

    def gather_blocks(self, part):
        """Every rank's BN block partials ([blocks_r, O] or [2, blocks_r, O]) concatenated along the blocks in rank order: the
        order in which the stages fold them."""
        if self.world == 1:
            return part
        nb = [_native.bn_blocks(n) for n in self.rows]
        width = max(nb)
        stacked = part.dim() == 3
        p = part.permute(1, 0, 2) if stacked else part                     # blocks first
        pad = p.new_zeros((width,) + tuple(p.shape[1:]))
        pad[:p.size(0)] = p
        full = pad.new_empty((self.world * width,) + tuple(pad.shape[1:]))
        _gather_into(full, pad, self.group)
        out = torch.cat([full[r * width:r * width + nb[r]] for r in range(self.world) if nb[r] > 0], dim=0)
        return (out.permute(1, 0, 2) if stacked else out).contiguous()

    def gather_stats(self, stat):
        """[world, B, 4]: every rank's [B, 4] row statistics of the list softmax in rank order (one all-gather)."""
        return _gather(stat, self.group, self.world).view(self.world, stat.size(0), 4)

    def all_reduce(self, t):
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t


class _GatherRowsFn(torch.autograd.Function):
    """Layer output rows -> [N, O] on every rank. Backward: the rank's rows of the incoming gradient, all-reduced first when it
    holds partials (`reduce`: a layer the next layer reads, whose gx is a partial [N, O] on every rank). The incoming gradient
    goes through .contiguous(): a contiguous one is passed through (and, with `reduce` on more than one rank, all-reduced in
    place), every other layout is copied."""

    @staticmethod
    def forward(ctx, y, ex, reduce):
        ctx.ex, ctx.reduce = ex, reduce
        return ex.gather_rows(y.contiguous())

    @staticmethod
    def backward(ctx, g):
        ex = ctx.ex
        g = g.contiguous()
        if ctx.reduce:
            # in place, without the [N, O] copy a clone costs (20 GB at configs[4]): `g` is the gradient autograd accumulated for
            # the gathered output, and this node is its only reader — the output has no other grad_fn consumer of it and no hook
            ex.all_reduce(g)
        return g[ex.n0:ex.n1].contiguous(), None, None


class _AllReduceGradFn(torch.autograd.Function):
    """Identity; the gradient is summed over the ranks (d x_trunk = sum_r G_r^T ent_r: each rank scores its own entities).
    The incoming gradient is always copied, whatever its layout: the result is a contiguous tensor with a storage of its own."""

    @staticmethod
    def forward(ctx, x, ex):
        ctx.ex = ex
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        # cloned ([B, O]: small): `g` may be the very tensor the scorer's backward returned for other uses
        return ctx.ex.all_reduce(g.contiguous().clone()), None


class _RankZeroGradFn(torch.autograd.Function):
    """Identity; only rank 0 passes the gradient on: a gradient that every rank computes in full (a replicated computation on
    complete inputs) joins partial ones, and the sum over the ranks must count it once. The incoming gradient is passed through
    as it is on rank 0, in any layout; no kernel reads it."""

    @staticmethod
    def forward(ctx, x, ex):
        ctx.ex = ex
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.ex.rank == 0 else torch.zeros_like(g)), None


def _trunk(conv2, src_emb, rel_emb, generator):
    """ConvE.trunk with its two dropouts drawn from `generator` (None: torch's default generator, as ConvE.trunk)."""
    if generator is None or not conv2.training:
        return conv2.trunk(src_emb, rel_emb)
    if conv2._hip_trunk_train(src_emb, rel_emb):      # the HIP training trunk draws the same two masks from `generator`
        return conv2._trunk_train(src_emb, rel_emb, generator)
    p = conv2.params
    o = p.gcn_out_dim
    stack = torch.cat([src_emb.view(-1, 1, o), rel_emb.view(-1, 1, o)], dim=1)
    stack = stack.transpose(2, 1).reshape(-1, 1, 2 * p.k_w, p.k_h)
    x = _drawn_dropout(F.relu(conv2.bn1(conv2.conv_e(conv2.bn0(stack)))), conv2.feature_drop.p, generator)
    return conv2._tail(conv2.fc(x.view(-1, conv2.flat_sz)), generator, True)      # (the HIP tail with MGCN_QUERY_TRAIN=hip)


def _agreed_seed(group, device):
    """A fresh random 62-bit seed that every rank of `group` agrees on: rank 0 draws it from its default generator (which
    advances, so every call gives a new seed) and broadcasts it. A collective: every rank calls it at the same point."""
    t = torch.randint(0, 1 << 62, (1,), dtype=torch.int64).to(device)
    dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return int(t.item())


def broadcast_sampler(sampler, group=None, device=None):
    """The sampling.NegativeSampler of rank 0 on every rank of `group`, once, ahead of training: the table is DATA, so no rank
    depends on its own pow; nothing is exchanged per step afterwards. Rank 0 passes its sampler, the others pass
    None (or anything: it is ignored). Two broadcasts, the length and then the table, on `device` (default: rank 0's sampler's
    device there, the current GPU elsewhere); the result lives on that device. A collective. Without a process group: the
    sampler itself."""
    from .sampling import NegativeSampler
    world, rank = _world_rank(group)
    if world == 1:
        return sampler if device is None else sampler.to(device)
    if device is None:
        device = sampler.device if rank == 0 and sampler is not None and sampler.device.type == 'cuda' else torch.device('cuda', torch.cuda.current_device())
    src = dist.get_global_rank(group, 0) if group is not None else 0
    n = torch.tensor([sampler.num_entities if rank == 0 else 0], dtype=torch.int64).to(device)
    dist.broadcast(n, src=src, group=group)
    table = sampler.table.to(device) if rank == 0 else torch.empty(int(n.item()), dtype=torch.int64, device=device)
    dist.broadcast(table, src=src, group=group)
    return NegativeSampler(table)


def _world_rank(group):
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    return world, (dist.get_rank(group) if world > 1 else 0)


def _sharded_setup(model, graph, group, what):
    """(csr, exchange) for this rank, or NativeError for a model / graph the sharded step cannot train."""
    world, rank = _world_rank(group)
    csr = graph.csr(model.relation_embedding.size(0) + 1)
    b = csr.balanced_bounds(world)
    n0, n1 = b[rank], b[rank + 1]
    ent_identity, edge_identity = model._graph_facts(graph)
    if not (ent_identity and edge_identity):
        raise _native.NativeError('%s: the graph\'s entity and edge ids must be the identity (data_loader.py:113,147-149 builds '
                                  'them so): the table shards are laid out by edge position' % what)
    if model._edge_shard is None:
        if world > 1:
            raise _native.NativeError('%s: the model holds whole per-edge tables; at %d ranks fill a model built with '
                                      'params.edge_table_rows through dist.shard_model_tables for destinations [%d, %d)'
                                      % (what, world, n0, n1))
        model._use_slot_order(csr)           # one rank: the whole slot-ordered table is the shard of [0, N)
    elif model._edge_shard[0] is not csr or model._edge_shard[1:] != (n0, n1):
        raise _native.NativeError('%s: the model holds the table shard of destinations %s, this rank owns (%d, %d)'
                                  % (what, model._edge_shard[1:], n0, n1))
    if not csr.mirrored:
        raise _native.NativeError('%s: the edge list is not mirror-symmetric' % what)
    return csr, _Exchange(b, rank, group, world)


def _complete_params(model):
    """Replicated parameters whose gradient every rank computes in full: the ConvE trunk, the encoder's BN affine pair (global
    statistics) and the last layer's relation projection (fed by the trunk alone). All others are partial sums over the ranks."""
    layers = [model.conv1] + list(model.conv1_extra)
    ps = [p for n, p in model.conv2.named_parameters() if n != 'bias']
    for layer in layers:
        ps += [layer.ent_bn.weight, layer.ent_bn.bias]
    ps.append(layers[-1].rels_weight)
    return {id(p) for p in ps}


def _trunk_statistics(model):
    """The ConvE trunk's BN running statistics: every rank updates them from its own (replicated) trunk forward, which MIOpen
    does not promise to reduce in the same order on every rank."""
    return [b for b in model.conv2.buffers() if b.is_floating_point()]


def _bucket_grads(model):
    """Point the .grad of every replicated parameter at a view of ONE zeroed flat buffer before the backward: autograd then
    accumulates into the views in place, and the bucket is reduced without staging a copy of d entity_embedding [N, D]. A tail
    of the buffer carries the trunk's running statistics. Returns (buffer, [(parameter, view)]). The per-edge table shards keep
    their own, local gradients."""
    shard = {id(p) for _, p in model._edge_tables()}
    params = [p for p in model.parameters() if id(p) not in shard and p.requires_grad]
    tail = sum(b.numel() for b in _trunk_statistics(model))
    flat = torch.zeros(sum(p.numel() for p in params) + tail, dtype=torch.float32, device=model.entity_embedding.device)
    views, off = [], 0
    for p in params:
        v = flat[off:off + p.numel()].view_as(p)
        p.grad = v
        views.append((p, v))
        off += p.numel()
    return flat, views


def _reduce_bucket(model, ex, flat, views):
    """One all-reduce of the flat bucket: partial sums from every rank, complete gradients and the trunk's running statistics
    from rank 0 only (each counted once, and every rank ends with the same bits whatever the determinism of the replicated
    computation)."""
    complete = _complete_params(model)
    for p, v in views:
        if p.grad is not v:              # (autograd replaced the view instead of accumulating into it: move the values in)
            v.copy_(p.grad)
            p.grad = v
        if id(p) in complete and ex.rank != 0:
            v.zero_()
    stats = _trunk_statistics(model)
    off = flat.numel() - sum(b.numel() for b in stats)
    if ex.rank == 0 and stats:
        flat[off:] = torch.cat([b.reshape(-1) for b in stats])
    ex.all_reduce(flat)
    for b in stats:
        b.copy_(flat[off:off + b.numel()].view_as(b))
        off += b.numel()


def clip_grad_norm_sharded(model, max_norm, group=None):
    """torch.nn.utils.clip_grad_norm_ over the model's parameters with the GLOBAL norm: the per-parameter norms in parameter
    order (torch._foreach_norm, as torch), the table shards' norms replaced by their norm over all ranks (all-reduced squares),
    then the norm of those norms. With one rank this is clip_grad_norm_'s value bit for bit. Returns the total norm."""
    world, _ = _world_rank(group)
    params = [p for p in model.parameters() if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    norms = list(torch._foreach_norm([p.grad for p in params], 2.0))
    if world > 1:
        shard = {id(p) for _, p in model._edge_tables()}
        idx = [i for i, p in enumerate(params) if id(p) in shard]
        if idx:
            sq = torch.stack([norms[i] for i in idx]) ** 2
            dist.all_reduce(sq, op=dist.ReduceOp.SUM, group=group)
            for j, i in enumerate(idx):
                norms[i] = sq[j].sqrt()
    total = torch.linalg.vector_norm(torch.stack(norms), 2.0)
    torch.nn.utils.clip_grads_with_norm_(params, max_norm, total)
    return total


def _shard_sq_reducer(model, group):
    """`reduce_sq_norms` of optim.ClipAdam.clip_and_step for the destination-partitioned model: the table shards' sums of
    squares become their sums over all ranks (SUM all-reduce), as in clip_grad_norm_sharded; the replicated parameters'
    gradients are already complete on every rank."""
    shard = {id(p) for _, p in model._edge_tables()}

    def reduce(sq, params):
        idx = [i for i, p in enumerate(params) if id(p) in shard]
        if idx:
            part = torch.stack([sq[i] for i in idx])
            dist.all_reduce(part, op=dist.ReduceOp.SUM, group=group)
            for j, i in enumerate(idx):
                sq[i].copy_(part[j])
    return reduce


def train_step_sharded(model, graph, src, rel, index, optimizer, lbl_smooth=0.0, clip=None, group=None, generator=None, loss='bce'):
    """One training step (main.py:59-70: forward, BCE against the train index's targets, backward, clipping, optimizer) of the
    destination-partitioned model: rank r owns destinations [n0, n1) = graph.csr(...).balanced_bounds(W)[r:r + 2], the table
    shards of `dist.shard_model_tables` for that range (a whole-table model only at W = 1) and entity rows [n0, n1) of the
    scorer; `entity_embedding`, `relation_embedding`, the layer weights, BN and ConvE are replicated. Every rank passes the same
    batch (src, rel [B]), `index` = DataLoader.train_index() on the device, and the same optimizer type over model.parameters().
    Data flow: per layer the rank aggregates its destinations, runs the training-mode products and epilogue with
    GLOBAL batch statistics, applies its own dropout masks to its rows and all-gathers the rows; every rank runs the ConvE trunk
    on the whole batch and scores its own entities (global mean); the backward reduces each gradient once — the trunk's input
    gradient and every inner layer output's by all-reduce inside the backward, all replicated parameters in one flat bucket
    after it; the table shards' gradients stay local.

    Dropout. By default (params.dropout = 'torch') the layer masks are each rank's own draws for its rows, and the trunk's masks,
    which must be the same on every rank, come from `generator` (a torch.Generator on the device, seeded identically on every
    rank) or, without one at W > 1, from a per-step generator seeded from a fresh seed the group agrees on; with one rank the
    step then computes what forward_loss + backward + clip_grad_norm_ + step compute bit for bit only at dropout 0.
    With params.dropout = 'counter' (or MGCN_DROPOUT=counter) every keep bit is a pure function of (model.dropout_seed,
    model.dropout_step, site, global row, column): the rank's layer rows and gcn_drop take row0 = n0, every rank
    derives the same trunk keys, so no generator is read and no seed is exchanged (`generator` is ignored), and the masks do not
    depend on the partition. The call uses the current step for all its sites and then increments it, as one training-mode
    MGCN.encode does; every rank must hold the same (dropout_seed, dropout_step). With one rank the step then equals
    forward_loss + backward + clip_grad_norm_ + step bit for bit AT ANY DROPOUT.
    loss = 'softmax': the softmax cross-entropy over the whole table instead (forward_loss(loss='softmax')): each
    rank scores its own rows, the ranks' [B, 4] row statistics make one all-gather and are merged in rank order (_ScoreCEFn with
    the exchange), lbl_smooth is spread over the global table; the ranks' losses and d x add up, d ent and d bias are local.
    Returns the global loss (0-dim tensor, detached)."""
    refuse_table_loss('train_step_sharded', loss)
    ex, ent, xt = _sharded_trunk(model, graph, src, rel, optimizer, group, generator, 'train_step_sharded')
    keys = index.query_keys(src, rel)
    if loss == 'softmax':
        out = table_ce_stage(xt, ent, _own_bias(model, ex), keys, index, lbl_smooth, ex.total, ex.n0, ex)
    else:
        out = table_bce_stage(model, xt, ent, _own_bias(model, ex), keys, index, lbl_smooth, ex.total, ex.n0, ex.world)
    return _sharded_finish(model, ex, out, optimizer, clip, group)


def _own_bias(model, ex):
    """The scorer's bias of this rank's entity rows (one rank: the parameter itself, not a view of all of it)."""
    return model.conv2.bias if ex.world == 1 else model.conv2.bias[ex.n0:ex.n1]


def _sharded_trunk(model, graph, src, rel, optimizer, group, generator, what):
    """What the sharded steps share up to the scorer: the refusals and setup, the gradients zeroed, the partitioned encoder (per
    layer: aggregate, train epilogue, dropout, row gather) and the ConvE trunk of the whole batch, its output behind
    _AllReduceGradFn at W > 1 (every rank's scorer returns a partial d x). Returns (exchange, ent = this rank's rows [n1 - n0, O]
    of the last layer's output, xt = the trunk's output [B, O])."""
    model._refuse_training_ee16(what, training=True)
    csr, ex = _sharded_setup(model, graph, group, what)
    n0, n1, W = ex.n0, ex.n1, ex.world
    model.train()
    optimizer.zero_grad()
    layers = [model.conv1] + list(model.conv1_extra)
    tables = [model.edge_embeddings] + list(model.edge_embeddings_extra)
    for layer in layers:
        bn = layer.ent_bn
        if not (bn.track_running_stats and bn.momentum is not None and bn.affine and
                _native.matmul_tn_supported(layer.in_channels, layer.out_channels)):
            raise _native.NativeError('%s: layer %s is outside the HIP training path' % (what, layer))
    x, rel_e = model.entity_embedding, model.relation_embedding
    drop_ctx = model._begin_dropout_step()       # (seed, step) with the counter-based dropout on, else None
    # this step's graph: every rank rewrites the whole record array, which it holds; csr itself with the switches off
    step = step_csr(model, csr, drop_ctx, (src, rel), what)
    for li, (layer, table) in enumerate(zip(layers, tables)):
        last = li == len(layers) - 1
        bn = layer.ent_bn
        rels = torch.cat([rel_e, layer.loop_rel], dim=0)
        agg = _AggregateFn.apply(x, rels, table, step, (n0, n1))
        x_own = x if (n0, n1) == (0, x.size(0)) else x[n0:n1]
        a_loop = (x_own * rels[-1]) * layer.loop_edge
        keys = None if drop_ctx is None else \
            tuple(_native.dropout_key(drop_ctx[0], drop_ctx[1], _native.dropout_layer_site(li, w)) for w in (0, 1)) + (n0,)
        y = _LayerTrainFn.apply(agg, a_loop, layer.in_weight, layer.out_weight, layer.loop_weight, layer.bias, bn.weight,
                                bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, layer.drop.p, keys, ex)
        with torch.no_grad():
            bn.num_batches_tracked += 1
        rel_e = torch.matmul(_RankZeroGradFn.apply(rels, ex) if (last and W > 1) else rels, layer.rels_weight)[:-1]
        if drop_ctx is not None:
            y = counter_dropout(y, model.params.gcn_drop, drop_ctx[0], drop_ctx[1], _native.dropout_layer_site(li, 2), row0=n0)
        else:
            y = F.dropout(y, p=model.params.gcn_drop, training=True)
        x = _GatherRowsFn.apply(y, ex, not last) if W > 1 else y
    ent = y.contiguous()
    if drop_ctx is not None:
        generator = None         # the trunk finds (seed, step) in conv2._drop_ctx: the same keys on every rank
    elif W > 1 and generator is None and (model.conv2.feature_drop.p > 0 or model.conv2.hidden_drop.p > 0):
        generator = torch.Generator(device=ent.device)
        generator.manual_seed(_agreed_seed(group, ent.device))
    xt = _trunk(model.conv2, query_rows(model, x, src), query_rows(model, rel_e, rel), generator)
    if W > 1:
        xt = _AllReduceGradFn.apply(xt, ex)
    return ex, ent, xt


def _sharded_finish(model, ex, loss, optimizer, clip, group):
    """What the sharded steps share after the scorer: the backward into the flat bucket, its one reduction, clipping and the
    optimizer step, and the ranks' losses added up. Returns the global loss (0-dim tensor, detached)."""
    W = ex.world
    bucket = _bucket_grads(model) if W > 1 else None
    loss.backward()
    if W > 1:
        _reduce_bucket(model, ex, *bucket)
    if hasattr(optimizer, 'clip_and_step'):              # optim.ClipAdam: clip=None is a plain step
        optimizer.clip_and_step(clip, reduce_sq_norms=_shard_sq_reducer(model, group) if W > 1 else None)
    else:
        if clip is not None:
            clip_grad_norm_sharded(model, clip, group)
        optimizer.step()
    loss = loss.detach().clone()
    return ex.all_reduce(loss)


def train_epoch_sharded(model, queries, index, graph, optimizer, params, batch_size, generator=None, group=None, loss='bce'):
    """One epoch of train_step_sharded, as harness.train_device_labels: `queries` [Q, 2] int64 (DataLoader.train_queries()),
    `index` = DataLoader.train_index() on the device, shuffled with `generator` — which must be seeded identically on every rank
    so that every rank takes the same batches. Without one every call draws a new order: at W = 1 from torch's default
    generator (as harness.train_device_labels, which one epoch then equals bit for bit at dropout 0), at W > 1 from a fresh seed
    that rank 0 draws and broadcasts. Clips at params.clip_grad, smooths with params.lbl_smooth. `loss` is train_step_sharded's;
    under 'softmax' the epoch's last batch, whatever its size, takes _ScoreCEFn's second form. Returns the mean of the steps'
    global losses."""
    from .utils import RunningAverage
    refuse_table_loss('train_epoch_sharded', loss)
    world, _ = _world_rank(group)
    dev = model.entity_embedding.device
    if generator is None and world > 1:
        generator = torch.Generator()
        generator.manual_seed(_agreed_seed(group, dev))
    model.train()
    loss_avg = RunningAverage()
    queries = queries.to(dev)
    order = torch.randperm(queries.size(0), generator=generator).to(dev)
    extra = {} if loss == 'bce' else {'loss': loss}           # the default is the call as it was
    for i in range(0, queries.size(0), batch_size):
        q = queries.index_select(0, order[i:i + batch_size])
        step_loss = train_step_sharded(model, graph, q[:, 0], q[:, 1], index, optimizer, lbl_smooth=params.lbl_smooth,
                                  clip=params.clip_grad, group=group, **extra)
        loss_avg.update(step_loss.item())
    return loss_avg()


def train_step_sharded_candidates(model, graph, src, rel, cand, index, optimizer, labels=None, lbl_smooth=0.0, clip=None, group=None,
                                  generator=None, loss='bce', logq=None, run_split=None):
    """train_step_sharded on per-query candidate lists (MGCN.forward_loss_candidates) in place of the
    rank's whole entity shard: everything up to and including the ConvE trunk is train_step_sharded's (same refusals, same
    dropout rules, same collectives), then rank r scores only the list positions whose id lies in its rows [n0, n1). No
    [B, N_local] block, mask or GEMM over the shard exists; the scoring stage costs B K dim on the ranks together.
    cand [B, K] int64 global ids: EVERY RANK PASSES THE SAME BLOCK (the caller's contract; harness.draw_candidates gives it
    without an exchange). `labels` [B, K] uint8 / bool: the global labels of draw_candidates(labels=True), or any block that is
    right at the positions this rank owns; None: looked up on the device for the rank's rows (_native.cand_labels with
    ent_row0 = n0). `index` = DataLoader.train_index() on the device (only read without `labels`).
    The mean runs over all B K positions on every rank (hot / cold smoothed with the GLOBAL entity count): the ranks' losses
    add up (one all-reduce of the scalar), d x is a partial sum reduced once inside the backward, d ent and d bias are the
    rank's rows and complete; the flat bucket, clipping and optimizer calls are train_step_sharded's. With one rank the step
    computes what forward_loss_candidates + backward + clip_grad_norm_ + step compute, bit for bit (at any dropout with
    params.dropout = 'counter'). A rank without entity rows scores nothing and joins every collective.
    loss = 'softmax': the softmax cross-entropy over each list instead (forward_loss_candidates(loss='softmax')):
    a row's maximum, sum and counts span the ranks, so the step makes one more collective, an all-gather of the [B, 4] row
    statistics (_CandCEFn with the exchange); lbl_smooth is spread over the list; the ranks' losses add up as above.
    logq (None: the above, unchanged): f32 [N] over the WHOLE table, sampling.NegativeSampler.logq on the device, softmax only
    (forward_loss_candidates(logq=...)): the rank hands its scoring stage bias[n0:n1] - logq[n0:n1].
    run_split (None: the above, unchanged): forward_loss_candidates(run_split=...), DESIGN §4.16, THE SAME VALUE ON EVERY RANK: a
    run is cut from its own first entry, so a rank's rows keep the bits of the one-rank step with the same run_split.
    Returns the global loss (0-dim tensor, detached)."""
    what = 'train_step_sharded_candidates'
    model._refuse_training_ee16(what, training=True)      # (before the list is looked at: the refusal _sharded_trunk repeats)
    cand = refuse_list_step(what, model, src.numel(), cand, labels, loss, logq, run_split)
    if labels is None and index is None:
        raise _native.NativeError('%s: give index or labels' % what)
    ex, ent, xt = _sharded_trunk(model, graph, src, rel, optimizer, group, generator, what)
    keys = index.query_keys(src, rel) if labels is None else None
    loss = list_loss_stage(xt, ent, _own_bias(model, ex), cand, labels, index, keys, lbl_smooth, loss, logq, ex.total, ex.n0, ex,
                           run_split=run_split)
    return _sharded_finish(model, ex, loss, optimizer, clip, group)


def train_epoch_sharded_candidates(model, queries, index, graph, optimizer, params, batch_size, num_neg, draw_seed, first_step=0,
                                   generator=None, group=None, loss='bce', sampler=None, run_split=None):
    """One epoch of train_step_sharded_candidates on counter-drawn lists, as harness.train_sampled_negatives(draw_seed=...): the
    shuffle of train_epoch_sharded (`generator` seeded identically on every rank, or a seed the group agrees on), the key check
    once, and per step i the lists and global labels of harness.draw_candidates(q, index, N, num_neg, draw_seed, first_step + i,
    labels=True), drawn on every rank with no exchange. Every rank passes the same draw_seed and first_step (the steps done in
    earlier epochs; a checkpoint stores the two). Clips at params.clip_grad, smooths with params.lbl_smooth. Returns the mean of
    the steps' global losses. loss: 'bce' or 'softmax', handed to every step.
    sampler (None: uniform negatives, unchanged): a sampling.NegativeSampler on the device, THE SAME TABLE ON EVERY RANK
    (broadcast_sampler gives it): the negatives follow its table, and the softmax steps take its logq; nothing is exchanged per
    step. run_split (None: unchanged) is handed to every step."""
    from .harness import check_query_keys, draw_candidates
    kind = loss             # (`loss` below is a step's result)
    from .utils import RunningAverage
    world, _ = _world_rank(group)
    dev = model.entity_embedding.device
    if generator is None and world > 1:
        generator = torch.Generator()
        generator.manual_seed(_agreed_seed(group, dev))
    model.train()
    loss_avg = RunningAverage()
    queries = queries.to(dev)
    order = torch.randperm(queries.size(0), generator=generator).to(dev)
    n_ent = model.entity_embedding.size(0)
    check_query_keys(queries, index)      # every query has a key: checked once, not per step
    for k, i in enumerate(range(0, queries.size(0), batch_size)):
        q = queries.index_select(0, order[i:i + batch_size])
        cand, labels = draw_candidates(q, index, n_ent, num_neg, draw_seed, int(first_step) + k, labels=True, sampler=sampler)
        loss = train_step_sharded_candidates(model, graph, q[:, 0], q[:, 1], cand, index, optimizer, labels=labels,
                                             lbl_smooth=params.lbl_smooth, clip=params.clip_grad, group=group, loss=kind,
                                             logq=sampler.logq if sampler is not None and kind == 'softmax' else None,
                                             run_split=run_split)
        loss_avg.update(loss.item())
    return loss_avg()
