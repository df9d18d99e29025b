"""Float64 restatement of the training trajectories of tests/golden/traj_syn_a_{C,D,E,F}.npz: traj_ref's eight
steps on syn_a with what traj_ref leaves out -- counter-based dropout at all five sites, a second layer, edge dropout with
own-triple removal, and the two list losses on counter-drawn lists, uniform and weighted -- and switches for the deliberate
mistakes such a trajectory must catch.

  C  one layer, dropout p = 0.3 at every site (dropout_seed 7), full-table BCE
  D  C with two layers; the second layer's step-0 state is in the fixture (sd0_*)
  E  C's dropout, edge_drop = 0.2 with edge_drop_queries, list BCE on K = 16 uniform lists (draw_seed 11)
  F  C's dropout, list softmax on weighted lists (one hub entity), logq on; run_split = 16 on the GPU routes

Every random choice is an exact integer function of (seed, step, site, row, column): the masks come from dropout_ref, the kept
edges and their float32 norms from edge_drop_ref, the lists and labels from cand_draw_ref / cand_alias_ref, the alias table from
cand_alias_ref.build. Nothing random is restated here. The dropout step and the draw step of training step s are s - 1; an
eval forward draws nothing and advances nothing. Layer masks have entity ids as rows (sites 4 li + {0 in, 1 out, 2 gcn_drop}),
the trunk's masks the batch row (sites 0x1000 over [B, flat_sz] and 0x1001 over [B, O]); hidden dropout sits before bn2; the
scorer reads the all_ent that gcn_drop has been through; the edge norms stay float32 values (oracle.compute_norm's on the full
graph, edge_drop_ref.edge_norms' on a step's kept list: both norms of a kept edge are re-derived from the kept undirected list).
The list BCE is the mean over all B K positions with hot / cold smoothed by 1 / N; the softmax spreads eps over the list's live
positions, subtracts logq from every logit, the positive's included, and averages over the B queries. With every switch off run()
is traj_ref.run (test_traj_ext_host.py: to 1e-12 relative on A).

The generator tests/golden/gen/make_traj_ext.py runs this module in float64 for the fixtures and in float32 with permuted batch
rows (masks, lists and labels permuted with them) for the twins that give gap_* and bar_* = 16 gap_*.

Mutants (MUTANTS maps each to the trajectories on which the host test asserts that it leaves a bar by 10 x or more):
  masks_swapped            a layer's in mask drawn from the out site and the other way round
  layer2_sites_of_layer1   the second layer draws the first layer's three sites (D only: the others have one layer)
  drop_step_stuck          the dropout step never advances: every step draws step 0's masks and kept edges
  drop_step_eval           the eval after step 4 advances the dropout step: steps 5 .. 8 draw one step ahead
  clean_ent_scored         the scorer reads all_ent before gcn_drop (the trunk's rows stay the dropped ones)
  feature_mask_per_channel one keep bit per (row, filter) spread over the filter's map, in place of one per element
  hidden_after_bn2         relu(drop(bn2(z))) in place of relu(bn2(drop(z)))
  no_rescale_gcn           the last layer's gcn_drop keeps without the factor 1 / (1 - p). (The site is chosen by arithmetic: a
                           training-mode BatchNorm follows the in / out, feature and hidden sites and divides most of a constant
                           factor out again; the scorer reads gcn_drop's output as it is.)
  edges_directed           the 2E directed edges are dropped independently (bit d of a [2E, 1] mask), E only
  full_graph_norms         a kept edge keeps the norm of the full graph, E only
  own_triple_one_way       own-triple removal drops the query's direction and keeps the reverse edge, E only
  bce_over_b               the list BCE divided by B in place of B K, E only
  bce_smooth_eps_k         the list BCE smoothed with eps / K in place of 1 / N, E only
  ce_positive_no_logq      the softmax corrects the negatives' logits alone, F only
  ce_logq_added            z + logq in place of z - logq, F only
  draw_step_stuck          the draw step never advances: every step draws step 0's stream
NOT_SHOWN: ce_mean_over_positive (the softmax's mean over the queries that have a positive) is the unmutated trajectory on these
batches, because every query of A's batches has a known tail in the train index and column 0 of its list names one: both
divisors are B at every step. The host test asserts that equality instead."""
import glob
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mgcn_oracle as O

from . import cand_alias_ref as CA
from . import cand_draw_ref as CD
from . import dropout_ref as D
from . import edge_drop_ref as ER
from . import traj_ref as T

TAGS = ('C', 'D', 'E', 'F')
OFF = dict(layers=1, p=0.0, dropout_seed=0, edge_drop=0.0, edge_drop_queries=False, loss='table', num_neg=0, draw_seed=0,
           weighted=False, run_split=0)
CONFIG = {
    'C': dict(OFF, p=0.3, dropout_seed=7),
    'D': dict(OFF, p=0.3, dropout_seed=7, layers=2),
    'E': dict(OFF, p=0.3, dropout_seed=7, edge_drop=0.2, edge_drop_queries=True, loss='bce', num_neg=15, draw_seed=11),
    'F': dict(OFF, p=0.3, dropout_seed=7, loss='softmax', num_neg=15, draw_seed=11, weighted=True, run_split=16),
}
HUB, HUB_WEIGHT = 17, 12          # F: entity 17 has 12 times the weight of every other entity
LAYER2_SEED, LAYER2_TABLE_SCALE = 20, 5.0
GAP_CAP = 1e-3                    # x lr: A's cap, asserted by the generator of every held tensor's twin gap
# F only. conv2.bn0.bias adds one constant to every input of conv_e, so every output channel moves by a constant, which the
# training-mode bn1 subtracts again: its gradient is mathematically zero, and what Adam steps on is weight_decay x the parameter
# plus the gradient's rounding noise. The list softmax's gradients are ten times the BCE's (norms 7 .. 23), the noise with them,
# and the float32 twins part by 1.3e-3 lr there (1.2e-3 .. 2e-3 on every seed, hub weight and max_norm tried). As B's three such
# biases, it is held to 2 x the sum of lr (traj_ref.exempt_cap) in F. Nothing else is exempt: the buffers that read it
# (conv2.bn1.running_mean among them) stay below the cap and are held to their bars.
EXEMPT = {'C': (), 'D': (), 'E': (), 'F': ('conv2.bn0.bias',)}
MUTANTS = {'masks_swapped': ('C', 'D'), 'layer2_sites_of_layer1': ('D',), 'drop_step_stuck': ('C', 'E'), 'drop_step_eval': ('C', 'F'),
           'clean_ent_scored': ('C', 'D', 'E'), 'feature_mask_per_channel': ('C',), 'hidden_after_bn2': ('C',),
           'no_rescale_gcn': ('C', 'D'), 'edges_directed': ('E',), 'full_graph_norms': ('E',), 'own_triple_one_way': ('E',),
           'bce_over_b': ('E',), 'bce_smooth_eps_k': ('E',), 'ce_positive_no_logq': ('F',), 'ce_logq_added': ('F',),
           'draw_step_stuck': ('E', 'F')}
NOT_SHOWN = ('ce_mean_over_positive',)

_fixtures = {}


def fixture_paths(tag):
    """traj_syn_a_<tag>.npz and its parts traj_syn_a_<tag>.1.npz, ... (every file stays under make_golden's PART_BYTES)."""
    first = os.path.join(T.GOLDEN, 'traj_syn_a_%s.npz' % tag)
    return [first] + sorted(glob.glob(os.path.join(T.GOLDEN, 'traj_syn_a_%s.*.npz' % tag)))


def fixture(tag):
    """The arrays of a trajectory's files as one dict (loaded once, never modified)."""
    if tag not in _fixtures:
        arrays = {}
        for path in fixture_paths(tag):
            with np.load(path) as z:
                arrays.update((k, z[k]) for k in z.files)
        _fixtures[tag] = arrays
    return _fixtures[tag]


def config_of(fx):
    """The configuration a fixture records (its cfg_* entries) as CONFIG's dict."""
    cfg = {}
    for k, v in OFF.items():
        a = fx['cfg_' + k]
        cfg[k] = str(a) if isinstance(v, str) else type(v)(a)
    return cfg


# ------------------------------------------------------------------------------------------------- the integer inputs
def layer_prefixes(layers):
    """[(parameter prefix, per-edge table name)] of the layers, the model's names."""
    return [('conv1.', 'edge_embeddings')] + [('conv1_extra.%d.' % i, 'edge_embeddings_extra.%d' % i) for i in range(layers - 1)]


def layer2_state(g):
    """The step-0 state of D's second layer (24 -> 24) under a fixed generator seed: oracle.init_layer_state, a per-edge table of
    the golden tables' scale, and the batch counter. float32 / int64, as a checkpoint holds them."""
    gen = torch.Generator().manual_seed(LAYER2_SEED)
    dim, rows = int(g.hp['gcn_out_dim']), g['dl_edge_index'].shape[1]
    sd = O.init_layer_state('conv1_extra.0.', dim, dim, gen)
    sd['conv1_extra.0.ent_bn.num_batches_tracked'] = torch.zeros((), dtype=torch.int64)
    bound = LAYER2_TABLE_SCALE * math.sqrt(6.0 / (rows + dim))
    sd['edge_embeddings_extra.0'] = (torch.rand((rows, dim), generator=gen) * 2 - 1) * bound
    return sd


def start_state(fx, g, cfg):
    """The state every route starts from: syn_a's golden state, and for two layers the fixture's sd0_* entries."""
    sd = dict(g.state_dict())
    if cfg['layers'] > 1:
        sd.update((k[4:], torch.from_numpy(np.ascontiguousarray(v))) for k, v in fx.items() if k.startswith('sd0_'))
        assert len(sd) > len(g.state_dict())
    return sd


def train_index(g):
    """(keys, ptr, tails, num_rel_ids) of the train split as dist.FilterIndex.from_known lays them out: keys s * 2R + r ascending,
    the tails of a run ascending."""
    r2 = 2 * int(g['dl_num_relation'])
    items = sorted((s * r2 + r, sorted(ts)) for (s, r), ts in T.label_lists(g).items())
    ptr = [0]
    for _, ts in items:
        ptr.append(ptr[-1] + len(ts))
    return (torch.tensor([k for k, _ in items], dtype=torch.int64), torch.tensor(ptr, dtype=torch.int64),
            torch.tensor([t for _, ts in items for t in ts], dtype=torch.int32), r2)


def alias_weights(n):
    w = [1] * n
    w[HUB] = HUB_WEIGHT
    return w


def logq_of(table):
    """sampling.NegativeSampler.logq from the table in Python integers: float32(log(max(cnt, 1) / 2^32)) [N]."""
    return torch.tensor([math.log(max(c, 1) / float(CA.TWO32)) for c in CA.counts(table)], dtype=torch.float64).to(torch.float32)


def norm_table(length):
    """T[d] = d^-1/2 as the feeder forms it in float32 (tests/test_edge_drop_host.py pins mgcn_edge_drop_table_host to it)."""
    t = np.zeros(length, dtype=np.float32)
    t[1:] = (np.float32(1.0) / np.sqrt(np.arange(1, length, dtype=np.float32))).astype(np.float32)
    return t


def _directed_norms(N, ei, kept2, table):
    """edge_drop_ref.edge_norms for a kept set given per DIRECTED edge (the mutants' only): degree by source within a half."""
    E = ei.shape[1] // 2
    out = np.zeros(2 * E, dtype=np.float32)
    for h in range(2):
        deg = [0] * N
        for d in range(h * E, (h + 1) * E):
            if kept2[d]:
                deg[int(ei[0, d])] += 1
        for d in range(h * E, (h + 1) * E):
            if kept2[d]:
                out[d] = np.float32(table[deg[int(ei[0, d])]]) * np.float32(table[deg[int(ei[1, d])]])
    return out


def drop_step_of(step, mutant=None):
    if mutant == 'drop_step_stuck':
        return 0
    return step - 1 + (1 if mutant == 'drop_step_eval' and step > 4 else 0)


def step_inputs(cfg, g, q, step, mutant=None, table=None):
    """Everything drawn for training step `step` (1-based) on the queries q [B, 2], as CPU tensors: the keep masks (bool) of the
    layers `in<li>`, `out<li>`, `gcn<li>` [N, O] and of the trunk `feat` [B, flat_sz], `hidden` [B, O]; with edge switches on
    `kept` [E] bool, `forced` [E] uint8 and `norms` [2E] float32; with a list loss `cand` [B, K] int64 and `label` [B, K] uint8."""
    hp = g.hp
    N, dim, B = int(g['dl_num_entity']), int(hp['gcn_out_dim']), q.size(0)
    flat = (2 * hp['k_w'] - hp['kernel_size'] + 1) * (hp['k_h'] - hp['kernel_size'] + 1) * hp['num_filter']
    seed, dstep, p = cfg['dropout_seed'], drop_step_of(step, mutant), cfg['p']
    out = {}
    if p > 0:
        thr = D.threshold(p)

        def keep(site, rows, cols):
            return torch.from_numpy(D.mask(D.key(seed, dstep, site), rows, cols, 0, thr).astype(bool))
        for li in range(cfg['layers']):
            at = 0 if mutant == 'layer2_sites_of_layer1' else li
            w_in, w_out = (1, 0) if mutant == 'masks_swapped' else (0, 1)
            out['in%d' % li] = keep(D.layer_site(at, w_in), N, dim)
            out['out%d' % li] = keep(D.layer_site(at, w_out), N, dim)
            out['gcn%d' % li] = keep(D.layer_site(at, 2), N, dim)
        out['feat'] = keep(D.SITE_FEATURE, B, flat)
        out['hidden'] = keep(D.SITE_HIDDEN, B, dim)
        if mutant == 'feature_mask_per_channel':
            per = flat // hp['num_filter']
            out['feat'] = out['feat'][:, ::per].repeat_interleave(per, dim=1)
    if cfg['edge_drop'] > 0 or cfg['edge_drop_queries']:
        ei, et = g.t('dl_edge_index'), g.t('dl_edge_attr')[0]
        E, R = ei.size(1) // 2, int(g['dl_num_relation'])
        tab = norm_table(E + 2)
        qkeys = [s * 2 * R + r for s, r in q.tolist()]
        forced = ER.flags(ei, et, R, qkeys) if cfg['edge_drop_queries'] else np.zeros(E, dtype=np.uint8)
        kept = ER.kept_edges(seed, dstep, cfg['edge_drop'], E, forced)
        out['forced'], out['kept'] = torch.from_numpy(forced), torch.from_numpy(kept)
        if mutant == 'edges_directed':
            bits = D.mask(D.key(seed, dstep, ER.SITE), 2 * E, 1, 0, D.threshold(cfg['edge_drop']))[:, 0].astype(bool)
            norms = _directed_norms(N, ei.numpy(), bits & ~np.concatenate((forced, forced)).astype(bool), tab)
        elif mutant == 'own_triple_one_way':
            want = set(qkeys)
            named = np.array([k in want for k in ER.edge_keys(ei, et, R)])
            norms = _directed_norms(N, ei.numpy(), np.concatenate((ER.keep_bits(seed, dstep, cfg['edge_drop'], E),) * 2) & ~named, tab)
        elif mutant == 'full_graph_norms':
            norms = ER.edge_norms(N, ei, np.ones(E, dtype=bool), tab) * np.concatenate((kept, kept))
        else:
            norms = ER.edge_norms(N, ei, kept, tab)
        out['norms'] = torch.from_numpy(norms.astype(np.float32))
    if cfg['loss'] != 'table':
        keys, ptr, tails, r2 = train_index(g)
        qkey = q[:, 0] * r2 + q[:, 1]
        k = CD.key(cfg['draw_seed'], 0 if mutant == 'draw_step_stuck' else step - 1)
        K = 1 + cfg['num_neg']
        if cfg['weighted']:
            out['cand'], out['label'] = CA.draw(qkey, keys, ptr, tails, N, K, k, table)
        else:
            out['cand'], out['label'] = CD.draw(qkey, keys, ptr, tails, N, K, k)
    return out


ROW_KEYS = ('feat', 'hidden', 'cand', 'label')       # the inputs whose rows are batch rows: a twin permutes them with the batch


# ------------------------------------------------------------------------------------------------- the model, any float dtype
def _drop(x, keep, p, rescale=True):
    return x * keep.to(x.dtype) * (1.0 / (1.0 - p) if rescale else 1.0)


def forward(sd, hp, cfg, src, rel, edge_index, edge_attr, training, inp=None, mutant=None):
    """(x [B, O], ent [N, O]): the trunk's output for the queries and the entity rows the scorer reads. `inp`: step_inputs' dict in training mode with dropout, edge or list switches on; an eval forward takes none."""
    inp = inp if training and inp is not None else {}
    p = cfg['p'] if 'feat' in inp else 0.0
    edge_type = edge_attr[0]
    E, N = edge_type.size(0) // 2, sd['entity_embedding'].size(0)
    in_idx, out_idx = edge_index[:, :E], edge_index[:, E:]
    if 'norms' in inp:
        n_in, n_out = inp['norms'][:E], inp['norms'][E:]
    else:
        n_in, n_out = O.compute_norm(in_idx, N), O.compute_norm(out_idx, N)
    loop_idx = torch.stack([torch.arange(N), torch.arange(N)])
    x, rels_in = sd['entity_embedding'], sd['relation_embedding']
    layers = layer_prefixes(cfg['layers'])
    clean = None
    for li, (pre, table) in enumerate(layers):
        ee = sd[table].index_select(0, edge_attr[1])
        rels = torch.cat([rels_in, sd[pre + 'loop_rel']], dim=0)
        loop_type = torch.full((N,), rels.size(0) - 1, dtype=torch.long)
        in_res = O._propagate(x, in_idx, edge_type[:E], n_in, ee[:E], rels, sd[pre + 'in_weight'])
        out_res = O._propagate(x, out_idx, edge_type[E:], n_out, ee[E:], rels, sd[pre + 'out_weight'])
        loop_res = O._propagate(x, loop_idx, loop_type, None, sd[pre + 'loop_edge'].expand(N, -1), rels, sd[pre + 'loop_weight'])
        if p > 0:
            in_res, out_res = _drop(in_res, inp['in%d' % li], p), _drop(out_res, inp['out%d' % li], p)
        out = (in_res + out_res + loop_res) / 3
        if sd.get(pre + 'bias') is not None:
            out = out + sd[pre + 'bias']
        clean = torch.tanh(T._bn(out, sd, pre + 'ent_bn', training, mutant))
        x = clean
        if p > 0:
            x = _drop(clean, inp['gcn%d' % li], p, rescale=not (mutant == 'no_rescale_gcn' and li == len(layers) - 1))
        rels_in = torch.matmul(rels, sd[pre + 'rels_weight'])[:-1]
    all_ent, all_rel = x, rels_in
    dim = hp['gcn_out_dim']
    stack = torch.cat([all_ent.index_select(0, src).view(-1, 1, dim), all_rel.index_select(0, rel).view(-1, 1, dim)], dim=1)
    stack = torch.transpose(stack, 2, 1).reshape(-1, 1, 2 * hp['k_w'], hp['k_h'])
    z = T._bn(stack, sd, 'conv2.bn0', training, mutant)
    z = F.conv2d(z, sd['conv2.conv_e.weight'], sd.get('conv2.conv_e.bias'))
    z = F.relu(T._bn(z, sd, 'conv2.bn1', training, mutant))
    z = z.reshape(z.size(0), -1)
    if p > 0:
        z = _drop(z, inp['feat'], p)
    z = F.linear(z, sd['conv2.fc.weight'], sd['conv2.fc.bias'])
    if p > 0 and mutant != 'hidden_after_bn2':
        z = _drop(z, inp['hidden'], p)
    z = T._bn(z, sd, 'conv2.bn2', training, mutant)
    if p > 0 and mutant == 'hidden_after_bn2':
        z = _drop(z, inp['hidden'], p)
    return F.relu(z), (clean if mutant == 'clean_ent_scored' else all_ent)


def smoothed_targets(lbl_smooth, num_entities):
    """(hot, cold) = (1 - eps) y + 1 / N for y = 1, 0 in float32, as the dataset forms its rows (data_loader.py:41-43)."""
    y = np.array([1.0, 0.0], dtype=np.float32)
    if lbl_smooth != 0.0:
        y = (1.0 - lbl_smooth) * y + (1.0 / int(num_entities))
    return float(y[0]), float(y[1])


def list_logits(x, ent, bias, cand):
    n = ent.size(0)
    live = (cand >= 0) & (cand < n)
    row = torch.where(live, cand, torch.zeros_like(cand))
    return (ent[row] * x[:, None, :]).sum(2) + bias[row], live, row


def list_bce(x, ent, bias, cand, label, lbl_smooth, mutant=None):
    """Mean over ALL B K positions of the BCE of the list's logits against hot / cold; a dead position adds nothing and counts."""
    z, live, _ = list_logits(x, ent, bias, cand)
    B, K = cand.shape
    hot, cold = smoothed_targets(lbl_smooth, ent.size(0))
    if mutant == 'bce_smooth_eps_k':
        hot, cold = (1.0 - lbl_smooth) + lbl_smooth / K, lbl_smooth / K
    y = torch.where(label.bool(), torch.tensor(hot, dtype=z.dtype), torch.tensor(cold, dtype=z.dtype))
    terms = F.binary_cross_entropy_with_logits(z, y, reduction='none')
    return torch.where(live, terms, torch.zeros_like(terms)).sum() / (B if mutant == 'bce_over_b' else B * K)


def list_ce(x, ent, bias, cand, label, lbl_smooth, logq, mutant=None):
    """Softmax cross-entropy over each list (cand_ce_ref.ref_list_ce's loss under autograd): logits z - logq[id] at every live
    position, targets (1 - eps) / n_pos on the list's known tails plus eps / n_live on every live position, rows without a
    positive add nothing, the mean runs over the B queries."""
    z, live, row = list_logits(x, ent, bias, cand)
    pos = label.bool() & live
    if logq is not None:
        corr = logq.to(z.dtype)[row]
        if mutant == 'ce_positive_no_logq':
            corr = torch.where(pos, torch.zeros_like(corr), corr)
        z = z + corr if mutant == 'ce_logq_added' else z - corr
    zl = torch.where(live, z, torch.full_like(z, float('-inf')))
    lp = zl - torch.logsumexp(zl, 1, keepdim=True)
    n_pos, n_live = pos.sum(1, keepdim=True), live.sum(1, keepdim=True)
    q = (1.0 - lbl_smooth) * pos.to(z.dtype) / n_pos.clamp(min=1) + lbl_smooth / n_live.clamp(min=1).to(z.dtype)
    act = live & (n_pos > 0)
    count = int((n_pos > 0).sum()) if mutant == 'ce_mean_over_positive' else cand.size(0)
    return -torch.where(act, q * lp, torch.zeros_like(lp)).sum() / count


def adam_update(p, m, v, g, coef, t, lr, betas, eps, weight_decay):
    """traj_ref.adam_update in p's own dtype (a float32 twin keeps every operand in float32, as torch.optim.Adam does)."""
    b1, b2 = betas
    gc = coef * g.to(p.dtype)
    if weight_decay != 0:
        gc = gc + weight_decay * p
    m += (gc - m) * (1 - b1)
    v.mul_(b2).add_((1 - b2) * gc * gc)
    step_size, bc2_sqrt = lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
    p -= step_size * m / (v.sqrt() / bc2_sqrt + eps)


def run(fx, g, cfg, mutant=None, sd0=None, dtype=torch.float64, perm_seed=None, table=None, logq=None):
    """The trajectory of configuration `cfg` over the batches and optimiser settings of `fx` (a fixture, or the dict the
    generator starts from: lr, weight_decay, max_norm, betas, eps, lbl_smooth, lr_step, lr_after, snaps, eval_steps, q_*,
    eval_triple) on the conftest.Golden case `g`, from the state sd0 (default start_state). dtype / perm_seed: a rounding twin in
    that dtype with every batch's rows permuted (the same mathematics). `table` / `logq`: the alias table (a list of ints) and
    the float32 correction of a weighted configuration. Returns dict(loss, norm, snaps, evals, inputs [8 step_inputs dicts in
    the fixture's row order])."""
    assert mutant is None or mutant in MUTANTS or mutant in NOT_SHOWN
    hp = g.hp
    edge_index, edge_attr = g.t('dl_edge_index'), g.t('dl_edge_attr')
    N = int(g['dl_num_entity'])
    lists = T.label_lists(g)
    sd0 = start_state(fx, g, cfg) if sd0 is None else sd0
    sd = {k: (v.to(dtype, copy=True) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    params = [k for k in sd if T.is_parameter(k)]
    m = {k: torch.zeros_like(sd[k]) for k in params}
    v = {k: torch.zeros_like(sd[k]) for k in params}
    lr, wd, max_norm = float(fx['lr']), float(fx['weight_decay']), float(fx['max_norm'])
    betas, eps, smooth = (float(fx['beta1']), float(fx['beta2'])), float(fx['eps']), float(fx['lbl_smooth'])
    ev = torch.from_numpy(np.asarray(fx['eval_triple']))
    gen = None if perm_seed is None else torch.Generator().manual_seed(perm_seed)
    out = dict(loss=[], norm=[], snaps={}, evals={}, inputs=[])
    for step, q in enumerate(T.batches(fx), 1):
        inp = step_inputs(cfg, g, q, step, mutant, table)
        out['inputs'].append(inp)
        y = T.label_rows(q, lists, N, smooth) if cfg['loss'] == 'table' else None
        if gen is not None:
            perm = torch.randperm(q.size(0), generator=gen)
            q, y = q[perm], (None if y is None else y[perm])
            inp = {k: (x[perm] if k in ROW_KEYS else x) for k, x in inp.items()}
        leaf = dict(sd)
        for k in params:
            leaf[k] = sd[k].detach().clone().requires_grad_(True)
        x, ent = forward(leaf, hp, cfg, q[:, 0], q[:, 1], edge_index, edge_attr, True, inp, mutant)
        if cfg['loss'] == 'table':
            loss = F.binary_cross_entropy(O.score_all(x, ent, leaf['conv2.bias']), y.to(dtype))
        elif cfg['loss'] == 'bce':
            loss = list_bce(x, ent, leaf['conv2.bias'], inp['cand'], inp['label'], smooth, mutant)
        else:
            loss = list_ce(x, ent, leaf['conv2.bias'], inp['cand'], inp['label'], smooth, logq, mutant)
        grads = dict(zip(params, torch.autograd.grad(loss, [leaf[k] for k in params])))
        norm = math.sqrt(sum(float((grads[k].double() ** 2).sum()) for k in params))
        coef = min(max_norm / (norm + 1e-6), 1.0)
        for k in params:
            adam_update(sd[k], m[k], v[k], grads[k], coef, step, lr, betas, eps, wd)
        out['loss'].append(float(loss.detach()))
        out['norm'].append(norm)
        if step in fx['snaps']:
            out['snaps'][step] = {k: t.clone() for k, t in sd.items()}
        if step == int(fx['lr_step']):
            lr = float(fx['lr_after'])
        if step in fx['eval_steps']:
            with torch.no_grad():
                x, ent = forward(sd, hp, cfg, ev[:, 0], ev[:, 1], edge_index, edge_attr, False)
                out['evals'][step] = O.score_all(x, ent, sd['conv2.bias'])
    return out


def run_fixture(tag, g, mutant=None):
    """run() of a committed fixture with its own configuration, table and logq."""
    fx = fixture(tag)
    cfg = config_of(fx)
    table = [int(t) for t in fx['alias_table']] if cfg['weighted'] else None
    logq = torch.from_numpy(fx['logq']) if cfg['weighted'] else None
    return run(fx, g, cfg, mutant, table=table, logq=logq)
