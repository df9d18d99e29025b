"""Float64 restatement of the multi-step training trajectories of tests/golden/traj_syn_a_{A,B}.npz, with switches for the
deliberate mistakes a trajectory test must catch.

The fixtures are the reference's own training loop (its model, its dataset's smoothed labels, clip_grad_norm_, Adam with L2
weight decay, StepLR, an evaluation between epochs) run in float64 by tests/golden/gen/make_golden.py (run_trajectory), with
`gap_*` = the worst distance of the reference's float32 rounding twins from that run and bar_* = margin x gap_*. This module
restates one step from the formulas of oracle/mgcn_oracle.py under torch autograd, with BatchNorm written out (so that its
conventions can be bent) and Adam in the update order of tests/adam_ref.py. test_traj_ref_host.py pins the unmutated
restatement to the fixtures at 1/1000 of the bars and shows that every mutant leaves a bar by a factor of ten or more: what the
GPU routes of test_gpu_trajectory.py are held to is then known to separate a wrong convention from rounding.

Mutants (MUTANTS maps each to the trajectories on which the host test asserts that it is caught):
  adamw            decoupled weight decay (p *= 1 - lr wd) instead of L2 (g += wd p)
  wd_in_norm       weight decay added to the gradients before the norm is taken (and so clipped with them)
  no_bc2           v's bias correction dropped
  stale_t          Adam's t not advanced by the step-5 batch (the eager interlude of a captured route)
  lr_ignored       the scheduler's new lr never reaches the update
  biased_var       the biased batch variance written to running_var
  momentum_swapped running = 0.1 running + 0.9 batch
  smooth_eps_n     labels (1 - eps) y + eps / N instead of (1 - eps) y + 1 / N
  no_clip          clipping skipped
  always_clip      max_norm / norm without the min(., 1)
  loss_over_b      loss averaged over B instead of B N
  eval_in_train    the evaluation after step 4 run in training mode (it rewrites the running statistics)
Two of them cannot show on every trajectory, for reasons of arithmetic and not of tolerance. A has weight decay and clips at
every step; B has neither weight decay nor a step-independent coefficient. adamw and wd_in_norm do nothing at weight_decay 0 (B).
loss_over_b multiplies every gradient by N: where every step is clipped (A) the coefficient divides that factor out again
and the state moves by the 1e-6 of clip_grad_norm_'s denominator only, so it is asserted on B, where it turns the steps with
coef = 1 into clipped ones (its loss is N times the fixture's on both). always_clip needs steps with coef = 1: B. no_clip under
weight decay: A."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mgcn_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TRAJECTORIES = ('A', 'B')
SIZES = (16, 16, 16, 16, 5, 16, 16, 16)
MOMENTUM, BN_EPS = 0.1, 1e-5
EXEMPT_B = ('conv2.bn0.bias', 'conv2.conv_e.bias', 'conv2.fc.bias', 'conv2.bn0.weight', 'conv2.bn1.running_mean',
            'conv2.bn1.running_var', 'conv2.bn2.running_mean')
MUTANTS = {'adamw': ('A',), 'wd_in_norm': ('A',), 'no_bc2': ('A', 'B'), 'stale_t': ('A', 'B'), 'lr_ignored': ('A', 'B'),
           'biased_var': ('A', 'B'), 'momentum_swapped': ('A', 'B'), 'smooth_eps_n': ('A', 'B'), 'no_clip': ('A',),
           'always_clip': ('B',), 'loss_over_b': ('B',), 'eval_in_train': ('A', 'B')}
MAX_FILE_BYTES = 1 << 20
GAP_CAP = {'A': 1e-3, 'B': 5e-3}          # x lr: what the generator asserted of every held tensor's twin_gap

_fixtures = {}


def fixture(tag):
    """The arrays of traj_syn_a_<tag>.npz as a dict (loaded once, never modified)."""
    if tag not in _fixtures:
        with np.load(os.path.join(GOLDEN, 'traj_syn_a_%s.npz' % tag)) as z:
            _fixtures[tag] = {k: z[k] for k in z.files}
    return _fixtures[tag]


def fixture_path(tag):
    return os.path.join(GOLDEN, 'traj_syn_a_%s.npz' % tag)


def names(fx):
    return [str(k) for k in fx['names']]


def held(fx):
    """Names of the tensors held to a bar (all but B's seven)."""
    ex = set(str(k) for k in fx['exempt'])
    return [k for k in names(fx) if k not in ex]


def bar_of(fx, name, step):
    return float(fx['bar_sd'][names(fx).index(name), list(fx['snaps']).index(step)])


def exempt_cap(fx, step):
    """2 x the sum of the lr over the steps so far: an Adam step is at most about lr."""
    lrs = [float(fx['lr']) if s <= int(fx['lr_step']) else float(fx['lr_after']) for s in range(1, step + 1)]
    return 2.0 * sum(lrs)


def snapshot(fx, step):
    """The fixture's state dict after `step` as float64 / int64 tensors."""
    pre = 'sd%d_' % step
    return {k[len(pre):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in fx.items() if k.startswith(pre)}


def batches(fx):
    return [torch.from_numpy(fx['q_%d' % i]) for i in range(1, len(SIZES) + 1)]


def label_lists(g):
    """{(src, rel): known tails over train} of a conftest.Golden case."""
    trip, ptr, idx = g['dl_q_train_triple'], g['dl_q_train_label_ptr'], g['dl_q_train_label_idx']
    return {(int(t[0]), int(t[1])): idx[ptr[i]:ptr[i + 1]].tolist() for i, t in enumerate(trip)}


def label_rows(q, lists, num_entity, lbl_smooth, mutant=None):
    """The training dataset's rows of the queries q [B, 2]: float32, as the dataset forms them (oracle.label_row)."""
    rows = []
    for s, r in q.tolist():
        if mutant == 'smooth_eps_n':
            y = O.label_row(lists[(s, r)], num_entity)
            rows.append((1.0 - lbl_smooth) * y + (lbl_smooth / num_entity))
        else:
            rows.append(O.label_row(lists[(s, r)], num_entity, training=True, lbl_smooth=lbl_smooth))
    return torch.stack(rows)


# ------------------------------------------------------------------------------------------------- the model, float64
def _bn(x, sd, name, training, mutant=None):
    """nn.BatchNorm1d / 2d over every dimension but 1: batch statistics (biased variance) in training mode, where the running
    mean and the UNBIASED variance are blended in with momentum 0.1 and the batch counter advances; the running ones in eval."""
    dims = [d for d in range(x.dim()) if d != 1]
    shape = [1, -1] + [1] * (x.dim() - 2)
    if training:
        n = x.numel() // x.size(1)
        mean = x.mean(dims)
        var = ((x - mean.view(shape)) ** 2).mean(dims)
        with torch.no_grad():
            mom = 1.0 - MOMENTUM if mutant == 'momentum_swapped' else MOMENTUM
            stat = var if mutant == 'biased_var' else var * (n / (n - 1.0))
            sd[name + '.running_mean'].mul_(1 - mom).add_(mom * mean)
            sd[name + '.running_var'].mul_(1 - mom).add_(mom * stat)
            sd[name + '.num_batches_tracked'] += 1
    else:
        mean, var = sd[name + '.running_mean'], sd[name + '.running_var']
    y = (x - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS)
    return y * sd[name + '.weight'].view(shape) + sd[name + '.bias'].view(shape)


def forward(sd, hp, src, rel, edge_index, edge_attr, training, mutant=None):
    """Scores [B, N] (oracle.mgcn_forward's sequence at dropout 0, BatchNorm through _bn). The edge norms stay the float32 values
    of oracle.compute_norm, as in the reference run in float64."""
    edge_type = edge_attr[0]
    E, N = edge_type.size(0) // 2, sd['entity_embedding'].size(0)
    x, ee = sd['entity_embedding'], sd['edge_embeddings'].index_select(0, edge_attr[1])
    rels = torch.cat([sd['relation_embedding'], sd['conv1.loop_rel']], dim=0)
    in_idx, out_idx = edge_index[:, :E], edge_index[:, E:]
    loop_idx = torch.stack([torch.arange(N), torch.arange(N)])
    loop_type = torch.full((N,), rels.size(0) - 1, dtype=torch.long)
    in_res = O._propagate(x, in_idx, edge_type[:E], O.compute_norm(in_idx, N), ee[:E], rels, sd['conv1.in_weight'])
    out_res = O._propagate(x, out_idx, edge_type[E:], O.compute_norm(out_idx, N), ee[E:], rels, sd['conv1.out_weight'])
    loop_res = O._propagate(x, loop_idx, loop_type, None, sd['conv1.loop_edge'].expand(N, -1), rels, sd['conv1.loop_weight'])
    out = (in_res + out_res + loop_res) / 3
    if sd.get('conv1.bias') is not None:
        out = out + sd['conv1.bias']
    all_ent = torch.tanh(_bn(out, sd, 'conv1.ent_bn', training, mutant))
    all_rel = torch.matmul(rels, sd['conv1.rels_weight'])[:-1]
    # the trunk (oracle.conve_trunk)
    dim = hp['gcn_out_dim']
    stack = torch.cat([all_ent.index_select(0, src).view(-1, 1, dim), all_rel.index_select(0, rel).view(-1, 1, dim)], dim=1)
    stack = torch.transpose(stack, 2, 1).reshape(-1, 1, 2 * hp['k_w'], hp['k_h'])
    z = _bn(stack, sd, 'conv2.bn0', training, mutant)
    z = F.conv2d(z, sd['conv2.conv_e.weight'], sd.get('conv2.conv_e.bias'))
    z = F.relu(_bn(z, sd, 'conv2.bn1', training, mutant))
    z = F.linear(z.reshape(z.size(0), -1), sd['conv2.fc.weight'], sd['conv2.fc.bias'])
    z = F.relu(_bn(z, sd, 'conv2.bn2', training, mutant))
    return O.score_all(z, all_ent, sd['conv2.bias'])


def is_parameter(name):
    return 'running_' not in name and 'num_batches_tracked' not in name


def adam_update(p, m, v, g, coef, t, lr, betas, eps, weight_decay, bc2=True):
    """One update of one tensor in place, float64: tests/adam_ref.adam_ref's order of operations; bc2=False drops v's correction."""
    b1, b2 = betas
    gc = coef * g.double()
    if weight_decay != 0:
        gc = gc + weight_decay * p
    m += (gc - m) * (1 - b1)
    v.mul_(b2).add_((1 - b2) * gc * gc)
    step_size, bc2_sqrt = lr / (1 - b1 ** t), (math.sqrt(1 - b2 ** t) if bc2 else 1.0)
    p -= step_size * m / (v.sqrt() / bc2_sqrt + eps)


def run(fx, g, mutant=None):
    """The trajectory of fixture `fx` on the conftest.Golden case `g` (syn_a) in float64, with one mutant or none. Returns
    dict(loss [8], norm [8], snaps {step: state dict}, evals {step: scores [16, N]})."""
    assert mutant is None or mutant in MUTANTS
    hp = g.hp
    edge_index, edge_attr = g.t('dl_edge_index'), g.t('dl_edge_attr')
    N = int(g['dl_num_entity'])
    lists = label_lists(g)
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in g.state_dict().items()}
    params = [k for k in sd if is_parameter(k)]
    m = {k: torch.zeros_like(sd[k]) for k in params}
    v = {k: torch.zeros_like(sd[k]) for k in params}
    lr, wd, max_norm = float(fx['lr']), float(fx['weight_decay']), float(fx['max_norm'])
    betas, eps, smooth = (float(fx['beta1']), float(fx['beta2'])), float(fx['eps']), float(fx['lbl_smooth'])
    ev = torch.from_numpy(fx['eval_triple'])
    out = dict(loss=[], norm=[], snaps={}, evals={})
    t = 0
    for step, q in enumerate(batches(fx), 1):
        y = label_rows(q, lists, N, smooth, mutant).double()
        leaf = dict(sd)
        for k in params:
            leaf[k] = sd[k].detach().clone().requires_grad_(True)
        score = forward(leaf, hp, q[:, 0], q[:, 1], edge_index, edge_attr, True, mutant)
        loss = F.binary_cross_entropy(score, y)
        if mutant == 'loss_over_b':
            loss = loss * N
        grads = dict(zip(params, torch.autograd.grad(loss, [leaf[k] for k in params])))
        if mutant == 'wd_in_norm':
            grads = {k: grads[k] + wd * sd[k] for k in params}
        norm = math.sqrt(sum(float((grads[k] ** 2).sum()) for k in params))
        coef = max_norm / (norm + 1e-6)
        if mutant == 'no_clip':
            coef = 1.0
        elif mutant != 'always_clip':
            coef = min(coef, 1.0)
        if not (mutant == 'stale_t' and step == 5):
            t += 1
        for k in params:
            if mutant == 'adamw':
                sd[k].mul_(1 - lr * wd)
            l2 = 0.0 if mutant in ('adamw', 'wd_in_norm') else wd
            adam_update(sd[k], m[k], v[k], grads[k], coef, t, lr, betas, eps, l2, bc2=mutant != 'no_bc2')
        out['loss'].append(float(loss.detach()))
        out['norm'].append(norm)
        if step in fx['snaps']:
            out['snaps'][step] = {k: x.clone() for k, x in sd.items()}
        if step == int(fx['lr_step']) and mutant != 'lr_ignored':
            lr = float(fx['lr_after'])
        if step in fx['eval_steps']:
            with torch.no_grad():
                out['evals'][step] = forward(sd, hp, ev[:, 0], ev[:, 1], edge_index, edge_attr,
                                             mutant == 'eval_in_train' and step == int(fx['lr_step']), mutant)
    return out


def filtered_ranks(scores, fx):
    """1 + the number of unfiltered entities that score above the target, per recorded eval query; scores [16, N] on the CPU."""
    ev = torch.from_numpy(fx['eval_triple'])
    rows = torch.arange(ev.size(0))
    target = scores[rows, ev[:, 2]]
    masked = torch.where(torch.from_numpy(fx['eval_label']).bool(), torch.full_like(scores, -1e7), scores)
    masked[rows, ev[:, 2]] = target
    return 1 + (masked > target[:, None]).sum(1)


def decided(fx, step):
    """Mask of the eval queries whose rank the fixture's scores decide by more than twice the score bar."""
    j = list(fx['eval_steps']).index(step)
    return torch.from_numpy(fx['eval%d_decide' % step]) > 2 * float(fx['bar_eval'][j])


def worst_ratio(got_sd, fx, step, only=None):
    """(ratio, name): the largest |got - fixture| / bar over the held tensors at a snapshot."""
    want = snapshot(fx, step)
    worst = (0.0, None)
    for k in (held(fx) if only is None else only):
        r = float((got_sd[k].double().cpu() - want[k]).abs().max()) / bar_of(fx, k, step)
        if not math.isfinite(r):
            return math.inf, k
        worst = max(worst, (r, k))
    return worst
