"""One eval-mode layer (model.py:82-118 of the reference) in float64, written from the edge list and the layer's parameters
alone, as the yardstick of the fused layer kernels (tests/test_gpu_fused_tiles.py) — CPU torch / numpy, nothing of the
library: no slot layout, no row pointers, no hub tables. The per-edge table is taken in REFERENCE EDGE ORDER.

    layer_f64(...)  -> out, rel_out, B, y     (float64 numpy)
    bar(B)          -> 4 * 2^-24 * B + 2e-7   the numeric contract of include/mgcn_hip.h (2b), its numbers as they stand there

B[n, o] = sum_k |a_k| |w_k| * |gamma_o| / (3 sqrt(var_o + eps)) is the condition of the pre-activation: what one unit roundoff
on every product moves y by (|tanh'| <= 1 carries it to the output). As in tests/test_gpu_round3.py::_layer_f64, which the
header names as the contract's test, |a_k| is the sum of the MAGNITUDES of the messages that make up the aggregate a_k (the
aggregate itself is a rounded f32 sum of them), over the three modes.

layer_f32_slots(...) is the other side of the host test (tests/test_fused_ref_host.py): the same layer evaluated
straightforwardly in f32 — messages summed per destination in slot order, then `@` — with the value-only perturbations that
test applies. It takes the slot order as a permutation of the edges (`perm`: slot -> reference edge) and nothing else of the
layout."""
import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2e-7


def bar(B):
    """include/mgcn_hip.h (2b): |out - exact| <= 4 u B + 2e-7, u = 2^-24."""
    return 4 * U * B + FLOOR


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def layer_f64(p, x, rel, ee, edge_index, edge_type):
    """p: the layer's parameters as arrays — in_weight, out_weight, loop_weight, rels_weight [D, O]; loop_rel, loop_edge [D];
    bias [O] or None; bn_mean, bn_var, bn_gamma, bn_beta [O]; eps. x [N, D], rel [2R, D], ee [2E, D] (reference edge order),
    edge_index [2, 2E], edge_type [2E]. Returns float64 arrays (out [N, O], rel_out [2R, O], B [N, O], y [N, O])."""
    x, rel, ee = _t64(x), _t64(rel), _t64(ee)
    ei = torch.as_tensor(np.asarray(edge_index), dtype=torch.int64)
    et = torch.as_tensor(np.asarray(edge_type), dtype=torch.int64)
    N, D = x.shape
    E = ei.size(1) // 2
    rels = torch.cat([rel, _t64(p['loop_rel']).reshape(1, D)], 0)                # model.py:86
    z = torch.zeros((N, np.asarray(p['in_weight']).shape[1]), dtype=torch.float64)
    B = torch.zeros_like(z)
    for lo, hi, wname in ((0, E, 'in_weight'), (E, 2 * E, 'out_weight')):         # model.py:88-90, 99-100
        row, col = ei[0, lo:hi], ei[1, lo:hi]
        deg = torch.bincount(row, minlength=N).double()                          # compute_norm, model.py:72-80
        inv = deg.pow(-0.5)
        inv[torch.isinf(inv)] = 0
        norm = inv[row] * inv[col]
        msg = x[row] * rels[et[lo:hi]] * ee[lo:hi] * norm[:, None]               # model.py:114-118 (the weight after the sum)
        w = _t64(p[wname])
        z += torch.zeros((N, D), dtype=torch.float64).index_add_(0, col, msg) @ w
        B += torch.zeros((N, D), dtype=torch.float64).index_add_(0, col, msg.abs()) @ w.abs()
    a_loop = x * rels[-1] * _t64(p['loop_edge']).reshape(1, D)                    # model.py:91-94, 101
    w = _t64(p['loop_weight'])
    z = (z + a_loop @ w) / 3                                                      # model.py:103 (eval: no dropout)
    B = B + a_loop.abs() @ w.abs()
    if p.get('bias') is not None:
        z = z + _t64(p['bias'])                                                   # model.py:104-105
    inv = _t64(p['bn_gamma']) / torch.sqrt(_t64(p['bn_var']) + float(p['eps']))  # model.py:106, running statistics
    y = (z - _t64(p['bn_mean'])) * inv + _t64(p['bn_beta'])
    B = B * inv.abs() / 3
    rel_out = rel @ _t64(p['rels_weight'])                                        # model.py:107 ([:-1]: without the loop row)
    return torch.tanh(y).numpy(), rel_out.numpy(), B.numpy(), y.numpy()


def layer_f32_slots(p, x, rel, ee, edge_index, edge_type, perm, drop_slot=None, scale_shift=0):
    """The layer in plain f32: per half the messages in slot order (`perm`[s] = reference edge of slot s), summed per
    destination in that order, then one `@` per mode, / 3, bias, BN as scale and shift, tanh. Value-only perturbations:
    drop_slot = s leaves slot s out of its row's sum; scale_shift = 1 takes every column's BN scale from its neighbour."""
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    x, rel, ee = f(x), f(rel), f(ee)
    ei, et, perm = np.asarray(edge_index), np.asarray(edge_type), np.asarray(perm)
    N, D = x.shape
    E = ei.shape[1] // 2
    rels = np.concatenate([rel, f(p['loop_rel']).reshape(1, D)], 0)
    keep = np.ones(perm.shape[0], dtype=bool)
    if drop_slot is not None:
        keep[drop_slot] = False
    z = None
    for h, wname in ((0, 'in_weight'), (1, 'out_weight')):
        row, col = ei[0, h * E:(h + 1) * E], ei[1, h * E:(h + 1) * E]
        deg = np.bincount(row, minlength=N).astype(np.float32)
        with np.errstate(divide='ignore'):
            inv = deg ** np.float32(-0.5)
        inv[np.isinf(inv)] = 0
        edges = perm[keep & ((perm >= E) == bool(h))]                             # this half's edges in slot order
        src, dst = ei[0, edges], ei[1, edges]
        msg = x[src] * rels[et[edges]] * ee[edges] * (inv[src] * inv[dst])[:, None]
        agg = torch.zeros((N, D), dtype=torch.float32).index_add_(0, torch.from_numpy(dst), torch.from_numpy(msg)).numpy()
        u = agg @ f(p[wname])
        z = u if z is None else z + u
    z = (z + (x * rels[-1] * f(p['loop_edge']).reshape(1, D)) @ f(p['loop_weight'])) / np.float32(3)
    if p.get('bias') is not None:
        z = z + f(p['bias'])
    scale = f(p['bn_gamma']) / np.sqrt(f(p['bn_var']) + np.float32(p['eps']))
    shift = f(p['bn_beta']) - f(p['bn_mean']) * scale
    if scale_shift:
        scale = np.roll(scale, scale_shift)
    return np.tanh(z * scale + shift)
