"""Counter-based dropout (csrc/dropout.hip) against torch's mask sequence, in one process: (a) the layer's in / out mask pass on
[40 943, 200] at p = 0.1 -- torch's four ops per mask (empty_like.bernoulli_.bool, u * m, .mul_) against one mgcn_dropout_apply_pair
launch in place; (b) the backward pair, two masked gradients from one gu; (c) gcn_drop (F.dropout against mgcn_dropout_apply);
(d) the WN18RR-shape training step (1 layer) at B = 128 and 1 024 with params.dropout 'torch' and 'counter', and
torch.cuda.max_memory_allocated of one step both ways. HIP events, the median of --reps after --warmup, the variants alternating
rep by rep. The algorithmic bytes of the pair pass are 16 per element pair (read and write two f32), set against 6.3 TB/s.
One JSON line per measurement.

    python tools/bench_dropout.py [--batches 128 1024] [--reps 30] [--warmup 5] [--out profiles/bench_dropout.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (shapes + graph generator)
from tools.bench_trunk_train import GEOM, alternate  # noqa: E402

HBM_TBS = 6.3
N, O = 40943, 200


def mask_pass(pkg, dev):
    nat = pkg._native
    g = torch.Generator().manual_seed(1)
    u_in, u_out, gu = (torch.randn(N, O, generator=g).to(dev) for _ in range(3))
    p, keep = 0.1, 0.9
    inv_keep = 1.0 / keep
    k_in, k_out = nat.dropout_key(0, 0, 0), nat.dropout_key(0, 0, 1)
    state = {}

    def torch_fwd():
        m_in = torch.empty_like(u_in).bernoulli_(keep).bool()
        m_out = torch.empty_like(u_out).bernoulli_(keep).bool()
        state['m'] = (m_in, m_out)
        return (u_in * m_in).mul_(inv_keep), (u_out * m_out).mul_(inv_keep)

    def counter_fwd():
        return nat.dropout_apply_pair(u_in, k_in, u_out, k_out, 0, p, out_a=u_in, out_b=u_out)      # in place, as the layer does

    torch_fwd()

    def torch_bwd():
        m_in, m_out = state['m']
        return (gu * m_in).mul_(inv_keep), (gu * m_out).mul_(inv_keep)

    def counter_bwd():
        return nat.dropout_apply_pair(gu, k_in, gu, k_out, 0, p)

    def torch_gcn():
        return torch.nn.functional.dropout(u_in, p=0.3, training=True)

    def counter_gcn():
        return nat.dropout_apply(u_in, k_in, 0, 0.3)

    return {'mask_pass_fwd_pair': (torch_fwd, counter_fwd, 16 * N * O), 'mask_pass_bwd_pair': (torch_bwd, counter_bwd, 12 * N * O),
            'gcn_drop_fwd': (torch_gcn, counter_gcn, 8 * N * O)}


def step_pair(pkg, dev, B):
    shape = bench.SHAPES['wn18rr']
    n, R, E = shape['N'], shape['R'], shape['E']
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    fns = {}
    g = torch.Generator().manual_seed(2)
    trip = torch.stack([torch.randint(0, n, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1).to(dev)
    known = {}
    for s_, r_ in trip.tolist():
        known.setdefault((s_, r_), set()).update(int(v) for v in torch.randint(0, n, (4,), generator=g))
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    for switch in ('torch', 'counter'):
        params = types.SimpleNamespace(gcn_in_dim=100, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, lbl_smooth=0.1, gcn_layers=1,
                                       clip_grad=1.0, device=dev, dropout=switch, **GEOM)
        graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
        graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(n), n, None
        graph.to(dev)
        torch.manual_seed(0)
        model = pkg.MGCN(n, R, E, params).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def run(model=model, opt=opt, graph=graph):
            opt.zero_grad()
            loss = model.forward_loss(trip[:, 0], trip[:, 1], graph, index, lbl_smooth=0.1)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=1.0)
            opt.step()
        fns[switch] = run
    return fns


def peak_memory(fns):
    """max_memory_allocated over one step of each variant, above what is allocated before the step (MiB)."""
    out = {}
    for name, fn in fns.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[name] = round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[128, 1024])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'bench_dropout.json'),
                    help='the JSON lines are written to this file as well')
    args = ap.parse_args()
    os.environ.pop('MGCN_DROPOUT', None)           # the step's two variants are chosen by params.dropout
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    lines = []
    for what, (tfn, cfn, nbytes) in mask_pass(pkg, dev).items():
        t = alternate({'torch': tfn, 'counter': cfn}, args.reps, args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append({'what': what, 'rows': N, 'cols': O, 'reps': args.reps, 'torch_ms': round(med['torch'], 4),
                      'counter_ms': round(med['counter'], 4), 'speedup': round(med['torch'] / med['counter'], 3),
                      'torch_min_ms': round(min(t['torch']), 4), 'counter_min_ms': round(min(t['counter']), 4),
                      'counter_fraction_of_%g_TBs' % HBM_TBS: round(nbytes / (med['counter'] * 1e-3) / (HBM_TBS * 1e12), 4)})
    for B in args.batches:
        fns = step_pair(pkg, dev, B)
        t = alternate(fns, args.reps, args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        mem = peak_memory(fns)
        lines.append({'what': 'train_step_wn18rr_1layer', 'batch': B, 'reps': args.reps, 'torch_ms': round(med['torch'], 4),
                      'counter_ms': round(med['counter'], 4), 'speedup': round(med['torch'] / med['counter'], 3),
                      'torch_min_ms': round(min(t['torch']), 4), 'counter_min_ms': round(min(t['counter']), 4),
                      'torch_step_peak_mib': mem['torch'], 'counter_step_peak_mib': mem['counter']})
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
