"""The training step's query path on stock torch against the HIP kernels of csrc/query_train.hip, in one process, on the
WN18RR shape (N = 40 943 entities, 2R = 22 relation rows, O = 200) at B = 128 and B = 1024:
  query_path_fwd_bwd        the two query-row gathers all_ent[src], all_rel[rel] and the trunk's tail hidden_drop -> bn2 -> relu
                            (fed s + r), forward and backward down to the two tables' gradients;
  train_step_wn18rr_1layer  the whole training step (forward_loss, backward, clip, Adam) with one layer, the other switches at
                            their defaults;
each for three variants alternating rep by rep: torch's default, torch under use_deterministic_algorithms(True) (its sort-based
index_add_ in place of float atomics), and params.query_path_train = 'hip'. HIP events, the median of --reps after --warmup.
One JSON line per measurement; run the whole command twice and compare the lines (the spread between the runs is the
yardstick of any difference).

    python tools/bench_query_train.py [--batches 128 1024] [--reps 20] [--warmup 5] [--out FILE] [--skip-step]
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

GEOM = dict(k_w=10, k_h=20, kernel_size=7, num_filter=200, gcn_out_dim=200, bias=False)
VARIANTS = ('torch', 'torch_deterministic', 'hip')


def alternate(fns, reps, warmup):
    """{name: [ms per rep]} of the callables, alternating, each rep between two HIP events."""
    times = {k: [] for k in fns}
    for i in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    return times


def deterministic(fn):
    def run():
        torch.use_deterministic_algorithms(True, warn_only=True)
        try:
            fn()
        finally:
            torch.use_deterministic_algorithms(False)
    return run


def path_fns(pkg, dev, B):
    shape = bench.SHAPES['wn18rr']
    N, R, O = shape['N'], shape['R'], GEOM['gcn_out_dim']
    g = torch.Generator().manual_seed(3)
    ent, rel_t = torch.randn(N, O, generator=g).to(dev).requires_grad_(True), torch.randn(2 * R, O, generator=g).to(dev).requires_grad_(True)
    src, rel = torch.randint(0, N, (B,), generator=g).to(dev), torch.randint(0, 2 * R, (B,), generator=g).to(dev)
    gy = torch.randn(B, O, generator=g).to(dev)
    fns = {}
    for name in VARIANTS:
        params = types.SimpleNamespace(feat_drop=0.3, hidden_drop=0.3, query_path_train='hip' if name == 'hip' else 'torch', **GEOM)
        torch.manual_seed(0)
        conv = pkg.model.ConvE(params, 10).to(dev).train()
        owner = types.SimpleNamespace(training=True, params=params)

        def run(conv=conv, owner=owner):
            ent.grad = rel_t.grad = None
            for p in conv.bn2.parameters():
                p.grad = None
            z = pkg.model.query_rows(owner, ent, src) + pkg.model.query_rows(owner, rel_t, rel)
            (conv._tail(z, None, False) * gy).sum().backward()
        fns[name] = deterministic(run) if name == 'torch_deterministic' else run
    return fns


def step_fns(pkg, dev, B):
    shape = bench.SHAPES['wn18rr']
    N, R, E = shape['N'], shape['R'], shape['E']
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    fns = {}
    g = torch.Generator().manual_seed(2)
    trip = torch.stack([torch.randint(0, N, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1).to(dev)
    known = {}
    for s_, r_ in trip.tolist():
        known.setdefault((s_, r_), set()).update(int(v) for v in torch.randint(0, N, (4,), generator=g))
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    for name in VARIANTS:
        params = types.SimpleNamespace(gcn_in_dim=100, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, lbl_smooth=0.1, gcn_layers=1,
                                       clip_grad=1.0, device=dev, query_path_train='hip' if name == 'hip' else 'torch', **GEOM)
        graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
        graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
        graph.to(dev)
        torch.manual_seed(0)
        model = pkg.MGCN(N, R, E, params).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def run(model=model, opt=opt, graph=graph):
            opt.zero_grad()
            loss = model.forward_loss(trip[:, 0], trip[:, 1], graph, index, lbl_smooth=0.1)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=1.0)
            opt.step()
        fns[name] = deterministic(run) if name == 'torch_deterministic' else run
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[128, 1024])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_query_train: no GPU (this measurement has no CPU fallback)')
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    for name in ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN'):
        os.environ.pop(name, None)
    lines = []
    for B in args.batches:
        for what, make in (('query_path_fwd_bwd', path_fns),) + (() if args.skip_step else (('train_step_wn18rr_1layer', step_fns),)):
            t = alternate(make(pkg, dev, B), args.reps, args.warmup)
            med = {k: statistics.median(v) for k, v in t.items()}
            line = {'what': what, 'batch': B, 'reps': args.reps}
            for k in VARIANTS:
                line[k + '_ms'] = round(med[k], 4)
                line[k + '_min_ms'] = round(min(t[k]), 4)
            line['hip_over_torch'] = round(med['hip'] / med['torch'], 3)
            line['hip_over_torch_deterministic'] = round(med['hip'] / med['torch_deterministic'], 3)
            lines.append(line)
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, 'a') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
