"""The destination-partitioned training step at one rank against the one-GPU step, at a benchmark shape: wall-clock per step
of dist.train_step_sharded (W = 1) and of forward_loss + backward + clip + Adam, from the same state. With --profile, the
aggregation backward kernels of both (mgcn_aggregate_bwd_shard's agg_bwd_shard_* against mgcn_aggregate_bwd's agg_bwd_*) are
timed by a child run under `rocprofv3 --kernel-trace --stats` (--kernels mode: the two backward entry points only, same inputs).
One JSON line. Every GPU step of the caller belongs under its own `timeout`.

    python tools/bench_train_sharded.py [--shape wn18rr] [--layers 1] [--steps 20] [--batch 128] [--profile]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (shapes + graph generator)


def _setup(args, pkg, dev):
    shape = bench.SHAPES[args.shape]
    N, R, E = shape['N'], shape['R'], shape['E']
    params = types.SimpleNamespace(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, k_w=10,
                                   k_h=20, num_filter=200, kernel_size=7, bias=False, lbl_smooth=0.1,
                                   gcn_layers=args.layers, clip_grad=1.0, device=dev)
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    graph.to(dev)
    g = torch.Generator().manual_seed(2)
    known = {}
    for s, r, o in zip(torch.randint(0, N, (8 * N,), generator=g).tolist(), torch.randint(0, 2 * R, (8 * N,), generator=g).tolist(),
                       torch.randint(0, N, (8 * N,), generator=g).tolist()):
        known.setdefault((s, r), set()).add(o)
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    keys = list(known)
    pick = torch.randint(0, len(keys), (args.batch,), generator=g).tolist()
    q = torch.tensor([keys[i] for i in pick], dtype=torch.int64, device=dev)
    return N, R, E, params, graph, index, q


def _time(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def _kernels(args, pkg, dev):
    """Both backward entry points on the same inputs, `steps` times each (for the profiler)."""
    N, R, E, params, graph, _, _ = _setup(args, pkg, dev)
    csr = graph.csr(2 * R + 1)
    g = torch.Generator().manual_seed(3)
    D = 100
    x, rel = torch.randn(N, D, generator=g).to(dev), torch.randn(2 * R + 1, D, generator=g).to(dev)
    ee, gr = torch.randn(2 * E, D, generator=g).to(dev), torch.randn(N, 2 * D, generator=g).to(dev)
    for _ in range(args.steps):
        pkg._native.aggregate_bwd(csr, x, rel, ee, gr)
        pkg._native.aggregate_bwd_shard(csr, x, rel, ee, gr, (0, N))
    torch.cuda.synchronize()


def _profile(args):
    """Run --kernels under rocprofv3 and sum the kernels' mean times per entry point (us per call)."""
    out = tempfile.mkdtemp(prefix='bts_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'run', '--', sys.executable,
           os.path.abspath(__file__), '--kernels', '--shape', args.shape, '--steps', str(args.steps)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if not stats:
        raise RuntimeError('rocprofv3 wrote no kernel statistics under %s' % out)
    full, shard, both, rows = 0.0, 0.0, 0.0, {}
    with open(stats[0]) as f:
        for row in csv.DictReader(f):
            name, calls, total = row['Name'], int(row['Calls']), float(row['TotalDurationNs'])
            if 'agg_' not in name:
                continue                                                 # (the one-off index build: torch sorts and scans)
            rows[re.sub(r'^void \(anonymous namespace\)::', '', name).split('(')[0]] = round(total / calls / 1e3, 2)   # us / launch
            per_step = total / args.steps / 1e3
            if 'agg_bwd_shard' in name:
                shard += per_step
            elif 'grel_final' in name or 'hub_fold' in name:
                both += per_step / 2                                     # launched once per call by both entry points
            else:
                full += per_step
    full, shard = full + both, shard + both
    return dict(bwd_full_us=round(full, 2), bwd_shard_us=round(shard, 2), bwd_ratio=round(shard / full, 3) if full else None,
                kernels_us=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='wn18rr', choices=sorted(bench.SHAPES))
    ap.add_argument('--layers', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--kernels', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    if args.kernels:
        return _kernels(args, pkg, dev)
    N, R, E, params, graph, index, q = _setup(args, pkg, dev)
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(pkg.MGCN(N, R, E, params).to(dev))
    one, shd = models
    opt_one = torch.optim.Adam(one.parameters(), lr=1e-3)
    opt_shd = torch.optim.Adam(shd.parameters(), lr=1e-3)

    def step_one():
        one.train()
        opt_one.zero_grad()
        loss = one.forward_loss(q[:, 0], q[:, 1], graph, index, lbl_smooth=params.lbl_smooth)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(parameters=one.parameters(), max_norm=params.clip_grad)
        opt_one.step()

    def step_shd():
        pkg.dist.train_step_sharded(shd, graph, q[:, 0], q[:, 1], index, opt_shd, lbl_smooth=params.lbl_smooth,
                                    clip=params.clip_grad)

    res = dict(shape=args.shape, layers=args.layers, batch=args.batch, steps=args.steps)
    res['one_gpu_step_ms'] = round(_time(step_one, args.steps), 3)
    res['sharded_w1_step_ms'] = round(_time(step_shd, args.steps), 3)
    res['step_ratio'] = round(res['sharded_w1_step_ms'] / res['one_gpu_step_ms'], 3)
    if args.profile:
        res.update(_profile(args))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
