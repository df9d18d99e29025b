"""The training-mode ConvE trunk on the torch modules against the HIP kernels of csrc/conve_train.hip, in one process:
the trunk's forward + backward alone at the production geometry (10, 20, 7, 200), and the whole training step
(forward_loss, backward, clip, Adam) on the WN18RR shape with one layer, at B = 128 and B = 1024. HIP events, the median
of --reps after --warmup, the two paths alternating rep by rep. One JSON line per measurement; run the whole command
twice and compare the lines (the spread between the runs is the yardstick of the speed-up).

    python tools/bench_trunk_train.py [--batches 128 1024] [--reps 20] [--warmup 5] [--out FILE] [--launches]
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
PEAK_TF = 155.0          # f32 MFMA peak the three products are set against


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


def trunk_pair(pkg, dev, B):
    fns = {}
    g = torch.Generator().manual_seed(3)
    s0, r0, gy = (torch.randn(B, 200, generator=g).to(dev) for _ in range(3))
    for switch in ('torch', 'hip'):
        params = types.SimpleNamespace(feat_drop=0.3, hidden_drop=0.3, conve_trunk_train=switch, **GEOM)
        torch.manual_seed(0)
        conv = pkg.model.ConvE(params, 10).to(dev).train()

        def run(conv=conv):
            s, r = s0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
            for p in conv.parameters():
                p.grad = None
            (conv.trunk(s, r) * gy).sum().backward()
        fns[switch] = run
    return fns


def step_pair(pkg, dev, B):
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
    for switch in ('torch', 'hip'):
        params = types.SimpleNamespace(gcn_in_dim=100, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, lbl_smooth=0.1, gcn_layers=1,
                                       clip_grad=1.0, device=dev, conve_trunk_train=switch, **GEOM)
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
        fns[switch] = run
    return fns


def launches(pkg, dev, B):
    """Per-launch times of the HIP trunk from torch's profiler (kernel name -> mean microseconds over 5 passes)."""
    from torch.profiler import ProfilerActivity, profile
    run = trunk_pair(pkg, dev, B)['hip']
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        if 'tt_' in ev.key:
            name = ev.key[ev.key.index('tt_'):].split('(')[0].split('E')[0]
            out[name] = out.get(name, 0.0) + getattr(ev, 'device_time_total', getattr(ev, 'cuda_time_total', 0.0)) / 5.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[128, 1024])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    ap.add_argument('--launches', action='store_true', help='also the per-launch split of the HIP trunk (torch profiler)')
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    os.environ.pop('MGCN_TRUNK_TRAIN', None)
    lines = []
    for B in args.batches:
        for what, pair in (('trunk_fwd_bwd', trunk_pair),) + ((() if args.skip_step else (('train_step_wn18rr_1layer', step_pair),))):
            t = alternate(pair(pkg, dev, B), args.reps, args.warmup)
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append({'what': what, 'batch': B, 'reps': args.reps, 'torch_ms': round(med['torch'], 4), 'hip_ms': round(med['hip'], 4),
                          'speedup': round(med['torch'] / med['hip'], 3),
                          'torch_min_ms': round(min(t['torch']), 4), 'hip_min_ms': round(min(t['hip']), 4)})
        if args.launches:
            per = launches(pkg, dev, B)
            h, w = 2 * GEOM['k_w'] - GEOM['kernel_size'] + 1, GEOM['k_h'] - GEOM['kernel_size'] + 1
            flop = 2.0 * B * GEOM['gcn_out_dim'] * GEOM['num_filter'] * h * w          # one product: 2 B O K, K = F H W
            line = {'what': 'hip_trunk_launches_us', 'batch': B, 'launches': {k: round(v, 1) for k, v in sorted(per.items())}}
            for k in ('tt_fc_fwd_kernel', 'tt_dw_kernel', 'tt_gh_kernel'):
                if per.get(k):
                    line[k + '_fraction_of_%g_TF' % PEAK_TF] = round(flop / (per[k] * 1e-6) / (PEAK_TF * 1e12), 4)
            lines.append(line)
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, 'a') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
