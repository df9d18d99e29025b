"""Gradient clipping + Adam on the WN18RR shape (one and two layers), in one process: (a) clip_grad_norm_ + torch.optim.Adam
with its defaults, (b) the same with Adam(fused=True) where this torch build takes it, (c) optim.ClipAdam.clip_and_step on
the kernels of csrc/optim.hip. Two measurements each: the clip-plus-optimizer part alone, on the gradients of one real
forward_loss + backward (restored before every repetition, outside the timed span: clip_grad_norm_ rescales them in place),
and the whole training step. HIP events, the median of --reps after --warmup, the variants alternating rep by rep. Then the
device time of every optim.hip kernel (torch profiler) with its share of 6.3 TB/s on the algorithmic bytes (4 per parameter
for the norm, 28 for the update). One JSON line per measurement.

    python tools/bench_adam.py [--layers 1 2] [--batch 128] [--reps 20] [--warmup 5] [--out profiles/bench_adam.json]
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
KERNELS = {'sq_partial_kernel': 4, 'sq_fold_kernel': 0, 'clip_coef_kernel': 0, 'adam_step_kernel': 28}   # bytes per parameter
CLIP = 1.0


def variants(pkg):
    out = {'torch_default': lambda ps: torch.optim.Adam(ps, lr=1e-3)}
    try:
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(4, device='cuda'))], lr=1e-3, fused=True)
        out['torch_fused'] = lambda ps: torch.optim.Adam(ps, lr=1e-3, fused=True)
    except (RuntimeError, TypeError, ValueError) as err:
        print(json.dumps({'what': 'note', 'torch_fused': 'not accepted by this torch build: %s' % err}))
    out['clip_adam'] = lambda ps: pkg.optim.ClipAdam(ps, lr=1e-3)
    return out


def clip_and_step(model, opt):
    if hasattr(opt, 'clip_and_step'):
        opt.clip_and_step(CLIP)
    else:
        torch.nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=CLIP)
        opt.step()


def setup(pkg, dev, layers, B):
    shape = bench.SHAPES['wn18rr']
    N, R, E = shape['N'], shape['R'], shape['E']
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    g = torch.Generator().manual_seed(2)
    trip = torch.stack([torch.randint(0, N, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1).to(dev)
    known = {}
    for s_, r_ in trip.tolist():
        known.setdefault((s_, r_), set()).update(int(v) for v in torch.randint(0, N, (4,), generator=g))
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    runs = {}
    for name, make in variants(pkg).items():
        params = types.SimpleNamespace(gcn_in_dim=100, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, lbl_smooth=0.1,
                                       gcn_layers=layers, clip_grad=CLIP, device=dev, **GEOM)
        graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
        graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
        graph.to(dev)
        torch.manual_seed(0)
        model = pkg.MGCN(N, R, E, params).to(dev).train()
        opt = model.attach_optimizer(make(model.parameters()))

        def backward(model=model, opt=opt, graph=graph):
            opt.zero_grad()
            model.forward_loss(trip[:, 0], trip[:, 1], graph, index, lbl_smooth=0.1).backward()
        runs[name] = (model, opt, backward)
    return runs


def measure(pkg, dev, layers, B, reps, warmup):
    runs = setup(pkg, dev, layers, B)
    lines, part, whole = [], {}, {}
    for name, (model, opt, backward) in runs.items():
        backward()
        saved = [(p, p.grad.clone()) for p in model.parameters() if p.grad is not None]

        def optimizer_part(model=model, opt=opt):
            clip_and_step(model, opt)

        def restore(saved=saved):
            for p, g in saved:
                p.grad.copy_(g)

        def step(model=model, opt=opt, backward=backward):
            backward()
            clip_and_step(model, opt)
        part[name], whole[name] = (optimizer_part, restore), step
    nparams = sum(p.numel() for p in next(iter(runs.values()))[0].parameters() if p.grad is not None)
    times = {k: [] for k in part}
    for i in range(warmup + reps):                       # like `alternate`, with the gradients restored outside the events
        for name, (fn, restore) in part.items():
            restore()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    for what, t in (('clip_plus_optimizer', times), ('train_step', alternate(whole, reps, warmup))):
        line = {'what': what, 'shape': 'wn18rr', 'layers': layers, 'batch': B, 'reps': reps, 'parameters': nparams}
        for k, v in t.items():
            line[k + '_ms'] = round(statistics.median(v), 4)
            line[k + '_min_ms'] = round(min(v), 4)
        lines.append(line)
    lines.append(kernel_times(runs['clip_adam'], nparams, layers, B))
    return lines


def kernel_times(run, nparams, layers, B, passes=5):
    from torch.profiler import ProfilerActivity, profile
    model, opt, backward = run
    backward()
    for _ in range(3):
        clip_and_step(model, opt)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(passes):
            clip_and_step(model, opt)
        torch.cuda.synchronize()
    line = {'what': 'optim_hip_kernels', 'shape': 'wn18rr', 'layers': layers, 'batch': B, 'parameters': nparams, 'kernels': {}}
    for ev in prof.key_averages():
        for k, nbytes in KERNELS.items():
            if k in ev.key:
                us = getattr(ev, 'device_time_total', getattr(ev, 'cuda_time_total', 0.0)) / passes
                entry = line['kernels'].setdefault(k, {'us_per_step': 0.0, 'launches_per_step': 0})
                entry['us_per_step'] = round(entry['us_per_step'] + us, 2)
                entry['launches_per_step'] += ev.count // passes
    for k, entry in line['kernels'].items():
        if KERNELS[k] and entry['us_per_step'] > 0:
            entry['fraction_of_%g_TBs' % HBM_TBS] = round(KERNELS[k] * nparams / (entry['us_per_step'] * 1e-6) / (HBM_TBS * 1e12), 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'bench_adam.json'),
                    help='the JSON lines are written to this file as well')
    args = ap.parse_args()
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    lines = []
    for layers in args.layers:
        lines += measure(pkg, dev, layers, args.batch, max(args.reps, 20), args.warmup)
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
