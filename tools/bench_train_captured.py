"""The captured training step (kgc-gcn_amd/captured.py) against the eager step at a benchmark shape: one layer,
B = 128 and B = 1024, two configurations (counter dropout + ClipAdam + torch trunk; every HIP switch on). Eager and captured
alternate in ONE process, each on its own model built from the same seed. Per (configuration, batch) it reports

    event_ms          HIP-event time per step over a block of steps (the device's view, launches back to back)
    wall_ms           wall time per step with one synchronisation per 50 steps
    eager_item_ms     wall time of the eager loop with loss.item() after every step, as harness.train_device_labels runs today
    peak_bytes        peak allocated bytes of each path on its own (torch's allocator): what the path keeps resident (model, graph,
                      optimizer state, gradients, and for the captured path the graph's private pool) plus the highest transient
                      allocation above that during a block of steps
    resident_bytes    bytes allocated while the path is idle, above what was allocated before it was built
    held_bytes        bytes RESERVED from the device after torch.cuda.empty_cache(), above what was reserved before the path was
                      built: the eager path gives its cached blocks back, the captured path's graph keeps its private pool, so
                      held_bytes - resident_bytes of the captured path is what the pool holds beyond the live tensors

one JSON line per measurement on stdout; with --out FILE the lines are appended to FILE as well.

    python tools/bench_train_captured.py [--shape wn18rr] [--batches 128,1024] [--steps 200] [--rounds 3] [--out FILE]
"""
import argparse
import gc
import importlib
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (shapes + graph generator)

CONFIGS = {'torch_trunk': {}, 'all_hip': {'conve_trunk_train': 'hip', 'query_path_train': 'hip'}}
SYNC_EVERY = 50


def build(pkg, shape, dev, over):
    N, R, E = shape['N'], shape['R'], shape['E']
    params = types.SimpleNamespace(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20,
                                   num_filter=200, kernel_size=7, bias=False, lbl_smooth=0.1, gcn_layers=1, clip_grad=1.0, device=dev,
                                   dropout='counter', **over)
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    graph.to(dev)
    torch.manual_seed(0)
    model = pkg.MGCN(N, R, E, params).to(dev).train()
    return model, graph, params, pkg.ClipAdam(model.parameters(), lr=1e-3)


def batches_and_index(pkg, shape, B, count, dev):
    N, R = shape['N'], shape['R']
    g = torch.Generator().manual_seed(2)
    qs = [torch.stack([torch.randint(0, N, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1) for _ in range(count)]
    known = {}
    for q in qs:
        tails = torch.randint(0, N, (B, 4), generator=g).tolist()
        for (s, r), ts in zip(q.tolist(), tails):
            known.setdefault((s, r), set()).update(ts)
    return [q.to(dev) for q in qs], pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='wn18rr', choices=sorted(bench.SHAPES))
    ap.add_argument('--batches', default='128,1024')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--configs', default=','.join(sorted(CONFIGS)))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    shape = bench.SHAPES[args.shape]
    sink = open(args.out, 'a') if args.out else None

    def emit(**row):
        line = json.dumps(row, sort_keys=True)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()

    for config in args.configs.split(','):
        for B in (int(b) for b in args.batches.split(',')):
            qs, index = batches_and_index(pkg, shape, B, 16, dev)
            paths = {}
            for path in ('eager', 'captured'):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base, base_reserved = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
                model, graph, params, opt = build(pkg, shape, dev, CONFIGS[config])
                if path == 'captured':
                    step = pkg.CapturedTrainStep(model, graph, index, opt, lbl_smooth=params.lbl_smooth, clip=params.clip_grad)
                else:
                    def step(src, rel, model=model, graph=graph, opt=opt, params=params):
                        opt.zero_grad()
                        loss = model.forward_loss(src, rel, graph, index, lbl_smooth=params.lbl_smooth)
                        loss.backward()
                        opt.clip_and_step(params.clip_grad)
                        return loss.detach()
                step(qs[0][:, 0], qs[0][:, 1])
                step(qs[1][:, 0], qs[1][:, 1])
                for q in qs[2:6]:                                  # (the captured path captures on the first of these)
                    step(q[:, 0], q[:, 1])
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                resident = torch.cuda.memory_allocated() - base
                pool = torch.cuda.memory_reserved() - base_reserved
                if path == 'captured':
                    assert step.captures == 1 and not step.disabled, 'the step was not captured'
                paths[path] = (step, resident, pool)

            def run(step, n, item=False):
                """(event ms, wall ms) per step over n steps; item: loss.item() after every step."""
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                start = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for i in range(n):
                    q = qs[i % len(qs)]
                    loss = step(q[:, 0], q[:, 1])
                    if item:
                        loss.item()
                    elif (i + 1) % SYNC_EVERY == 0:
                        torch.cuda.synchronize()
                e1.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / n
                return e0.elapsed_time(e1) / n, wall, torch.cuda.max_memory_allocated() - start

            for rnd in range(args.rounds):                          # eager and captured alternate
                for path in ('eager', 'captured'):
                    step, resident, pool = paths[path]
                    event_ms, wall_ms, transient = run(step, args.steps)
                    row = dict(shape=args.shape, config=config, batch=B, path=path, round=rnd, steps=args.steps, event_ms=round(event_ms, 4),
                               wall_ms=round(wall_ms, 4), peak_bytes=int(resident + transient))
                    if path == 'eager':
                        row['eager_item_ms'] = round(run(step, args.steps, item=True)[1], 4)
                    emit(**row)
            for path in ('eager', 'captured'):
                step, resident, pool = paths[path]
                row = dict(shape=args.shape, config=config, batch=B, path=path, summary='memory', held_bytes=int(pool), resident_bytes=int(resident))
                if path == 'captured':
                    row.update(captures=step.captures, replays=step.replays, eager_steps=step.eager_steps)
                emit(**row)
            del paths, step, model, graph, params, opt           # (nothing of this pair may be alive when the next base is read)
            gc.collect()
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
