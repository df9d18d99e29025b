"""The captured sampled-negative step (captured.CapturedCandidateStep) against the eager list step, in one process:
the WN18RR shape with one layer, every HIP switch on, counter dropout and ClipAdam; B in {128, 1024}, K = 1 + num_neg in {64, 512},
both losses. Three routes, each on its own model built from the same seed, all drawing their lists from (seed, step):
    item      one step of harness.train_sampled_negatives(draw_seed=...) as it runs today: loss.item() after every step
    eager     the same step in a loop that never waits for the device
    captured  one call of CapturedCandidateStep (a replay: the capture is asserted before anything is timed)
The method is tools/bench_cand_train.py's (its helpers are imported): the routes of a point are timed in alternation, ROUNDS
windows each of back-to-back calls between device events after a warm-up; the median and the fastest window are reported, and next
to them the median wall time per call of the same windows (enqueue + the one synchronisation that ends a window). pool_bytes is
what the graph's private pool holds beyond the live tensors: bytes reserved minus bytes allocated after torch.cuda.empty_cache(),
above the same difference before the captured path was built (tools/bench_train_captured.py's held - resident).
Every run APPENDS one JSON line per point to --out; run the command twice.
Usage: python tools/bench_cand_captured.py [--out FILE.json] [--rounds 7]"""
import argparse
import gc
import json
import os
import statistics
import time

import torch

from bench_cand_train import bench, calls_for, dev, pkg
from bench_train_captured import CONFIGS, batches_and_index, build

SEED = 1234
POINTS = [(B, K, loss) for B in (128, 1024) for K in (64, 512) for loss in ('bce', 'softmax')]


def window(fn, calls):
    """(device us, wall us) per call of one window of back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3, (time.perf_counter() - t0) / calls * 1e6


def routes_for(shape, B, K, loss, qs, index):
    """({route: fn}, the captured step, pool bytes)."""
    N = shape['N']
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    slack = torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    model, graph, params, opt = build(pkg, shape, dev, CONFIGS['all_hip'])
    step = pkg.CapturedCandidateStep(model, graph, index, opt, K - 1, SEED, loss=loss, lbl_smooth=params.lbl_smooth, clip=params.clip_grad)
    turn = [0]

    def captured():
        q = qs[turn[0] % len(qs)]
        turn[0] += 1
        return step(q[:, 0], q[:, 1])

    for _ in range(4):
        captured()
    torch.cuda.synchronize()
    assert step.captures == 1 and step.replays == 2 and not step.disabled, 'the step was not captured'
    torch.cuda.empty_cache()
    pool = torch.cuda.memory_reserved() - torch.cuda.memory_allocated() - slack

    def eager_route(item):
        model, graph, params, opt = build(pkg, shape, dev, CONFIGS['all_hip'])
        k = [0]

        def fn():
            q = qs[k[0] % len(qs)]
            cand, labels = pkg.harness.draw_candidates(q, index, N, K - 1, SEED, k[0], labels=True)
            k[0] += 1
            opt.zero_grad()
            out = model.forward_loss_candidates(q[:, 0], q[:, 1], cand, graph, labels=labels, lbl_smooth=params.lbl_smooth, loss=loss)
            out.backward()
            opt.clip_and_step(params.clip_grad)
            return out.item() if item else out

        return fn

    return {'item': eager_route(True), 'eager': eager_route(False), 'captured': captured}, step, int(pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    shape = bench.SHAPES['wn18rr']
    rows = []
    for B, K, loss in POINTS:
        qs, index = batches_and_index(pkg, shape, B, 16, dev)
        routes, step, pool = routes_for(shape, B, K, loss, qs, index)
        calls = {k: calls_for(fn) for k, fn in routes.items()}
        dev_us, wall_us = {k: [] for k in routes}, {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                d, w = window(fn, calls[k])
                dev_us[k].append(d)
                wall_us[k].append(w)
        r = dict(shape='wn18rr', layers=1, B=B, K=K, loss=loss, rounds=args.rounds, pool_bytes=pool, captures=step.captures,
                 replays=step.replays, eager_steps=step.eager_steps)
        for k in routes:
            r[k + '_us'] = round(statistics.median(dev_us[k]), 2)
            r[k + '_min_us'] = round(min(dev_us[k]), 2)
            r[k + '_wall_us'] = round(statistics.median(wall_us[k]), 2)
        r['item_over_captured'] = round(r['item_us'] / r['captured_us'], 3)
        r['eager_over_captured'] = round(r['eager_us'] / r['captured_us'], 3)
        assert step.captures == 1 and not step.disabled
        rows.append(r)
        print(json.dumps(r), flush=True)
        del routes, step
        gc.collect()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
