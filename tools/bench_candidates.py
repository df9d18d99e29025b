"""Candidate-list scoring (mgcn_score_candidates, include/mgcn_hip.h (13)) against the two other routes to the same [B, K]
scores, in one process: device microseconds per call at the WN18RR shape (N 40 943, dim 200, B 128) for K in {1, 64, 512,
4096}, and one point at N = 2 000 000, K = 512, where the full pass writes a 1 GB score block. Routes:
  candidates   _native.score_candidates (one launch into a caller-held block)
  fwd_gather   _native.score_fwd into [B, N], then torch.gather: the only route before this entry point existed
  torch_dot    sigmoid((ent[cand] * x[:, None]).sum(-1) + bias[cand]) on torch ops (other bits: not a drop-in)
The routes of a point are timed in alternation, ROUNDS windows each of back-to-back calls between device events after a
warm-up; the median and the fastest window are reported, with the bytes each route has to move by its shapes (gathered rows
K B dim 4 for the list; N dim 4 + B N 4 for the full pass). Every run APPENDS one JSON line per point to --out.
Usage: python tools/bench_candidates.py [--out FILE.json] [--rounds 7]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module('kgc-gcn_amd')
nat = pkg._native
dev = torch.device('cuda:0')
DIM, B = 200, 128
POINTS = [(40943, 1), (40943, 64), (40943, 512), (40943, 4096), (2000000, 512)]


def window_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def calls_for(fn, window_ms=30.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    once_ms = max(window_us(fn, 1) * 1e-3, 1e-3)
    return max(3, min(400, int(window_ms / once_ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(0)
    tables = {}
    rows = []
    for N, K in POINTS:
        if N not in tables:
            tables.clear()                                   # one table resident at a time
            tables[N] = (torch.randn(N, DIM, device=dev, generator=g) * 0.1, torch.randn(N, device=dev, generator=g) * 0.2)
        ent, bias = tables[N]
        x = torch.randn(B, DIM, device=dev, generator=g) * 0.3
        cand = torch.randint(0, N, (B, K), device=dev, generator=g)
        out = torch.empty((B, K), device=dev)
        routes = {
            'candidates': lambda: nat.score_candidates(x, ent, bias, cand, out=out),
            'fwd_gather': lambda: nat.score_fwd(x, ent, bias).gather(1, cand),
            'torch_dot': lambda: torch.sigmoid((ent[cand] * x[:, None, :]).sum(-1) + bias[cand]),
        }
        same = torch.equal(routes['candidates'](), routes['fwd_gather']())
        calls = {k: calls_for(fn) for k, fn in routes.items()}
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                times[k].append(window_us(fn, calls[k]))
        r = dict(N=N, dim=DIM, B=B, K=K, rounds=args.rounds, bit_identical_to_fwd_gather=bool(same),
                 list_bytes=K * B * DIM * 4, full_pass_bytes=N * DIM * 4 + B * N * 4)
        for k in routes:
            r[k + '_us'] = round(statistics.median(times[k]), 2)
            r[k + '_min_us'] = round(min(times[k]), 2)
        r['candidates_gather_GBs'] = round(r['list_bytes'] / (r['candidates_us'] * 1e-6) / 1e9, 1)
        r['speedup_vs_fwd_gather'] = round(r['fwd_gather_us'] / r['candidates_us'], 2)
        r['speedup_vs_torch_dot'] = round(r['torch_dot_us'] / r['candidates_us'], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
