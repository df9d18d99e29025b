"""Filtered top-k (mgcn_score_topk) against the other ways to spend the same score block: device microseconds per call at
the WN18RR (N 40 943) and FB15k-237 (N 14 541) shapes, O = 200, for B = 128 queries and for all of the test split's
queries (tail + head: 6 268 / 40 932), k in {10, 100}. Columns:
  topk        mgcn_score_topk, no filter
  topk_filt   mgcn_score_topk with the bit-packed filter (30 % of the bits set)
  rank        mgcn_score_rank on the same block and filter (the fused evaluation kernel; k does not apply)
  fwd+topk    mgcn_score_fwd into [B, N], then torch.topk (no filter, no tie rule: the route the package had)
Each figure is the mean over a window of back-to-back calls timed with device events after a warm-up.
Usage: python tools/bench_topk.py [--out FILE.json]"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module('kgc-gcn_amd')
nat = pkg._native
dev = torch.device('cuda:0')
SHAPES = [('wn18rr', 40943, 6268), ('fb15k237', 14541, 40932)]
O = 200


def device_us(fn, min_ms=200.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    once = max(a.elapsed_time(b), 1e-3)
    n = max(5, min(500, int(min_ms / once)))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, Q in SHAPES:
        ent = torch.randn(N, O, device=dev, generator=g) * 0.1
        bias = torch.randn(N, device=dev, generator=g) * 0.2
        for B in (128, Q):
            x = torch.randn(B, O, device=dev, generator=g) * 0.3
            dense = torch.rand(B, (N + 31) // 32 * 32, device=dev, generator=g) < 0.3
            bits = (dense.view(B, -1, 32).long() << torch.arange(32, device=dev)).sum(2)
            mask = (((bits + (1 << 31)) % (1 << 32)) - (1 << 31)).to(torch.int32).contiguous()
            obj = torch.randint(0, N, (B,), device=dev, generator=g)
            tgt = nat.score_target(x, ent, bias, obj)
            counts = torch.zeros((B, 3), dtype=torch.int64, device=dev)
            rank_us = device_us(lambda: nat.score_rank(x, ent, bias, obj, tgt, mask=mask, counts=counts))
            for k in (10, 100):
                r = dict(shape=name, N=N, O=O, B=B, k=k, rank_us=round(rank_us, 1))
                r['topk_us'] = round(device_us(lambda: nat.score_topk(x, ent, bias, k)), 1)
                r['topk_filt_us'] = round(device_us(lambda: nat.score_topk(x, ent, bias, k, mask=mask)), 1)
                r['fwd_us'] = round(device_us(lambda: nat.score_fwd(x, ent, bias)), 1)
                r['fwd_torch_topk_us'] = round(device_us(lambda: torch.topk(nat.score_fwd(x, ent, bias), k, dim=1)), 1)
                rows.append(r)
                print(json.dumps(r), flush=True)
    print('%-9s %6s %3s | %9s %9s %9s %9s %12s' % ('shape', 'B', 'k', 'topk', 'topk_filt', 'rank', 'fwd', 'fwd+topk'))
    for r in rows:
        print('%-9s %6d %3d | %9.1f %9.1f %9.1f %9.1f %12.1f' % (r['shape'], r['B'], r['k'], r['topk_us'], r['topk_filt_us'],
                                                               r['rank_us'], r['fwd_us'], r['fwd_torch_topk_us']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
