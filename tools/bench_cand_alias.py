"""Weighted candidate lists (include/mgcn_hip.h (17)) against uniform ones, in one process.
  draw    lists AND labels of B = 128 queries, K in {64, 512, 4096}, N in {40 943, 2 000 000}:
            uniform    harness.draw_candidates(labels=True): one mgcn_cand_draw launch
            weighted   the same call with sampler=...: one mgcn_cand_draw_alias launch (one 8-byte table word per negative)
          device microseconds per call;
  stage   the softmax scoring stage forward + backward (model._CandCEFn, its plan sort included) with leaves x [B, dim],
          all_ent [N, dim], bias [N] at dim = 200, on a uniform and on a weighted list of the same point; the weighted route
          forms bias - logq inside the timed call, as the step does; with every list the longest run of its cand_plan (the plan
          entries that name one entity: cand_bwd_ent_kernel walks a run with ONE wave however long it is).
The sampler is NegativeSampler.from_degrees (power 0.75, shift 1) of a Zipf(1.1) degree vector, 8 N edge ends spread as
tools/bench_skew.py spreads destinations. The routes of a point are timed in alternation, ROUNDS windows each of back-to-back
calls between device events after a warm-up; the median and the fastest window are reported. Every run APPENDS one JSON line per
point to --out (run the command twice).
Usage: python tools/bench_cand_alias.py [--out FILE.json] [--rounds 7]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_cand_draw import query_index  # noqa: E402  (tools/ is the script's directory: the same queries and index)
from bench_cand_train import B, DIM, POINTS, measure  # noqa: E402  (the same windows and points)

pkg = importlib.import_module('kgc-gcn_amd')
nat = pkg._native
dev = torch.device('cuda:0')
ZIPF, ENDS_PER_ENTITY = 1.1, 8


def zipf_degrees(N, seed=0):
    """deg [N] int64: ENDS_PER_ENTITY * N edge ends drawn with p ~ 1 / rank^ZIPF over a random permutation of the entities."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, N + 1) ** ZIPF
    ends = rng.permutation(N)[rng.choice(N, size=ENDS_PER_ENTITY * N, p=p / p.sum())]
    return torch.from_numpy(np.bincount(ends, minlength=N))


def longest_run(cand, N):
    """The longest stretch of cand_plan entries that name one entity."""
    perm, n_live = nat.cand_plan(cand, N)
    rows = cand.reshape(-1)[perm[:n_live]]
    return int(torch.unique_consecutive(rows, return_counts=True)[1].max()) if n_live else 0


def points(rounds):
    rows = []
    g = torch.Generator().manual_seed(0)
    gd = torch.Generator(device=dev).manual_seed(0)
    step = [0]
    table = {}
    for N, K in POINTS:
        if N not in table:
            table.clear()                                    # one table resident at a time
            torch.cuda.empty_cache()
            deg = zipf_degrees(N)
            table[N] = ((torch.randn(N, DIM, device=dev, generator=gd) * 0.1).requires_grad_(True),
                        (torch.randn(N, device=dev, generator=gd) * 0.2).requires_grad_(True),
                        pkg.NegativeSampler.from_degrees(deg).to(dev), int(deg.max()))
        ent, bias, sampler, max_deg = table[N]
        index, q = query_index(N, g)

        def uniform():
            step[0] += 1
            return pkg.harness.draw_candidates(q, index, N, K - 1, 1234, step[0], labels=True)

        def weighted():
            step[0] += 1
            return pkg.harness.draw_candidates(q, index, N, K - 1, 1234, step[0], labels=True, sampler=sampler)

        r = dict(section='draw', N=N, B=B, K=K, rounds=rounds, zipf=ZIPF, max_degree=max_deg,
                 max_nq=round(float(sampler.logq.max().exp()), 2))
        r.update(measure({'uniform': uniform, 'weighted': weighted}, rounds))
        r['weighted_over_uniform'] = round(r['weighted_us'] / r['uniform_us'], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)

        x = (torch.randn(B, DIM, device=dev, generator=gd) * 0.3).requires_grad_(True)
        lists = {'uniform': pkg.harness.draw_candidates(q, index, N, K - 1, 1234, 0, labels=True),
                 'weighted': pkg.harness.draw_candidates(q, index, N, K - 1, 1234, 0, labels=True, sampler=sampler)}

        def stage(name):
            cand, labels = lists[name]
            logq = sampler.logq if name == 'weighted' else None

            def run():
                for t in (x, ent, bias):
                    t.grad = None
                pkg.model._CandCEFn.apply(x, ent, bias if logq is None else bias - logq, cand, labels, 0.1).backward()
            return run

        r = dict(section='stage', loss='softmax', N=N, dim=DIM, B=B, K=K, rounds=rounds, zipf=ZIPF,
                 uniform_longest_run=longest_run(lists['uniform'][0], N), weighted_longest_run=longest_run(lists['weighted'][0], N))
        r.update(measure({'uniform': stage('uniform'), 'weighted': stage('weighted')}, rounds))
        r['weighted_over_uniform'] = round(r['weighted_us'] / r['uniform_us'], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    rows = points(args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
