"""The list backward with split runs (include/mgcn_hip.h (18)) against the one-wave-per-run backward, in one process.
  stage   the softmax scoring stage forward + backward (model._CandCEFn, its plan sort included) with leaves x [B, dim],
          all_ent [N, dim], bias [N] at B = 128, dim = 200, K in {64, 512, 4096}, N in {40 943, 2 000 000}, on the uniform and
          on the weighted list of tools/bench_cand_alias.py (the same sampler, the same draw), with run_split in
          {None, 32, 64, 128, 256}; every list's longest run is recorded;
  step    one WN18RR-shape eager training step (tools/bench_cand_train.py's model, counter dropout, ClipAdam) on weighted lists at
          K = 512, loss='softmax' with the sampler's logq, run_split None against --step-split (default: the fastest split of
          this run's stage point N = 40 943, K = 512, weighted).
The routes of a point are timed in alternation, ROUNDS windows each of back-to-back calls between device events after a warm-up;
the median and the fastest window are reported. Every run APPENDS one JSON line per point to --out: run the command twice, the
spread between the two runs is what a ratio has to exceed.
Usage: python tools/bench_cand_split.py [--out FILE.json] [--rounds 7] [--step-split S]"""
import argparse
import importlib
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from bench_cand_alias import longest_run, zipf_degrees  # noqa: E402  (tools/ is the script's directory)
from bench_cand_draw import query_index  # noqa: E402
from bench_cand_train import B, DIM, POINTS, measure  # noqa: E402  (the same windows and points)

pkg = importlib.import_module('kgc-gcn_amd')
nat = pkg._native
dev = torch.device('cuda:0')
SPLITS = (None, 32, 64, 128, 256)


def name_of(split):
    return 'none' if split is None else 's%d' % split


def stage_points(rounds):
    rows = []
    g = torch.Generator().manual_seed(0)
    gd = torch.Generator(device=dev).manual_seed(0)
    table = {}
    for N, K in POINTS:
        if N not in table:
            table.clear()                                    # one table resident at a time
            torch.cuda.empty_cache()
            table[N] = ((torch.randn(N, DIM, device=dev, generator=gd) * 0.1).requires_grad_(True),
                        (torch.randn(N, device=dev, generator=gd) * 0.2).requires_grad_(True),
                        pkg.NegativeSampler.from_degrees(zipf_degrees(N)).to(dev))
        ent, bias, sampler = table[N]
        index, q = query_index(N, g)
        x = (torch.randn(B, DIM, device=dev, generator=gd) * 0.3).requires_grad_(True)
        lists = {'uniform': pkg.harness.draw_candidates(q, index, N, K - 1, 1234, 0, labels=True),
                 'weighted': pkg.harness.draw_candidates(q, index, N, K - 1, 1234, 0, labels=True, sampler=sampler)}
        for kind, (cand, labels) in lists.items():
            logq = sampler.logq if kind == 'weighted' else None

            def stage(split):
                def run():
                    for t in (x, ent, bias):
                        t.grad = None
                    pkg.model._CandCEFn.apply(x, ent, bias if logq is None else bias - logq, cand, labels, 0.1, 0, None, split).backward()
                return run

            r = dict(section='stage', loss='softmax', lists=kind, N=N, dim=DIM, B=B, K=K, rounds=rounds, longest_run=longest_run(cand, N))
            r.update(measure({name_of(s): stage(s) for s in SPLITS}, rounds))
            for s in SPLITS[1:]:
                r['none_over_' + name_of(s)] = round(r['none_us'] / r[name_of(s) + '_us'], 3)
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def step_point(rounds, split, num_neg=511):
    shape = bench.SHAPES['wn18rr']
    N, R, E = shape['N'], shape['R'], shape['E']
    params = types.SimpleNamespace(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20,
                                   num_filter=200, kernel_size=7, bias=False, lbl_smooth=0.1, gcn_layers=1, clip_grad=1.0, device=dev,
                                   dropout='counter', conve_trunk_train='hip', query_path_train='hip')
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    graph.to(dev)
    torch.manual_seed(0)
    model = pkg.MGCN(N, R, E, params).to(dev).train()
    opt = pkg.ClipAdam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(2)
    q = torch.stack([torch.randint(0, N, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1)
    known = {}
    for (s, r), ts in zip(q.tolist(), torch.randint(0, N, (B, 4), generator=g).tolist()):
        known.setdefault((s, r), set()).update(ts)
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    q = q.to(dev)
    sampler = pkg.NegativeSampler.from_degrees(zipf_degrees(N)).to(dev)
    count = [0]

    def step(run_split):
        def run():
            count[0] += 1
            cand, labels = pkg.harness.draw_candidates(q, index, N, num_neg, 1234, count[0], labels=True, sampler=sampler)
            opt.zero_grad()
            model.forward_loss_candidates(q[:, 0], q[:, 1], cand, graph, labels=labels, lbl_smooth=0.1, loss='softmax', logq=sampler.logq,
                                          run_split=run_split).backward()
            opt.clip_and_step(params.clip_grad)
        return run

    cand = pkg.harness.draw_candidates(q, index, N, num_neg, 1234, 0, labels=True, sampler=sampler)[0]
    r = dict(section='step', shape='wn18rr', loss='softmax', lists='weighted', N=N, dim=DIM, B=B, K=num_neg + 1, rounds=rounds, layers=1,
             run_split=split, longest_run=longest_run(cand, N),
             note='the weighted draw is inside the step; every HIP switch on, counter dropout, ClipAdam, eager')
    r.update(measure({'none': step(None), name_of(split): step(split)}, rounds))
    r['none_over_' + name_of(split)] = round(r['none_us'] / r[name_of(split) + '_us'], 3)
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--step-split', type=int, default=None)
    args = ap.parse_args()
    rows = stage_points(args.rounds)
    split = args.step_split
    if split is None:
        at = next(r for r in rows if (r['N'], r['K'], r['lists']) == (40943, 512, 'weighted'))
        split = min(SPLITS[1:], key=lambda s: at[name_of(s) + '_us'])
    rows += step_point(args.rounds, split)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
