"""Counter-drawn candidate lists (include/mgcn_hip.h (15)), in one process.
  draw    lists AND labels of B = 128 queries, K in {64, 512, 4096}, N in {40 943, 2 000 000}:
            draw     harness.draw_candidates(labels=True): one mgcn_cand_draw launch
            sample   harness.sample_candidates(check=False) + _native.cand_labels: the generator route
          device microseconds per call;
  step    one whole training step at the WN18RR shape, one layer (encoder, query rows, trunk, list loss, backward, ClipAdam),
          K in {64, 512}, lists drawn inside the step on both routes:
            sharded  draw_candidates + dist.train_step_sharded_candidates at one rank
            single   draw_candidates + MGCN.forward_loss_candidates + backward + ClipAdam.clip_and_step
The routes of a point are timed in alternation, ROUNDS windows each of back-to-back calls between device events after a warm-up;
the median and the fastest window are reported. Every run APPENDS one JSON line per point to --out (run the command twice).
Usage: python tools/bench_cand_draw.py [--out FILE.json] [--rounds 7] [--no-step]"""
import argparse
import importlib
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (shapes + graph generator)
from bench_cand_train import B, DIM, POINTS, measure  # noqa: E402  (tools/ is the script's directory: the same windows and points)

pkg = importlib.import_module('kgc-gcn_amd')
nat = pkg._native
dev = torch.device('cuda:0')


def query_index(N, g):
    """B queries (subject b, relation 0) with four known tails each."""
    known = {(b, 0): set(torch.randint(0, N, (4,), generator=g).tolist()) for b in range(B)}
    index = pkg.dist.FilterIndex.from_known(known, 1).to(dev)
    q = torch.stack([torch.arange(B), torch.zeros(B, dtype=torch.int64)], 1).to(dev)
    return index, q


def draw_points(rounds):
    rows = []
    g = torch.Generator().manual_seed(0)
    gd = torch.Generator(device=dev).manual_seed(0)
    step = [0]
    for N, K in POINTS:
        index, q = query_index(N, g)
        keys = index.query_keys(q[:, 0], q[:, 1])

        def draw():
            step[0] += 1
            return pkg.harness.draw_candidates(q, index, N, K - 1, 1234, step[0], labels=True)

        def sample():
            cand = pkg.harness.sample_candidates(q, index, N, K - 1, generator=gd, check=False)
            return cand, nat.cand_labels(keys, index.keys, index.ptr, index.tails, cand, N)

        r = dict(section='draw', N=N, B=B, K=K, rounds=rounds)
        r.update(measure({'draw': draw, 'sample': sample}, rounds))
        r['speedup_vs_sample'] = round(r['sample_us'] / r['draw_us'], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def step_points(rounds, ks=(64, 512)):
    shape = bench.SHAPES['wn18rr']
    N, R, E = shape['N'], shape['R'], shape['E']
    params = types.SimpleNamespace(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20,
                                   num_filter=200, kernel_size=7, bias=False, lbl_smooth=0.1, gcn_layers=1, clip_grad=1.0, device=dev,
                                   dropout='counter', conve_trunk_train='hip', query_path_train='hip')
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    graph.to(dev)
    models = []
    for _ in range(2):                      # one model per route, from the same initial values
        torch.manual_seed(0)
        m = pkg.MGCN(N, R, E, params).to(dev).train()
        models.append((m, pkg.ClipAdam(m.parameters(), lr=1e-3)))
    (m_sh, opt_sh), (m_one, opt_one) = models
    g = torch.Generator().manual_seed(2)
    q = torch.stack([torch.randint(0, N, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1)
    known = {}
    for (s, r), ts in zip(q.tolist(), torch.randint(0, N, (B, 4), generator=g).tolist()):
        known.setdefault((s, r), set()).update(ts)
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    q = q.to(dev)
    rows = []
    for K in ks:
        steps = {'sharded': 0, 'single': 0}

        def sharded(K=K):
            steps['sharded'] += 1
            cand, labels = pkg.harness.draw_candidates(q, index, N, K - 1, 1234, steps['sharded'], labels=True)
            pkg.dist.train_step_sharded_candidates(m_sh, graph, q[:, 0], q[:, 1], cand, index, opt_sh, labels=labels, lbl_smooth=0.1,
                                                   clip=params.clip_grad)

        def single(K=K):
            steps['single'] += 1
            cand, labels = pkg.harness.draw_candidates(q, index, N, K - 1, 1234, steps['single'], labels=True)
            opt_one.zero_grad()
            m_one.forward_loss_candidates(q[:, 0], q[:, 1], cand, graph, labels=labels, lbl_smooth=0.1).backward()
            opt_one.clip_and_step(params.clip_grad)

        r = dict(section='step', shape='wn18rr', N=N, dim=DIM, B=B, K=K, rounds=rounds, layers=1, world=1,
                 note='lists drawn inside the step on both routes; every HIP switch on, counter dropout, ClipAdam')
        r.update(measure({'sharded': sharded, 'single': single}, rounds))
        r['sharded_over_single'] = round(r['sharded_us'] / r['single_us'], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    rows = draw_points(args.rounds)
    if not args.no_step:
        rows += step_points(args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
