"""Training on candidate lists (include/mgcn_hip.h (14)) against the full-table loss, in one process.
  stage   the scoring stage forward + backward with leaves x [B, dim], all_ent [N, dim], bias [N] at B = 128, dim = 200,
          N in {40 943, 2 000 000}, K in {64, 512, 4096}:
            cand   _native.cand_labels + model._CandBCEFn (its plan sort included) + backward
            full   _native.filter_mask + model._ScoreBCEFn + backward (the [N, B] gradient block, two GEMMs over N rows)
          device microseconds per call and the peak allocation above what is resident before the call;
  run     the degenerate list: every query's column 0 is the SAME entity, a run of B plan entries walked by one wave;
  step    one whole training step at the WN18RR shape (encoder, query rows, trunk, loss, backward, ClipAdam) on each route.
The routes of a point are timed in alternation, ROUNDS windows each of back-to-back calls between device events after a warm-up;
the median and the fastest window are reported. Every run APPENDS one JSON line per point to --out.
Usage: python tools/bench_cand_train.py [--out FILE.json] [--rounds 7] [--no-step]"""
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

pkg = importlib.import_module('kgc-gcn_amd')
nat = pkg._native
dev = torch.device('cuda:0')
DIM, B = 200, 128
POINTS = [(40943, 64), (40943, 512), (40943, 4096), (2000000, 64), (2000000, 512), (2000000, 4096)]


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


def peak_bytes(fn, clear):
    """Peak allocation of one call above what is resident before it. `clear` drops what the previous call left behind (the
    leaves' .grad, an [N, dim] block among them) BEFORE the baseline is read: the call itself clears them too, but only after
    it has started, and they would otherwise be counted in the baseline and missing from the peak."""
    clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - base)


def measure(routes, rounds):
    calls = {k: calls_for(fn) for k, fn in routes.items()}
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(window_us(fn, calls[k]))
    out = {}
    for k in routes:
        out[k + '_us'] = round(statistics.median(times[k]), 2)
        out[k + '_min_us'] = round(min(times[k]), 2)
    return out


def stage_routes(x, ent, bias, cand, index, keys, N):
    hot, cold = nat.smoothed_targets(0.1, N)
    leaves = (x, ent, bias)

    def clear():
        for t in leaves:
            t.grad = None

    def cand_route():
        clear()
        labels = nat.cand_labels(keys, index.keys, index.ptr, index.tails, cand, N)
        pkg.model._CandBCEFn.apply(x, ent, bias, cand, labels, hot, cold).backward()

    def full_route():
        clear()
        mask = nat.filter_mask(keys, index.keys, index.ptr, index.tails, N)
        pkg.model._ScoreBCEFn.apply(x, ent, bias, mask, hot, cold).backward()

    return {'cand': cand_route, 'full': full_route}, clear


def query_index(N, g):
    """B queries with four known tails each (keys 0 .. B - 1)."""
    known = {(b, 0): set(torch.randint(0, N, (4,), generator=g).tolist()) for b in range(B)}
    index = pkg.dist.FilterIndex.from_known(known, 1).to(dev)
    keys = index.query_keys(torch.arange(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
    return index, keys


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
                        (torch.randn(N, device=dev, generator=gd) * 0.2).requires_grad_(True), query_index(N, g))
        ent, bias, (index, keys) = table[N]
        x = (torch.randn(B, DIM, device=dev, generator=gd) * 0.3).requires_grad_(True)
        cand = torch.randint(0, N, (B, K), device=dev, generator=gd)
        cand[:, 0] = index.tails[index.ptr[:-1]].long()      # column 0: a known tail of the query
        for degenerate in ((False, True) if K == 64 else (False,)):
            if degenerate:
                cand = cand.clone()
                cand[:, 0] = 12345                           # one entity named by every query: a run of B
            routes, clear = stage_routes(x, ent, bias, cand, index, keys, N)
            r = dict(section='run' if degenerate else 'stage', N=N, dim=DIM, B=B, K=K, rounds=rounds,
                     list_bytes=3 * K * B * DIM * 4, full_block_bytes=B * N * 4)
            r.update(measure(routes if not degenerate else {'cand': routes['cand']}, rounds))
            r['cand_peak_bytes'] = peak_bytes(routes['cand'], clear)
            if not degenerate:
                r['full_peak_bytes'] = peak_bytes(routes['full'], clear)
                r['speedup_vs_full'] = round(r['full_us'] / r['cand_us'], 2)
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def step_points(rounds, num_neg=(63, 511)):
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
    gd = torch.Generator(device=dev).manual_seed(3)

    def finish(loss):
        loss.backward()
        opt.clip_and_step(params.clip_grad)

    def full_step():
        opt.zero_grad()
        finish(model.forward_loss(q[:, 0], q[:, 1], graph, index, lbl_smooth=0.1))

    rows = []
    for nn in num_neg:
        def cand_step(nn=nn):
            opt.zero_grad()
            cand = pkg.harness.sample_candidates(q, index, N, nn, generator=gd, check=False)   # (as train_sampled_negatives calls it)
            finish(model.forward_loss_candidates(q[:, 0], q[:, 1], cand, graph, index=index, lbl_smooth=0.1))

        routes = {'cand': cand_step, 'full': full_step}
        r = dict(section='step', shape='wn18rr', N=N, dim=DIM, B=B, K=nn + 1, rounds=rounds, layers=1,
                 note='sampling of the lists is inside the cand step; every HIP switch on, counter dropout, ClipAdam')
        r.update(measure(routes, rounds))
        clear = lambda: opt.zero_grad(set_to_none=True)
        r['cand_peak_bytes'], r['full_peak_bytes'] = peak_bytes(cand_step, clear), peak_bytes(full_step, clear)
        r['speedup_vs_full'] = round(r['full_us'] / r['cand_us'], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    rows = stage_points(args.rounds)
    if not args.no_step:
        rows += step_points(args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
