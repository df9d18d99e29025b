"""Edge dropout and own-triple removal: what this step's records cost. In one process, the routes alternating
window by window, the median of --windows windows, the whole measurement --runs times:

  (a) the rewrite alone on the WN18RR-shape graph: mgcn_edge_drop_records at p = 0.2 without flags, and the zero fill + the flags
      kernel of a batch + the rewrite with them; --calls calls per window, host clock around a window that ends in a synchronise;
  (b) the WN18RR-shape eager training step (1 layer, counter dropout 0.3, HIP trunk and query path, ClipAdam) at each batch size
      with the switches off, with edge_drop = 0.2, and with edge_drop = 0.2 + edge_drop_queries; --steps steps per window.

The yardstick of "switches off" is the parent commit in the same session: run this file with --root <checkout of the parent, its
library built> --routes off (a tree without the switches ignores them) and compare the two `off` lines.

    python tools/bench_edge_drop.py [--root DIR] [--routes off p02 p02_queries] [--batches 128 1024] [--out profiles/bench_edge_drop.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = dict(k_w=10, k_h=20, kernel_size=7, num_filter=200, gcn_out_dim=200, bias=False)
ROUTES = {'off': (0.0, False), 'p02': (0.2, False), 'p02_queries': (0.2, True)}


def windows(fns, n_windows, per_window, warmup):
    """{name: [ms per call, one entry per window]}: the callables alternate window by window; a window is `per_window` calls
    between two synchronises on the host clock."""
    out = {k: [] for k in fns}
    for w in range(warmup + n_windows):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_window):
                fn()
            torch.cuda.synchronize()
            if w >= warmup:
                out[name].append((time.perf_counter() - t0) * 1e3 / per_window)
    return out


def graph_and_batch(pkg, bench, dev, B):
    shape = bench.SHAPES['wn18rr']
    n, R, E = shape['N'], shape['R'], shape['E']
    edge_index, edge_attr = bench.synth_graph(shape, seed=0)
    # the batch's queries are edges of the graph, as a training batch's are: their edges exist and are removed
    g = torch.Generator().manual_seed(2)
    pick = torch.randint(0, 2 * E, (B,), generator=g)
    trip = torch.stack([edge_index[0, pick], edge_attr[0, pick]], 1).to(dev)
    known = {}
    for (s_, r_), o_ in zip(trip.tolist(), edge_index[1, pick].tolist()):
        known.setdefault((s_, r_), set()).add(int(o_))
    index = pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)
    return shape, edge_index, edge_attr, trip, index


def make_graph(pkg, shape, edge_index, edge_attr, dev):
    graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(shape['N']), shape['N'], None
    return graph.to(dev)


def rewrite_alone(pkg, bench, dev, B):
    nat = pkg._native
    shape, edge_index, edge_attr, trip, _ = graph_and_batch(pkg, bench, dev, B)
    csr = make_graph(pkg, shape, edge_index, edge_attr, dev).csr(2 * shape['R'] + 1)
    st = csr.edge_drop_state()
    qkey = trip[:, 0] * (2 * shape['R']) + trip[:, 1]
    step = [0]

    def plain():
        step[0] += 1
        return nat.edge_drop_records(csr, st, nat.dropout_key(1, step[0], nat.EDGE_DROP_SITE), 0.2)

    def with_flags():
        step[0] += 1
        forced = nat.edge_flags_from_queries(qkey, st, csr.num_edges_half)
        return nat.edge_drop_records(csr, st, nat.dropout_key(1, step[0], nat.EDGE_DROP_SITE), 0.2, forced)

    return {'rewrite': plain, 'flags_and_rewrite': with_flags}, 2 * csr.num_edges_half, st.max_run


def step_routes(pkg, bench, dev, B, routes):
    shape, edge_index, edge_attr, trip, index = graph_and_batch(pkg, bench, dev, B)
    fns = {}
    for name in routes:
        p, by_queries = ROUTES[name]
        params = types.SimpleNamespace(gcn_in_dim=100, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, lbl_smooth=0.1, gcn_layers=1, clip_grad=1.0,
                                       device=dev, dropout='counter', conve_trunk_train='hip', query_path_train='hip', edge_drop=p,
                                       edge_drop_queries=by_queries, **GEOM)
        graph = make_graph(pkg, shape, edge_index, edge_attr, dev)
        torch.manual_seed(0)
        model = pkg.MGCN(shape['N'], shape['R'], shape['E'], params).to(dev).train()
        opt = pkg.ClipAdam(model.parameters(), lr=1e-3)

        def run(model=model, opt=opt, graph=graph):
            opt.zero_grad()
            loss = model.forward_loss(trip[:, 0], trip[:, 1], graph, index, lbl_smooth=0.1)
            loss.backward()
            opt.clip_and_step(1.0)
        fns[name] = run
    return fns


def summary(times):
    return {k: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=HERE, help='the checkout whose package and bench.py are measured')
    ap.add_argument('--routes', nargs='+', default=list(ROUTES), choices=list(ROUTES))
    ap.add_argument('--batches', type=int, nargs='+', default=[128, 1024])
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--steps', type=int, default=20, help='training steps per window')
    ap.add_argument('--calls', type=int, default=200, help='rewrite calls per window')
    ap.add_argument('--warmup', type=int, default=1, help='untimed windows per route')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'bench_edge_drop.json'), help='the JSON lines are written to this file as well')
    args = ap.parse_args()
    for name in ('MGCN_EDGE_DROP', 'MGCN_EDGE_DROP_QUERIES', 'MGCN_DROPOUT'):      # the routes are chosen by the params
        os.environ.pop(name, None)
    sys.path.insert(0, os.path.abspath(args.root))
    bench = importlib.import_module('bench')
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    lines = []
    for run in range(args.runs):
        if hasattr(pkg._native, 'edge_drop_records') and set(args.routes) != {'off'}:
            fns, slots, max_run = rewrite_alone(pkg, bench, dev, args.batches[0])
            lines.append(dict(what='rewrite_alone_wn18rr', run=run, slots=slots, max_run=max_run, batch=args.batches[0], calls_per_window=args.calls,
                              windows=args.windows, record_bytes=2 * 16 * slots, **summary(windows(fns, args.windows, args.calls, args.warmup))))
        for B in args.batches:
            fns = step_routes(pkg, bench, dev, B, args.routes)
            lines.append(dict(what='train_step_wn18rr_1layer', run=run, batch=B, steps_per_window=args.steps, windows=args.windows,
                              root=os.path.relpath(os.path.abspath(args.root), HERE), **summary(windows(fns, args.windows, args.steps, args.warmup))))
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
