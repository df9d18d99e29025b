"""The softmax cross-entropy over the full entity table (include/mgcn_hip.h (20)) against the table BCE and against stock torch,
in one process.
  stage   the scoring stage forward + backward with leaves x [B, dim], all_ent [N, dim], bias [N] at dim = 200,
          B in {128, 1024}, N in {40 943, 2 000 000}:
            ce      _native.filter_mask + autograd._ScoreCEFn (logits, merge over tiles, finish) + backward
            bce     _native.filter_mask + autograd._ScoreBCEFn + backward (one launch; the ce stage is this plus one more pass
                    over [N, B] and a merge)
            torch   what a user would write without (20): _native.label_rows for the [B, N] 0/1 block, soft targets
                    (1 - eps) y / n_pos + eps / N, x @ all_ent.T + bias, F.cross_entropy with probability targets, autograd
          device microseconds per call and the peak allocation above what is resident before the call; the ce and torch losses
          of the same inputs are recorded side by side;
  step    one whole eager training step at the WN18RR shape (encoder, query rows, trunk, loss, backward, ClipAdam), B = 128, under
          loss='bce' and loss='softmax'.
The method is tools/bench_cand_train.py's (its helpers are imported): the routes of a point are timed in alternation, ROUNDS
windows each of back-to-back calls between device events after a warm-up; the median and the fastest window are reported. The
windows hold Python's enqueueing too: where a route's launches are shorter than the time Python needs to enqueue them (the
N = 40 943 points, the whole step), the figure is Python's enqueue rate and not kernel time; the kernels' own times are NOT
MEASURED here. Every run APPENDS one JSON line per point to --out; run the command twice.
Usage: python tools/bench_table_ce.py [--out FILE.json] [--rounds 7] [--no-step]"""
import argparse
import json
import os
import types

import torch
import torch.nn.functional as F

from bench_cand_train import DIM, bench, dev, measure, nat, peak_bytes, pkg

EPS = 0.1
POINTS = [(40943, 128), (40943, 1024), (2000000, 128), (2000000, 1024)]


def query_index(N, B, g):
    """B queries with four known tails each (keys 0 .. B - 1)."""
    known = {(b, 0): set(torch.randint(0, N, (4,), generator=g).tolist()) for b in range(B)}
    index = pkg.dist.FilterIndex.from_known(known, 1).to(dev)
    keys = index.query_keys(torch.arange(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
    return index, keys


def stage_routes(x, ent, bias, index, keys, N):
    hot, cold = nat.smoothed_targets(EPS, N)
    leaves = (x, ent, bias)
    last = {}

    def clear():
        for t in leaves:
            t.grad = None

    def ce_route():
        clear()
        mask = nat.filter_mask(keys, index.keys, index.ptr, index.tails, N)
        loss = pkg.autograd._ScoreCEFn.apply(x, ent, bias, mask, EPS)
        loss.backward()
        last['ce'] = loss.detach()

    def bce_route():
        clear()
        mask = nat.filter_mask(keys, index.keys, index.ptr, index.tails, N)
        pkg.autograd._ScoreBCEFn.apply(x, ent, bias, mask, hot, cold).backward()

    def torch_route():
        clear()
        y = nat.label_rows(keys, index.keys, index.ptr, index.tails, N)
        q = (1.0 - EPS) * y / y.sum(1, keepdim=True).clamp(min=1.0) + EPS / N
        loss = F.cross_entropy(x @ ent.t() + bias, q)
        loss.backward()
        last['torch'] = loss.detach()

    return {'ce': ce_route, 'bce': bce_route, 'torch': torch_route}, clear, last


def stage_points(rounds):
    rows = []
    g = torch.Generator().manual_seed(0)
    gd = torch.Generator(device=dev).manual_seed(0)
    table = {}
    for N, B in POINTS:
        if N not in table:
            table.clear()                                    # one table resident at a time
            torch.cuda.empty_cache()
            table[N] = ((torch.randn(N, DIM, device=dev, generator=gd) * 0.1).requires_grad_(True),
                        (torch.randn(N, device=dev, generator=gd) * 0.2).requires_grad_(True))
        ent, bias = table[N]
        index, keys = query_index(N, B, g)
        x = (torch.randn(B, DIM, device=dev, generator=gd) * 0.3).requires_grad_(True)
        routes, clear, last = stage_routes(x, ent, bias, index, keys, N)
        r = dict(section='stage', N=N, dim=DIM, B=B, rounds=rounds, lbl_smooth=EPS, block_bytes=B * N * 4)
        r.update(measure(routes, rounds))
        for k, fn in routes.items():
            r[k + '_peak_bytes'] = peak_bytes(fn, clear)
        r['loss_ce'], r['loss_torch'] = float(last['ce']), float(last['torch'])
        r['ce_over_bce'] = round(r['ce_us'] / r['bce_us'], 2)
        r['torch_over_ce'] = round(r['torch_us'] / r['ce_us'], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del routes, clear, x
        torch.cuda.empty_cache()
    return rows


def step_points(rounds, B=128):
    shape = bench.SHAPES['wn18rr']
    N, R, E = shape['N'], shape['R'], shape['E']
    params = types.SimpleNamespace(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20,
                                   num_filter=200, kernel_size=7, bias=False, lbl_smooth=EPS, gcn_layers=1, clip_grad=1.0, device=dev,
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
    last = {}

    def step(kind):
        opt.zero_grad()
        loss = model.forward_loss(q[:, 0], q[:, 1], graph, index, lbl_smooth=EPS, loss=kind)
        loss.backward()
        opt.clip_and_step(params.clip_grad)
        last[kind] = loss.detach()

    routes = {'bce': lambda: step('bce'), 'ce': lambda: step('softmax')}
    r = dict(section='step', shape='wn18rr', N=N, dim=DIM, B=B, rounds=rounds, layers=1,
             note='eager step, every HIP switch on, counter dropout, ClipAdam; both losses train the same model in alternation')
    r.update(measure(routes, rounds))
    clear = lambda: opt.zero_grad(set_to_none=True)   # noqa: E731
    r['bce_peak_bytes'], r['ce_peak_bytes'] = peak_bytes(routes['bce'], clear), peak_bytes(routes['ce'], clear)
    r['loss_bce'], r['loss_ce'] = float(last['bce']), float(last['softmax'])
    r['ce_over_bce'] = round(r['ce_us'] / r['bce_us'], 3)
    print(json.dumps(r), flush=True)
    return [r]


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
