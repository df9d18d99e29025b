"""The softmax cross-entropy over candidate lists (include/mgcn_hip.h (16)) against the list BCE and against stock torch, in one
process: the scoring stage forward + backward with leaves x [B, dim], all_ent [N, dim], bias [N] at B = 128, dim = 200,
N in {40 943, 2 000 000}, K in {64, 512, 4096}:
    ce      _native.cand_labels + model._CandCEFn (logits, merge, finish; its plan sort included) + backward
    bce     _native.cand_labels + model._CandBCEFn + backward (the list route's other loss: three launches fewer)
    torch   _native.cand_labels, then what a user would write without (16): all_ent[cand] gathered into [B, K, dim], bmm,
            F.cross_entropy with probability targets, autograd (index_add_ with float atomics into all_ent.grad)
device microseconds per call and the peak allocation above what is resident before the call; the ce and torch losses of the
same inputs are recorded side by side. The method is tools/bench_cand_train.py's (its helpers are imported): the routes of a
point are timed in alternation, ROUNDS windows each of back-to-back calls between device events after a warm-up; the median and
the fastest window are reported. Every run APPENDS one JSON line per point to --out; run the command twice.
Usage: python tools/bench_cand_ce.py [--out FILE.json] [--rounds 7]"""
import argparse
import json
import os

import torch
import torch.nn.functional as F

from bench_cand_train import B, DIM, POINTS, dev, measure, nat, peak_bytes, pkg, query_index

EPS = 0.1


def stage_routes(x, ent, bias, cand, index, keys, N):
    hot, cold = nat.smoothed_targets(EPS, N)
    leaves = (x, ent, bias)
    K = cand.size(1)
    last = {}

    def clear():
        for t in leaves:
            t.grad = None

    def ce_route():
        clear()
        labels = nat.cand_labels(keys, index.keys, index.ptr, index.tails, cand, N)
        loss = pkg.model._CandCEFn.apply(x, ent, bias, cand, labels, EPS)
        loss.backward()
        last['ce'] = loss.detach()

    def bce_route():
        clear()
        labels = nat.cand_labels(keys, index.keys, index.ptr, index.tails, cand, N)
        pkg.model._CandBCEFn.apply(x, ent, bias, cand, labels, hot, cold).backward()

    def torch_route():
        clear()
        lab = nat.cand_labels(keys, index.keys, index.ptr, index.tails, cand, N).float()
        z = torch.bmm(ent[cand], x[:, :, None]).squeeze(2) + bias[cand]          # every id of these lists is a row of the table
        q = (1.0 - EPS) * lab / lab.sum(1, keepdim=True).clamp(min=1.0) + EPS / K
        loss = F.cross_entropy(z, q)
        loss.backward()
        last['torch'] = loss.detach()

    return {'ce': ce_route, 'bce': bce_route, 'torch': torch_route}, clear, last


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
        routes, clear, last = stage_routes(x, ent, bias, cand, index, keys, N)
        r = dict(section='stage', N=N, dim=DIM, B=B, K=K, rounds=rounds, lbl_smooth=EPS, gathered_block_bytes=K * B * DIM * 4)
        r.update(measure(routes, rounds))
        for k, fn in routes.items():
            r[k + '_peak_bytes'] = peak_bytes(fn, clear)
        r['loss_ce'], r['loss_torch'] = float(last['ce']), float(last['torch'])
        r['ce_over_bce'] = round(r['ce_us'] / r['bce_us'], 2)
        r['torch_over_ce'] = round(r['torch_us'] / r['ce_us'], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    rows = stage_points(args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
