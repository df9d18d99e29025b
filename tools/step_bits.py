"""The bits of a few training steps, for comparing two commits whose launches should be the same: on a synthetic graph of 300
entities, with fixed seeds, params.dropout = 'counter', the HIP trunk and query path and ClipAdam, three steps each of
    forward_loss                    MGCN.forward_loss + backward + clip_and_step
    cand_bce                        MGCN.forward_loss_candidates(loss='bce'), labels looked up in the index
    cand_softmax_logq               MGCN.forward_loss_candidates(loss='softmax', logq=...) on lists drawn by entity weight
    sharded                         dist.train_step_sharded with one rank
    sharded_cand_bce                dist.train_step_sharded_candidates(loss='bce') with one rank
    sharded_cand_softmax_logq       dist.train_step_sharded_candidates(loss='softmax', logq=...) with one rank
every form on a model of its own built from the same seed. After each step one line per form with the loss's bits and a
position-weighted checksum of the bits of every entry of state_dict() (parameters and BN buffers). The kernels have a fixed
summation order and no float atomics, so two runs print the same text, and so do two commits that launch the same kernels on the
same operands: diff the outputs. For another commit, copy this file into a checkout of it and point MGCN_LIB at one built library.

    python tools/step_bits.py > bits.txt"""
import importlib
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the graph generator)

SHAPE = dict(N=300, R=5, E=1500)
B, K, STEPS, SEED, SMOOTH, CLIP = 128, 33, 3, 1234, 0.1, 1.0
FORMS = ('forward_loss', 'cand_bce', 'cand_softmax_logq', 'sharded', 'sharded_cand_bce', 'sharded_cand_softmax_logq')


def build(pkg, dev):
    N, R, E = SHAPE['N'], SHAPE['R'], SHAPE['E']
    params = types.SimpleNamespace(gcn_in_dim=100, gcn_out_dim=200, gcn_drop=0.3, hidden_drop=0.3, feat_drop=0.3, k_w=10, k_h=20,
                                   num_filter=200, kernel_size=7, bias=False, lbl_smooth=SMOOTH, gcn_layers=2, clip_grad=CLIP, device=dev,
                                   dropout='counter', dropout_seed=7, conve_trunk_train='hip', query_path_train='hip')
    edge_index, edge_attr = bench.synth_graph(SHAPE, seed=0)
    graph = pkg.Graph(edge_index=edge_index, edge_attr=edge_attr)
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    graph.to(dev)
    torch.manual_seed(0)
    model = pkg.MGCN(N, R, E, params).to(dev).train()
    return model, graph, pkg.ClipAdam(model.parameters(), lr=1e-3)


def batches_and_index(pkg, dev):
    N, R = SHAPE['N'], SHAPE['R']
    g = torch.Generator().manual_seed(2)
    qs = [torch.stack([torch.randint(0, N, (B,), generator=g), torch.randint(0, 2 * R, (B,), generator=g)], 1) for _ in range(STEPS)]
    known = {}
    for q in qs:
        for (s, r), ts in zip(q.tolist(), torch.randint(0, N, (B, 4), generator=g).tolist()):
            known.setdefault((s, r), set()).update(ts)
    return [q.to(dev) for q in qs], pkg.dist.FilterIndex.from_known(known, 2 * R).to(dev)


def checksum(model):
    total = 0
    for name, t in model.state_dict().items():
        v = t.detach().reshape(-1)
        v = (v.view(torch.int32) if v.dtype == torch.float32 else v).to(torch.int64)
        w = torch.arange(v.numel(), device=v.device) % 65521 + 1
        total = (total * 1000003 + int((v * w).sum().item())) & 0xffffffffffffffff
    return total


def main():
    pkg = importlib.import_module('kgc-gcn_amd')
    dev = torch.device('cuda', 0)
    N = SHAPE['N']
    qs, index = batches_and_index(pkg, dev)
    sampler = pkg.NegativeSampler.from_degrees(index=index, num_entities=N).to(dev)
    for form in FORMS:
        model, graph, opt = build(pkg, dev)
        for k, q in enumerate(qs):
            src, rel = q[:, 0], q[:, 1]
            weighted = form.endswith('logq')
            kind = 'softmax' if weighted else 'bce'
            if 'cand' in form:
                cand, labels = pkg.harness.draw_candidates(q, index, N, K - 1, SEED, k, labels=True, sampler=sampler if weighted else None)
                labels, logq = (labels, sampler.logq) if weighted else (None, None)      # bce: the labels are looked up in the index
            if form == 'sharded':
                loss = pkg.dist.train_step_sharded(model, graph, src, rel, index, opt, lbl_smooth=SMOOTH, clip=CLIP)
            elif form.startswith('sharded'):
                loss = pkg.dist.train_step_sharded_candidates(model, graph, src, rel, cand, index, opt, labels=labels, lbl_smooth=SMOOTH,
                                                              clip=CLIP, loss=kind, logq=logq)
            else:
                opt.zero_grad()
                if form == 'forward_loss':
                    loss = model.forward_loss(src, rel, graph, index, lbl_smooth=SMOOTH)
                else:
                    loss = model.forward_loss_candidates(src, rel, cand, graph, index=None if weighted else index, labels=labels,
                                                         lbl_smooth=SMOOTH, loss=kind, logq=logq)
                loss.backward()
                opt.clip_and_step(CLIP)
                loss = loss.detach()
            bits = int(loss.view(torch.int32).item()) & 0xffffffff
            print('%-26s step %d  loss %08x (%.6f)  state %016x' % (form, k, bits, float(loss), checksum(model)), flush=True)
            if not torch.isfinite(loss):
                raise SystemExit('%s: the loss is not finite' % form)


if __name__ == '__main__':
    main()
