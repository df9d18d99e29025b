"""The layer launches on an f32 per-edge table and on its bf16 form, alternating in ONE process on one GPU:

    python tools/bench_ee16.py [--out profiles/bench_ee16.json] [--reps 20] [--shapes wn18rr,fb15k237]

Per shape (bench.py's synthetic WN18RR and FB15k-237 graphs, two layers 100 -> 200 -> 200) two eval-mode models stay resident:
the bf16 model (params.edge_table_dtype = 'bf16') and an f32 model whose tables hold the same, rounded values — the yardstick:
the f32 path is the parent's code unchanged. Every launch pair is checked to give bit-identical rows before it is timed. Each
layer's fused launch is timed with device events, f32 and bf16 alternating, median of --reps after warm-up; so is the whole
encoder step (MGCN.encode, replayed from its captured graph). The command measures everything TWICE ("runs") so that the spread
of a repeated measurement stands beside every difference. Also reported: the tables' bytes and the device memory each resident
model allocates. Recorded, not asserted."""
import argparse
import importlib
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the shapes and the synthetic graphs of the flagship benchmark)

DEV = 'cuda:0'


def build_models(pkg, shape_name, D, O):
    shape = bench.SHAPES[shape_name]
    zipf = 1.1 if shape_name == 'fb15k237' else 0.0
    alloc0 = torch.cuda.memory_allocated(DEV)
    m32, graph, params, _, _ = bench.make_model(pkg, shape, DEV, 2, 0, zipf, D=D, O=O)
    p16 = types.SimpleNamespace(**dict(vars(params), edge_table_dtype='bf16'))
    m16 = pkg.MGCN(shape['N'], shape['R'], shape['E'], p16)
    sd = {k: v.detach().cpu() for k, v in m32.state_dict().items()}
    m16.load_state_dict(sd)                                                  # rounds the tables
    alloc1 = torch.cuda.memory_allocated(DEV)                                # graph + the f32 model
    m16.to(DEV).eval()
    alloc2 = torch.cuda.memory_allocated(DEV)
    with torch.no_grad():                                                    # the yardstick's tables: the rounded values, as f32
        for (_, a), (_, b) in zip(m32._edge_tables(), m16._edge_tables()):
            a.data.copy_(b.data.float())
    tables = lambda m: sum(p.numel() * p.element_size() for _, p in m._edge_tables())
    params_bytes = lambda m: sum(p.numel() * p.element_size() for p in m.parameters())
    mem = {'table_bytes_f32': tables(m32), 'table_bytes_bf16': tables(m16), 'parameter_bytes_f32': params_bytes(m32),
           'parameter_bytes_bf16': params_bytes(m16), 'allocated_bytes_bf16_model': alloc2 - alloc1,
           'allocated_bytes_graph_plus_f32_model': alloc1 - alloc0}
    return m32, m16, graph, mem


def layer_launchers(pkg, model, graph, csr):
    """One closure per layer that launches it as MGCNConv.forward does in eval mode; the inputs are the previous layer's rows."""
    nat = pkg._native
    out = []
    with torch.no_grad():
        x, rel = model.entity_embedding.detach(), model.relation_embedding.detach()
        for layer, (_, table) in zip([model.conv1] + list(model.conv1_extra), model._edge_tables()):
            bn = layer.ent_bn
            rows = torch.empty((x.size(0), layer.out_channels), device=DEV)
            rel_out = torch.empty((rel.size(0), layer.out_channels), device=DEV)
            args = (csr, x.contiguous(), rel.contiguous(), layer.loop_rel.reshape(-1), table.detach(), True, layer.loop_edge.reshape(-1),
                    layer.derived_weights()[1], layer.out_channels, layer.bias, bn.running_mean, bn.running_var, bn.weight, bn.bias,
                    bn.eps, rows)
            kw = dict(rels_weight=layer.rels_weight.detach().contiguous(), rel_out=rel_out)
            fn = (lambda a, k: lambda: nat.layer_fwd_fused(*a, **k))(args, kw)
            fn()
            out.append((fn, rows, rel_out))
            x, rel = rows, rel_out
    return out


def alternate(fa, fb, reps, warmup=10):
    """Median device time (us) of fa and of fb, launched alternately."""
    ta, tb = [], []
    for i in range(warmup + reps):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                acc.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def measure(pkg, shape_name, reps, D=100, O=200):
    nat = pkg._native
    m32, m16, graph, mem = build_models(pkg, shape_name, D, O)
    with torch.no_grad():
        e32, r32 = m32.encode(graph)
        e16, r16 = m16.encode(graph)
        same = bool(torch.equal(e32, e16) and torch.equal(r32, r16))
    csr = graph.csr(m32.relation_embedding.size(0) + 1)
    l32, l16 = layer_launchers(pkg, m32, graph, csr), layer_launchers(pkg, m16, graph, csr)
    same = same and all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(l32, l16)) and \
        bool(torch.equal(l32[-1][1], e32))
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    res = {'shape': dict(bench.SHAPES[shape_name], D=D, O=O, layers=2), 'bit_identical_rows': same, 'memory': mem, 'runs': []}
    dims = [D, O]
    res['kernel_generation'] = [int(nat.lib().mgcn_fused_kernel_generation(dims[i], O, csr.num_nodes, int(
        csr.workgroup_bounds(0, csr.num_nodes, cus) is not None))) for i in range(2)]

    def step(m):
        def run():
            with torch.no_grad():
                m.encode(graph)
        return run
    for m in (m32, m16):
        m.params.cache_encoder = False
    for _ in range(2):
        run = {'layer_us': []}
        for (fa, _, _), (fb, _, _) in zip(l32, l16):
            a, b = alternate(fa, fb, reps)
            run['layer_us'].append({'f32': round(a, 2), 'bf16': round(b, 2), 'bf16_over_f32': round(b / a, 4)})
        a, b = alternate(step(m32), step(m16), reps)
        run['encode_step_us'] = {'f32': round(a, 2), 'bf16': round(b, 2), 'bf16_over_f32': round(b / a, 4)}
        res['runs'].append(run)
    nat.check_fused_status(DEV)
    del m32, m16, graph, l32, l16
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_ee16.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shapes', default='wn18rr,fb15k237')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ee16: no GPU; nothing is measured without one')
    os.environ.pop('MGCN_EE', None)
    pkg = importlib.import_module('kgc-gcn_amd')
    result = {'device': torch.cuda.get_device_name(0), 'reps': args.reps,
              'method': 'device events around one launch (layer) or one captured-graph replay (encode step); f32 and bf16 launches '
                        'alternate; median of reps after 10 warm-up pairs; two runs in one process',
              'shapes': {}}
    for name in args.shapes.split(','):
        result['shapes'][name] = measure(pkg, name, args.reps)
    text = json.dumps(result, indent=1)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
