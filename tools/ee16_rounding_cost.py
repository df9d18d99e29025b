"""What rounding the per-edge tables to bf16 costs a model, on the golden fixtures:

    python tools/ee16_rounding_cost.py [--out profiles/ee16_rounding_cost.json]

For toy_small, syn_a, syn_b and syn_c (tests/golden: the fixtures' own graphs, weights and evaluation queries) the f32 model
and the bf16 model loaded from the same state dict score every valid / test query in both directions: the largest score
difference, how many filtered ranks change, and the MRR of both. The fixtures' weights are UNTRAINED (seeded initial values), so
this is the effect of the rounding on those scores only; what it does to a trained model's metrics is not measured here."""
import argparse
import importlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.conftest import GOLDEN, golden  # noqa: E402

DEV = 'cuda:0'
CASES = ['toy_small', 'syn_a', 'syn_b', 'syn_c']
SPLITS = ('valid_tail', 'valid_head', 'test_tail', 'test_head')


def model_for(pkg, g, **over):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**dict(g.hp, **over))
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    model.load_state_dict(g.state_dict(), strict=False)
    return model.to(DEV).eval(), dl, params


def case_report(pkg, name):
    g = golden(name)
    layers = 1 + sum(1 for k in g.state_dict() if k.startswith('edge_embeddings_extra.'))
    m32, dl, params = model_for(pkg, g, gcn_layers=layers)
    m16, dl16, _ = model_for(pkg, g, gcn_layers=layers, edge_table_dtype='bf16')
    assert m16.edge_embeddings.dtype == torch.bfloat16
    worst, changed, total, rr32, rr16 = 0.0, 0, 0, 0.0, 0.0
    for split in SPLITS:
        trip = g.t('dl_q_%s_triple' % split).to(DEV)
        ds = dl._get_dataset(split, params)
        label = torch.stack([ds[i][1] for i in range(len(ds))]).to(DEV)
        with torch.no_grad():
            s32, s16 = m32(trip[:, 0], trip[:, 1], dl.graph), m16(trip[:, 0], trip[:, 1], dl16.graph)
            c32, _ = m32.rank_counts(trip[:, 0], trip[:, 1], trip[:, 2].contiguous(), label, dl.graph)
            c16, _ = m16.rank_counts(trip[:, 0], trip[:, 1], trip[:, 2].contiguous(), label, dl16.graph)
        k32, k16 = 1 + c32[:, 0] + c32[:, 1], 1 + c16[:, 0] + c16[:, 1]        # filtered rank under the stable tie rule
        worst = max(worst, float((s32 - s16).abs().max()))
        changed += int((k32 != k16).sum())
        total += int(trip.size(0))
        rr32 += float((1.0 / k32.double()).sum())
        rr16 += float((1.0 / k16.double()).sum())
    pkg._native.check_fused_status(DEV)
    return {'queries': total, 'layers': layers, 'largest_score_difference': worst, 'ranks_changed': changed,
            'mrr_f32': rr32 / total, 'mrr_bf16': rr16 / total, 'mrr_difference': rr16 / total - rr32 / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ee16_rounding_cost.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ee16_rounding_cost: the models run on a GPU only')
    os.environ.pop('MGCN_EE', None)
    pkg = importlib.import_module('kgc-gcn_amd')
    result = {'note': 'golden fixtures, UNTRAINED weights; the effect on a trained model is not measured', 'cases': {}}
    for name in CASES:
        result['cases'][name] = case_report(pkg, name)
    with open(args.out, 'w') as f:
        f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
