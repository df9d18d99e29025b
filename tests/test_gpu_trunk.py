"""The HIP ConvE query trunk (csrc/conve_trunk.hip, paragraph (8) of include/mgcn_hip.h) on a real MI355X: held to the
float64 reference and the bar of tests/trunk_ref.py through the C ABI, to the goldens through the model, and to its own
promises (a row's bits do not depend on the batch, the chunking or the launch form; non-finite rows stay alone; the pack
follows the weights; the switch dispatches as documented; bad arguments are refused and nothing is written)."""
import copy
import os
import types

import numpy as np
import pytest
import torch

from . import dense_ref as R
from . import trunk_ref as T
from .conftest import FULL_CASES, GOLDEN, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = [T.case_id(c) for c in T.GRID]
EINVAL, EUNSUPPORTED = 1, 3
SMALL = (4, 8, 3, 8, False)


def pack_of(nat, case, sd):
    d = lambda k: sd[k].to(DEV).float().contiguous() if k in sd else None
    bn = lambda n: (d('conv2.%s.running_mean' % n), d('conv2.%s.running_var' % n), d('conv2.%s.weight' % n),
                    d('conv2.%s.bias' % n), T.BN_EPS)
    return nat.conve_pack(T.geometry(case), d('conv2.conv_e.weight'), d('conv2.conv_e.bias'), d('conv2.fc.weight'),
                          d('conv2.fc.bias'), bn('bn0'), bn('bn1'), bn('bn2'))


def conve_module(pkg, case, sd=None, **over):
    """A ConvE decoder of the grid case on the GPU, in eval mode, loaded with trunk_ref.weights (or `sd`)."""
    params = types.SimpleNamespace(**dict(T.hyper(case), **over))
    conv = pkg.model.ConvE(params, 10)
    sd = T.weights(case) if sd is None else sd
    res = conv.load_state_dict({k[len('conv2.'):]: v for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {'bias', 'bn0.num_batches_tracked', 'bn1.num_batches_tracked',
                                                                 'bn2.num_batches_tracked'}
    return conv.to(DEV).eval()


def module_sd(conv):
    return {'conv2.' + k: v.detach().cpu() for k, v in conv.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------- 1
PARITY = [(c, b) for c in T.GRID for b in T.BATCHES] + [(c, b) for c in T.LIMIT_GRID for b in T.LIMIT_BATCHES]


@pytest.mark.parametrize('case,B', PARITY, ids=['%s-%d' % (T.case_id(c), b) for c, b in PARITY])
def test_grid_parity_through_the_c_abi(pkg, case, B):
    """The grid, and the limits of the domain (trunk_ref.LIMIT_GRID: up to 1024 taps, one output position, F = 1 and
    F > 256), to the same bar."""
    nat = pkg._native
    geom, O = T.geometry(case), case[0] * case[1]
    assert nat.conve_supported(*geom)
    sd = T.weights(case)
    pack = pack_of(nat, case, sd)
    # (a) no index vectors: rows 0 .. B-1 of both tables, output in a guarded buffer with ldo > O
    s, r = (t.to(DEV) for t in T.queries(case, B))
    want, bar = T.ref_trunk(case, sd, s, r)
    out = R.Guarded(B, O, O + 5, DEV)
    nat.conve_trunk(geom, pack, s, None, r, None, out=out.view)
    out.check('conve_trunk ' + T.case_id(case))
    ratio = R.max_ratio(out.view, want, bar)
    err = float((out.view.double() - want).abs().max())
    print('%s B=%d: %.4f of the bar, largest |got - ref64| = %.3g' % (T.case_id(case), B, ratio, err))
    assert ratio <= 1.0
    # (b) the same queries picked out of two tables by index vectors: the same bits
    g = R.gen(R.seed_of(11, B, *geom))
    ent, rel = R.pm_uniform((57, O), g).to(DEV), R.pm_uniform((23, O), g).to(DEV)
    si, ri = torch.randint(0, 57, (B,), generator=g).to(DEV), torch.randint(0, 23, (B,), generator=g).to(DEV)
    want_i, bar_i = T.ref_trunk(case, sd, ent[si], rel[ri])
    out_i = R.Guarded(B, O, O + 3, DEV)
    nat.conve_trunk(geom, pack, ent, si, rel, ri, out=out_i.view)
    out_i.check('conve_trunk (indexed) ' + T.case_id(case))
    assert R.max_ratio(out_i.view, want_i, bar_i) <= 1.0
    assert torch.equal(out_i.view, nat.conve_trunk(geom, pack, ent[si].contiguous(), None, rel[ri].contiguous(), None))
    # (c) one segment (P <= 4): no batch has a workspace, and the call succeeds with a NULL one -- the same bits
    if T.launch_figures(case)['PQ'] == 1:
        lib = nat.lib()
        assert lib.mgcn_conve_trunk_workspace(B, *geom) == 0
        out_n = R.Guarded(B, O, O + 1, DEV)
        rc = lib.mgcn_conve_trunk_fwd(B, *geom, s.data_ptr(), O, B, None, r.data_ptr(), O, B, None, pack.data_ptr(), out_n.ptr(), O + 1,
                                      None, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mgcn_last_error()
        torch.cuda.synchronize()
        out_n.check('conve_trunk (NULL workspace) ' + T.case_id(case))
        assert torch.equal(out_n.view, out.view)


# ---------------------------------------------------------------------------------------------------------------- 2
def _loader(pkg, g, **over):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**dict(g.hp, **over))
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    return dl, params


def _model(pkg, g, **over):
    dl, params = _loader(pkg, g, **over)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    missing = model.load_state_dict(g.state_dict(), strict=False)
    assert not missing.unexpected_keys
    return model.to(DEV), dl, params


# rows whose GOLDEN margin (smallest distance from the target score to an unfiltered other score) is at most 4e-5, twice
# the score bar: fixed by the goldens alone
EXCLUDED = {'toy_small': (0, 24), 'syn_a': (1, 96), 'syn_b': (30, 160)}


@pytest.mark.parametrize('case', FULL_CASES)
def test_goldens_with_the_hip_trunk(pkg, case):
    g = golden(case)
    model, dl, params = _model(pkg, g, conve_trunk='hip')
    model.eval()
    excluded = total = 0
    for split in ('valid_tail', 'valid_head', 'test_tail', 'test_head'):
        trip = g.t('dl_q_%s_triple' % split).to(DEV)
        ds = dl._get_dataset(split, params)
        label = torch.stack([ds[i][1] for i in range(len(ds))]).to(DEV)
        with torch.no_grad():
            score = model(trip[:, 0], trip[:, 1], dl.graph)
            counts, target = model.rank_counts(trip[:, 0], trip[:, 1], trip[:, 2].contiguous(), label, dl.graph)
        ref_score = g['eval_%s_score' % split]
        print('%s %s: largest |score - golden| = %.3g' % (case, split, float(np.abs(score.cpu().numpy() - ref_score).max())))
        np.testing.assert_allclose(score.cpu().numpy(), ref_score, rtol=0, atol=2e-5)
        # rank_counts against a torch recount on the same scores
        rows = torch.arange(trip.size(0), device=DEV)
        assert torch.equal(target, score[rows, trip[:, 2]])
        masked = torch.where(label >= 1, torch.full_like(score, -1e7), score)
        masked[rows, trip[:, 2]] = target
        eq = masked == target[:, None]
        eq[rows, trip[:, 2]] = False
        idx = torch.arange(score.size(1), device=DEV)[None, :]
        assert torch.equal(counts[:, 0], (masked > target[:, None]).sum(1))
        assert torch.equal(counts[:, 2], eq.sum(1))
        assert torch.equal(counts[:, 1], (eq & (idx < trip[:, 2:3])).sum(1))
        # the reference's ranks on every row whose golden margin exceeds 4e-5
        ref, ref_t = torch.from_numpy(ref_score), torch.from_numpy(g['eval_%s_target' % split])
        gap = (ref - ref_t[:, None]).abs()
        gap[torch.arange(ref.size(0)), trip[:, 2].cpu()] = 1.0
        gap[label.cpu() >= 1] = 1.0
        safe = gap.min(1).values > 4e-5
        assert int(torch.from_numpy(g['eval_%s_ties' % split]).sum()) == 0
        ranks = (1 + counts[:, 0] + counts[:, 1]).cpu()
        assert torch.equal(ranks[safe], torch.from_numpy(g['eval_%s_ranks' % split])[safe])
        excluded += int((~safe).sum())
        total += safe.numel()
    assert (excluded, total) == EXCLUDED[case]
    assert model.conv2._pack_count == 1                       # the HIP trunk ran, on one pack
    iters = dl.get_data_loaders(g.hp['batch_size'], 0, params)
    for split in ('valid', 'test'):
        res = pkg.harness.evaluate(model, iters, dl.graph, params, split)
        assert abs(float(res['mrr']) - float(g['evaluate_%s_mrr' % split])) <= 1e-4
    assert model.conv2._pack_count == 1


# ---------------------------------------------------------------------------------------------------------------- 3
KS9 = (10, 20, 9, 32, False)


def test_rows_are_bit_identical_across_batches_chunks_and_launch_forms(pkg):
    """At the production geometry, and at the same image with ks = 9 (the generic convolution, 81 taps)."""
    assert KS9 in T.LIMIT_GRID and KS9[:2] == T.PRODUCTION[:2]
    for case in (T.PRODUCTION, KS9):
        _rows_are_bit_identical(pkg, case)


def _rows_are_bit_identical(pkg, case):
    nat = pkg._native
    geom, O = T.geometry(case), 200
    pack = pack_of(nat, case, T.weights(case))
    g = R.gen(12)
    ent, rel = R.pm_uniform((500, O), g).to(DEV), R.pm_uniform((40, O), g).to(DEV)
    Q = 1000
    si, ri = torch.randint(0, 500, (Q,), generator=g).to(DEV), torch.randint(0, 40, (Q,), generator=g).to(DEV)
    run = lambda a, b: nat.conve_trunk(geom, pack, ent, a.contiguous(), rel, b.contiguous())
    one = run(si, ri)
    assert bool(torch.isfinite(one).all()) and float(one.max()) > 0
    ws = nat.lib().mgcn_conve_trunk_workspace
    assert ws(Q, *geom) > 0 and ws(1, *geom) > 0 and ws(2048, *geom) > 0       # segments across workgroups
    # alone
    alone = torch.cat([run(si[i:i + 1], ri[i:i + 1]) for i in range(Q)])
    assert torch.equal(alone, one)
    # at another position of a shuffled batch
    perm = torch.randperm(Q, generator=g).to(DEV)
    shuffled = run(si[perm], ri[perm])
    assert torch.equal(shuffled, one[perm])
    # chunks (trunk_chunk) of 128 and of 2048, over 3 copies of the queries
    si3, ri3, one3 = si.repeat(3), ri.repeat(3), one.repeat(3, 1)
    for chunk in (128, 2048):
        got = torch.cat([run(si3[i:i + chunk], ri3[i:i + chunk]) for i in range(0, 3 * Q, chunk)])
        assert torch.equal(got, one3), chunk
    # the other launch form: a batch large enough that every wave walks all segments itself (no workspace)
    big = torch.cat([torch.randperm(Q, generator=g) for _ in range(9)]).to(DEV)
    assert ws(big.numel(), *geom) == 0
    assert torch.equal(run(si[big], ri[big]), one[big])


def test_sharded_evaluation_does_not_depend_on_the_trunk_chunk(pkg):
    g = golden('syn_c')
    model, dl, params = _model(pkg, g, conve_trunk='hip')
    model.eval()
    gen = R.gen(13)
    n, r2 = dl.num_entity, 2 * dl.num_relation
    queries = torch.stack([torch.randint(0, n, (3000,), generator=gen), torch.randint(0, r2, (3000,), generator=gen),
                           torch.randint(0, n, (3000,), generator=gen)], dim=1)
    filt = dl.filter_index().to(DEV)
    a = pkg.dist.evaluate_sharded(model, dl.graph, queries, filt, batch_size=256, trunk_chunk=128)
    b = pkg.dist.evaluate_sharded(model, dl.graph, queries, filt, batch_size=256, trunk_chunk=2048)
    assert model.conv2._pack_count == 1
    assert a['count'] == b['count'] and a['mrr'] == b['mrr'] and a['mr'] == b['mr']


# ---------------------------------------------------------------------------------------------------------------- 4
MANY_TAPS = (16, 32, 17, 4, True)


@pytest.mark.parametrize('case', [T.PRODUCTION, SMALL, MANY_TAPS], ids=[T.case_id(T.PRODUCTION), T.case_id(SMALL), T.case_id(MANY_TAPS)])
def test_non_finite_rows_stay_alone(pkg, case):
    nat = pkg._native
    geom = T.geometry(case)
    pack = pack_of(nat, case, T.weights(case))
    s, r = (t.to(DEV) for t in T.queries(case, 200))
    clean = nat.conve_trunk(geom, pack, s, None, r, None)
    s2, r2 = s.clone(), r.clone()
    s2[17, 5] = float('nan')
    r2[101, 3] = float('inf')
    got = nat.conve_trunk(geom, pack, s2, None, r2, None)
    for row in (17, 101):
        assert not bool(torch.isfinite(got[row]).all()), row
    keep = torch.ones(200, dtype=torch.bool, device=DEV)
    keep[17] = keep[101] = False
    assert torch.equal(got[keep], clean[keep])
    assert bool(torch.isfinite(clean).all())


# ---------------------------------------------------------------------------------------------------------------- 5
def test_pack_follows_the_weights(pkg):
    case = T.GRID[4]                                                       # O = 512, conv bias
    conv = conve_module(pkg, case, conve_trunk='hip')
    s, r = (t.to(DEV) for t in T.queries(case, 63))

    def check(what):
        with torch.no_grad():
            got = conv.trunk(s, r)
        want, bar = T.ref_trunk(case, module_sd(conv), s, r)
        assert R.max_ratio(got, want, bar) <= 1.0, what
        return got

    y0 = check('first')
    ptr, count = conv._pack.data_ptr(), conv._pack_count
    assert count == 1
    assert torch.equal(check('unchanged'), y0)
    assert (conv._pack.data_ptr(), conv._pack_count) == (ptr, 1)           # same buffer, no pack launch
    with torch.no_grad():
        conv.bn1.running_var.mul_(1.7)                                     # in place
    y1 = check('bn1.running_var')
    assert not torch.equal(y1, y0) and (conv._pack.data_ptr(), conv._pack_count) == (ptr, 2)
    opt = torch.optim.SGD([conv.fc.weight], lr=0.05)
    conv.fc.weight.grad = R.pm_uniform(tuple(conv.fc.weight.shape), R.gen(14)).to(DEV)
    opt.step()
    y2 = check('optimizer step')
    assert not torch.equal(y2, y1) and (conv._pack.data_ptr(), conv._pack_count) == (ptr, 3)
    conv.load_state_dict({k[len('conv2.'):]: v for k, v in T.weights(case, seed=1).items()}, strict=False)
    y3 = check('load_state_dict')
    assert not torch.equal(y3, y2) and conv._pack.data_ptr() == ptr and conv._pack_count == 4
    assert torch.equal(check('unchanged again'), y3) and conv._pack_count == 4


# ---------------------------------------------------------------------------------------------------------------- 6
def test_dispatch(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_TRUNK', raising=False)
    case = SMALL
    s, r = (t.to(DEV) for t in T.queries(case, 40))
    on, off = conve_module(pkg, case, conve_trunk='hip'), conve_module(pkg, case)
    taken = lambda m: getattr(m, '_pack_count', 0)
    with torch.no_grad():
        y_off, y_on = off.trunk(s, r), on.trunk(s, r)
    assert taken(on) == 1 and taken(off) == 0                              # the stated case, and only with the switch
    assert float((y_on - y_off).abs().max()) <= 2e-5
    # the parent's path with the switch off: today's code on today's modules
    with torch.no_grad():
        x = torch.cat([s.view(-1, 1, 32), r.view(-1, 1, 32)], dim=1).transpose(2, 1).reshape(-1, 1, 8, 8)
        x = torch.relu(off.bn1(off.conv_e(off.bn0(x))))
        parent = torch.relu(off.bn2(off.fc(x.view(-1, off.flat_sz)))).contiguous()
    assert torch.equal(y_off, parent)
    # grad mode on: torch
    assert torch.equal(on.trunk(s, r).detach(), off.trunk(s, r).detach()) and taken(on) == 1
    # training mode: torch (same dropout masks from the same seed, same running-statistics updates)
    a, b = copy.deepcopy(on).train(), copy.deepcopy(off).train()
    outs = []
    for m in (a, b):
        torch.manual_seed(5)
        outs.append(m.trunk(s, r))
    assert torch.equal(outs[0], outs[1]) and torch.equal(a.bn1.running_var, b.bn1.running_var) and taken(a) == 1
    with torch.no_grad():                                                  # ... also with grad mode off
        outs = []
        for m in (a, b):
            torch.manual_seed(6)
            outs.append(m.trunk(s, r))
    assert torch.equal(outs[0], outs[1]) and taken(a) == 1
    # trunk_indexed: the gather inside the kernel gives the rows of index_select + trunk
    g = R.gen(15)
    ent, rel = R.pm_uniform((30, 32), g).to(DEV), R.pm_uniform((12, 32), g).to(DEV)
    si, ri = torch.randint(0, 30, (40,), generator=g).to(DEV), torch.randint(0, 12, (40,), generator=g).to(DEV)
    with torch.no_grad():
        assert torch.equal(on.trunk_indexed(ent, si, rel, ri), on.trunk(ent[si], rel[ri]))
        assert torch.equal(off.trunk_indexed(ent, si, rel, ri), off.trunk(ent.index_select(0, si), rel.index_select(0, ri)))
    # the environment variable overrides params in both directions
    with torch.no_grad():
        monkeypatch.setenv('MGCN_TRUNK', 'hip')
        assert torch.equal(off.trunk(s, r), y_on) and taken(off) == 1
        monkeypatch.setenv('MGCN_TRUNK', 'torch')
        before = taken(on)
        assert torch.equal(on.trunk(s, r), y_off) and taken(on) == before
    monkeypatch.delenv('MGCN_TRUNK')
    # a geometry the kernel does not take (O = 1024) falls back without raising
    wide = (32, 32, 3, 2, False)
    assert not pkg._native.conve_supported(*T.geometry(wide))
    sd = T.weights(wide)
    w_on, w_off = conve_module(pkg, wide, sd=sd, conve_trunk='hip'), conve_module(pkg, wide, sd=sd)
    sw, rw = (t.to(DEV) for t in T.queries(wide, 9))
    with torch.no_grad():
        assert torch.equal(w_on.trunk(sw, rw), w_off.trunk(sw, rw)) and taken(w_on) == 0


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_write_nothing(pkg):
    nat = pkg._native
    lib = nat.lib()
    case, B = SMALL, 5
    geom, O = T.geometry(case), 32
    pack = pack_of(nat, case, T.weights(case))
    s, r = (t.to(DEV) for t in T.queries(case, B))
    out = R.Guarded(B, O, O + 4, DEV)
    nbytes = lib.mgcn_conve_trunk_workspace(B, *geom)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(batch=B, geom=geom, ent=s.data_ptr(), rel=r.data_ptr(), packed=pack.data_ptr(), dst=out.ptr(), wsp=ws.data_ptr(),
             ws_bytes=nbytes, rows=B):
        return lib.mgcn_conve_trunk_fwd(batch, *geom, ent, O, rows, None, rel, O, rows, None, packed, dst, O + 4, wsp, ws_bytes, stream)

    k_w, k_h, ks, f, o = geom
    bad = [('null ent', dict(ent=None)), ('null rel', dict(rel=None)), ('null pack', dict(packed=None)), ('null out', dict(dst=None)),
           ('null workspace', dict(wsp=None)), ('k_w k_h != O', dict(geom=(k_w, k_h, ks, f, o + 1))),
           ('kernel too large', dict(geom=(k_w, k_h, k_h + 1, f, o))), ('kernel 0', dict(geom=(k_w, k_h, 0, f, o))),
           ('no filters', dict(geom=(k_w, k_h, ks, 0, o))), ('negative batch', dict(batch=-1)),
           ('workspace one byte short', dict(ws_bytes=nbytes - 1)), ('fewer rows than queries', dict(rows=B - 1))]
    for what, kw in bad:
        assert call(**kw) == EINVAL, what
        assert lib.mgcn_last_error()
    assert call(geom=(32, 32, 3, 2, 1024)) == EUNSUPPORTED
    assert lib.mgcn_conve_packed_bytes(32, 32, 3, 2, 1024) == 0 and lib.mgcn_conve_packed_bytes(k_w, k_h, ks, f, o + 1) == 0
    assert lib.mgcn_conve_pack(k_w, k_h, k_h + 1, f, o, *([None] * 2), None, 0, None, *([None] * 4 + [1e-5]) * 3, None, 0, stream) == EINVAL
    assert call(batch=0, wsp=None, ws_bytes=0) == 0                                      # a no-op
    torch.cuda.synchronize()
    assert out.untouched()
    assert call() == 0                                                                   # and the good call works
    torch.cuda.synchronize()
    out.check('conve_trunk_fwd')
    want, bar = T.ref_trunk(case, T.weights(case), s, r)
    assert R.max_ratio(out.view, want, bar) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 8
def test_integration_stub_from_encoder_output_to_scores(pkg):
    """The second ctypes block of INTEGRATION.md section 2, executed after the first: encoder output -> scores through the C ABI
    alone, bit for bit the model's scores with the HIP trunk."""
    import re
    text = open(os.path.join(os.path.dirname(GOLDEN), '..', 'INTEGRATION.md')).read()
    blocks = re.findall(r"```python\n(.*?)```", text[text.index('## 2. Operator level'):text.index('## 3. Multi-GPU')], re.S)
    assert len(blocks) == 2
    ns = {}
    for block in blocks:
        exec(block.replace("'kgc-gcn_amd/csrc/libmgcn_hip.so'", repr(pkg._native.LIB_PATH)), ns)
    g = golden('syn_b')
    model, dl, params = _model(pkg, g, conve_trunk='hip')
    model.eval()
    trip = g.t('dl_q_test_tail_triple').to(DEV)
    with torch.no_grad():
        want = model(trip[:, 0], trip[:, 1], dl.graph)
        all_ent, all_rel = model.encode(dl.graph)
        geom = (params.k_w, params.k_h, params.kernel_size, params.num_filter, params.gcn_out_dim)
        packed = ns['pack_trunk'](model.conv2, geom)
        got = ns['query_scores'](all_ent.contiguous(), all_rel.contiguous(), trip[:, 0].contiguous(), trip[:, 1].contiguous(),
                                 packed, geom, model.conv2.bias)
    assert torch.equal(got, want)
