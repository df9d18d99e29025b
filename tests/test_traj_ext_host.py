"""CPU-only tests of the extended trajectory fixtures (tests/golden/traj_syn_a_{C,D,E,F}.npz) and of their float64 restatement
(tests/traj_ext_ref.py): (a) with every switch off the restatement is traj_ref.run, and its two list losses are the float64
references of cand_train_ref / cand_ce_ref; (b) it reproduces every fixture at 1/1000 of the bars; (c) the integer inputs the
fixtures store are what the C host twins of the kernels produce; (d) each deliberate mistake leaves a bar by a factor of ten or
more on the trajectories named for it; (e) the fixtures meet the conditions their generator asserted. Together: the bars
test_gpu_trajectory_ext.py holds the GPU routes to separate a wrong composition of the pieces from float32 rounding."""
import os

import numpy as np
import pytest
import torch

from . import cand_alias_ref as CA
from . import cand_ce_ref
from . import cand_train_ref
from . import dropout_ref as D
from . import edge_drop_ref as ER
from . import traj_ext_ref as X
from . import traj_ref as T
from .conftest import golden

TIGHT = 1e-3            # (b): the share of a bar the float64 restatement may use
CAUGHT = 10.0           # (d): the least distance / bar of a mutant, on one held tensor at the last snapshot
LIST_TAGS = ('E', 'F')

_runs = {}


def _run(tag, mutant=None):
    """One trajectory of the restatement, computed once and shared (never modified by the tests)."""
    if (tag, mutant) not in _runs:
        _runs[(tag, mutant)] = X.run_fixture(tag, golden('syn_a'), mutant)
    return _runs[(tag, mutant)]


# ------------------------------------------------------------------------------------------------- (a)
def test_with_every_switch_off_it_is_traj_ref():
    fx, g = T.fixture('A'), golden('syn_a')
    want, got = T.run(fx, g), X.run(fx, g, X.OFF)

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    assert rel(torch.tensor(got['loss']), torch.tensor(want['loss'])) <= 1e-12
    assert rel(torch.tensor(got['norm']), torch.tensor(want['norm'])) <= 1e-12
    for step in want['snaps']:
        for k, v in want['snaps'][step].items():
            assert rel(got['snaps'][step][k].double(), v.double()) <= 1e-12, (step, k)
    for step in want['evals']:
        assert rel(got['evals'][step], want['evals'][step]) <= 1e-12
    assert not any(got['inputs'])                        # nothing is drawn with the switches off


def test_run_leaves_its_start_state_alone():
    """A float32 twin starts from float32 tensors: run() must copy them (Tensor.to(same dtype) alone would alias the golden arrays)."""
    g = golden('syn_a')
    before = {k: v.clone() for k, v in g.state_dict().items()}
    X.run(T.fixture('A'), g, X.CONFIG['C'], dtype=torch.float32, perm_seed=3)
    assert all(torch.equal(v, g.state_dict()[k]) for k, v in before.items())


@pytest.mark.parametrize('tag', LIST_TAGS)
def test_list_losses_are_the_float64_references(tag):
    """list_bce / list_ce under autograd against cand_train_ref.ref_list_bce / cand_ce_ref.ref_list_ce on the fixture's step-1 lists:
    the loss, d x and d bias, with the divisor B K (BCE) or B (softmax) and, for the softmax, bias - logq handed over as the bias."""
    fx, g = X.fixture(tag), golden('syn_a')
    cand, label = torch.from_numpy(fx['cand_1']), torch.from_numpy(fx['label_1'])
    B, K = cand.shape
    gen = torch.Generator().manual_seed(5)
    N, dim = int(g['dl_num_entity']), int(g.hp['gcn_out_dim'])
    x = torch.randn((B, dim), generator=gen, dtype=torch.float64).requires_grad_(True)
    ent = torch.randn((N, dim), generator=gen, dtype=torch.float64) * 0.5
    bias = (torch.randn(N, generator=gen, dtype=torch.float64) * 0.1).requires_grad_(True)
    smooth = float(fx['lbl_smooth'])
    if tag == 'E':
        got = X.list_bce(x, ent, bias, cand, label, smooth)
        hot, cold = X.smoothed_targets(smooth, N)
        want = cand_train_ref.ref_list_bce(x.detach(), ent, bias.detach(), cand, label, hot, cold, 1.0 / (B * K))
    else:
        logq = torch.from_numpy(fx['logq'])
        got = X.list_ce(x, ent, bias, cand, label, smooth, logq)
        want = cand_ce_ref.ref_list_ce(x.detach(), ent, bias.detach() - logq.double(), cand, label, smooth, 1.0 / B)
    dx, dbias = torch.autograd.grad(got, [x, bias])
    assert abs(float(got) - want['loss']) <= 1e-12 * abs(want['loss'])
    assert float((dx - want['dx']).abs().max()) <= 1e-12 * float(want['dx'].abs().max())
    assert float((dbias - want['d_bias']).abs().max()) <= 1e-12 * float(want['d_bias'].abs().max())


# ------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize('tag', X.TAGS)
def test_restatement_reproduces_the_fixture(tag):
    fx, run = X.fixture(tag), _run(tag)
    for i in range(len(T.SIZES)):
        assert abs(run['loss'][i] - fx['loss'][i]) <= TIGHT * fx['bar_loss'][i], i
        assert abs(run['norm'][i] - fx['norm'][i]) <= TIGHT * fx['bar_norm'][i], i
    assert sorted(run['snaps']) == sorted(int(s) for s in fx['snaps'])
    for step in run['snaps']:
        want = T.snapshot(fx, step)
        for k in T.names(fx):                            # the exempt tensors too: float64 against float64 has no noise to exempt
            ratio = float((run['snaps'][step][k] - want[k]).abs().max()) / T.bar_of(fx, k, step)
            assert ratio <= TIGHT, (step, k, ratio)
        assert sorted(run['snaps'][step]) == sorted(want)
        for k in want:
            if k.endswith('num_batches_tracked'):
                assert int(run['snaps'][step][k]) == int(want[k]) == step
    for j, step in enumerate(int(s) for s in fx['eval_steps']):
        score = torch.from_numpy(fx['eval%d_score' % step])
        assert float((run['evals'][step] - score).abs().max()) <= TIGHT * fx['bar_eval'][j]
        assert torch.equal(T.filtered_ranks(run['evals'][step], fx), torch.from_numpy(fx['eval%d_rank' % step]))
    for i, inp in enumerate(run['inputs'], 1):
        if 'cand' in inp:
            assert np.array_equal(inp['cand'].numpy(), fx['cand_%d' % i]) and np.array_equal(inp['label'].numpy(), fx['label_%d' % i])
        if 'kept' in inp:
            assert np.array_equal(np.packbits(inp['kept'].numpy()), fx['kept_%d' % i])
            assert np.array_equal(np.packbits(inp['forced'].numpy().astype(bool)), fx['forced_%d' % i])


# ------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('tag', X.TAGS)
def test_masks_are_the_host_twins(pkg, tag):
    """Every keep mask the restatement applied, at steps 1, 5 (the 5-row batch) and 8, against mgcn_dropout_mask_host under the
    package's own key: layer sites with entity rows, trunk sites with batch rows."""
    nat, cfg, run = pkg._native, X.config_of(X.fixture(tag)), _run(tag)
    assert (nat.DROPOUT_SITE_FEATURE, nat.DROPOUT_SITE_HIDDEN) == (D.SITE_FEATURE, D.SITE_HIDDEN)
    sites = {'feat': D.SITE_FEATURE, 'hidden': D.SITE_HIDDEN}
    for li in range(cfg['layers']):
        sites.update({'in%d' % li: nat.dropout_layer_site(li, 0), 'out%d' % li: nat.dropout_layer_site(li, 1),
                      'gcn%d' % li: nat.dropout_layer_site(li, 2)})
    for step in (1, 5, 8):
        inp = run['inputs'][step - 1]
        for name, site in sites.items():
            m = inp[name]
            got = nat.dropout_mask_host(m.size(0), m.size(1), nat.dropout_key(cfg['dropout_seed'], step - 1, site), 0, cfg['p'])
            assert torch.equal(got.bool(), m), (step, name)
            assert 0.6 < float(m.float().mean()) < 0.8
        assert inp['feat'].size(0) == T.SIZES[step - 1]


@pytest.mark.parametrize('tag', LIST_TAGS)
def test_lists_are_the_host_twins(pkg, tag):
    """The stored lists and labels of every step against mgcn_cand_draw_host / mgcn_cand_draw_alias_host on the package's train
    index layout; F's table against mgcn_alias_build_host and its logq against sampling.NegativeSampler's."""
    nat, fx, g = pkg._native, X.fixture(tag), golden('syn_a')
    cfg = X.config_of(fx)
    keys, ptr, tails, r2 = X.train_index(g)
    known = {k: v for k, v in T.label_lists(g).items()}
    index = pkg.dist.FilterIndex.from_known(known, r2)
    assert torch.equal(index.keys, keys) and torch.equal(index.ptr, ptr) and torch.equal(index.tails, tails)
    table = None
    if cfg['weighted']:
        table = nat.alias_build_host(torch.from_numpy(fx['alias_weights']))
        assert torch.equal(table, torch.from_numpy(fx['alias_table']))
        assert torch.equal(table, CA.table_tensor(CA.build(X.alias_weights(int(g['dl_num_entity'])))))
        sampler = pkg.sampling.NegativeSampler(table)
        assert torch.equal(sampler.logq, torch.from_numpy(fx['logq'])) and torch.equal(sampler.logq, X.logq_of(CA.build(fx['alias_weights'])))
    for step, q in enumerate(T.batches(fx), 1):
        key = nat.dropout_key(cfg['draw_seed'], step - 1, nat.CAND_DRAW_SITE)
        cand, label = nat.cand_draw_host(index.query_keys(q[:, 0], q[:, 1]), keys, ptr, tails, int(g['dl_num_entity']), 1 + cfg['num_neg'],
                                         key, labels=True, table=table)
        assert torch.equal(cand, torch.from_numpy(fx['cand_%d' % step])), step
        assert torch.equal(label, torch.from_numpy(fx['label_%d' % step])), step


def test_kept_edges_are_the_host_twin(pkg):
    """E: the record rewrite of mgcn_edge_drop_records_host with the flags of the step's queries against the norms the restatement
    aggregated with, bit for bit, at every step; the directed-norm helper the mutants use is edge_drop_ref.edge_norms on an
    undirected kept set."""
    nat, fx, g, run = pkg._native, X.fixture('E'), golden('syn_a'), _run('E')
    cfg = X.config_of(fx)
    ei, et = g.t('dl_edge_index'), g.t('dl_edge_attr')[0]
    N, E = int(g['dl_num_entity']), ei.size(1) // 2
    host = nat.csr_build_host(N, 2 * int(g['dl_num_relation']) + 1, ei, et)
    longest = nat.max_run_host(host['rowptr'], host['hubinfo'], host['chunks'], host['num_chunks'])
    table = nat.edge_drop_table_host(longest + 1)
    assert np.array_equal(table.numpy().view(np.int32), X.norm_table(longest + 1).view(np.int32))
    for step, inp in enumerate(run['inputs'], 1):
        key = nat.dropout_key(cfg['dropout_seed'], step - 1, nat.EDGE_DROP_SITE)
        rec, _ = nat.edge_drop_records_host(host, table, key, cfg['edge_drop'], inp['forced'].contiguous())
        assert np.array_equal(rec.numpy(), ER.records(host, inp['norms'].numpy())), step
        kept2 = np.concatenate((inp['kept'].numpy(),) * 2)
        assert np.array_equal(X._directed_norms(N, ei.numpy(), kept2, X.norm_table(E + 2)).view(np.int32), inp['norms'].numpy().view(np.int32))
        assert bool((inp['norms'][~torch.from_numpy(kept2)] == 0).all())


# ------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize('mutant', sorted(X.MUTANTS))
def test_each_mutant_leaves_a_bar(mutant):
    """On every trajectory MUTANTS names for it, the mutant moves at least one held tensor at the last snapshot by CAUGHT x its
    bar or more: a GPU route with that mistake fails test_gpu_trajectory_ext.py."""
    assert X.MUTANTS[mutant]
    for tag in X.MUTANTS[mutant]:
        fx = X.fixture(tag)
        last = int(fx['snaps'][-1])
        ratio, name = T.worst_ratio(_run(tag, mutant)['snaps'][last], fx, last)
        print('RATIO mutant %s on %s: %.3g x the bar of %s' % (mutant, tag, ratio, name))
        assert ratio >= CAUGHT, (tag, ratio, name)


def test_the_mutants_are_the_sixteen_and_each_trajectory_is_used():
    assert len(X.MUTANTS) == 16 and X.NOT_SHOWN == ('ce_mean_over_positive',)
    assert {tag for tags in X.MUTANTS.values() for tag in tags} == set(X.TAGS)
    # the softmax's mean over the queries with a positive: every list's column 0 is a known tail, so the divisor is B either way
    fx = X.fixture('F')
    assert all(bool(fx['label_%d' % i][:, 0].all()) for i in range(1, 9))
    same, ref = _run('F', 'ce_mean_over_positive'), _run('F')
    assert same['loss'] == ref['loss'] and all(torch.equal(v, ref['snaps'][8][k]) for k, v in same['snaps'][8].items())


# ------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize('tag', X.TAGS)
def test_fixture_conditions(tag):
    fx, a, g = X.fixture(tag), T.fixture('A'), golden('syn_a')
    cfg = X.config_of(fx)
    assert cfg == X.CONFIG[tag]
    coef = fx['coef']
    np.testing.assert_allclose(coef, np.minimum(float(fx['max_norm']) / (fx['norm'] + 1e-6), 1.0), rtol=0, atol=1e-15)
    assert (coef < 1).any() and (coef == 1).any()
    # A's batches, optimiser, schedule and eval queries
    for k in ('lr', 'weight_decay', 'lr_after', 'lbl_smooth', 'beta1', 'beta2', 'eps', 'lr_step', 'eval_steps', 'eval_triple', 'eval_label',
              'snaps') + tuple('q_%d' % i for i in range(1, 9)):
        assert np.array_equal(fx[k], a[k]), k
    assert float(fx['lr']) == 0.01 and float(fx['weight_decay']) == 0.01 and [int(s) for s in fx['snaps']] == [1, 4, 5, 8]
    assert float(fx['margin']) == 16.0 and int(fx['twins']) >= 8
    paths = X.fixture_paths(tag)
    for path in paths:
        assert os.path.getsize(path) < T.MAX_FILE_BYTES
        with np.load(path) as z:
            assert sum(z[k].nbytes for k in z.files) < 1000000
    # the twin gaps: positive, the bars 16 x them, every held tensor's below the cap; F's one exempt tensor as argued in traj_ext_ref
    assert tuple(str(k) for k in fx['exempt']) == X.EXEMPT[tag]
    rows = [T.names(fx).index(k) for k in T.held(fx)]
    assert len(rows) == len(T.names(fx)) - len(fx['exempt'])
    assert 0 < fx['gap_sd'].min() and fx['gap_sd'][rows].max() < X.GAP_CAP * float(fx['lr'])
    for what in ('sd', 'loss', 'norm', 'eval'):
        assert (fx['gap_' + what] > 0).all() and np.array_equal(fx['bar_' + what], 16.0 * fx['gap_' + what])
    # every tensor of the start state is in the fixture, every snapshot holds all of them
    sd = X.start_state(fx, g, cfg)
    assert sorted(T.names(fx)) == sorted(k for k in sd if not k.endswith('num_batches_tracked'))
    assert len(sd) == len(g.state_dict()) + (12 if tag == 'D' else 0)
    for step in fx['snaps']:
        assert sorted(T.snapshot(fx, int(step))) == sorted(sd)
    if tag == 'D':
        want = X.layer2_state(g)
        assert all(sd[k].dtype == v.dtype and torch.equal(sd[k].reshape(-1), v.reshape(-1)) for k, v in want.items())
    for step in (4, 8):
        assert torch.equal(T.filtered_ranks(torch.from_numpy(fx['eval%d_score' % step]), fx), torch.from_numpy(fx['eval%d_rank' % step]))
        undecided = int((~T.decided(fx, step)).sum())
        assert undecided == int(fx['eval%d_undecided' % step]) <= 1
    # what the configuration must exercise
    if tag == 'E':
        E = g['dl_edge_index'].shape[1] // 2
        for i in range(1, 9):
            kept, forced = np.unpackbits(fx['kept_%d' % i])[:E].astype(bool), np.unpackbits(fx['forced_%d' % i])[:E].astype(bool)
            bits = ER.keep_bits(cfg['dropout_seed'], i - 1, cfg['edge_drop'], E)
            assert forced.any() and (~bits).any() and np.array_equal(kept, bits & ~forced)
    if tag in LIST_TAGS:
        assert all(fx['cand_%d' % i].shape == (T.SIZES[i - 1], 16) and fx['cand_%d' % i].min() >= 0 for i in range(1, 9))
        assert sum(int(fx['label_%d' % i][:, 1:].sum()) for i in range(1, 9)) >= 1          # a drawn negative that is a known tail
    if tag == 'F':
        named = [int((fx['cand_%d' % i] == int(fx['hub'])).sum()) for i in range(1, 9)]
        assert max(named) > cfg['run_split'] == 16
