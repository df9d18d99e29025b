"""CPU-only tests of the trajectory fixtures (tests/golden/traj_syn_a_{A,B}.npz) and of their float64 restatement
(tests/traj_ref.py): (a) the restatement reproduces the reference's float64 run at 1/1000 of every bar, (b) each deliberate
mistake leaves a bar by a factor of ten or more, (c) the fixtures meet the conditions their generator asserted. Together: the
bars test_gpu_trajectory.py holds the GPU routes to separate a wrong convention from float32 rounding."""
import os

import numpy as np
import pytest
import torch

from . import adam_ref
from . import traj_ref as T
from .conftest import golden

TIGHT = 1e-3            # (a): the share of a bar the float64 restatement may use (float64 twins sit nine orders below float32 ones)
CAUGHT = 10.0           # (b): the least distance / bar of a mutant, on one held tensor at the last snapshot

_runs = {}


def _run(tag, mutant=None):
    """One trajectory of the restatement, computed once and shared (never modified by the tests)."""
    if (tag, mutant) not in _runs:
        _runs[(tag, mutant)] = T.run(T.fixture(tag), golden('syn_a'), mutant)
    return _runs[(tag, mutant)]


# ------------------------------------------------------------------------------------------------- the restatement's parts
def test_forward_is_the_oracles_in_float64():
    """traj_ref.forward (BatchNorm written out) against oracle.mgcn_forward (F.batch_norm) on syn_a in float64, in eval mode and
    in training mode, the running statistics it leaves included."""
    g = golden('syn_a')
    O = T.O
    q = T.batches(T.fixture('A'))[0]
    ei, ea = g.t('dl_edge_index'), g.t('dl_edge_attr')
    for training in (False, True):
        a = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in g.state_dict().items()}
        b = {k: v.clone() for k, v in a.items()}
        with torch.no_grad():
            got = T.forward(a, g.hp, q[:, 0], q[:, 1], ei, ea, training)
            want = O.mgcn_forward(b, dict(g.hp, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0), q[:, 0], q[:, 1], ei, ea, training=training)
        assert float((got - want).abs().max()) < 1e-13
        for k in a:
            if 'running_' in k:
                assert float((a[k] - b[k]).abs().max()) < 1e-13, k
                assert training != torch.equal(a[k], g.state_dict()[k].double()), k
        assert all(int(a[k]) == int(training) for k in a if k.endswith('num_batches_tracked'))


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_update_is_adam_refs(wd):
    gen = torch.Generator().manual_seed(3)
    p, g = torch.randn(37, generator=gen, dtype=torch.float64), torch.randn(37, generator=gen, dtype=torch.float64)
    a = [p.clone(), torch.zeros_like(p), torch.zeros_like(p)]
    b = [p.clone(), torch.zeros_like(p), torch.zeros_like(p)]
    for t in (1, 2, 3):
        T.adam_update(a[0], a[1], a[2], g * t, 0.37, t, 0.01, (0.9, 0.999), 1e-8, wd)
        adam_ref.adam_ref(b[0], b[1], b[2], g * t, 0.37, t, 0.01, (0.9, 0.999), 1e-8, wd)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], p)


# ------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize('tag', T.TRAJECTORIES)
def test_restatement_reproduces_the_fixture(tag):
    """Every loss, pre-clip norm, snapshot tensor and eval block within TIGHT of its bar; num_batches_tracked exactly; B's seven
    exempt tensors within their cap (they are exempt here too)."""
    fx, run = T.fixture(tag), _run(tag)
    for i in range(len(T.SIZES)):
        assert abs(run['loss'][i] - fx['loss'][i]) <= TIGHT * fx['bar_loss'][i], i
        assert abs(run['norm'][i] - fx['norm'][i]) <= TIGHT * fx['bar_norm'][i], i
    assert sorted(run['snaps']) == sorted(int(s) for s in fx['snaps'])
    for step in run['snaps']:
        ratio, name = T.worst_ratio(run['snaps'][step], fx, step)
        print('RATIO restatement %s step %d %.3g (%s)' % (tag, step, ratio, name))
        assert ratio <= TIGHT, (step, name, ratio)
        want = T.snapshot(fx, step)
        for k in want:
            if k.endswith('num_batches_tracked'):
                assert int(run['snaps'][step][k]) == int(want[k]) == step
        for k in fx['exempt']:
            assert float((run['snaps'][step][str(k)] - want[str(k)]).abs().max()) <= T.exempt_cap(fx, step)
    for j, step in enumerate(fx['eval_steps']):
        step = int(step)
        score = torch.from_numpy(fx['eval%d_score' % step])
        assert float((run['evals'][step] - score).abs().max()) <= TIGHT * fx['bar_eval'][j]
        assert torch.equal(T.filtered_ranks(run['evals'][step], fx), torch.from_numpy(fx['eval%d_rank' % step]))


# ------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize('mutant', sorted(T.MUTANTS))
def test_each_mutant_leaves_a_bar(mutant):
    """On every trajectory MUTANTS names for it, the mutant moves at least one held tensor at the last snapshot by CAUGHT x its
    bar or more: a GPU route with that mistake fails test_gpu_trajectory.py."""
    assert T.MUTANTS[mutant]
    for tag in T.MUTANTS[mutant]:
        fx = T.fixture(tag)
        last = int(fx['snaps'][-1])
        ratio, name = T.worst_ratio(_run(tag, mutant)['snaps'][last], fx, last)
        print('RATIO mutant %s on %s: %.3g x the bar of %s' % (mutant, tag, ratio, name))
        assert ratio >= CAUGHT, (tag, ratio, name)


def test_the_mutants_are_the_twelve_and_each_trajectory_is_used():
    assert len(T.MUTANTS) == 12
    assert {tag for tags in T.MUTANTS.values() for tag in tags} == set(T.TRAJECTORIES)
    # loss_over_b is asserted on B for its state (every step of A is clipped, which divides the factor N out again); its loss is
    # N times the fixture's on both trajectories
    for tag in T.TRAJECTORIES:
        fx = T.fixture(tag)
        n = int(golden('syn_a')['dl_num_entity'])
        assert abs(_run(tag, 'loss_over_b')['loss'][0] - n * fx['loss'][0]) < 1e-9


# ------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('tag', T.TRAJECTORIES)
def test_fixture_conditions(tag):
    fx = T.fixture(tag)
    coef = fx['coef']
    np.testing.assert_allclose(coef, np.minimum(float(fx['max_norm']) / (fx['norm'] + 1e-6), 1.0), rtol=0, atol=1e-15)
    if tag == 'A':
        assert (coef < 1).all() and float(fx['weight_decay']) == 0.01 and float(fx['lr']) == 0.01
        assert len(fx['exempt']) == 0 and [int(s) for s in fx['snaps']] == [1, 4, 5, 8]
    else:
        assert (coef < 1).any() and (coef == 1).any() and float(fx['weight_decay']) == 0.0 and float(fx['lr']) == 0.001
        assert sorted(str(k) for k in fx['exempt']) == sorted(T.EXEMPT_B) and [int(s) for s in fx['snaps']] == [4, 8]
    assert [fx['q_%d' % i].shape[0] for i in range(1, 9)] == list(T.SIZES) and T.SIZES[4] == 5
    train = golden('syn_a')['dl_q_train_triple']
    assert train.shape[0] % 16 == 5
    assert np.array_equal(np.concatenate([fx['q_%d' % i] for i in range(1, 9)]), train[:sum(T.SIZES), :2])     # dataset order
    assert float(fx['lr_after']) == 0.5 * float(fx['lr']) and int(fx['lr_step']) == 4 and [int(s) for s in fx['eval_steps']] == [4, 8]
    assert (float(fx['beta1']), float(fx['beta2']), float(fx['eps']), float(fx['lbl_smooth'])) == (0.9, 0.999, 1e-8, 0.1)
    assert float(fx['margin']) == 16.0 and int(fx['twins']) >= 8
    assert os.path.getsize(T.fixture_path(tag)) < T.MAX_FILE_BYTES
    assert sum(a.nbytes for a in fx.values()) < 1000000
    # the twin gaps: positive, the bars 16 x them, every held tensor's below the cap
    rows = [T.names(fx).index(k) for k in T.held(fx)]
    assert len(rows) == len(T.names(fx)) - len(fx['exempt'])
    assert 0 < fx['gap_sd'][rows].min() and fx['gap_sd'][rows].max() < T.GAP_CAP[tag] * float(fx['lr'])
    for what in ('sd', 'loss', 'norm', 'eval'):
        assert (fx['gap_' + what] > 0).all() and np.array_equal(fx['bar_' + what], 16.0 * fx['gap_' + what])
    # every tensor of the golden state is in the fixture, every snapshot holds all of them
    sd = golden('syn_a').state_dict()
    assert sorted(T.names(fx)) == sorted(k for k in sd if not k.endswith('num_batches_tracked'))
    for step in fx['snaps']:
        assert sorted(T.snapshot(fx, int(step))) == sorted(sd)
    # the recorded ranks are those of the recorded scores; in A at most one query per block is left undecided by twice the
    # score bar (B's eval scores read the exempt running statistics: the reference's own twins leave no rank decided there)
    assert fx['eval_triple'].shape == (16, 3) and np.array_equal(fx['eval_triple'], golden('syn_a')['dl_q_valid_tail_triple'][:16])
    for step in (4, 8):
        assert torch.equal(T.filtered_ranks(torch.from_numpy(fx['eval%d_score' % step]), fx), torch.from_numpy(fx['eval%d_rank' % step]))
        undecided = int((~T.decided(fx, step)).sum())
        assert undecided == int(fx['eval%d_undecided' % step])
        if tag == 'A':
            assert undecided <= 1
