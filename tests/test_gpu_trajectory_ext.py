"""Multi-step training on a real MI355X (`-m gpu`) against the float64 trajectories of tests/golden/traj_syn_a_{C,D,E,F}.npz
(tests/traj_ext_ref.py, written by tests/golden/gen/make_traj_ext.py): the eight steps of test_gpu_trajectory.py on
syn_a with counter-based dropout p = 0.3 at all five sites (C), a second layer (D), edge dropout with own-triple removal and the
list BCE on counter-drawn lists (E), the list softmax on weighted lists with logq and run_split = 16 (F). All HIP switches on,
dropout = 'counter', three routes per trajectory:
  eager     C, D: MGCN.forward_loss + ClipAdam.clip_and_step; E, F: harness.draw_candidates + MGCN.forward_loss_candidates + ClipAdam
  captured  C, D: captured.CapturedTrainStep; E, F: captured.CapturedCandidateStep (warm-up, capture, replays, the eager 5-query
            step, replays again)
  sharded   C, D: dist.train_step_sharded; E, F: dist.train_step_sharded_candidates, on one rank
Every loss, every norm where the route returns one, every state tensor at every snapshot and both eval blocks lie within the
fixture's bars (16 x the worst distance of the restatement's own float32 twins; tests/test_traj_ext_host.py shows that each of
sixteen wrong compositions leaves a bar by a factor of ten or more); num_batches_tracked exactly; filtered ranks equal wherever
the fixture decides them; F's one exempt tensor (traj_ext_ref.EXEMPT) gets the cap 2 x sum of lr. The lists and labels each route
drew equal the fixture's (the captured step's own blocks included); dropout_step and the captured step's draw_step end at 8 (the
other two routes are handed step - 1 by the test); the three routes agree bit for bit. Every check prints `RATIO ...` (pytest -s) before it asserts."""
import types

import pytest
import torch

from . import traj_ext_ref as X
from . import traj_ref as T
from .conftest import golden
from .test_gpu_query_train import ALL_ON, DEV, _loader
from .test_gpu_trajectory import SWITCHES

pytestmark = pytest.mark.gpu
ROUTES = ('eager', 'captured', 'sharded')

_runs = {}


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _setup(pkg, tag):
    """(model, loader, params, cfg) from the fixture's step-0 state with its configuration, in training mode."""
    g, fx = golden('syn_a'), X.fixture(tag)
    cfg = X.config_of(fx)
    over = dict(ALL_ON, dropout='counter', dropout_seed=cfg['dropout_seed'], gcn_drop=cfg['p'], hidden_drop=cfg['p'], feat_drop=cfg['p'],
                lbl_smooth=float(fx['lbl_smooth']), gcn_layers=cfg['layers'], edge_drop=cfg['edge_drop'], edge_drop_queries=cfg['edge_drop_queries'])
    dl, params = _loader(pkg, g, **over)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    loaded = model.load_state_dict(X.start_state(fx, g, cfg), strict=False)
    assert not loaded.unexpected_keys and not loaded.missing_keys
    for layer in [model.conv1] + list(model.conv1_extra):
        layer.drop.p = cfg['p']
    assert len(model.conv1_extra) == cfg['layers'] - 1
    model.to(DEV).train()
    return model, dl, params, cfg


def _trajectory(pkg, tag, route, run_split='fixture'):
    """One run of a route over a fixture's batches: dict(loss [8 device scalars], norm [8] or None, snaps, evals, cand, label,
    counters)."""
    fx = X.fixture(tag)
    model, dl, params, cfg = _setup(pkg, tag)
    lr, wd, max_norm, smooth = float(fx['lr']), float(fx['weight_decay']), float(fx['max_norm']), float(fx['lbl_smooth'])
    lists = cfg['loss'] != 'table'
    opt = pkg.ClipAdam(model.parameters(), lr=lr, weight_decay=wd)
    idx = dl.train_index().to(DEV)
    sampler = pkg.NegativeSampler.from_weights(torch.from_numpy(fx['alias_weights'])).to(DEV) if cfg['weighted'] else None
    logq = sampler.logq if sampler is not None and cfg['loss'] == 'softmax' else None
    split = (cfg['run_split'] or None) if run_split == 'fixture' else run_split
    kind = dict(loss=cfg['loss'], run_split=split) if lists else {}
    step_fn = None
    if route == 'captured' and lists:
        step_fn = pkg.CapturedCandidateStep(model, dl.graph, idx, opt, cfg['num_neg'], cfg['draw_seed'], lbl_smooth=smooth, clip=max_norm,
                                            sampler=sampler, **kind)
    elif route == 'captured':
        step_fn = pkg.CapturedTrainStep(model, dl.graph, idx, opt, lbl_smooth=smooth, clip=max_norm)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    ev = torch.from_numpy(fx['eval_triple']).to(DEV)
    out = dict(loss=[], norm=[], snaps={}, evals={}, replays=[], cand=[], label=[])
    for step, q in enumerate(T.batches(fx), 1):
        q = q.to(DEV)
        src, rel = q[:, 0].contiguous(), q[:, 1].contiguous()
        if lists and route != 'captured':
            cand, labels = pkg.harness.draw_candidates(q, idx, dl.num_entity, cfg['num_neg'], cfg['draw_seed'], step - 1, labels=True, sampler=sampler)
            out['cand'].append(cand.clone())
            out['label'].append(labels.clone())
        if route == 'captured':
            loss = step_fn(src, rel)
            out['replays'].append(step_fn.replays)
            if lists:
                out['cand'].append(step_fn.cand.clone())
                out['label'].append(step_fn.labels.clone())
        elif route == 'eager':
            opt.zero_grad()
            if lists:
                loss = model.forward_loss_candidates(src, rel, cand, dl.graph, labels=labels, lbl_smooth=smooth, logq=logq, **kind)
            else:
                loss = model.forward_loss(src, rel, dl.graph, idx, lbl_smooth=smooth)
            loss.backward()
            out['norm'].append(opt.clip_and_step(max_norm).detach().clone())
        elif lists:
            loss = pkg.dist.train_step_sharded_candidates(model, dl.graph, src, rel, cand, idx, opt, labels=labels, lbl_smooth=smooth,
                                                          clip=max_norm, logq=logq, **kind)
        else:
            loss = pkg.dist.train_step_sharded(model, dl.graph, src, rel, idx, opt, lbl_smooth=smooth, clip=max_norm)
        out['loss'].append(loss.detach().clone())
        if step in fx['snaps']:
            out['snaps'][step] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if step == int(fx['lr_step']):
            sched.step()
            assert opt.param_groups[0]['lr'] == float(fx['lr_after'])
        if step in fx['eval_steps']:
            model.eval()
            with torch.no_grad():
                out['evals'][step] = model(ev[:, 0], ev[:, 1], dl.graph).clone()
            model.train()
    out['final'] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out['counters'] = types.SimpleNamespace(
        captured=None if step_fn is None else (step_fn.captures, step_fn.replays, step_fn.eager_steps, step_fn.disabled),
        hip_steps=getattr(opt, '_hip_step_count', None), torch_steps=getattr(opt, '_torch_step_count', None),
        adam_t=sorted({float(st['step']) for st in opt.state.values()}), dropout_step=model.dropout_step,
        draw_step=getattr(step_fn, 'draw_step', None), edge_drops=getattr(model, '_edge_drop_count', 0))
    return out


def _run(pkg, tag, route):
    """The route's trajectory, run once and shared by the tests (never modified)."""
    if (tag, route) not in _runs:
        _runs[(tag, route)] = _trajectory(pkg, tag, route)
    return _runs[(tag, route)]


def _ratios(fx, run, tag, route):
    """{what: worst |got - float64| / bar} of a run, each printed; and whether the exempt tensors keep their cap."""
    worst = {}
    loss = torch.stack(run['loss']).double().cpu()
    worst['loss'] = float(((loss - torch.from_numpy(fx['loss'])).abs() / torch.from_numpy(fx['bar_loss'])).max())
    if run['norm']:
        norm = torch.stack(run['norm']).double().cpu()
        worst['norm'] = float(((norm - torch.from_numpy(fx['norm'])).abs() / torch.from_numpy(fx['bar_norm'])).max())
    exempt_ok = True
    for step, sd in sorted(run['snaps'].items()):
        want = T.snapshot(fx, step)
        assert sorted(sd) == sorted(want)
        ratio, name = T.worst_ratio(sd, fx, step)
        worst['state@%d' % step] = ratio
        print('RATIO trajectory %s %s state after step %d: %.4f (%s)' % (tag, route, step, ratio, name))
        for k in want:
            if k.endswith('num_batches_tracked'):
                assert int(sd[k]) == int(want[k]) == step, k
        for k in fx['exempt']:
            gap = float((sd[str(k)].double().cpu() - want[str(k)]).abs().max())
            print('CAP   trajectory %s %s %s after step %d: %.3g of %.3g' % (tag, route, k, step, gap, T.exempt_cap(fx, step)))
            exempt_ok = exempt_ok and gap <= T.exempt_cap(fx, step)
    for j, step in enumerate(int(s) for s in fx['eval_steps']):
        got = run['evals'][step].double().cpu()
        worst['eval@%d' % step] = float((got - torch.from_numpy(fx['eval%d_score' % step])).abs().max()) / float(fx['bar_eval'][j])
    for what, ratio in worst.items():
        print('RATIO trajectory %s %s %s %.4f' % (tag, route, what, ratio))
    return worst, exempt_ok


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('tag', X.TAGS)
def test_route_stays_on_the_float64_trajectory(pkg, tag, route):
    fx, run = X.fixture(tag), _run(pkg, tag, route)
    cfg = X.config_of(fx)
    assert sorted(run['snaps']) == sorted(int(s) for s in fx['snaps'])
    assert bool(run['norm']) == (route == 'eager')               # the captured and the sharded step return the loss alone
    worst, exempt_ok = _ratios(fx, run, tag, route)
    ranks_ok = True
    for step in (int(s) for s in fx['eval_steps']):
        decided = T.decided(fx, step)
        assert int((~decided).sum()) <= 1
        same = T.filtered_ranks(run['evals'][step].double().cpu(), fx) == torch.from_numpy(fx['eval%d_rank' % step])
        ranks_ok = ranks_ok and bool(same[decided].all())
    # the integer inputs: the lists and labels every route drew (the captured step's own blocks, eager interlude included)
    if cfg['loss'] != 'table':
        assert len(run['cand']) == len(run['label']) == len(T.SIZES)
        for i, cand in enumerate(run['cand'], 1):
            assert torch.equal(cand.cpu(), torch.from_numpy(fx['cand_%d' % i])), ('cand', i)
        for i, label in enumerate(run['label'], 1):
            assert torch.equal(label.cpu(), torch.from_numpy(fx['label_%d' % i])), ('label', i)
    c = run['counters']
    print('COUNTERS trajectory %s %s %s' % (tag, route, vars(c)))
    assert c.adam_t == [float(len(T.SIZES))] and (c.hip_steps, c.torch_steps) == (len(T.SIZES), 0)
    assert c.dropout_step == len(T.SIZES)                        # once per training step, never by an eval
    if cfg['edge_drop'] > 0:
        assert c.edge_drops >= 1
    if route == 'captured':
        # two warm-up steps, the capture with its first replay, one more; the 5-query batch runs eagerly; steps 6 to 8 are replays
        assert c.captured == (1, 5, 3, False) and run['replays'] == [0, 0, 1, 2, 2, 3, 4, 5]
        if cfg['loss'] != 'table':
            assert c.draw_step == len(T.SIZES)
    bad = {what: ratio for what, ratio in worst.items() if not ratio <= 1.0}
    assert not bad, 'worst |got - float64| / bar above 1: %s' % bad
    assert exempt_ok and ranks_ok


@pytest.mark.parametrize('tag', X.TAGS)
def test_hip_routes_agree_bit_for_bit_over_the_trajectory(pkg, tag):
    """The eager step, the captured step (its eager interlude at step 5 included) and the one-rank sharded step at dropout 0.3:
    every loss, every snapshot, both eval blocks, the final state and the drawn lists have the same bits."""
    runs = [_run(pkg, tag, route) for route in ROUTES]
    first = runs[0]
    for route, run in zip(ROUTES[1:], runs[1:]):
        for i, (a, b) in enumerate(zip(first['loss'], run['loss'])):
            assert torch.equal(a, b), (route, 'loss', i + 1, float(a), float(b))
        for step in first['snaps']:
            for k, v in first['snaps'][step].items():
                assert torch.equal(v, run['snaps'][step][k]), (route, step, k)
        for step in first['evals']:
            assert torch.equal(first['evals'][step], run['evals'][step]), (route, 'eval', step)
        for k, v in first['final'].items():
            assert torch.equal(v, run['final'][k]), (route, 'final', k)
        for i, (a, b) in enumerate(zip(first['cand'], run['cand'])):
            assert torch.equal(a, b), (route, 'cand', i + 1)
        for i, (a, b) in enumerate(zip(first['label'], run['label'])):
            assert torch.equal(a, b), (route, 'label', i + 1)


def test_run_split_keeps_the_first_loss_and_stays_on_the_trajectory(pkg):
    """F's eager route without run_split: the loss of step 1 has the bits of the run with run_split = 16 (the loss and d x never
    depend on the split; the entity rows' gradient of the hub entity, named more than 16 times, is summed in another order from
    there on), and the whole run stays inside the fixture's bars."""
    fx = X.fixture('F')
    split = _run(pkg, 'F', 'eager')
    named = [int((c == int(fx['hub'])).sum()) for c in split['cand']]
    assert max(named) > 16 and X.config_of(fx)['run_split'] == 16
    whole = _trajectory(pkg, 'F', 'eager', run_split=None)
    assert torch.equal(whole['loss'][0], split['loss'][0])
    worst, exempt_ok = _ratios(fx, whole, 'F', 'eager-unsplit')
    bad = {what: ratio for what, ratio in worst.items() if not ratio <= 1.0}
    assert not bad and exempt_ok, bad
