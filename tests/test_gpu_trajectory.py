"""Multi-step training on a real MI355X (`-m gpu`) against the reference's float64 trajectories (tests/golden/traj_syn_a_{A,B}.npz,
written by tests/golden/gen/make_golden.py run_trajectory): 8 steps on syn_a (60 entities) from its golden state with
label smoothing, clipping, Adam with L2 weight decay, a halved lr after step 4, a 5-query batch at step 5 and an eval-mode
forward after steps 4 and 8, on four routes:
  default   model(...), model.loss, clip_grad_norm_, torch.optim.Adam: the body of harness.train, default switches
  clipadam  conve_trunk_train = query_path_train = 'hip', MGCN.forward_loss on the device label index, ClipAdam.clip_and_step
  captured  the same with dropout = 'counter' at p = 0 through captured.CapturedTrainStep (warm-up, capture, replays, the eager
            step-5 batch, replays again)
  sharded   dist.train_step_sharded on one rank
Every loss, every state tensor at every snapshot and both eval blocks lie within the fixture's bars (16 x the worst distance of
the reference's own float32 rounding twins from its float64 run; tests/test_traj_ref_host.py shows that each of twelve wrong
conventions leaves a bar by a factor of ten or more); num_batches_tracked exactly; filtered ranks equal wherever the fixture
decides them by more than twice the score bar. B's seven exempt tensors (tests/traj_ref.py) get the cap 2 x sum of lr.
The last three routes equal each other bit for bit over the whole trajectory, and the eval after step 4 leaves the later bits alone.
Every check prints `RATIO ...` (pytest -s) before it asserts."""
import types

import pytest
import torch

from . import traj_ref as T
from .conftest import golden
from .test_gpu_query_train import ALL_ON, DEV, _loader

pytestmark = pytest.mark.gpu
ROUTES = ('default', 'clipadam', 'captured', 'sharded')
BIT_EQUAL = ('clipadam', 'captured', 'sharded')
SWITCHES = ('MGCN_QUERY_TRAIN', 'MGCN_TRUNK_TRAIN', 'MGCN_TRUNK', 'MGCN_DROPOUT', 'MGCN_TRAIN_TORCH', 'MGCN_EDGE_DROP',
            'MGCN_EDGE_DROP_QUERIES')

_runs = {}


@pytest.fixture(autouse=True)
def _no_switch_from_the_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _setup(pkg, route):
    """(model, loader) from the golden state of syn_a at dropout 0 with the route's switches, in training mode."""
    g = golden('syn_a')
    over = dict(gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, lbl_smooth=0.1)
    if route != 'default':
        over.update(ALL_ON)
    if route == 'captured':
        over['dropout'] = 'counter'
    dl, params = _loader(pkg, g, **over)
    dl.graph.to(DEV)
    model = pkg.MGCN(dl.num_entity, dl.num_relation, dl.num_edge, params)
    assert not model.load_state_dict(g.state_dict(), strict=False).unexpected_keys
    model.conv1.drop.p = 0.0
    model.to(DEV).train()
    return model, dl, params


def _trajectory(pkg, tag, route, with_eval=True):
    """One run of a route over a fixture's batches: dict(loss [8 device scalars], norm [8] or None, snaps, evals, counters)."""
    fx = T.fixture(tag)
    model, dl, params = _setup(pkg, route)
    lr, wd, max_norm, smooth = float(fx['lr']), float(fx['weight_decay']), float(fx['max_norm']), float(fx['lbl_smooth'])
    if route == 'default':
        opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
        ds = dl._get_dataset('train', params)
        at = {q['triple'][:2]: i for i, q in enumerate(dl.triplets['train'])}
    else:
        opt = pkg.ClipAdam(model.parameters(), lr=lr, weight_decay=wd)
        idx = dl.train_index().to(DEV)
    step_fn = pkg.CapturedTrainStep(model, dl.graph, idx, opt, lbl_smooth=smooth, clip=max_norm) if route == 'captured' else None
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    ev = torch.from_numpy(fx['eval_triple']).to(DEV)
    out = dict(loss=[], norm=[], snaps={}, evals={}, replays=[])
    for step, q in enumerate(T.batches(fx), 1):
        src, rel = q[:, 0].to(DEV), q[:, 1].to(DEV)
        if route == 'default':
            labels = torch.stack([ds[at[(s, r)]][1] for s, r in q.tolist()]).to(DEV)
            opt.zero_grad()
            loss = model.loss(model(src, rel, dl.graph), labels)
            loss.backward()
            out['norm'].append(torch.nn.utils.clip_grad_norm_(parameters=model.parameters(), max_norm=max_norm).detach().clone())
            opt.step()
        elif route == 'clipadam':
            opt.zero_grad()
            loss = model.forward_loss(src, rel, dl.graph, idx, lbl_smooth=smooth)
            loss.backward()
            out['norm'].append(opt.clip_and_step(max_norm).detach().clone())
        elif route == 'captured':
            loss = step_fn(src, rel)
            out['replays'].append(step_fn.replays)
        else:
            loss = pkg.dist.train_step_sharded(model, dl.graph, src, rel, idx, opt, lbl_smooth=smooth, clip=max_norm)
        out['loss'].append(loss.detach().clone())
        if step in fx['snaps']:
            out['snaps'][step] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if step == int(fx['lr_step']):
            sched.step()
            assert opt.param_groups[0]['lr'] == float(fx['lr_after'])
        if with_eval and step in fx['eval_steps']:
            model.eval()
            with torch.no_grad():
                out['evals'][step] = model(ev[:, 0], ev[:, 1], dl.graph).clone()
            model.train()
    out['final'] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out['counters'] = types.SimpleNamespace(
        captured=None if step_fn is None else (step_fn.captures, step_fn.replays, step_fn.eager_steps, step_fn.disabled),
        hip_steps=getattr(opt, '_hip_step_count', None), torch_steps=getattr(opt, '_torch_step_count', None),
        adam_t=sorted({float(st['step']) for st in opt.state.values()}))
    return out


def _run(pkg, tag, route):
    """The route's trajectory, run once and shared by the tests (never modified)."""
    if (tag, route) not in _runs:
        _runs[(tag, route)] = _trajectory(pkg, tag, route)
    return _runs[(tag, route)]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('tag', T.TRAJECTORIES)
def test_route_stays_on_the_float64_trajectory(pkg, tag, route):
    fx, run = T.fixture(tag), _run(pkg, tag, route)
    worst = {}
    loss = torch.stack(run['loss']).double().cpu()
    worst['loss'] = float(((loss - torch.from_numpy(fx['loss'])).abs() / torch.from_numpy(fx['bar_loss'])).max())
    if run['norm']:
        norm = torch.stack(run['norm']).double().cpu()
        worst['norm'] = float(((norm - torch.from_numpy(fx['norm'])).abs() / torch.from_numpy(fx['bar_norm'])).max())
    else:
        assert route in ('captured', 'sharded')              # these return the loss alone
    assert sorted(run['snaps']) == sorted(int(s) for s in fx['snaps'])
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
    ranks_ok = True
    for j, step in enumerate(int(s) for s in fx['eval_steps']):
        got = run['evals'][step].double().cpu()
        worst['eval@%d' % step] = float((got - torch.from_numpy(fx['eval%d_score' % step])).abs().max()) / float(fx['bar_eval'][j])
        decided = T.decided(fx, step)
        assert tag != 'A' or int((~decided).sum()) <= 1
        same = T.filtered_ranks(got, fx) == torch.from_numpy(fx['eval%d_rank' % step])
        ranks_ok = ranks_ok and bool(same[decided].all())
    for what, ratio in worst.items():
        print('RATIO trajectory %s %s %s %.4f' % (tag, route, what, ratio))
    c = run['counters']
    print('COUNTERS trajectory %s %s %s' % (tag, route, vars(c)))
    assert c.adam_t == [float(len(T.SIZES))]
    if route != 'default':
        assert (c.hip_steps, c.torch_steps) == (len(T.SIZES), 0)
    if route == 'captured':
        # two warm-up steps, the capture with its first replay, one more; the 5-query batch runs eagerly; steps 6 to 8 are replays
        assert c.captured == (1, 5, 3, False) and run['replays'] == [0, 0, 1, 2, 2, 3, 4, 5]
    bad = {what: ratio for what, ratio in worst.items() if not ratio <= 1.0}
    assert not bad, 'worst |got - float64| / bar above 1: %s' % bad
    assert exempt_ok and ranks_ok


@pytest.mark.parametrize('tag', T.TRAJECTORIES)
def test_hip_routes_agree_bit_for_bit_over_the_trajectory(pkg, tag):
    """forward_loss + ClipAdam, the captured step and the one-rank sharded step at dropout 0: every loss (the step after the
    eager interlude included), every snapshot, both eval blocks and the final state have the same bits."""
    runs = [_run(pkg, tag, route) for route in BIT_EQUAL]
    first = runs[0]
    for route, run in zip(BIT_EQUAL[1:], runs[1:]):
        for i, (a, b) in enumerate(zip(first['loss'], run['loss'])):
            assert torch.equal(a, b), (route, 'loss', i + 1, float(a), float(b))
        for step in first['snaps']:
            for k, v in first['snaps'][step].items():
                assert torch.equal(v, run['snaps'][step][k]), (route, step, k)
        for step in first['evals']:
            assert torch.equal(first['evals'][step], run['evals'][step]), (route, 'eval', step)
        for k, v in first['final'].items():
            assert torch.equal(v, run['final'][k]), (route, 'final', k)


def test_an_eval_between_epochs_leaves_the_training_bits_alone(pkg):
    """The clipadam route once more without the two eval-mode forwards: the same losses and the same final state, bit for bit
    (the eval fills the encoder cache and captures the encoder's graph; neither may reach the following steps)."""
    with_eval = _run(pkg, 'A', 'clipadam')
    without = _trajectory(pkg, 'A', 'clipadam', with_eval=False)
    assert not without['evals']
    for i, (a, b) in enumerate(zip(with_eval['loss'], without['loss'])):
        assert torch.equal(a, b), ('loss', i + 1)
    for k, v in with_eval['final'].items():
        assert torch.equal(v, without['final'][k]), k
