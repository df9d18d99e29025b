"""Writes tests/golden/traj_syn_a_{C,D,E,F}.npz: the float64 trajectories of tests/traj_ext_ref.py on syn_a over
fixture A's batches and optimiser settings, with the worst distance of that restatement's own float32 twins as gap_* and
bar_* = 16 gap_*. CPU only: needs neither the reference checkout nor a GPU, only `oracle`, tests/*_ref and the committed syn_a
and trajectory A fixtures.

    python tests/golden/gen/make_traj_ext.py > profiles/traj_ext_twin_gaps.txt

The files are written with fixed zip time stamps, so a second run on the same CPU reproduces them byte for byte. A trajectory
whose arrays exceed PART_BYTES is stored as traj_syn_a_<tag>.npz, traj_syn_a_<tag>.1.npz, ... (traj_ext_ref.fixture merges them)."""
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cand_alias_ref as CA      # noqa: E402
from tests import traj_ext_ref as X         # noqa: E402
from tests import traj_ref as T             # noqa: E402
from tests.conftest import golden           # noqa: E402

MARGIN = 16.0                  # the project's TRAJ_MARGIN
PART_BYTES = 1000000           # make_golden.PART_BYTES: raw array bytes per file
TWIN_PERMS, TWIN_THREADS = 4, (1, 8)
SNAPS = (1, 4, 5, 8)
# candidates for max_norm, first one that clips some steps and leaves others alone (the float64 norms measured at p = 0.3: full-table
# BCE 0.8 .. 1.6, list BCE 1.3 .. 3.1, list softmax 7 .. 23). F does not try 12 and 12.5: there coef g + weight_decay p of ONE element of
# edge_embeddings cancels to 1e-8 at step 1, where Adam's first step g / (|g| + eps) turns float32 rounding into 0.06 lr, and the cap
# below refuses the run.
MAX_NORM = {'C': (1.1, 1.0, 1.2), 'D': (1.1, 1.0, 1.2), 'E': (1.9, 1.7, 2.1), 'F': (13.0, 11.0, 14.0)}
FROM_A = ('lr', 'weight_decay', 'lr_after', 'lbl_smooth', 'beta1', 'beta2', 'eps', 'lr_step', 'eval_steps', 'eval_triple', 'eval_label')
_DEFAULT_THREADS = torch.get_num_threads()


def _coefs(norms, max_norm):
    return [min(max_norm / (n + 1e-6), 1.0) for n in norms]


def _write_npz(path, arrays):
    """np.savez_compressed with every member stamped 1980-01-01: the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def _write_parts(tag, arrays):
    """The arrays in order, a new file whenever the next array would take the current one past PART_BYTES. Every file is written
    before a stale part of an earlier, longer split is removed."""
    parts, size = [{}], 0
    for k, a in arrays.items():
        if a.nbytes >= PART_BYTES:
            raise ValueError('trajectory %s: array %r alone holds %d bytes, no file may hold %d' % (tag, k, a.nbytes, PART_BYTES))
        if parts[-1] and size + a.nbytes >= PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    paths = []
    for i, part in enumerate(parts):
        assert sum(a.nbytes for a in part.values()) < PART_BYTES
        paths.append(os.path.join(T.GOLDEN, 'traj_syn_a_%s%s.npz' % (tag, '' if i == 0 else '.%d' % i)))
        _write_npz(paths[-1], part)
        assert os.path.getsize(paths[-1]) < T.MAX_FILE_BYTES
    for stale in X.fixture_paths(tag):
        if stale not in paths:
            os.remove(stale)
    return paths


def make(tag):
    g, a = golden('syn_a'), T.fixture('A')
    cfg = X.CONFIG[tag]
    N = int(g['dl_num_entity'])
    base = {k: a[k] for k in FROM_A}
    base.update(snaps=np.array(SNAPS), margin=MARGIN)
    for i in range(1, len(T.SIZES) + 1):
        base['q_%d' % i] = a['q_%d' % i]
    sd0 = dict(g.state_dict())
    extra = X.layer2_state(g) if cfg['layers'] > 1 else {}
    sd0.update(extra)
    table = CA.build(X.alias_weights(N)) if cfg['weighted'] else None
    logq = X.logq_of(table) if cfg['weighted'] else None

    def once(max_norm, dtype=torch.float64, perm_seed=None, threads=None):
        if threads is not None:
            torch.set_num_threads(threads)
        try:
            return X.run(dict(base, max_norm=max_norm), g, cfg, sd0=sd0, dtype=dtype, perm_seed=perm_seed, table=table, logq=logq)
        finally:
            torch.set_num_threads(_DEFAULT_THREADS)

    for max_norm in MAX_NORM[tag]:
        ref = once(max_norm)
        coefs = _coefs(ref['norm'], max_norm)
        if any(c < 1 for c in coefs) and any(c == 1 for c in coefs):
            break
        print('traj %s: max_norm %g clips %d of 8 steps: float64 norms %s' % (tag, max_norm, sum(c < 1 for c in coefs),
                                                                            ' '.join('%.4f' % n for n in ref['norm'])))
    else:
        raise AssertionError('trajectory %s: no max_norm candidate clips some steps and not others' % tag)

    # what the configuration must exercise
    if cfg['edge_drop'] > 0:
        for i, inp in enumerate(ref['inputs']):
            bits = X.ER.keep_bits(cfg['dropout_seed'], i, cfg['edge_drop'], inp['kept'].numel())
            assert int((~bits).sum()) >= 1 and int(inp['forced'].sum()) >= 1 and int((~inp['kept']).sum()) >= int(inp['forced'].sum())
    if cfg['loss'] != 'table':
        assert all(int(inp['cand'].min()) >= 0 and bool(inp['label'][:, 0].all()) for inp in ref['inputs'])     # every query has a tail
        assert sum(int(inp['label'][:, 1:].sum()) for inp in ref['inputs']) >= 1                                 # a negative that is a known tail
    if cfg['weighted']:
        named = [int((inp['cand'] == X.HUB).sum()) for inp in ref['inputs']]
        assert max(named) > cfg['run_split'], named
        print('traj %s: list positions that name the hub entity %d per step: %s (run_split %d)' % (tag, X.HUB, named, cfg['run_split']))

    names = [k for k in ref['snaps'][SNAPS[0]] if not k.endswith('num_batches_tracked')]
    gap_sd = np.zeros((len(names), len(SNAPS)))
    gap_loss, gap_norm, gap_eval = np.zeros(len(T.SIZES)), np.zeros(len(T.SIZES)), np.zeros(len(base['eval_steps']))
    n_twins = 0
    for threads in TWIN_THREADS:
        for perm in range(TWIN_PERMS):
            tw = once(max_norm, torch.float32, perm_seed=1000 * threads + perm, threads=threads)
            n_twins += 1
            for j, s in enumerate(SNAPS):
                for i, k in enumerate(names):
                    gap_sd[i, j] = max(gap_sd[i, j], float((tw['snaps'][s][k].double() - ref['snaps'][s][k]).abs().max()))
                for k in ref['snaps'][s]:
                    if k.endswith('num_batches_tracked'):
                        assert int(tw['snaps'][s][k]) == int(ref['snaps'][s][k]) == s
            gap_loss = np.maximum(gap_loss, np.abs(np.array(tw['loss']) - np.array(ref['loss'])))
            gap_norm = np.maximum(gap_norm, np.abs(np.array(tw['norm']) - np.array(ref['norm'])))
            for j, s in enumerate(base['eval_steps']):
                gap_eval[j] = max(gap_eval[j], float((tw['evals'][int(s)].double() - ref['evals'][int(s)]).abs().max()))
            assert [c < 1 for c in _coefs(tw['norm'], max_norm)] == [c < 1 for c in coefs]      # no twin crosses the clip threshold
    assert n_twins >= 8
    again = once(max_norm, perm_seed=99)
    exempt = X.EXEMPT[tag]
    assert set(exempt) <= set(names)
    held = np.array([k not in exempt for k in names])
    f64_gap = max(float((again['snaps'][s][k] - ref['snaps'][s][k]).abs().max()) for s in SNAPS for k in names if k not in exempt)
    assert f64_gap < 1e-12, f64_gap
    lr = float(base['lr'])
    worst = gap_sd[held].max()
    assert worst < X.GAP_CAP * lr, 'trajectory %s: a held twin gap of %.3g is not below %g lr' % (tag, worst, X.GAP_CAP)
    assert gap_sd.min() > 0 and gap_loss.min() > 0 and gap_norm.min() > 0 and gap_eval.min() > 0

    out = dict(base, max_norm=max_norm, twins=n_twins, loss=np.array(ref['loss']), norm=np.array(ref['norm']), coef=np.array(coefs),
               names=np.array(names), exempt=np.array(exempt, dtype='U64'), gap_sd=gap_sd, gap_loss=gap_loss, gap_norm=gap_norm,
               gap_eval=gap_eval, bar_sd=MARGIN * gap_sd, bar_loss=MARGIN * gap_loss, bar_norm=MARGIN * gap_norm, bar_eval=MARGIN * gap_eval)
    for k, v in cfg.items():
        out['cfg_' + k] = np.array(v)
    for s in SNAPS:
        for k, v in ref['snaps'][s].items():
            out['sd%d_%s' % (s, k)] = (v.to(torch.int64) if k.endswith('num_batches_tracked') else v.double()).numpy()
    for k, v in extra.items():
        out['sd0_' + k] = v.numpy()
    ev, lab = torch.from_numpy(base['eval_triple']), torch.from_numpy(base['eval_label']).bool()
    rows = torch.arange(ev.size(0))
    for j, s in enumerate(int(s) for s in base['eval_steps']):
        pred = ref['evals'][s]
        target = pred[rows, ev[:, 2]]
        masked = torch.where(lab, torch.full_like(pred, -1e7), pred)
        diff = (masked - target[:, None]).abs()
        diff[rows, ev[:, 2]] = float('inf')
        decide = diff.min(1).values                     # the smallest score difference that decides the filtered rank
        assert float(decide.min()) > 0                  # no tie
        undecided = int((decide <= 2 * MARGIN * gap_eval[j]).sum())
        print('  eval after step %d: score gap %.3g, deciding differences %s' % (s, gap_eval[j], ' '.join('%.2g' % d for d in sorted(decide.tolist()))))
        assert undecided <= 1, 'trajectory %s, eval after step %d: %d ranks are closer than twice the score bar' % (tag, s, undecided)
        out['eval%d_undecided' % s] = np.array(undecided)
        out['eval%d_score' % s] = pred.numpy()
        out['eval%d_rank' % s] = T.filtered_ranks(pred, base).numpy()
        out['eval%d_decide' % s] = decide.numpy()
    for i, inp in enumerate(ref['inputs'], 1):
        if 'cand' in inp:
            out['cand_%d' % i], out['label_%d' % i] = inp['cand'].numpy(), inp['label'].numpy()
        if 'kept' in inp:
            out['kept_%d' % i], out['forced_%d' % i] = np.packbits(inp['kept'].numpy()), np.packbits(inp['forced'].numpy().astype(bool))
    if cfg['weighted']:
        out.update(alias_weights=np.array(X.alias_weights(N), dtype=np.int64), alias_table=CA.table_tensor(table).numpy(), logq=logq.numpy(),
                   hub=np.array(X.HUB))
    arrays = {k: np.asarray(v) for k, v in out.items()}
    paths = _write_parts(tag, arrays)
    print('traj %s max_norm=%g coef=%s files=%s' % (tag, max_norm, ' '.join('%.3f' % c for c in coefs),
                                                   ' '.join('%s:%d' % (os.path.basename(p), os.path.getsize(p)) for p in paths)))
    print('  worst held twin_gap / lr = %.3g, loss gap %.3g, norm gap %.3g, eval gap %s, float64 permuted rows %.3g' % (
        worst / lr, gap_loss.max(), gap_norm.max(), gap_eval, f64_gap))
    for i, k in enumerate(names):
        print('  %-40s %s%s' % (k, ' '.join('%.3g' % (x / lr) for x in gap_sd[i]), '  (exempt)' if k in exempt else ''))


if __name__ == '__main__':
    torch.manual_seed(0)
    for tag in (sys.argv[1:] or X.TAGS):
        make(tag)
