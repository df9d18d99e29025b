"""The counter-drawn candidate lists (include/mgcn_hip.h (15)) on a real MI355X: the launch against
mgcn_cand_draw_host (the same inline function, which tests/test_cand_draw_host.py holds to the Python-integer definition), the
labels against mgcn_cand_labels of the drawn list, padding, slices and refusals."""
import pytest
import torch

from . import cand_draw_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LABEL_CAP = 2 ** 31 - 65          # the largest n_local mgcn_cand_labels takes; the grid's tails are far below it


def _on(dev, *ts):
    return [t.to(dev) for t in ts]


@pytest.mark.parametrize('row0', R.GRID_ROW0)
@pytest.mark.parametrize('N', R.GRID_N)
def test_device_draw_equals_host_draw_on_the_grid(pkg, N, row0):
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    dkeys, dptr, dtails = _on(DEV, keys, ptr, tails)
    k = R.key(1234, 5)
    Bm, Km = max(R.GRID_B), max(R.GRID_K)
    q = R.grid_queries(Bm)
    dq = q.to(DEV)
    want_c, want_l = nat.cand_draw_host(q, keys, ptr, tails, N, Km, k, row0=row0)
    for B in R.GRID_B:
        for K in R.GRID_K:
            cand, label = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, k, row0=row0)
            assert cand.dtype == torch.int64 and label.dtype == torch.uint8
            assert torch.equal(cand.cpu(), want_c[:B, :K]) and torch.equal(label.cpu(), want_l[:B, :K]), (B, K, N, row0)
            only, none = nat.cand_draw(dq[:B], dkeys, dptr, dtails, N, K, k, row0=row0, labels=False)
            assert none is None and torch.equal(only, cand)


def test_more_than_one_workgroup_and_a_grid_stride(pkg):
    """B K / 2 above 2048 x 256 units, so that every workgroup strides: 1100 x 1001 positions."""
    nat = pkg._native
    keys, ptr, tails = R.grid_index()
    q = R.grid_queries(1100)
    k = R.key(5, 6)
    want_c, want_l = nat.cand_draw_host(q, keys, ptr, tails, 40943, 1001, k, row0=2 ** 32 - 7)
    cand, label = nat.cand_draw(q.to(DEV), *_on(DEV, keys, ptr, tails), 40943, 1001, k, row0=2 ** 32 - 7)
    assert torch.equal(cand.cpu(), want_c) and torch.equal(label.cpu(), want_l)


@pytest.mark.parametrize('N,row0', [(7, 0), (40943, 3), (2 ** 40, 2 ** 32 + 1)])
def test_labels_padding_and_slices_on_the_device(pkg, N, row0):
    nat = pkg._native
    keys, ptr, tails = _on(DEV, *R.grid_index())
    q = R.grid_queries(8).to(DEV)
    k = R.key(3, 9)
    B, K = 8, 65
    cand, label = nat.cand_draw(q, keys, ptr, tails, N, K, k, row0=row0)
    # the GLOBAL label is mgcn_cand_labels of the drawn list (tails are int32 and below LABEL_CAP: an id at or above it is no tail)
    assert torch.equal(label, nat.cand_labels(q, keys, ptr, tails, cand, min(N, LABEL_CAP), ent_row0=0))
    assert bool((label[:, 0] == (cand[:, 0] != -1).to(torch.uint8)).all()) and int(label[:, 0].sum()) > 0
    # padded outputs keep their pads; without labels a poisoned label buffer is left alone
    cbuf = torch.full((B + 1, K + 7), -77, dtype=torch.int64, device=DEV)
    lbuf = torch.full((B + 1, K + 11), 77, dtype=torch.uint8, device=DEV)
    got_c, got_l = nat.cand_draw(q, keys, ptr, tails, N, K, k, row0=row0, out=(cbuf[:B, 3:3 + K], lbuf[:B, 5:5 + K]))
    assert got_c.data_ptr() == cbuf[:B, 3:3 + K].data_ptr() and torch.equal(got_c, cand) and torch.equal(got_l, label)
    probe_c, probe_l = cbuf.clone(), lbuf.clone()
    probe_c[:B, 3:3 + K], probe_l[:B, 5:5 + K] = -77, 77
    assert bool((probe_c == -77).all()) and bool((probe_l == 77).all())
    lbuf.fill_(77)
    lib = nat.lib()
    assert lib.mgcn_cand_draw(B, K, N, q.data_ptr(), keys.numel(), keys.data_ptr(), ptr.data_ptr(), tails.data_ptr(), tails.numel(),
                              k, row0, cbuf.data_ptr(), K + 7, None, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((lbuf == 77).all()) and torch.equal(cbuf[:B, :K], cand)
    # slices equal the whole
    a = nat.cand_draw(q[:3], keys, ptr, tails, N, K, k, row0=row0)
    b = nat.cand_draw(q[3:], keys, ptr, tails, N, K, k, row0=row0 + 3)
    assert torch.equal(torch.cat([a[0], b[0]]), cand) and torch.equal(torch.cat([a[1], b[1]]), label)
    if N == 2 ** 40:
        assert int(cand.max()) >= 2 ** 32


def test_malformed_runs_on_the_device(pkg):
    nat = pkg._native
    k = R.key(7, 0)
    q = torch.tensor([10, 20, 30, 40])
    for keys, ptr, tails in R.malformed_index():
        want = nat.cand_draw_host(q, keys, ptr, tails, 7, 5, k)
        got = nat.cand_draw(q.to(DEV), *_on(DEV, keys, ptr, tails), 7, 5, k)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
        assert int((want[0][:, 0] == -1).sum()) == 3


def test_draw_candidates_feeds_the_loss(pkg):
    """harness.draw_candidates on a loader's index: column 0 is a known tail of its query, the labels are cand_labels' of the
    list, the same (seed, step) gives the same block and another step another one."""
    import os
    import types
    from .conftest import GOLDEN, golden
    g = golden('syn_b')
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        params = types.SimpleNamespace(**g.hp)
        params.device = torch.device(DEV)
        dl = pkg.DataLoader(os.path.basename(g.data_dir), params)
    finally:
        os.chdir(cwd)
    idx = dl.train_index().to(DEV)
    q = dl.train_queries().to(DEV)[:37]
    N = dl.num_entity
    cand, label = pkg.harness.draw_candidates(q, idx, N, 12, 99, 4, labels=True)
    assert tuple(cand.shape) == (37, 13) and torch.equal(cand, pkg.harness.draw_candidates(q, idx, N, 12, 99, 4))
    keys = idx.query_keys(q[:, 0], q[:, 1])
    assert torch.equal(label, pkg._native.cand_labels(keys, idx.keys, idx.ptr, idx.tails, cand, N))
    assert bool((label[:, 0] == 1).all()) and bool((cand[:, 0] >= 0).all())
    assert not torch.equal(cand, pkg.harness.draw_candidates(q, idx, N, 12, 99, 5))
    pkg.harness.check_query_keys(q, idx)
    with pytest.raises(ValueError):
        pkg.harness.check_query_keys(torch.tensor([[N + 5, 0]], device=DEV), idx)


def test_refused_calls_write_nothing(pkg):
    nat = pkg._native
    lib = nat.lib()
    keys, ptr, tails = _on(DEV, *R.grid_index())
    q = R.grid_queries(4).to(DEV)
    cbuf = torch.full((4, 8), -77, dtype=torch.int64, device=DEV)
    lbuf = torch.full((4, 8), 77, dtype=torch.uint8, device=DEV)
    good = dict(batch=4, n_cand=8, N=7, q=q.data_ptr(), nk=4, keys=keys.data_ptr(), ptr=ptr.data_ptr(), tails=tails.data_ptr(), nt=9,
                c=cbuf.data_ptr(), ldc=8, l=lbuf.data_ptr(), ldl=8)
    bad = [dict(q=None), dict(ptr=None), dict(c=None), dict(keys=None), dict(tails=None), dict(batch=-1), dict(n_cand=0), dict(N=0),
           dict(N=2 ** 40 + 1), dict(ldc=7), dict(ldl=7), dict(nk=-1), dict(nt=-1)]
    stream = torch.cuda.current_stream().cuda_stream
    for over in bad:
        a = dict(good, **over)
        rc = lib.mgcn_cand_draw(a['batch'], a['n_cand'], a['N'], a['q'], a['nk'], a['keys'], a['ptr'], a['tails'], a['nt'], 1, 0, a['c'],
                                a['ldc'], a['l'], a['ldl'], stream)
        assert rc == 1, over
    torch.cuda.synchronize()
    assert bool((cbuf == -77).all()) and bool((lbuf == 77).all())
    with pytest.raises(nat.NativeError):
        nat.cand_draw(q, keys, ptr, tails, 7, 8, 1, out=cbuf[:, :7])
    with pytest.raises(nat.NativeError):
        nat.cand_draw(q.cpu(), keys, ptr, tails, 7, 8, 1)
    assert bool((cbuf == -77).all())
