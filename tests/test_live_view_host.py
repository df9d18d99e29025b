"""The live view of the slot layout (include/mgcn_hip.h (1v), csrc/csr_build.cpp mgcn_csr_live_view_host), host only: the
slots whose folded norm is exactly 0 are left out, everything else keeps its canonical order and its first three words, and
the fourth word becomes the canonical slot index. Hand-built graphs; each asserts from its own canonical arrays that the
placement it is there for exists."""
import numpy as np
import pytest
import torch

from .live_graphs import edge_list, host_norms, run_states


def _build(pkg, N, R, half_in, half_out, hub_threshold=0, hub_chunk=4):
    ei, et = edge_list(half_in, half_out)
    host = pkg._native.csr_build_host(N, 2 * R + 1, ei, et, hub_threshold=hub_threshold, hub_chunk=hub_chunk)
    return host, pkg._native.csr_live_view_host(host['rowptr'], host['rec'])


def _check_view(host, live):
    """The live slots are exactly the canonical non-hub slots with a non-zero norm, in the same order per (half, destination);
    row = the canonical index, the first three words unchanged; live_rowptr monotone from 0 to L."""
    rp, rec, nrm = host['rowptr'].numpy(), host['rec'].numpy(), host_norms(host)
    lrp, lrec = live['live_rowptr'].numpy(), live['live_rec'].numpy()
    N = rp.shape[1] - 1
    L = live['num_live']
    flat = lrp.reshape(-1)
    assert flat[0] == 0 and flat[-1] == L and (np.diff(flat) >= 0).all() and lrp[0, N] == lrp[1, 0]
    assert lrp.dtype == np.int32 and lrec.shape == (max(L, 1), 4)
    covered = 0
    for h in range(2):
        for n in range(N):
            want = [s for s in range(rp[h, n], rp[h, n + 1]) if nrm[s] != 0.0]
            got = lrec[lrp[h, n]:lrp[h, n + 1]]
            assert got[:, 3].tolist() == want                                  # canonical index, canonical order
            assert np.array_equal(got[:, :3], rec[want, :3])                   # src, type, norm (bits) unchanged
            covered += rp[h, n + 1] - rp[h, n]
    assert L == int((nrm[rp[0, 0]:rp[1, N]] != 0).sum()) and live['num_dead'] == covered - L and live['num_dead'] > 0


def test_dead_runs_at_every_placement(pkg):
    """In-half: node 0 dead, node 8 = N - 1 dead, 4 and 5 adjacent dead runs, 2 a dead run between the live runs 1 and 3;
    node 2 is dead in the in-half and live in the out-half."""
    N, R = 9, 2
    # in-half: the sources are 1, 3, 6 only
    half_in = [(1, 0, 0), (3, 1, 1), (6, 1, 0), (1, 2, 1), (6, 3, 2), (3, 4, 3), (6, 5, 0), (1, 6, 1), (3, 8, 2), (6, 8, 3), (1, 2, 0)]
    # out-half: the sources are 0, 2, 5, 7
    half_out = [(0, 2, 1), (2, 5, 0), (5, 7, 3), (7, 0, 2), (0, 2, 0), (2, 1, 1), (5, 1, 2), (7, 3, 3), (0, 0, 1), (2, 7, 0), (5, 5, 2)]
    host, live = _build(pkg, N, R, half_in, half_out)
    st_in, st_out = run_states(host, 0), run_states(host, 1)
    assert st_in == 'dldlddled' and st_out == 'ldldelele'
    assert st_in[0] == 'd' and st_in[N - 1] == 'd' and 'dd' in st_in and 'ldl' in st_in
    assert st_in[2] == 'd' and st_out[2] == 'l'                               # dead in one half, live in the other
    assert 'd' in st_out and 'l' in st_out
    _check_view(host, live)
    lrp = live['live_rowptr'].numpy()
    assert lrp[0, 0] == lrp[0, 1] == 0 and lrp[0, N - 1] == lrp[0, N]         # the dead runs at both ends are empty in the view


def test_half_with_every_slot_dead(pkg):
    N, R = 5, 1
    half_in = [(0, 2, 0), (1, 3, 1), (0, 4, 0), (1, 2, 1)]                     # no destination is ever a source
    half_out = [(2, 0, 1), (0, 2, 0), (3, 3, 1), (2, 3, 0)]
    host, live = _build(pkg, N, R, half_in, half_out)
    assert set(run_states(host, 0)) == {'e', 'd'} and 'l' in run_states(host, 1)
    _check_view(host, live)
    lrp = live['live_rowptr'].numpy()
    assert (lrp[0] == 0).all() and live['num_live'] == lrp[1, N] > 0


def test_every_slot_of_the_graph_dead(pkg):
    N, R = 4, 1
    host, live = _build(pkg, N, R, [(0, 1, 0), (0, 2, 1)], [(3, 1, 0), (3, 2, 1)])
    assert set(run_states(host, 0)) | set(run_states(host, 1)) == {'e', 'd'}
    _check_view(host, live)
    assert live['num_live'] == 0 and live['num_dead'] == 4 and int(live['live_rowptr'].abs().sum()) == 0


def test_no_dead_slot_builds_no_view(pkg):
    N, R = 3, 1
    ring = [(0, 1, 0), (1, 2, 1), (2, 0, 0)]
    host, live = _build(pkg, N, R, ring, ring)
    assert run_states(host, 0) == 'lll' and run_states(host, 1) == 'lll' and live is None
    lib, nat = pkg._native.lib(), pkg._native
    import ctypes
    n_live, n_dead = ctypes.c_int64(-1), ctypes.c_int64(-1)                    # the sizing call: no outputs, counts only
    assert lib.mgcn_csr_live_view_host(N, host['rowptr'].data_ptr(), host['rec'].data_ptr(), None, None, 0,
                                       ctypes.byref(n_live), ctypes.byref(n_dead)) == 0
    assert (n_live.value, n_dead.value) == (6, 0)
    assert nat.ABI_VERSION == 4 and lib.mgcn_abi_version() == 4                # names were added, the ABI number stays


def test_no_edges_and_a_single_node(pkg):
    host, live = _build(pkg, 3, 1, [], [])                                     # E = 0
    assert host['rec'].numel() == 0 and live is None
    host, live = _build(pkg, 1, 1, [(0, 0, 0), (0, 0, 1)], [(0, 0, 1), (0, 0, 0)])   # N = 1: the only destination is a source
    assert run_states(host, 0) == 'l' and run_states(host, 1) == 'l' and live is None
    host, live = _build(pkg, 1, 1, [], [])
    assert live is None


def test_hub_runs_stay_empty_and_hub_slots_stay_out(pkg):
    """hub_threshold = 4: node 3 (six live slots in the in-half) and node 5 (five dead ones) are hubs, their canonical runs
    are empty and their slots sit in the hub region, which the view does not cover; node 4 between them is a plain dead run."""
    N, R = 7, 1
    half_in = [(0, 3, 0), (1, 3, 1), (3, 3, 0), (0, 3, 1), (1, 3, 0), (3, 3, 1),
               (0, 5, 0), (1, 5, 1), (3, 5, 0), (0, 5, 1), (1, 5, 0), (0, 4, 1), (3, 1, 0), (1, 0, 1), (0, 6, 0)]
    half_out = [(i % N, (i + 1) % N, i % 2) for i in range(len(half_in))]
    host, live = _build(pkg, N, R, half_in, half_out, hub_threshold=4, hub_chunk=4)
    rp, hub = host['rowptr'].numpy(), host['hubinfo'].numpy()
    assert host['num_chunks'] == 4 and hub[0, 3, 1] == 2 and hub[0, 5, 1] == 2          # 6 and 5 slots in chunks of 4
    assert rp[0, 3] == rp[0, 4] and rp[0, 5] == rp[0, 6]                                # the hubs' canonical runs are empty
    st = run_states(host, 0)
    assert st[3] == 'e' and st[5] == 'e' and st[4] == 'd' and st[6] == 'd' and st[1] == 'l'
    _check_view(host, live)
    lrp, lrec = live['live_rowptr'].numpy(), live['live_rec'].numpy()
    assert lrp[0, 3] == lrp[0, 4] and lrp[0, 5] == lrp[0, 6]
    hub_slots = set(range(int(host['chunks'][0, 0]), 2 * len(half_in)))                 # the hub region is the layout's tail
    assert len(hub_slots) == 11 and not hub_slots & set(lrec[:live['num_live'], 3].tolist())
    assert (host_norms(host)[sorted(hub_slots)] == 0).sum() == 5                        # (node 5's slots: dead, still in the region)


def test_bad_arguments_are_refused(pkg):
    nat = pkg._native
    host, _ = _build(pkg, 4, 1, [(0, 1, 0), (0, 2, 1)], [(3, 1, 0), (3, 2, 1)])
    with pytest.raises(nat.NativeError):
        nat.csr_live_view_host(host['rowptr'].to(torch.int64), host['rec'])
    bad = host['rowptr'].clone()
    bad[0, 2] = 9                                                                       # decreasing afterwards, past the records
    with pytest.raises(nat.NativeError):
        nat.csr_live_view_host(bad, host['rec'])
