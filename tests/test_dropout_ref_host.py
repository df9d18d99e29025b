"""The counter-based dropout bits without a GPU: the definition's known answers, mgcn_dropout_mask_host (the same
inline function the kernels call) against the numpy restatement tests/dropout_ref.py, keep rates, and the argument validation
of the new entry points (every check runs before the first HIP call)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from . import dropout_ref as R
from .conftest import ROOT

EINVAL = 1
ROW0S = (0, 7, 2 ** 32 - 3, 2 ** 40 + 1)
GRID_ROWS, GRID_COLS, GRID_P = (1, 63, 64, 65, 257), (1, 3, 4, 5, 100, 200, 201), (0.1, 0.3, 0.5)


def test_splitmix_keys_known_answers(pkg):
    assert R.sm(0) == 0xe220a8397b1dcdaf
    assert R.key(0, 0, 0) == 0x238275bc38fcbe91
    assert R.key(1234, 0, 0) == 0x52b6d2127195ace2
    assert R.key(1234, 5, 0x1001) == 0x2bbde2bebe8ae998
    for args in ((0, 0, 0), (1234, 0, 0), (1234, 5, 0x1001), (2 ** 63 + 5, 2 ** 40, 6)):
        assert pkg._native.dropout_key(*args) == R.key(*args)


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for ctr, k, want in kat:
        got = R.philox4x32_10(*ctr, *k)
        assert ' '.join('%08x' % int(w) for w in got) == want


def test_thresholds_and_pinned_bits(pkg):
    nat = pkg._native
    for p, t in ((0.3, 3006477107), (0.1, 3865470566), (0.5, 2147483648), (0.0, 2 ** 32 - 1), (1.0, 0)):
        assert R.threshold(p) == t and nat.dropout_threshold(p) == t
    k = R.key(1234, 5, 0x1001)
    assert ' '.join('%08x' % int(w) for w in R.words(k, 1, 4)[0]) == 'e4e93cf3 74f3160c 31d8219a a324bc25'
    bits = lambda m: ''.join(str(int(v)) for v in m)
    for row0, want in ((0, '011111011010'), (2 ** 32 + 7, '111010111101')):
        assert bits(R.mask(k, 1, 12, row0, R.threshold(0.3))[0]) == want
        assert bits(nat.dropout_mask_host(1, 12, k, row0, 0.3)[0]) == want
    assert nat.dropout_layer_site(3, 2) == 14 and (nat.DROPOUT_SITE_FEATURE, nat.DROPOUT_SITE_HIDDEN) == (0x1000, 0x1001)


@pytest.mark.parametrize('row0', ROW0S)
def test_host_mask_equals_reference_on_the_grid(pkg, row0):
    nat = pkg._native
    k = R.key(1234, 2, 5)
    for cols in GRID_COLS:
        ref = R.words(k, max(GRID_ROWS), cols, row0)                   # one reference per (row0, cols), shared by rows and p
        for p in GRID_P:
            want = (ref < np.uint64(R.threshold(p))).astype(np.uint8)
            for rows in GRID_ROWS:
                got = nat.dropout_mask_host(rows, cols, k, row0, p).numpy()
                assert np.array_equal(got, want[:rows]), (rows, cols, row0, p)


def test_host_mask_padded_rows_and_row_slices(pkg):
    """Bytes past `cols` of a padded row are not written, and rows [a, b) with row0 = a are that slice of the whole block."""
    lib = pkg._native.lib()
    k, thr = R.key(9, 1, 1), R.threshold(0.3)
    rows, cols, ld = 65, 5, 9
    buf = torch.full((rows, ld), 77, dtype=torch.uint8)
    assert lib.mgcn_dropout_mask_host(rows, cols, buf.data_ptr(), ld, k, 3, thr) == 0
    assert np.array_equal(buf[:, :cols].numpy(), R.mask(k, rows, cols, 3, thr)) and bool((buf[:, cols:] == 77).all())
    whole = pkg._native.dropout_mask_host(257, 201, k, 0, 0.3)
    for a, b in ((0, 64), (64, 129), (129, 257)):
        assert torch.equal(pkg._native.dropout_mask_host(b - a, 201, k, a, 0.3), whole[a:b])


@pytest.mark.parametrize('rows,cols,p', [(257, 200, 0.1), (257, 200, 0.3), (130, 100, 0.5), (1024, 3920, 0.3)])
def test_keep_rate_within_five_sigma(pkg, rows, cols, p):
    """Fixed inputs (seed 1234, step 0, site 0), so deterministic: |rate - keep| <= 5 sigma, sigma = sqrt(keep (1 - keep) / n)."""
    m = pkg._native.dropout_mask_host(rows, cols, R.key(1234, 0, 0), 0, p)
    n, keep = rows * cols, R.threshold(p) / 2.0 ** 32
    sigma = math.sqrt(keep * (1 - keep) / n)
    dev = abs(float(m.sum()) / n - keep) / sigma
    print('KEEP %dx%d p=%.1f: %.2f sigma' % (rows, cols, p, dev))
    assert dev <= 5.0
    assert set(np.unique(m.numpy())) <= {0, 1}


def test_step_site_seed_change_the_mask(pkg):
    nat = pkg._native
    base = nat.dropout_mask_host(64, 200, nat.dropout_key(1234, 0, 0), 0, 0.3)
    for other in ((1234, 1, 0), (1234, 0, 1), (1235, 0, 0), (1234, 0, 2), (1234, 0, 0x1000)):
        m = nat.dropout_mask_host(64, 200, nat.dropout_key(*other), 0, 0.3)
        frac = float((m != base).float().mean())
        assert 0.3 < frac < 0.54, (other, frac)            # independent masks differ on 2 keep (1 - keep) = 0.42 of the elements
    assert torch.equal(base, nat.dropout_mask_host(64, 200, nat.dropout_key(1234, 0, 0), 0, 0.3))
    assert not torch.equal(base[:63], nat.dropout_mask_host(63, 200, nat.dropout_key(1234, 0, 0), 1, 0.3))


def test_exports_and_header(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    for n in ('mgcn_dropout_apply', 'mgcn_dropout_apply_pair', 'mgcn_dropout_mask', 'mgcn_dropout_mask_host'):
        assert n in pkg._native.EXPORTS and n + '(' in header
    assert pkg._native.lib().mgcn_abi_version() == 4
    import __graft_entry__ as entry
    assert 'dropout.hip' in entry.SOURCES and len(entry.SOURCES) == 14


def test_argument_validation_without_a_gpu(pkg):
    """Every refusal comes before the first HIP call: MGCN_EINVAL on a machine with no GPU, nothing written."""
    lib = pkg._native.lib()
    buf = torch.zeros(64, dtype=torch.float32)
    other = torch.zeros(64, dtype=torch.float32)
    x, o = buf.data_ptr(), other.data_ptr()
    inf, nan = float('inf'), float('nan')
    bad_apply = [(-1, 4, x, 4, o, 4, 1.0), (2, 0, x, 4, o, 4, 1.0), (2, 4, None, 4, o, 4, 1.0), (2, 4, x, 4, None, 4, 1.0),
                 (2, 4, x, 3, o, 4, 1.0), (2, 4, x, 4, o, 3, 1.0), (2, 4, x, 4, o, 4, -1.0), (2, 4, x, 4, o, 4, inf),
                 (2, 4, x, 4, o, 4, nan), (2, 4, x, 4, x, 8, 1.0), (2 ** 40 + 1, 4, x, 4, o, 4, 1.0), (2 ** 40, 4, x, 2 ** 21, o, 4, 1.0)]
    for rows, cols, px, ldx, po, ldo, ik in bad_apply:
        assert lib.mgcn_dropout_apply(rows, cols, px, ldx, po, ldo, 1, 0, 5, ik, None) == EINVAL, (rows, cols, ldx, ldo, ik)
        assert lib.mgcn_last_error().decode().startswith('mgcn_dropout_apply:')
    third = torch.zeros(64, dtype=torch.float32).data_ptr()
    pair = lambda rows, cols, xa, lxa, oa, loa, xb, lxb, ob, lob, ik=1.0: lib.mgcn_dropout_apply_pair(
        rows, cols, xa, lxa, oa, loa, 1, xb, lxb, ob, lob, 2, 0, 5, ik, None)
    assert pair(2, 4, x, 4, o, 4, x, 4, o, 4) == EINVAL                   # one output for both sites
    assert pair(2, 4, None, 4, o, 4, x, 4, third, 4) == EINVAL
    assert pair(2, 4, x, 4, o, 4, x, 4, None, 4) == EINVAL
    assert pair(2, 4, x, 4, o, 4, x, 3, third, 4) == EINVAL
    assert pair(2, 4, x, 4, x, 5, o, 4, third, 4) == EINVAL               # in place with another leading dimension
    assert pair(2, 4, x, 4, o, 4, x, 4, third, 4, ik=nan) == EINVAL
    assert pair(-1, 4, x, 4, o, 4, x, 4, third, 4) == EINVAL
    assert lib.mgcn_last_error().decode().startswith('mgcn_dropout_apply_pair:')
    m = torch.zeros(64, dtype=torch.uint8).data_ptr()
    for rows, cols, pm, ldm in ((-1, 4, m, 4), (2, 0, m, 4), (2, 4, None, 4), (2, 4, m, 3), (2 ** 40 + 1, 4, m, 4)):
        assert lib.mgcn_dropout_mask(rows, cols, pm, ldm, 1, 0, 5, None) == EINVAL
        assert lib.mgcn_dropout_mask_host(rows, cols, pm, ldm, 1, 0, 5) == EINVAL
    assert bool((buf == 0).all()) and bool((other == 0).all())
    # rows == 0: nothing to do, no launch
    assert lib.mgcn_dropout_apply(0, 4, x, 4, o, 4, 1, 0, 5, 1.0, None) == 0
    assert lib.mgcn_dropout_mask(0, 4, m, 4, 1, 0, 5, None) == 0
    assert ctypes.sizeof(ctypes.c_uint64) == 8


def test_switch_default_and_override(pkg, monkeypatch):
    import types
    want = pkg.model._counter_dropout_wanted
    monkeypatch.delenv('MGCN_DROPOUT', raising=False)
    assert not want(types.SimpleNamespace()) and want(types.SimpleNamespace(dropout='counter'))
    monkeypatch.setenv('MGCN_DROPOUT', 'torch')
    assert not want(types.SimpleNamespace(dropout='counter'))
    monkeypatch.setenv('MGCN_DROPOUT', 'counter')
    assert want(types.SimpleNamespace()) and want(types.SimpleNamespace(dropout='torch'))


def test_load_checkpoint_restores_dropout_state(pkg, tmp_path):
    class Stub(object):
        state = None

        def load_state_dict(self, sd):
            self.loaded = sd

        def load_dropout_state(self, d):
            self.state = (int(d['dropout_seed']), int(d['dropout_step']))

    path = str(tmp_path / 'ckpt.pth.tar')
    torch.save({'state_dict': {}, 'dropout_state': {'dropout_seed': 3, 'dropout_step': 9}}, path)
    stub = Stub()
    pkg.utils.load_checkpoint(path, stub)
    assert stub.state == (3, 9)
    torch.save({'state_dict': {}}, path)                      # a checkpoint without it: the model's own state stays
    other = Stub()
    pkg.utils.load_checkpoint(path, other)
    assert other.state is None
