"""The host side of the captured sampled-negative step (kgc-gcn_amd/captured.py), without a GPU: the device-key draw
exists in the library, the header and EXPORTS under ABI 4, refuses a bad word pointer before any HIP call, the step word composes
to the list key, and the wrapper is exported and refuses a CPU model with nothing counted."""
import ctypes
import inspect
import os
import re

import pytest

from .conftest import ROOT

M64 = (1 << 64) - 1
SITE = 0x2000


def _sm(x):
    """One SplitMix64 step, restated from include/mgcn_hip.h (12)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_the_symbol_in_library_header_and_exports_under_abi_4(pkg):
    nat = pkg._native
    handle = ctypes.CDLL(nat.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'mgcn_hip.h')) as f:
        header = f.read()
    name = 'mgcn_cand_draw_dev'
    assert hasattr(handle, name) and name in nat.EXPORTS
    proto = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M)
    assert proto and 'const uint64_t *step_key_dev, uint64_t site' in ' '.join(proto.group(1).split())
    assert nat.ABI_VERSION == 4 and handle.mgcn_abi_version() == 4
    assert re.search(r'#define\s+MGCN_ABI_VERSION\s+4\b', header)


@pytest.mark.parametrize('batch', [0, 4])
def test_a_null_or_misaligned_word_is_refused_before_any_hip_call(pkg, batch):
    """MGCN_EINVAL (1) with the message set, whatever the batch; good pointers with batch == 0 launch nothing and return 0."""
    lib = pkg._native.lib()
    p = ctypes.c_void_p(64)
    for word in (None, ctypes.c_void_p(20), ctypes.c_void_p(1)):
        rc = lib.mgcn_cand_draw_dev(batch, 3, 7, p, 1, p, p, p, 1, word, SITE, 0, p, 3, p, 3, None)
        assert rc == 1
        assert b'mgcn_cand_draw_dev' in lib.mgcn_last_error() and b'step_key' in lib.mgcn_last_error()
    if batch == 0:
        assert lib.mgcn_cand_draw_dev(0, 3, 7, p, 1, p, p, p, 1, ctypes.c_void_p(24), SITE, 0, p, 3, p, 3, None) == 0
        assert lib.mgcn_cand_draw_dev(0, 3, 7, p, 1, p, p, p, 1, ctypes.c_void_p(24), SITE, 0, p, 3, None, 0, None) == 0
        # the by-value form's other checks hold in the device form too
        assert lib.mgcn_cand_draw_dev(0, 0, 7, p, 1, p, p, p, 1, ctypes.c_void_p(24), SITE, 0, p, 3, None, 0, None) == 1


def test_the_step_word_composes_to_the_list_key(pkg):
    nat = pkg._native
    edge = (0, 1, 7, 1234, 2 ** 32, 2 ** 63, M64)
    assert nat.CAND_DRAW_SITE == SITE
    for seed in edge:
        for step in edge:
            word = nat.dropout_step_key(seed, step)
            assert word == _sm(_sm(seed) ^ step)
            assert nat.dropout_key(seed, step, SITE) == _sm(word ^ SITE), (seed, step)


def test_wrapper_is_exported_and_refuses_a_cpu_model(pkg):
    import types

    import torch
    assert issubclass(pkg.CapturedCandidateStep, pkg.CapturedTrainStep) and pkg.captured.CapturedCandidateStep is pkg.CapturedCandidateStep
    params = types.SimpleNamespace(gcn_in_dim=8, gcn_out_dim=8, num_filter=2, kernel_size=3, k_w=2, k_h=4, bias=False, hidden_drop=0.0,
                                   feat_drop=0.0, gcn_drop=0.0)
    model = pkg.MGCN(5, 2, 6, params).train()
    opt = pkg.ClipAdam(model.parameters(), lr=1e-3)
    step = pkg.CapturedCandidateStep(model, None, None, opt, 4, 99, draw_step=5)
    src = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(pkg._native.NativeError, match='CPU'):
        step(src, src)
    assert step.captures == 0 and step.replays == 0 and step.eager_steps == 0 and not step.disabled
    assert (step.draw_seed, step.draw_step, step.num_neg, step.loss) == (99, 5, 4, 'bce')
    sig = inspect.signature(pkg.harness.train_sampled_negatives)
    assert 'captured' in sig.parameters and sig.parameters['captured'].default is None
    sig = inspect.signature(pkg.harness.draw_candidates)
    assert sig.parameters['step_key_dev'].default is None
