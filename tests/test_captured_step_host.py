"""The host side of the captured training step, without a GPU: the four device-scalar entry points exist in the
library and the header under ABI 4, the step word composes to the site keys, and ClipAdam's hyperparameter helper returns the
doubles of the formulas that used to stand inline in _hip_update."""
import ctypes
import os
import re

import pytest

from .conftest import ROOT

NEW_SYMBOLS = ('mgcn_adam_step_dev', 'mgcn_dropout_apply_dev', 'mgcn_dropout_apply_pair_dev', 'mgcn_dropout_mask_dev')
M64 = (1 << 64) - 1


def _sm(x):
    """One SplitMix64 step, restated from include/mgcn_hip.h (12)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_new_symbols_in_library_and_header_under_abi_4(pkg):
    nat = pkg._native
    handle = ctypes.CDLL(nat.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'mgcn_hip.h')) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert name in nat.EXPORTS, name
        assert re.search(r'^int %s\(' % name, header, re.M), name
    assert nat.ABI_VERSION == 4 and handle.mgcn_abi_version() == 4
    assert re.search(r'#define\s+MGCN_ABI_VERSION\s+4\b', header)


def test_the_device_forms_refuse_a_null_or_misaligned_scalar_pointer(pkg):
    """The checks that precede every launch need no GPU: a NULL or misaligned hyper / step word is MGCN_EINVAL."""
    lib = pkg._native.lib()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(18)
    n0 = (ctypes.c_int64 * 1)(0)
    arr = (ctypes.c_void_p * 1)(None)
    for hyper in (None, two):
        assert lib.mgcn_adam_step_dev(1, arr, arr, arr, arr, n0, None, hyper, 0.9, 0.999, 1e-8, 0.0, None) == 1
        assert lib.mgcn_last_error()
    for word in (None, ctypes.c_void_p(20)):
        assert lib.mgcn_dropout_apply_dev(0, 4, one, 4, one, 4, word, 0, 0, 1, 1.0, None) == 1
        assert lib.mgcn_dropout_apply_pair_dev(0, 4, one, 4, one, 4, 0, one, 4, two, 4, 1, word, 0, 1, 1.0, None) == 1
        assert lib.mgcn_dropout_mask_dev(0, 4, one, 4, word, 0, 0, 1, None) == 1
    # rows == 0 with good pointers launches nothing and succeeds
    assert lib.mgcn_dropout_apply_dev(0, 4, one, 4, one, 4, one, 0, 0, 1, 1.0, None) == 0
    assert lib.mgcn_dropout_mask_dev(0, 4, one, 4, one, 0, 0, 1, None) == 0


def test_step_key_composes_to_the_site_keys(pkg):
    nat = pkg._native
    edge = (0, 1, 7, 1234, 2 ** 32, 2 ** 63, M64)
    sites = (0, 1, 2, 4, 0x1000, 0x1001)
    for seed in edge:
        for step in edge:
            word = nat.dropout_step_key(seed, step)
            assert 0 <= word <= M64
            assert word == _sm(_sm(seed) ^ step)
            for site in sites:
                assert nat.dropout_key(seed, step, site) == _sm(word ^ site), (seed, step, site)
    assert nat.dropout_layer_site(0, 0) == 0 and nat.dropout_layer_site(1, 0) == 4
    assert (nat.DROPOUT_SITE_FEATURE, nat.DROPOUT_SITE_HIDDEN) == (0x1000, 0x1001)


@pytest.mark.parametrize('beta1,beta2,lr', [(0.9, 0.999, 1e-3), (0.5, 0.9, 0.25)])
def test_clip_adam_hyper_helper_is_the_old_inline_arithmetic(pkg, beta1, beta2, lr):
    group = {'betas': (beta1, beta2), 'lr': lr}
    for step in (1, 2, 1000):
        s = float(step)
        want = (lr / (1 - beta1 ** s), (1 - beta2 ** s) ** 0.5)              # the two lines _hip_update held
        got = pkg.ClipAdam._step_hyper(group, s)
        assert got == want and all(isinstance(v, float) for v in got)


def test_captured_step_is_exported_and_refuses_a_cpu_model(pkg):
    """The wrapper's refusals come before anything touches a GPU: a model on the CPU raises NativeError and captures nothing."""
    import types

    import torch
    params = types.SimpleNamespace(gcn_in_dim=8, gcn_out_dim=8, num_filter=2, kernel_size=3, k_w=2, k_h=4, bias=False, hidden_drop=0.0,
                                   feat_drop=0.0, gcn_drop=0.0)
    model = pkg.MGCN(5, 2, 6, params).train()
    opt = pkg.ClipAdam(model.parameters(), lr=1e-3)
    step = pkg.CapturedTrainStep(model, None, None, opt)
    src = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(pkg._native.NativeError, match='CPU'):
        step(src, src)
    assert step.captures == 0 and step.replays == 0 and step.eager_steps == 0 and not step.disabled
    assert 'captured' in pkg.harness.train_device_labels.__code__.co_varnames
