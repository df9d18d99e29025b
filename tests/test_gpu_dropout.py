"""The counter-based dropout (csrc/dropout.hip) on a real MI355X (`-m gpu`): the three kernels bit for bit against the
numpy restatement tests/dropout_ref.py over a grid of shapes, leading dimensions, base offsets, first rows and rates; the layer
Function with keys against float64 autograd with the reference's masks injected; the model's training step with the switch on
(reproducible, seed-dependent, resumable, eval untouched); one rank of train_step_sharded against the one-GPU step bit for bit at
dropout 0.3; two ranks against the one-process step of the same model."""
import numpy as np
import pytest
import torch

from . import dense_ref as D
from . import dropout_ref as R
from .test_gpu_train_sharded import _assemble, _batches, _job_batches, _models, _run_two_ranks

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = D.U

ROWS, COLS, PADS, OFFS = (1, 63, 64, 65, 257), (1, 3, 4, 5, 100, 200, 201), (0, 1, 4), (0, 1)
ROW0S, PS = (0, 7, 2 ** 32 - 3, 2 ** 40 + 1), (0.1, 0.3, 0.5)
KEY_A, KEY_B = R.key(1234, 3, 4), R.key(1234, 3, 5)
FILL = 7.5


def _inputs():
    """[257, 201] f32 with negative values, zeros of both signs, infinities and NaN in fixed places."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(max(ROWS), max(COLS), generator=g)
    flat = x.view(-1)
    for i, v in enumerate((0.0, -0.0, float('inf'), float('-inf'), float('nan'))):
        flat[i::13 + 2 * i] = v             # spread over every row of the grid
    flat[0], flat[1], flat[2] = float('nan'), float('inf'), -0.0
    return x


def _place(vals, ld, off, fill):
    """(whole buffer, view): `vals` [rows, cols] as a window with row stride ld starting `off` elements into a buffer of `fill`."""
    rows, cols = vals.shape
    full = torch.full((off + rows * ld + 3,), fill, dtype=vals.dtype, device=DEV)
    view = full[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(vals)
    return full, view


def _bits(t):
    """int32 bit patterns with every NaN made one value: equality of these is equality of the floats INCLUDING the sign of zeros."""
    if t.dtype != torch.float32:
        return t
    return torch.where(t.isnan(), torch.full_like(t, 1e30), t).view(torch.int32)


def _same(a, b):
    return (_bits(a) == _bits(b)).all()


@pytest.mark.parametrize('row0', ROW0S)
def test_kernels_equal_reference_on_the_grid(pkg, row0):
    """apply, apply_pair and mask against the reference for every (rows, cols, ld, base offset, p) of the grid at this row0: values
    bit for bit (dropped elements are +0.0 whatever the input held), padding untouched, in place = out of place, and a row slice
    launched with its own row0 = that slice of the whole launch. One device-side verdict per check, read back once."""
    nat = pkg._native
    x_all = _inputs()
    verdicts, labels = [], []

    def check(ok, *label):
        verdicts.append(ok.reshape(1))
        labels.append(label)

    for cols in COLS:
        words = [R.words(k, max(ROWS), cols, row0) for k in (KEY_A, KEY_B)]           # shared by every rows / p / layout below
        x_np = x_all[:, :cols].numpy()
        for p in PS:
            thr, inv = np.uint64(R.threshold(p)), np.float32(1.0 / (1.0 - p))
            keep = [w < thr for w in words]
            with np.errstate(all='ignore'):
                want = [torch.from_numpy(np.where(m, x_np * inv, np.float32(0.0)).astype(np.float32)).to(DEV) for m in keep]
            keep_t = [torch.from_numpy(m.astype(np.uint8)).to(DEV) for m in keep]
            for rows in ROWS:
                x = x_all[:rows, :cols].to(DEV)
                for pad in PADS:
                    for off in OFFS:
                        pt = (rows, cols, cols + pad, off, p)
                        ld = cols + pad
                        _, xv = _place(x, ld, off, FILL)
                        exp_a, ea = _place(want[0][:rows], ld, off, FILL)
                        exp_b, eb = _place(want[1][:rows], ld, off, FILL)
                        # apply, out of place into a padded window, then in place
                        full, ov = _place(torch.zeros_like(x), ld, off, FILL)
                        nat.dropout_apply(xv, KEY_A, row0, p, out=ov)
                        check(_same(full, exp_a), 'apply', *pt)
                        full, iv = _place(x, ld, off, FILL)
                        nat.dropout_apply(iv, KEY_A, row0, p, out=iv)
                        check(_same(full, exp_a), 'apply in place', *pt)
                        # pair from ONE input (the backward's shape), out of place; then in place on two windows
                        fa, oa = _place(torch.zeros_like(x), ld, off, FILL)
                        fb, ob = _place(torch.zeros_like(x), ld, off, FILL)
                        nat.dropout_apply_pair(xv, KEY_A, xv, KEY_B, row0, p, out_a=oa, out_b=ob)
                        check(_same(fa, exp_a) & _same(fb, exp_b), 'pair', *pt)
                        fa, ia = _place(x, ld, off, FILL)
                        fb, ib = _place(x, ld, off, FILL)
                        nat.dropout_apply_pair(ia, KEY_A, ib, KEY_B, row0, p, out_a=ia, out_b=ib)
                        check(_same(fa, exp_a) & _same(fb, exp_b), 'pair in place', *pt)
                        # dropped elements are +0.0 (bit pattern 0), also where the input held inf or NaN
                        check(((oa.view(torch.int32) == 0) | (keep_t[0][:rows] != 0)).all(), 'dropped are +0', *pt)
                        # keep bytes into a padded byte window
                        exp_m, _ = _place(keep_t[0][:rows], ld, off, 9)
                        fm, mv = _place(torch.zeros((rows, cols), dtype=torch.uint8), ld, off, 9)
                        nat.dropout_mask(rows, cols, KEY_A, row0, p, out=mv)
                        check(_same(fm, exp_m), 'mask', *pt)
                        if pad == 0 and off == 0:
                            mb = nat.dropout_mask(rows, cols, KEY_B, row0, p, device=DEV)
                            assert mb.dtype == torch.bool
                            check((mb == keep_t[1][:rows].bool()).all(), 'bool mask', *pt)
                        # rows [a, rows) launched with row0 + a are that slice of the whole launch
                        a = rows // 2
                        if rows > 1:
                            part = nat.dropout_apply(xv[a:], KEY_A, row0 + a, p)
                            check(_same(part, want[0][a:rows]), 'slice', *pt)
                            pm = nat.dropout_mask(rows - a, cols, KEY_A, row0 + a, p, device=DEV)
                            check(_same(pm.to(torch.uint8), keep_t[0][a:rows]), 'mask slice', *pt)
    res = torch.cat(verdicts).cpu()
    bad = [labels[i] for i in torch.nonzero(~res).flatten().tolist()]
    assert not bad, '%d of %d checks failed, first: %s' % (len(bad), len(labels), bad[:8])


def test_p_one_gives_zeros_and_wrappers_refuse_bad_layouts(pkg):
    nat = pkg._native
    x = torch.full((65, 201), float('nan'), device=DEV)
    out = nat.dropout_apply(x, KEY_A, 0, 1.0)
    assert bool((out.view(torch.int32) == 0).all())
    assert not bool(nat.dropout_mask(65, 201, KEY_A, 0, 1.0, device=DEV).any())
    with pytest.raises(nat.NativeError):
        nat.dropout_apply(x.t(), KEY_A, 0, 0.3)
    with pytest.raises(nat.NativeError):
        nat.dropout_apply(x.cpu(), KEY_A, 0, 0.3)
    with pytest.raises(nat.NativeError):
        nat.dropout_apply_pair(x, KEY_A, x, KEY_B, 0, 0.3, out_a=x, out_b=x)


# -- the layer Function with keys ------------------------------------------------------------------------------------
def _layer_ref(ts, m_in, m_out, inv_keep, rm, rv, gy, dtype):
    """The layer's formula with the masks injected, forward and backward through torch-CPU autograd in `dtype`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in ts]
    agg, a_loop, w_in, w_out, w_loop, bias, gamma, beta = leaves
    d = w_in.size(0)
    mi, mo = m_in.to(dtype), m_out.to(dtype)
    ik = torch.tensor(inv_keep, dtype=torch.float32).to(dtype)
    out = ((agg[:, :d] @ w_in) * mi * ik + (agg[:, d:] @ w_out) * mo * ik + a_loop @ w_loop) / 3 + bias
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = torch.tanh(torch.nn.functional.batch_norm(out, rm, rv, gamma, beta, True, 0.1, 1e-5))
    y.backward(gy.to(dtype))
    res = dict(y=y.detach(), rm=rm, rv=rv)
    res.update({n: t.grad for n, t in zip(('agg', 'a_loop', 'w_in', 'w_out', 'w_loop', 'bias', 'gamma', 'beta'), leaves)})
    return res, out.detach()


@pytest.mark.parametrize('N', [127, 129])
def test_layer_fn_with_keys_vs_float64(pkg, N):
    """_LayerTrainFn with (key_in, key_out, row0) at D = 100, O = 200, p = 0.1 against float64 autograd of the same formula with the
    reference's masks injected. Bars as for the same entry points at dropout 0: dense_ref.derived_bar -- 4 x what the same formula
    in torch-CPU f32 is off float64 on these inputs, floored at 8 u of the terms of the result's last additions, capped by
    test_training_layer_kernels_vs_torch_autograd's bars (y 2e-6, gradients 2e-5 of their largest entry) where torch-CPU f32
    itself meets them. The mask adds one f32 multiply per element, which the floors (relative to the sums' terms) cover.
    The Function saves no bool tensor."""
    Din, O, p, row0 = 100, 200, 0.1, 5
    g = torch.Generator().manual_seed(N)
    agg, a_loop = torch.randn(N, 2 * Din, generator=g) * 0.5, torch.randn(N, Din, generator=g) * 0.5
    ws = [torch.randn(Din, O, generator=g) * 0.1 for _ in range(3)]
    bias, gamma, beta = torch.randn(O, generator=g) * 0.1, torch.rand(O, generator=g) + 0.5, torch.randn(O, generator=g) * 0.1
    rm, rv = torch.randn(O, generator=g) * 0.05, torch.rand(O, generator=g) + 0.5
    gy = torch.randn(N, O, generator=g)
    ts = [agg, a_loop] + ws + [bias, gamma, beta]
    k_in, k_out = R.key(77, 2, R.layer_site(1, 0)), R.key(77, 2, R.layer_site(1, 1))
    thr = R.threshold(p)
    m_in, m_out = (torch.from_numpy(R.mask(k, N, O, row0, thr)) for k in (k_in, k_out))
    inv_keep = 1.0 / (1.0 - p)
    r64, out64 = _layer_ref(ts, m_in, m_out, inv_keep, rm, rv, gy, torch.float64)
    r32, _ = _layer_ref(ts, m_in, m_out, inv_keep, rm, rv, gy, torch.float32)
    cpu_err = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}

    leaves = [t.to(DEV).requires_grad_(True) for t in ts]
    rm1, rv1 = rm.to(DEV), rv.to(DEV)
    y = pkg.model._LayerTrainFn.apply(*leaves, rm1, rv1, 0.1, 1e-5, p, (k_in, k_out, row0))
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert saved and all(t.dtype == torch.float32 for t in saved), [t.dtype for t in saved]      # no bool / byte mask is kept
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    got = dict(y=y.detach(), rm=rm1, rv=rv1)
    got.update({n: t.grad for n, t in zip(('agg', 'a_loop', 'w_in', 'w_out', 'w_loop', 'bias', 'gamma', 'beta'), leaves)})

    # the terms of each result's last additions, in float64
    a64, l64, w64 = agg.double(), a_loop.double(), [w.double() for w in ws]
    z = out64.detach().requires_grad_(True)
    yy = torch.tanh(torch.nn.functional.batch_norm(z, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5))
    yy.backward(gy.double())
    gz64 = z.grad
    gu = gz64.abs() / 3
    g_in, g_out = gu * m_in * inv_keep, gu * m_out * inv_keep
    xh = (out64 - out64.mean(0)) / torch.sqrt(out64.var(0, unbiased=False) + 1e-5)
    gp = (gy.double() * (1 - r64['y'] ** 2)).abs()
    mag = {
        'agg': max(float((g_in @ w64[0].abs().t()).max()), float((g_out @ w64[1].abs().t()).max())),
        'a_loop': float((gu @ w64[2].abs().t()).max()),
        'w_in': float((a64[:, :Din].abs().t() @ g_in).max()), 'w_out': float((a64[:, Din:].abs().t() @ g_out).max()),
        'w_loop': float((l64.abs().t() @ gu).max()),
        'bias': float(gz64.abs().sum(0).max()), 'gamma': float((gp * xh.abs()).sum(0).max()), 'beta': float(gp.sum(0).max()),
    }
    today = {'y': 2e-6, 'rm': 1e-6 * float(r64['rm'].abs().max()) + 1e-7, 'rv': 1e-5 * float(r64['rv'].abs().min()) + 1e-7, 'bias': 2e-3}
    floors = {'y': 8 * U, 'rm': 8 * U * float(r64['rm'].abs().max()), 'rv': 8 * U * float(r64['rv'].abs().max())}
    for name in r64:
        floor = floors.get(name, 8 * U * mag.get(name, 0.0))
        cap = today.get(name, 2e-5 * float(r64[name].abs().max()))
        bar = D.derived_bar(cpu_err[name], floor, cap)
        err = float((got[name].detach().cpu().double() - r64[name]).abs().max())
        print('RATIO layer_drop N=%d %s %.4f (err %.3g, bar %.3g, cpu f32 %.3g)' % (N, name, err / bar, err, bar, cpu_err[name]))
        assert err <= bar, (name, err, bar)
    # the masks really are the reference's: the same call without keys (torch masks) differs, and the same keys reproduce the bits
    y2 = pkg.model._LayerTrainFn.apply(*[t.detach() for t in leaves], rm.to(DEV), rv.to(DEV), 0.1, 1e-5, p, (k_in, k_out, row0))
    assert torch.equal(y2, y.detach())


# -- the model's training step -------------------------------------------------------------------------------------
def _train_model(pkg, case, layers, seed=None):
    model, dl, params = _models(pkg, case, layers, dropout=0.3)
    for layer in [model.conv1] + list(model.conv1_extra):
        layer.drop.p = 0.3                                   # 0.3 on all five sites
    if seed is not None:
        model.dropout_seed = seed
    return model, dl, params


def _steps(model, dl, batches, opt=None):
    idx = dl.train_index().to(DEV)
    opt = opt or torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()
    losses = []
    for q in batches:
        opt.zero_grad()
        loss = model.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=0.5)
        opt.step()
        losses.append(float(loss.detach()))
    return losses, opt


def _equal_states(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize('hip', [False, True], ids=['torch_trunk', 'hip_trunk_and_query'])
@pytest.mark.parametrize('case,layers', [('syn_b', 1), ('syn_a', 2)])
def test_model_training_is_a_function_of_the_seed(pkg, monkeypatch, case, layers, hip):
    """Dropout 0.3 on all five sites with the switch on: two runs from the same seed give bit-identical parameters after 3 steps,
    another dropout_seed does not, load_dropout_state resumes mid-run to the same bits, and eval outputs do not see the switch."""
    monkeypatch.setenv('MGCN_DROPOUT', 'counter')
    if hip:
        monkeypatch.setenv('MGCN_TRUNK_TRAIN', 'hip')
        monkeypatch.setenv('MGCN_QUERY_TRAIN', 'hip')
    else:
        monkeypatch.delenv('MGCN_TRUNK_TRAIN', raising=False)
        monkeypatch.delenv('MGCN_QUERY_TRAIN', raising=False)
    torch.use_deterministic_algorithms(True, warn_only=True)      # (the torch trunk's index_select backward: no float atomics)
    try:
        a, dl, _ = _train_model(pkg, case, layers)
        batches = _batches(dl, 3)
        la, _ = _steps(a, dl, batches)
        assert a.dropout_state() == {'dropout_seed': 0, 'dropout_step': 3}
        if hip:
            assert getattr(a.conv2, '_trunk_train_count', 0) == 3 and getattr(a.conv2, '_tail_train_count', 0) == 3
        b, dl_b, _ = _train_model(pkg, case, layers)
        lb, _ = _steps(b, dl_b, batches)
        assert la == lb and _equal_states(a, b)
        c, dl_c, _ = _train_model(pkg, case, layers, seed=1)
        lc, _ = _steps(c, dl_c, batches)
        assert lc[0] != la[0] and not _equal_states(a, c)
        # resume: two steps, carry state_dict + optimizer state + dropout_state into a fresh model, one more step
        d, dl_d, _ = _train_model(pkg, case, layers)
        _, opt_d = _steps(d, dl_d, batches[:2])
        e, dl_e, _ = _train_model(pkg, case, layers, seed=99)
        e.load_state_dict(d.state_dict())
        e.load_dropout_state(d.dropout_state())
        opt_e = torch.optim.Adam(e.parameters(), lr=1e-3)
        e.load_optimizer_state_dict(opt_e, d.optimizer_state_dict(opt_d))
        le, _ = _steps(e, dl_e, batches[2:], opt_e)
        assert le[0] == la[2] and _equal_states(a, e)
        # the torch masks are other masks (the switch does something), and eval does not see the switch
        monkeypatch.setenv('MGCN_DROPOUT', 'torch')
        t, dl_t, _ = _train_model(pkg, case, layers)
        torch.manual_seed(0)
        lt, _ = _steps(t, dl_t, batches[:1])
        assert lt[0] != la[0] and t.dropout_state()['dropout_step'] == 0
        a.eval()
        q = batches[0]
        with torch.no_grad():
            off = a(q[:, 0], q[:, 1], dl.graph).clone()
        monkeypatch.setenv('MGCN_DROPOUT', 'counter')
        a._enc_cache = None
        with torch.no_grad():
            on = a(q[:, 0], q[:, 1], dl.graph)
        assert torch.equal(on, off) and a.dropout_state()['dropout_step'] == 3
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize('case,layers,shard', [('syn_b', 1, False), ('syn_a', 2, True)])
def test_world1_equals_one_gpu_step_at_dropout(pkg, monkeypatch, case, layers, shard):
    """The mirror of test_world1_equals_one_gpu_step at dropout 0.3 with the switch on: train_step_sharded with one rank and
    forward_loss + backward + clip_grad_norm_ + Adam, 3 steps each: losses, every parameter and BN statistic bit-identical."""
    monkeypatch.setenv('MGCN_DROPOUT', 'counter')
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        ref, dl, params = _models(pkg, case, layers, dropout=0.3)
        sm, dl_s, _ = _models(pkg, case, layers, dropout=0.3, shard=shard)
        for m in (ref, sm):
            for layer in [m.conv1] + list(m.conv1_extra):
                layer.drop.p = 0.3
        idx = dl.train_index().to(DEV)
        opt_r, opt_s = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.optim.Adam(sm.parameters(), lr=1e-3)
        ref.train()
        for q in _batches(dl, 3):
            opt_r.zero_grad()
            loss_r = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.1)
            loss_r.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=0.5)
            opt_r.step()
            loss_s = pkg.dist.train_step_sharded(sm, dl_s.graph, q[:, 0], q[:, 1], idx, opt_s, lbl_smooth=0.1, clip=0.5)
            assert torch.equal(loss_s, loss_r.detach())
    finally:
        torch.use_deterministic_algorithms(False)
    assert ref.dropout_state() == sm.dropout_state() == {'dropout_seed': 0, 'dropout_step': 3}
    sd_r, sd_s = ref.state_dict(), sm.state_dict()
    names = {'edge_embeddings'} | {'edge_embeddings_extra.%d' % i for i in range(layers - 1)}
    for k, v in sd_r.items():
        if k in names and shard:                                 # the shard model's state holds slot order
            v = v.index_select(0, ref._slot_csr.perm)
        assert torch.equal(sd_s[k], v), k


def test_two_ranks_dropout_match_single_step(pkg, monkeypatch):
    """Two processes over gloo (both on one GPU), one step of the 2-layer syn_b at dropout 0.3 with the switch on, against the
    one-process step of the same model with the same switch, with the tolerances test_two_ranks_one_gpu_match_golden_and_single_step
    uses at dropout 0: loss 1e-5, gradients rtol 2e-3 / atol 2e-5 scale + floor, tables 1e-5 after the step, replicated state
    bit-identical on both ranks. (Only the masks being the same on any partition makes this comparison possible.)"""
    monkeypatch.setenv('MGCN_DROPOUT', 'counter')               # spawned children inherit it
    name, case, layers, dropout = 'drop1', 'syn_b', 2, 0.3
    got = _run_two_ranks([(name, case, layers, dropout, 1)])
    ref, dl, params = _models(pkg, case, layers, dropout)
    idx = dl.train_index().to(DEV)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    q = _job_batches(name, case, dl, 1)[0]
    ref.train()
    opt.zero_grad()
    loss = ref.forward_loss(q[:, 0], q[:, 1], dl.graph, idx, lbl_smooth=0.0)
    loss.backward()
    want_grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    opt.step()
    inv = ref._slot_csr.inv_perm
    for n in want_grads:
        if n.startswith('edge_embeddings'):
            want_grads[n] = want_grads[n].index_select(0, inv)   # slot order -> reference order
    for r in (0, 1):
        print('LOSS rank %d %.8f one process %.8f' % (r, got[r][name]['losses'][0], float(loss.detach())))
        assert abs(got[r][name]['losses'][0] - float(loss.detach())) < 1e-5, r
    tgrads = _assemble(got, name, 'grads')
    for n, want in want_grads.items():
        gr = tgrads[n] if n.startswith('edge_embeddings') else got[0][name]['grads'][n]
        if not n.startswith('edge_embeddings'):
            assert np.array_equal(got[0][name]['grads'][n], got[1][name]['grads'][n]), n
        ref_g = want.cpu()
        scale = float(ref_g.abs().max()) + 1e-12
        floor = 2e-6 if n.startswith('conv2.') else 1e-9
        np.testing.assert_allclose(gr, ref_g.numpy(), rtol=2e-3, atol=2e-5 * scale + floor, err_msg=n)
    for k, v in got[0][name]['state'].items():                 # replicated state: the same bits on both ranks
        assert np.array_equal(v, got[1][name]['state'][k]), k
    ref_sd = ref.state_dict()
    for tname, t in _assemble(got, name, 'tables').items():
        np.testing.assert_allclose(t, ref_sd[tname].cpu().numpy(), rtol=0, atol=1e-5, err_msg=tname)
