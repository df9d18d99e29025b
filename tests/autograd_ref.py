"""Cases, gradient layouts and float64 restatements for the torch.autograd.Function classes of kgc-gcn_amd/model.py and
kgc-gcn_amd/dist.py: the layer between autograd and the C ABI, which turns whatever gradient a downstream op hands over into
pointers and leading dimensions. A plain CPU module: tests/test_autograd_ref_host.py checks the layout makers and holds every
restatement to plain float64 torch autograd of the oracle's formula; tests/test_gpu_autograd_contract.py holds the Functions to
them on the GPU.

Layouts of a gradient G [R, C] (make_layout; the same VALUES in every one of them):
  (a) contiguous   a tensor of its own;
  (b) window5      columns [0, C) of [R, C + 5] whose spare columns hold NaN;
  (c) offset3      columns [3, C + 3) of [R, C + 3] (what torch.cat([other [R, 3], y], 1) hands y): the base is 12 bytes past a
                   16-byte boundary and the row stride C + 3 is not a multiple of 4 (every case has C % 4 != 1);
  (d) transposed   strides (1, R);
  (e) rows         rows [1, R + 1) of a contiguous [R + 2, C];
  (f) rowexp       one row expanded, strides (0, 1) (what y.sum(0) * v hands y);
  (g) scalar       one value expanded, strides (0, 0) (what y.sum() hands y).

Shapes: one small case per Function, the smallest of its family's grid the Function takes with an output that has C % 4 != 1.
  aggregate   aggregate_ref.degree_profile(4) (42 nodes), D = 4 (ALIGNED_CASES[0]);
  layer       130 rows (one 128-row BN block and two rows), D = 5, O = 18: agg[:, 5:] starts 20 bytes into a row of 40 bytes, off
              the 16-byte grid in every row; matmul and matmul_tn take such windows on their guarded paths ((5, 18) is the guarded
              geometry of dense_ref.BN_TANH_CASES);
  trunk       (3, 8, 3, 6, conv bias), B = 17, feature dropout 0.2: trunk_train_ref.reference's own inputs;
  tail        B = 17, O = 32, p = 0.3: query_train_ref.tail_reference's own inputs;
  row gather  B = 17 into a 33 x 7 table, one index four times;
  dropout     [33, 12], p = 0.3, first global row 5: the contiguous and row-window gradients take the kernel's 16-byte path, the
              column windows (row strides 17 and 15) its scalar path;
  score       (3, 15, 4), the smallest of dense_ref.SCORE_CASES with more than one output element;
  score BCE   (4, 1, 4, 0.0), the smallest of dense_ref.BCE_CASES, and (36, 33, 4, 0.1), the smallest with more than one entity
              per axis and smoothed targets;
  list BCE    (B, K, N, dim) = (4, 15, 1000, 7), the smallest of test_gpu_cand_train's GRID with dead positions;
  list CE     (dim, K) = (4, 63) at B = 8, N = 97, smoothing 0.1: the smallest of test_gpu_cand_ce's GRID with every edge kind of
              cand_ce_ref planted and K no multiple of 64.

The scalar losses under an upstream gradient gl (section (3) of the tests). Every gradient of the three loss Functions is a sum
  r = sum_j g_j a_j                                                                              (j: list positions / entities / queries)
of the forward's d loss / d logit g_j times an operand a_j. The family's tests hold the unit-gradient result to a bar b1 that
carries g's own bar through the sum and adds the f32 sum itself (cand_ce_ref.grad_bars; list_grad_bars and score_bce_reference below
restate that for BCE). With gl = 3 the Functions compute either fl(g_j gl) first (_CandBCEFn, _CandCEFn: g * gl) and then the same
sum, or the same sum first and fl(r gl) last (_ScoreBCEFn). Both are linear in g, so an error e of the unit result becomes 3 e:
3 b1. The one extra rounding: fl(g_j 3) = 3 g_j (1 + d_j), |d_j| <= u = 2^-24, moves addend j by at most u |3 g_j a_j|, the sum by
at most 3 u sum_j |g_j a_j|; fl(3 r) moves the result by u |3 r| <= 3 u sum_j |g_j a_j| as well. So
  b3 = 3 b1 + 3 u sum_j |g_j a_j|,
and no constant is new. With gl = 0.25 (a power of two) every product, every fixed-order sum and g * gl itself scale exactly, so
the gradients are 0.25 times the unit ones bit for bit provided nothing underflows: the inputs must have float64 reference
gradients that are exactly zero or above 2^-100 in magnitude (scale_safe; the host test asserts it)."""
import collections
import functools
import math

import numpy as np
import torch
from . import aggregate_ref as A
from . import cand_ce_ref as E
from . import cand_train_ref as C
from . import dense_ref as R
from . import dropout_ref as DR
from . import query_train_ref as Q
from . import trunk_ref as T
from . import trunk_train_ref as TT

U = R.U
BN_EPS, BN_MOMENTUM = R.BN_EPS, R.BN_MOMENTUM

# ---------------------------------------------------------------------------------------------------------------- layouts
FREE_LAYOUTS = ('contiguous', 'window5', 'offset3', 'transposed', 'rows')       # (a) .. (e): any values
EXPANDED_LAYOUTS = ('rowexp', 'scalar')                                        # (f), (g): the values are not free


def make_layout(G, kind):
    """(view, base): the values of the 2-d f32 tensor G laid out as `kind` on G's device, and the allocation behind the view
    (what the test compares bit for bit before and after a backward). For 'rowexp' the values are G's first row in every row, for
    'scalar' G[0, 0] everywhere."""
    r, c = G.shape
    nan = float('nan')
    if kind == 'contiguous':
        base = G.clone().contiguous()
        return base, base
    if kind == 'window5':
        base = torch.full((r, c + 5), nan, dtype=G.dtype, device=G.device)
        view = base[:, :c]
    elif kind == 'offset3':
        assert (c + 3) % 4 != 0, 'C + 3 = %d is a multiple of 4: the row stride would stay on the 16-byte grid' % (c + 3)
        base = torch.full((r, c + 3), nan, dtype=G.dtype, device=G.device)
        view = base[:, 3:]
    elif kind == 'transposed':
        base = torch.empty((c, r), dtype=G.dtype, device=G.device)
        view = base.t()
    elif kind == 'rows':
        base = torch.full((r + 2, c), nan, dtype=G.dtype, device=G.device)
        view = base[1:r + 1]
    elif kind == 'rowexp':
        base = G[0].clone().contiguous()
        return base.unsqueeze(0).expand(r, c), base
    elif kind == 'scalar':
        base = G[0, 0].clone()
        return base.expand(r, c), base
    else:
        raise ValueError(kind)
    view.copy_(G)
    return view, base


def expected_layout(kind, r, c):
    """(strides, data_ptr() % 16) of make_layout(G [r, c], kind)[0] for a base allocation on a 16-byte boundary."""
    return {'contiguous': ((c, 1), 0), 'window5': ((c + 5, 1), 0), 'offset3': ((c + 3, 1), 12), 'transposed': ((1, r), 0),
            'rows': ((c, 1), (4 * c) % 16), 'rowexp': ((0, 1), 0), 'scalar': ((0, 0), 0)}[kind]


def bits(t):
    """The bit pattern of a tensor (NaN compares equal to itself): int32 words of f32, the bytes of anything else."""
    t = t.detach()
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32) if t.dim() else t.reshape(1).view(torch.int32)
    return t.contiguous().clone()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def scale_safe(grads64):
    """Whether every float64 reference gradient is exactly zero or above 2^-100 in magnitude: the condition under which scaling the
    loss by a power of two scales every f32 product and fixed-order sum exactly."""
    return all(bool(((v == 0) | (v.abs() > 2.0 ** -100)).all()) for v in grads64)


# ---------------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple('Case', 'name inputs extra G')
# inputs: OrderedDict name -> CPU f32 tensor, the differentiable inputs in the order of the Function's arguments;
# extra: everything else the call needs (CPU tensors, scalars); G: the upstream gradient [R, C] (None: a scalar loss)


def _od(*pairs):
    return collections.OrderedDict(pairs)


@functools.lru_cache(maxsize=None)
def aggregate_case():
    N, Rn, ei, et = A.degree_profile(4)
    D = A.ALIGNED_CASES[0].d
    inp = A.make_inputs('autograd-contract-aggregate', N, 2 * Rn + 1, ei.size(1), D)
    # (ee in EDGE-ID order here: the device test permutes it into slot order, and the reference's gee likewise)
    return Case('aggregate', _od(('x', inp.x), ('rel', inp.rel), ('ee', inp.ee)), dict(N=N, R=Rn, ei=ei, et=et, D=D), inp.g)


LAYER_N, LAYER_D, LAYER_O = 130, 5, 18
LAYER_NAMES = ('agg', 'a_loop', 'w_in', 'w_out', 'w_loop', 'bias', 'gamma', 'beta')


@functools.lru_cache(maxsize=None)
def layer_case():
    """The inputs of test_gpu_dropout.py::test_layer_fn_with_keys_vs_float64 at N = 130, D = 5, O = 18."""
    N, Din, O = LAYER_N, LAYER_D, LAYER_O
    g = R.gen(R.seed_of(71, N, Din, O))
    agg, a_loop = torch.randn(N, 2 * Din, generator=g) * 0.5, torch.randn(N, Din, generator=g) * 0.5
    # (that test's weights are 0.1 randn at D = 100: products of standard deviation 0.5. The same products at D = 5 need
    # 0.1 sqrt(100 / D); with 0.1 itself the pre-activation has a standard deviation of 0.07, batch norm multiplies every rounding of
    # it by rstd = 14, and y is no longer conditioned the way the family's absolute floor of 8 u on y assumes)
    ws = [torch.randn(Din, O, generator=g) * (0.1 * math.sqrt(100.0 / Din)) for _ in range(3)]
    bias, gamma, beta = torch.randn(O, generator=g) * 0.1, torch.rand(O, generator=g) + 0.5, torch.randn(O, generator=g) * 0.1
    rm, rv = torch.randn(O, generator=g) * 0.05, torch.rand(O, generator=g) + 0.5
    gy = torch.randn(N, O, generator=g)
    row0, p = 5, 0.3
    keys = (DR.key(77, 2, DR.layer_site(1, 0)), DR.key(77, 2, DR.layer_site(1, 1)))
    return Case('layer', _od(*zip(LAYER_NAMES, [agg, a_loop] + ws + [bias, gamma, beta])),
                dict(rm=rm, rv=rv, p=p, keys=keys, row0=row0), gy)


def layer_key_masks(case):
    """(m_in, m_out) bool [N, O] of the case's counter-based keys, from the definition (dropout_ref)."""
    thr = DR.threshold(case.extra['p'])
    return tuple(torch.from_numpy(DR.mask(k, LAYER_N, LAYER_O, case.extra['row0'], thr)).bool() for k in case.extra['keys'])


TRUNK = ((3, 8, 3, 6, True), 17, 0.2)
TRUNK_NAMES = ('s', 'r', 'conv_w', 'conv_b', 'fc_w', 'fc_b', 'g0', 'b0', 'g1', 'b1')
TRUNK_KEYS = ('conv_e.weight', 'conv_e.bias', 'fc.weight', 'fc.bias', 'bn0.weight', 'bn0.bias', 'bn1.weight', 'bn1.bias')
TRUNK_GRAD_OF = dict(s='ds', r='dr', conv_w='d_conv_w', conv_b='d_conv_b', fc_w='d_fc_w', fc_b='d_fc_b', g0='d_g0', b0='d_b0', g1='d_g1',
                     b1='d_b1')


@functools.lru_cache(maxsize=None)
def trunk_case():
    case, B, p = TRUNK
    sd, s, r, keep, inv_keep, gz = TT.inputs(case, B, p)
    ws = [sd['conv2.' + k].clone() for k in TRUNK_KEYS]
    stats = {k: sd['conv2.' + k].clone() for k in ('bn0.running_mean', 'bn0.running_var', 'bn1.running_mean', 'bn1.running_var')}
    return Case('trunk', _od(*zip(TRUNK_NAMES, [s, r] + ws)), dict(keep=keep, inv_keep=inv_keep, geom=T.geometry(case), stats=stats), gz)


TAIL = (17, 32, 0.3)


@functools.lru_cache(maxsize=None)
def tail_case():
    z, keep, inv_keep, gamma, beta, rm, rv, gx = Q.tail_inputs(*TAIL)
    return Case('tail', _od(('z', z), ('gamma', gamma), ('beta', beta)), dict(keep=keep, inv_keep=inv_keep, rm=rm, rv=rv), gx)


ROWS_B, ROWS_N, ROWS_DIM = 17, 33, 7


@functools.lru_cache(maxsize=None)
def rows_case():
    g = R.gen(R.seed_of(72, ROWS_B, ROWS_N, ROWS_DIM))
    table = R.pm_uniform((ROWS_N, ROWS_DIM), g)
    idx = torch.randint(0, ROWS_N, (ROWS_B,), generator=g)
    idx[[3, 9, 16]] = int(idx[0])                               # one row four times, not in consecutive b
    return Case('rows', _od(('table', table)), dict(idx=idx), Q.scatter_addends(ROWS_B, ROWS_DIM))


DROP = (33, 12, 0.3, 5)


@functools.lru_cache(maxsize=None)
def dropout_case():
    rows, cols, p, row0 = DROP
    g = R.gen(R.seed_of(73, rows, cols))
    return Case('dropout', _od(('x', R.pm_uniform((rows, cols), g))), dict(key=DR.key(91, 4, DR.SITE_HIDDEN), row0=row0, p=p),
                R.pm_uniform((rows, cols), g))


SCORE = (3, 15, 4)


@functools.lru_cache(maxsize=None)
def score_case():
    B, n, dim = SCORE
    x, ent, bias = R.score_inputs(B, n, dim, R.seed_of(74, B, n, dim))
    return Case('score', _od(('x', x), ('ent', ent), ('bias', bias)), {}, R.pm_uniform((B, n), R.gen(R.seed_of(75, B, n))))


def identity_case(rows=130, cols=18):
    """[rows, cols] for the three identity Functions of dist.py (the layer's output shape)."""
    g = R.gen(R.seed_of(76, rows, cols))
    return Case('identity', _od(('y', R.pm_uniform((rows, cols), g))), {}, R.pm_uniform((rows, cols), g))


BCE = [(4, 1, 4, 0.0), (36, 33, 4, 0.1)]


@functools.lru_cache(maxsize=None)
def bce_case(B, n, dim, smooth):
    x, ent, bias, hit = R.bce_inputs(B, n, dim)
    return Case('bce-%d-%d-%d' % (B, n, dim), _od(('x', x), ('ent', ent), ('bias', bias)), dict(hit=hit, smooth=smooth, n=n), None)


def smoothed(lbl_smooth, n):
    """_native.smoothed_targets restated: (hot, cold) evaluated in f32 as numpy does."""
    y = np.array([1.0, 0.0], dtype=np.float32)
    if lbl_smooth != 0.0:
        y = (1.0 - lbl_smooth) * y + (1.0 / int(n))
    return float(y[0]), float(y[1])


CAND_BCE = (4, 15, 1000, 7)
_DEAD = (-1, None, 2 ** 62, -2 ** 62)                  # None: N itself


@functools.lru_cache(maxsize=None)
def cand_bce_case():
    """test_gpu_cand_train.grid_inputs of its smallest case with dead positions, smoothing 0.1."""
    B, K, N, dim = CAND_BCE
    seed = R.seed_of(42, B, K, N, dim)
    g = R.gen(seed)
    x, ent, bias = R.pm_uniform((B, dim), g), R.pm_uniform((N, dim), g), R.pm_uniform((N,), g)
    cand = C.lists(N, B, K, seed + 1)
    for i, v in enumerate(_DEAD):
        cand[i % B, (3 * i + 1) % K] = N if v is None else v
    label = torch.rand((B, K), generator=g) < 0.3
    hot, cold = smoothed(0.1, N)
    return Case('cand_bce', _od(('x', x), ('ent', ent), ('bias', bias)), dict(cand=cand, label=label, hot=hot, cold=cold, N=N), None)


CAND_CE = (8, 63, 97, 4, 0.1)


@functools.lru_cache(maxsize=None)
def cand_ce_case():
    B, K, N, dim, eps = CAND_CE
    x, ent, bias, cand, label = E.problem(B, K, N, dim, R.seed_of(81, B, K, dim))
    return Case('cand_ce', _od(('x', x), ('ent', ent), ('bias', bias)), dict(cand=cand, label=label, eps=eps, N=N), None)


# ---------------------------------------------------------------------------------------------------------------- (4) restatements
def aggregate_reference(case, G):
    """{'out', 'x', 'rel', 'ee'} -> aggregate_ref.Ref (value, n, mag); ee in EDGE-ID order. Bar: aggregate_ref.bar_of."""
    e = case.extra
    x, rel, ee = case.inputs.values()
    gx, gee, grel = A.ref_grads(e['N'], e['ei'], e['et'], x, rel, ee, G)
    return dict(out=A.ref_forward(e['N'], e['ei'], e['et'], x, rel, ee), x=gx, rel=grel, ee=gee)


def layer_run(case, m_in, m_out, inv_keep, G, dtype):
    """_LayerTrainFn's formula in `dtype`: the three products, the keep-masks (bool [N, O] or None) scaled by inv_keep,
    dense_ref.ref_train_epilogue for the epilogue and its backward, and the backward's five products written out by the chain rule.
    Returns (results: y, rm, rv and the eight gradients by input name; the epilogue's own dict)."""
    agg, a_loop, w_in, w_out, w_loop, bias, gamma, beta = (t.to(dtype) for t in case.inputs.values())
    d = w_in.size(0)
    scale = lambda m: None if m is None else m.to(dtype) * inv_keep
    s_in, s_out = scale(m_in), scale(m_out)
    drop = lambda u, s: u if s is None else u * s
    u_in, u_out, u_loop = drop(agg[:, :d] @ w_in, s_in), drop(agg[:, d:] @ w_out, s_out), a_loop @ w_loop
    epi = R.ref_train_epilogue(u_in, u_out, u_loop, bias, gamma, beta, case.extra['rm'], case.extra['rv'], BN_MOMENTUM, BN_EPS, G, dtype=dtype)
    gu = epi['gu']
    g_in, g_out = drop(gu, s_in), drop(gu, s_out)
    out = dict(y=epi['y'], rm=epi['rm'], rv=epi['rv'], agg=torch.cat([g_in @ w_in.t(), g_out @ w_out.t()], 1), a_loop=gu @ w_loop.t(),
               w_in=agg[:, :d].t() @ g_in, w_out=agg[:, d:].t() @ g_out, w_loop=a_loop.t() @ gu, bias=epi['gz'].sum(0), gamma=epi['ggamma'],
               beta=epi['gbeta'])
    return out, epi


def layer_reference(case, m_in, m_out, inv_keep, G):
    """(r64, bars) of the layer under upstream gradient G: the logic and the constants of
    test_gpu_dropout.py::test_layer_fn_with_keys_vs_float64 -- dense_ref.derived_bar of what the same formula in torch-CPU f32 is off
    float64, floored at 8 u of the terms of each result's last additions, capped by the bars of
    test_training_layer_kernels_vs_torch_autograd where torch-CPU f32 itself meets them."""
    r64, epi = layer_run(case, m_in, m_out, inv_keep, G, torch.float64)
    r32, _ = layer_run(case, m_in, m_out, inv_keep, G, torch.float32)
    cpu_err = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}
    agg, a_loop, w_in, w_out, w_loop = (t.double() for t in list(case.inputs.values())[:5])
    d = w_in.size(0)
    scale = lambda m: 1.0 if m is None else m.double() * inv_keep
    gu = epi['gu'].abs()
    g_in, g_out = gu * scale(m_in), gu * scale(m_out)
    xh = (epi['z'] - epi['mean']) * epi['rstd']
    gp = (G.double() * (1 - r64['y'] ** 2)).abs()
    mag = {'agg': max(float((g_in @ w_in.abs().t()).max()), float((g_out @ w_out.abs().t()).max())),
           'a_loop': float((gu @ w_loop.abs().t()).max()),
           'w_in': float((agg[:, :d].abs().t() @ g_in).max()), 'w_out': float((agg[:, d:].abs().t() @ g_out).max()),
           'w_loop': float((a_loop.abs().t() @ gu).max()),
           'bias': float(epi['gz'].abs().sum(0).max()), 'gamma': float((gp * xh.abs()).sum(0).max()), 'beta': float(gp.sum(0).max())}
    today = {'y': 2e-6, 'rm': 1e-6 * float(r64['rm'].abs().max()) + 1e-7, 'rv': 1e-5 * float(r64['rv'].abs().min()) + 1e-7, 'bias': 2e-3}
    floors = {'y': 8 * U, 'rm': 8 * U * float(r64['rm'].abs().max()), 'rv': 8 * U * float(r64['rv'].abs().max())}
    bars = {}
    for name in r64:
        floor = floors.get(name, 8 * U * mag.get(name, 0.0))
        cap = today.get(name, 2e-5 * float(r64[name].abs().max()))
        bars[name] = R.derived_bar(cpu_err[name], floor, cap)
    return r64, bars


def trunk_reference():
    """trunk_train_ref.reference of the case: its gz is the case's G."""
    return TT.reference(*TRUNK)


def tail_reference():
    return Q.tail_reference(*TAIL)


def rows_reference(case, G):
    """d table, bit for bit: the sequential f32 loop of query_train_ref."""
    return Q.scatter_loop(case.extra['idx'], G, ROWS_N)


def dropout_reference(case, t):
    """Forward (t = x) or backward (t = G), bit for bit: dropout_ref.apply."""
    e = case.extra
    return torch.from_numpy(DR.apply(t.numpy(), e['key'], e['row0'], e['p']))


def score_reference(case, G):
    """(r64, bars) of _ScoreFn under G: s = sigmoid(z), gz = G s (1 - s), d x = gz ent, d ent = gz^T x, d bias = column sums.
    Bars, each from the one before: s by dense_ref.sigmoid_bar of the split kernel's logit bar; gz by that bar through s (1 - s)
    (slope |1 - 2 s|, second order bar^2) plus 4 u of its three products; the two products by gz's bar through the operand's
    magnitudes plus dense_ref.dot_bar of the sum; the column sum by cand_train_ref.gamma of its B addends."""
    x, ent, bias = case.inputs.values()
    s, z, mag = R.ref_scores(x, ent, bias)
    sbar = R.sigmoid_bar(s, R.split_logit_bar(mag))
    G = G.double()
    gz = G * s * (1 - s)
    gzbar = G.abs() * ((1 - 2 * s).abs() * sbar + sbar * sbar + 4 * U * s * (1 - s))
    xa, ea = x.double().abs(), ent.double().abs()
    B, n = gz.shape
    r64 = dict(s=s, x=gz @ ent.double(), ent=gz.t() @ x.double(), bias=gz.sum(0))
    bars = dict(s=sbar, x=gzbar @ ea + R.dot_bar(gz.abs() @ ea, n), ent=gzbar.t() @ xa + R.dot_bar(gz.abs().t() @ xa, B),
                bias=gzbar.sum(0) + C.gamma(B) * gz.abs().sum(0))
    return r64, bars


# ---------------------------------------------------------------------------------------------------------------- (3) scalar losses
def score_bce_reference(case, gl=1.0):
    """(r64, b1, mags) of _ScoreBCEFn: loss, and d x, d ent, d bias times gl; b1 the unit-gradient bars (dense_ref.bce_grad_bar of
    g carried through the sums' magnitudes, dense_ref.dot_bar of the two products, cand_train_ref.gamma of the row sum); mags the
    sums of |g_j a_j| behind the extra rounding of gl."""
    x, ent, bias = case.inputs.values()
    B, n = x.size(0), ent.size(0)
    hot, cold = smoothed(case.extra['smooth'], n)
    inv = 1.0 / (B * n)
    z, mag = R.ref_logits(x, ent, bias)
    y = torch.where(case.extra['hit'], torch.tensor(hot), torch.tensor(cold))
    loss, g, p = R.ref_bce(z, y, inv)
    gb = R.bce_grad_bar(g, p, y, R.dot_bar(mag, x.size(1)), inv)
    xa, ea, ga = x.double().abs(), ent.double().abs(), g.abs()
    r64 = dict(loss=float(loss), x=gl * (g @ ent.double()), ent=gl * (g.t() @ x.double()), bias=gl * g.sum(0))
    mags = dict(x=ga @ ea, ent=ga.t() @ xa, bias=ga.sum(0))
    b1 = dict(x=gb @ ea + R.dot_bar(mags['x'], n), ent=gb.t() @ xa + R.dot_bar(mags['ent'], B), bias=gb.sum(0) + C.gamma(B) * mags['bias'])
    return r64, b1, mags, dict(z=z, p=p, y=y, g=g, mag=mag)


def list_grad_bars(ref, gb, x, ent):
    """cand_ce_ref.grad_bars with g's bar handed in (gb [B, K], 0 at dead positions): (dx, d_ent, d_bias) bars and the sums of
    |g_j a_j| behind them."""
    x, ent = x.double(), ent.double()
    rows = ent[ref['row']].abs()
    B, K = ref['g'].shape
    ga = ref['g'].abs()
    mx = (ga[:, :, None] * rows).sum(1)
    n = ent.size(0)
    flat_row = ref['row'].reshape(-1)
    runs = int(torch.bincount(flat_row[ref['live'].reshape(-1)], minlength=1).max()) if bool(ref['live'].any()) else 1
    xa = x.abs().repeat_interleave(K, 0)
    add = lambda t, v: torch.zeros(t, dtype=torch.float64).index_add_(0, flat_row, v)
    me, mb = add((n, ent.size(1)), ga.reshape(-1)[:, None] * xa), add((n,), ga.reshape(-1))
    bars = dict(x=(gb[:, :, None] * rows).sum(1) + C.gamma(K + 2) * mx,
                ent=add((n, ent.size(1)), gb.reshape(-1)[:, None] * xa) + C.gamma(runs + 2) * me,
                bias=add((n,), gb.reshape(-1)) + C.gamma(runs + 2) * mb)
    return bars, dict(x=mx, ent=me, bias=mb)


def cand_bce_reference(case, gl=1.0):
    x, ent, bias = case.inputs.values()
    e = case.extra
    B, K = e['cand'].shape
    inv = 1.0 / (B * K)
    ref = C.ref_list_bce(x, ent, bias, e['cand'], e['label'], e['hot'], e['cold'], inv)
    gb = torch.where(ref['live'], R.bce_grad_bar(ref['g'], ref['p'], ref['y'], R.dot_bar(ref['mag'], x.size(1)), inv), torch.zeros_like(ref['g']))
    b1, mags = list_grad_bars(ref, gb, x, ent)
    r64 = dict(loss=ref['loss'], x=gl * ref['dx'], ent=gl * ref['d_ent'], bias=gl * ref['d_bias'])
    return r64, b1, mags, ref


def cand_ce_reference(case, gl=1.0):
    x, ent, bias = case.inputs.values()
    e = case.extra
    inv = 1.0 / e['cand'].size(0)
    ref = E.ref_list_ce(x, ent, bias, e['cand'], e['label'], e['eps'], inv)
    _, rowbar = E.logit_bars(ref, x.size(1))
    bx, be, bb = E.grad_bars(ref, x, ent, rowbar, inv)
    gb = torch.where(ref['live'], E.g_bar(ref, rowbar, inv), torch.zeros_like(ref['g']))
    _, mags = list_grad_bars(ref, gb, x, ent)
    r64 = dict(loss=ref['loss'], x=gl * ref['dx'], ent=gl * ref['d_ent'], bias=gl * ref['d_bias'])
    return r64, dict(x=bx, ent=be, bias=bb), mags, ref


def scaled_bars(b1, mags, gl):
    """b = |gl| b1 + |gl| u sum |g_j a_j| (the module docstring's derivation)."""
    return {k: abs(gl) * b1[k] + abs(gl) * U * mags[k] for k in b1}


def emul_list_f32(ref, case, gl):
    """The three sums of the list Functions in numpy f32 on g = f32(float64 g): g * gl rounded once, then cand_train_ref's
    emulations of the chunked d x and the plan-order d ent / d bias."""
    x, ent, _ = case.inputs.values()
    cand = case.extra['cand']
    g = (ref['g'].float().numpy() * np.float32(gl)).astype(np.float32)
    g = torch.from_numpy(g)
    perm, n_live = C.loop_plan(cand, ent.size(0))
    de, db = C.emul_ent_f32(g, cand, x, perm, n_live, ent.size(0))
    return dict(x=C.emul_dx_f32(g, cand, ent), ent=de, bias=db)


def emul_score_bce_f32(aux, case, gl):
    """_ScoreBCEFn's backward in torch-CPU f32 on g = f32(float64 g): the three results, then one multiply by gl each."""
    x, ent, _ = case.inputs.values()
    g = aux['g'].float()
    gl = torch.tensor(gl, dtype=torch.float32)
    return dict(x=(g @ ent) * gl, ent=(g.t() @ x) * gl, bias=g.sum(0) * gl)


def worst_share(got, r64, bars):
    """{name: max |got - r64| / bar}; an element whose bar is 0 must equal the reference exactly (share 0, else inf)."""
    out = {}
    for k, bar in bars.items():
        err = (got[k].detach().cpu().double().reshape(r64[k].shape) - r64[k]).abs()
        if not bool(torch.isfinite(err).all()):
            out[k] = math.inf
            continue
        bar = torch.as_tensor(bar, dtype=torch.float64).expand_as(err)
        zero = bar == 0
        if bool((err[zero] != 0).any()):
            out[k] = math.inf
            continue
        out[k] = float((err[~zero] / bar[~zero]).max()) if bool((~zero).any()) else 0.0
    return out
