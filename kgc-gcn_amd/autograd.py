"""The torch.autograd.Function classes of the training step, one definition each for the one-GPU step (model.py) and the
destination-partitioned step (dist.py). A trailing argument at its default gives the one-GPU launches; dist.py makes the rank's
rows explicit (`node_range`, `row0`, `num_entities`) and hands over its `_Exchange` (`ex`) where ranks exchange something. This
module imports _native only: an exchange is used through its methods. Every class says how it treats the incoming gradient
(tests/test_gpu_autograd_contract.py holds it to that).
"""
import torch

from . import _native


def _key_arg(k):
    """A dropout key as the autograd functions keep it: a plain int, or the device form as it is."""
    return k if isinstance(k, _native.DeviceKey) else int(k)


def _mm(a, b):
    return _native.matmul(a, b) if a.size(0) > 0 else a.new_zeros((0, b.size(1)))


def _mm_tn(a, b):
    return _native.matmul_tn(a, b) if a.size(0) > 0 else a.new_zeros((a.size(1), b.size(1)))


class _AggregateFn(torch.autograd.Function):
    """A[:, :D] / A[:, D:2D] = in-/out-half aggregates; gradients by the HIP backward kernels. `node_range` = (n0, n1): the
    aggregates [n1 - n0, 2D] of this rank's destinations from its table shard `ee`, backward by mgcn_aggregate_bwd_shard (gee
    complete, grel and gx partial: the ranks' sums add up); an empty range launches nothing in the forward.
    The incoming gradient goes through .contiguous(): a contiguous one is passed through, every other layout is copied."""

    @staticmethod
    def forward(ctx, x, rel, ee, csr, node_range=None):
        n0, n1 = (0, x.size(0)) if node_range is None else node_range
        out = torch.empty((n1 - n0, 2 * x.size(1)), dtype=torch.float32, device=x.device)
        if node_range is None:
            _native.aggregate_fwd(csr, x, rel, ee, True, None, out)
        elif n1 > n0:
            _native.aggregate_fwd(csr, x, rel, ee, True, None, out, node_range=(n0, n1), ee_sub=csr.shard_ee_sub(n0, n1), out_row0=n0)
        ctx.save_for_backward(x, rel, ee)
        ctx.csr, ctx.range = csr, node_range
        return out

    @staticmethod
    def backward(ctx, g):
        x, rel, ee = ctx.saved_tensors
        need = ctx.needs_input_grad
        if ctx.range is None:
            gx, gee, grel = _native.aggregate_bwd(ctx.csr, x, rel, ee, g.contiguous(), want_gx=need[0], want_gee=need[2], want_grel=need[1])
        else:
            gx, gee, grel = _native.aggregate_bwd_shard(ctx.csr, x, rel, ee, g.contiguous(), ctx.range, want_gx=need[0])
        return gx, grel, gee, None, None


class _LayerTrainFn(torch.autograd.Function):
    """Training-mode dense step + epilogue of one layer (model.py:103-106, 116 under .train()) on the HIP kernels:
    y = tanh(BN_batch((drop(A_in W_in) + drop(A_out W_out) + A_loop W_loop) / 3 (+ bias))). Products on the f32 MFMA
    kernels (forward A W, backward g W^T and the split-K A^T g; a product of zero rows launches nothing), batch statistics /
    normalisation / tanh and their backward on the reduction kernels of csrc/train_layer.hip; the running statistics are updated
    in place. Without `ex` the epilogue is the fused pair bn_tanh_train_fwd / _bwd. With `ex` (a dist._Exchange, one of a single
    rank included) the inputs are this rank's rows and the statistics are GLOBAL: the reductions run in the split stages (4s) and
    every rank's per-block partials go through ex.gather_blocks between them (forward: column sums, then centred sums; backward:
    the g_pre / g_pre * xhat sums).
    Dropout masks come from torch's generator (Bernoulli keep-masks scaled by 1 / keep, as F.dropout; a rank's own for its rows),
    or, with `drop_keys` = (key_in, key_out, row0), from the counter-based definition of csrc/dropout.hip: the bits
    of the GLOBAL rows (row0 = n0 on a rank), the same on any partition; one pair launch in place on the two products, no mask
    saved, and one pair launch in the backward that forms both gradients from gu.
    The incoming gradient is taken in any layout: a contiguous one is passed through, every other one is copied (by
    _native._bn_grad in the fused epilogue, by .contiguous() ahead of the split stages)."""

    @staticmethod
    def forward(ctx, agg, a_loop, w_in, w_out, w_loop, bias, gamma, beta, running_mean, running_var, momentum, eps, p_drop,
                drop_keys=None, ex=None):
        d = w_in.size(0)
        u_in, u_out = _mm(agg[:, :d], w_in.contiguous()), _mm(agg[:, d:], w_out.contiguous())
        u_loop = _mm(a_loop.contiguous(), w_loop.contiguous())
        # dropout keep-masks are saved as bool (1 byte per element, not a scaled f32 copy) and scaled by 1 / keep at use
        m_in = m_out = None
        ctx.inv_keep = 1.0
        ctx.drop = None
        if drop_keys is not None and p_drop > 0:      # counter-based: the bits are recomputed in the backward, nothing is saved
            ctx.drop = (_key_arg(drop_keys[0]), _key_arg(drop_keys[1]), int(drop_keys[2]), float(p_drop))
            _native.dropout_apply_pair(u_in, ctx.drop[0], u_out, ctx.drop[1], ctx.drop[2], ctx.drop[3], out_a=u_in, out_b=u_out)
        elif p_drop >= 1.0:                       # F.dropout(p=1) is all zeros (1 / keep would be 0 / 0)
            m_in = torch.zeros(u_in.shape, dtype=torch.bool, device=u_in.device)
            m_out, ctx.inv_keep = m_in, 0.0
            u_in, u_out = torch.zeros_like(u_in), torch.zeros_like(u_out)
        elif p_drop > 0:
            keep = 1.0 - p_drop
            ctx.inv_keep = 1.0 / keep
            m_in = torch.empty_like(u_in).bernoulli_(keep).bool()
            m_out = torch.empty_like(u_out).bernoulli_(keep).bool()
            u_in, u_out = (u_in * m_in).mul_(ctx.inv_keep), (u_out * m_out).mul_(ctx.inv_keep)   # as F.dropout: x * mask * (1 / keep)
        if ex is None:
            y, z, mean, rstd = _native.bn_tanh_train_fwd(u_in, u_out, u_loop, bias, gamma, beta, running_mean, running_var,
                                                         momentum, eps)
        else:
            z, part = _native.bn_train_stage_sum(u_in, u_out, u_loop, bias)
            mean, part = _native.bn_train_stage_center(z, ex.gather_blocks(part), ex.total)
            y, rstd = _native.bn_train_stage_finish(z, ex.gather_blocks(part), ex.total, mean, gamma, beta, running_mean,
                                                    running_var, momentum, eps)
        ctx.save_for_backward(agg, a_loop, w_in, w_out, w_loop, gamma, z, y, mean, rstd, m_in, m_out)
        ctx.has_bias, ctx.ex = bias is not None, ex
        return y

    @staticmethod
    def backward(ctx, gy):
        agg, a_loop, w_in, w_out, w_loop, gamma, z, y, mean, rstd, m_in, m_out = ctx.saved_tensors
        d = w_in.size(0)
        if ctx.ex is None:
            gz, gu, ggamma, gbeta = _native.bn_tanh_train_bwd(z, y, gy, mean, rstd, gamma)
        else:
            gy = gy.contiguous()
            parts = ctx.ex.gather_blocks(_native.bn_train_bwd_stage_sums(z, y, gy, mean, rstd))
            gz, gu, ggamma, gbeta = _native.bn_train_bwd_stage_apply(z, y, gy, mean, rstd, gamma, parts[0], parts[1], ctx.ex.total)
        if ctx.drop is not None:
            g_in, g_out = _native.dropout_apply_pair(gu, ctx.drop[0], gu, ctx.drop[1], ctx.drop[2], ctx.drop[3])
        else:
            g_in = (gu * m_in).mul_(ctx.inv_keep) if m_in is not None else gu
            g_out = (gu * m_out).mul_(ctx.inv_keep) if m_out is not None else gu
        need = ctx.needs_input_grad
        g_agg = g_loop = g_win = g_wout = g_wloop = None
        if need[0]:
            g_agg = torch.cat([_mm(g_in, w_in.t().contiguous()), _mm(g_out, w_out.t().contiguous())], dim=1)
        if need[1]:
            g_loop = _mm(gu, w_loop.t().contiguous())
        if need[2]:
            g_win = _mm_tn(agg[:, :d], g_in)
        if need[3]:
            g_wout = _mm_tn(agg[:, d:], g_out)
        if need[4]:
            g_wloop = _mm_tn(a_loop.contiguous(), gu)
        g_bias = gz.sum(0) if (ctx.has_bias and need[5]) else None
        return (g_agg, g_loop, g_win, g_wout, g_wloop, g_bias, ggamma, gbeta) + (None,) * 7


class _TrunkTrainFn(torch.autograd.Function):
    """Training-mode ConvE trunk from the gathered rows to the fc output (model.py:164-171 under .train()) on the kernels of
    csrc/conve_train.hip: z = fc(feature_drop(relu(bn1(conv_e(bn0(image(s, r))))))) with batch statistics, and its backward.
    Saves the workspace that holds the pre-BN convolution output c, the bool keep-mask (1 byte per element, scaled by
    1 / keep at use) and the batch statistics; the running statistics of bn0 / bn1 are updated in place.
    The incoming gradient is passed through when its last stride is 1 and its rows are at least O apart (contiguous, row windows,
    column windows at any offset); transposed and expanded ones (row stride 0) are copied."""

    @staticmethod
    def forward(ctx, s, r, conv_w, conv_b, fc_w, fc_b, g0, b0, g1, b1, bn0_stats, bn1_stats, keep, inv_keep, geom):
        z, saved, ws = _native.conve_train_fwd(geom, s, r, conv_w, conv_b, fc_w, fc_b, (g0, b0) + bn0_stats, (g1, b1) + bn1_stats,
                                               keep, inv_keep)
        ctx.save_for_backward(s, r, conv_w, fc_w, g0, b0, g1, b1, keep, saved, ws)
        ctx.geom, ctx.inv_keep, ctx.has_conv_bias, ctx.has_fc_bias = geom, inv_keep, conv_b is not None, fc_b is not None
        return z

    @staticmethod
    def backward(ctx, gz):
        s, r, conv_w, fc_w, g0, b0, g1, b1, keep, saved, ws = ctx.saved_tensors
        names = ('s', 'r', 'conv_w', 'conv_b', 'fc_w', 'fc_b', 'g0', 'b0', 'g1', 'b1')
        want = {n for i, n in enumerate(names) if ctx.needs_input_grad[i]}
        want -= set() if ctx.has_conv_bias else {'conv_b'}
        want -= set() if ctx.has_fc_bias else {'fc_b'}
        # rows at least O apart, the rule of _QueryRowsFn / _TrunkTailFn: a row-expanded gradient (strides (0, 1), what a
        # y.sum(0) downstream hands over) has a unit last stride and a leading dimension of 0, which the kernels refuse
        gz = gz if (gz.stride(1) == 1 and gz.stride(0) >= gz.size(1)) else gz.contiguous()
        g = _native.conve_train_bwd(ctx.geom, s, r, conv_w, fc_w, g0, b0, g1, b1, keep, ctx.inv_keep, saved, ws, gz, want)
        return tuple(g.get(n) for n in names) + (None,) * 5


class _QueryRowsFn(torch.autograd.Function):
    """table[idx] (model.py:35-36). The forward stays torch.index_select (a copy); the backward is the fixed-order row sum of
    csrc/query_train.hip, bit for bit the sequential loop d table[idx[b]] += g[b] in ascending b, instead of index_add_'s float
    atomics. The incoming gradient is passed through when its last stride is 1 and its rows are at least dim apart (contiguous,
    row windows, column windows at any offset); transposed and expanded ones are copied."""

    @staticmethod
    def forward(ctx, table, idx):
        ctx.save_for_backward(idx)
        ctx.num_rows = table.size(0)
        return torch.index_select(table, 0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        g = g if (g.stride(1) == 1 and g.stride(0) >= g.size(1)) else g.contiguous()
        return _native.query_rows_bwd(idx, g, ctx.num_rows), None


class _TrunkTailFn(torch.autograd.Function):
    """The trunk's tail x = relu(bn2(z keep inv_keep)) with batch statistics (model.py:173-175 under .train()) on the kernels of
    csrc/query_train.hip, one launch forward and one backward. Saves z, the bool keep-mask, the batch statistics and the output
    (the backward reads the relu mask from it); bn2's running statistics are updated in place.
    The incoming gradient is passed through when its last stride is 1 and its rows are at least O apart (contiguous, row windows,
    column windows at any offset); transposed and expanded ones are copied."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, momentum, eps, keep, inv_keep):
        x, saved = _native.conve_tail_fwd(z, keep, inv_keep, gamma, beta, running_mean, running_var, momentum, eps)
        ctx.save_for_backward(z, gamma, keep, saved, x)
        ctx.inv_keep = inv_keep
        return x

    @staticmethod
    def backward(ctx, gx):
        z, gamma, keep, saved, x = ctx.saved_tensors
        gx = gx if (gx.stride(1) == 1 and gx.stride(0) >= gx.size(1)) else gx.contiguous()
        want = {n for i, n in enumerate(('z', 'gamma', 'beta')) if ctx.needs_input_grad[i]}
        return _native.conve_tail_bwd(z, keep, ctx.inv_keep, x, saved, gamma, gx, want) + (None,) * 6


class _CounterDropoutFn(torch.autograd.Function):
    """Dropout of a matrix [rows, cols] whose keep bits are the counter-based ones of csrc/dropout.hip: a pure
    function of (key, row0 + row, col). Forward and backward are the same launch; nothing is saved but the scalars.
    The incoming gradient is passed through where _native.dropout_supported takes it (last stride 1, rows at least cols apart:
    contiguous, row and column windows; a misaligned one takes the kernel's scalar path); transposed and expanded ones are copied."""

    @staticmethod
    def forward(ctx, x, key, row0, p):
        ctx.args = (_key_arg(key), int(row0), float(p))
        x = x if _native.dropout_supported(x) else x.contiguous()
        return _native.dropout_apply(x, *ctx.args)

    @staticmethod
    def backward(ctx, g):
        g = g if _native.dropout_supported(g) else g.contiguous()
        return _native.dropout_apply(g, *ctx.args), None, None, None


class _ScoreFn(torch.autograd.Function):
    """sigmoid(x @ ent^T + bias): forward and both backward products on the HIP f32 MFMA tile kernel.
    The incoming gradient is read by torch's elementwise gs * s * (1 - s) in any layout; the kernels see that product's contiguous
    result only."""

    @staticmethod
    def forward(ctx, x, ent, bias):
        s = _native.score_fwd(x, ent, bias)
        ctx.save_for_backward(x, ent, s)
        return s

    @staticmethod
    def backward(ctx, gs):
        x, ent, s = ctx.saved_tensors
        gz = (gs * s * (1.0 - s)).contiguous()
        gzt = gz.t().contiguous() if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) else None
        gx = None
        if ctx.needs_input_grad[0]:
            # gx = gz [B, N] @ ent [N, O]: the reduction runs over the N entities, so it goes to the split-K transposed kernel
            # (K = N rows over <= 256 workgroups, partial products folded in order) — not to mgcn_matmul_f32's small-matrix
            # kernel, whose one lane would walk all N terms in one sequential chain
            gx = _native.matmul_tn(gzt, ent.contiguous()) if _native.matmul_tn_supported(gz.size(0), ent.size(1)) \
                else _native.matmul(gz, ent.contiguous())
        return (gx, _native.matmul(gzt, x.contiguous()) if ctx.needs_input_grad[1] else None,
                gz.sum(0) if ctx.needs_input_grad[2] else None)


class _ScoreBCEFn(torch.autograd.Function):
    """mean BCE(sigmoid(x @ ent^T + bias), targets) in ONE launch: the scores and the [B, N] targets are
    never materialised; the launch leaves d loss / d logits [N, B], the backward is two products on the HIP MFMA kernels
    (G x on the tile kernel, G^T ent on the split-K transposed kernel) and a row sum. `num_entities`: `ent` is this rank's
    entity rows and the mean runs over B x the GLOBAL entity count, so the ranks' losses and gradients add up to the whole table's.
    The incoming gradient is a scalar (a Python-scalar loss weight arrives as a 0-dim tensor, in any 0-dim view): it multiplies the
    three results by broadcasting and reaches no kernel."""

    @staticmethod
    def forward(ctx, x, ent, bias, mask, hot, cold, num_entities=None):
        loss, g = _native.score_bce_fwd(x, ent, bias, mask, hot, cold, num_entities=num_entities)
        ctx.save_for_backward(x, ent, g)
        return loss

    @staticmethod
    def backward(ctx, gl):
        x, ent, g = ctx.saved_tensors
        gx = None
        if ctx.needs_input_grad[0]:
            gx = (_native.matmul_tn(g, ent.contiguous()) if _native.matmul_tn_supported(g.size(1), ent.size(1))
                  else _native.matmul(g.t().contiguous(), ent.contiguous())) * gl
        return (gx,
                _native.matmul(g, x) * gl if ctx.needs_input_grad[1] else None,
                g.sum(1) * gl if ctx.needs_input_grad[2] else None, None, None, None, None)


class _ScoreCEFn(torch.autograd.Function):
    """softmax cross-entropy over the full entity table (include/mgcn_hip.h (20)): _CandCEFn's loss with every entity a list
    position. One launch of the tile kernel leaves the logits z [n, B] and a statistic per (tile of 32 entities, query); the
    tiles are merged per row by the kernel that merges the list chunks (_native.score_ce_fold: in two levels beyond 64 tiles); the finish overwrites z with d loss / d logit. The
    backward is _ScoreBCEFn's, on that g. No [B, N] labels, one [n, B] block, no float atomics. `eps` is spread over the
    `num_entities` entities of the GLOBAL table (default: the rows of `ent`).
    `ex`: `ent` / `bias` / `mask` are this rank's entity rows. With an exchange of more than one rank the [B, 4] row statistics
    make ONE all-gather (ex.gather_stats) and are merged over the ranks in rank order; the finish takes the global statistics.
    The rank's loss is the sum of its own entities' terms, so the ranks' losses and d x add up to the one-rank step's; d ent and
    d bias are the rank's rows, complete. A rank without rows passes the empty statistic on and joins the all-gather.
    A batch the logits launch refuses (B % 4 != 0, a misaligned x) forms z on the matmul kernel and the [B, 4] record with
    torch ops on the device (the counts through an int32 view) and goes through the same exchange, merge and finish; this second
    form holds a second [n, B] block while it forms the statistic (the launch path holds one).
    The incoming scalar gradient is handled as in _ScoreBCEFn."""

    @staticmethod
    def forward(ctx, x, ent, bias, mask, eps, num_entities=None, ex=None):
        B, n = x.size(0), ent.size(0)
        total = n if num_entities is None else int(num_entities)
        if n == 0 or B == 0:
            z = torch.empty((n, B), dtype=torch.float32, device=x.device)
            stat = _native.cand_ce_empty_stat(B, x.device)
        elif _native.score_ce_supported(x, ent):
            z, stat = _native.score_ce_logits(x, ent, bias, mask)
            stat = _native.score_ce_fold(stat, n)
        else:
            x, ent = x.contiguous(), ent.contiguous()
            z = _native.matmul(ent, x.t().contiguous()).add_(bias.view(-1, 1))
            m = z.max(0).values
            stat = torch.empty((B, 4), dtype=torch.float32, device=x.device)
            stat[:, 0], stat[:, 1] = m, z.sub(m).exp_().sum(0)      # (one [n, B] temporary next to z, freed before the finish)
            counts = stat.view(torch.int32)
            counts[:, 2], counts[:, 3] = n, _native.mask_popcount(mask, n)
        if ex is not None and ex.world > 1:
            stat = _native.cand_ce_merge(ex.gather_stats(stat), part_dim=0)
        loss, g, _ = _native.score_ce_finish(z, mask, stat, eps, max(total, 1))
        ctx.save_for_backward(x, ent, g)
        return loss

    @staticmethod
    def backward(ctx, gl):
        x, ent, g = ctx.saved_tensors
        if ent.size(0) == 0 or x.size(0) == 0:          # a rank without rows: nothing to multiply
            return (torch.zeros_like(x) if ctx.needs_input_grad[0] else None, torch.zeros_like(ent) if ctx.needs_input_grad[1] else None,
                    g.new_zeros(ent.size(0)) if ctx.needs_input_grad[2] else None, None, None, None, None)
        return _ScoreBCEFn.backward(ctx, gl)


def _save_plan(ctx, x, ent, cand, g, row0, run_split):
    """What the list backward of _CandBCEFn / _CandCEFn needs, saved on ctx: the plan of the rank's rows, and with a run_split
    its sorted keys too. No host read of the live count: the whole plan is handed over, its dead tail is skipped entry by entry."""
    ctx.row0, ctx.run_split = int(row0), run_split
    plan = _native.cand_plan(cand, ent.size(0), ent_row0=row0, count=False, keys=run_split is not None)
    ctx.n_live = plan[1]
    ctx.save_for_backward(x, ent, cand, g, plan[0], *plan[2:])


class _CandBCEFn(torch.autograd.Function):
    """mean BCE over per-query candidate lists (include/mgcn_hip.h (14)): one launch leaves the loss partials and d loss / d logit
    [B, K]; the backward is two fixed-order sums on the kernels of csrc/query_train.hip, d x over the gathered entity rows and
    d ent / d bias over the runs of a sorted plan into a zeroed block. Nothing of size [B, N] exists; no float atomics.
    `row0`: `ent` is this rank's entity rows [row0, row0 + ent.size(0)) (the ent_row0 / n_local form): list positions whose id
    another rank owns are dead here, they write g = 0, add no loss term and still count in the divisor B K, so the ranks' losses
    and d x add up to the one-rank step's; d ent and d bias are the rank's rows, complete.
    The incoming gradient is a scalar in any 0-dim view: it is folded into g [B, K] by broadcasting (g * gl, a fresh contiguous
    tensor) and reaches no kernel itself.
    `run_split` (None: the above, unchanged): d ent / d bias cut runs longer than it into pieces summed by different waves
    (include/mgcn_hip.h (18)); the forward then keeps the plan's sorted keys as well. Loss, g and d x do not see it."""

    @staticmethod
    def forward(ctx, x, ent, bias, cand, label, hot, cold, row0=0, run_split=None):
        _native.check_run_split('_CandBCEFn', run_split)      # (before the first launch)
        loss, g = _native.cand_bce_fwd(x, ent, bias, cand, label, hot, cold, ent_row0=row0)
        _save_plan(ctx, x, ent, cand, g, row0, run_split)
        return loss

    @staticmethod
    def backward(ctx, gl):
        x, ent, cand, g, perm = ctx.saved_tensors[:5]
        keys = ctx.saved_tensors[5] if ctx.run_split is not None else None
        # d x gl, d ent gl, d bias gl with gl folded into g [B, K] first: the sums are linear in g, and the [N, dim] block is
        # written once instead of being scaled in a second pass (gl = 1, the usual case, changes no bit of g)
        g = g * gl
        gx = _native.cand_bce_bwd_x(g, cand, ent, ent_row0=ctx.row0) if ctx.needs_input_grad[0] else None
        want = tuple(n for i, n in ((1, 'ent'), (2, 'bias')) if ctx.needs_input_grad[i])
        d_ent, d_bias = (None, None)
        if want:
            d_ent, d_bias = _native.cand_bce_bwd_ent(g, cand, x, perm, ctx.n_live, ent.size(0), ent_row0=ctx.row0, want=want,
                                                     run_split=ctx.run_split, keys=keys)
        return (gx, d_ent, d_bias) + (None,) * 6


class _CandCEFn(torch.autograd.Function):
    """softmax cross-entropy over per-query candidate lists (include/mgcn_hip.h (16)): logits and per-chunk statistics, their
    merge per row, then d loss / d logit [B, K] and the loss partials; the backward is _CandBCEFn's, on that g. `eps` smooths
    over the list. Nothing of size [B, N] exists; no float atomics.
    `row0`, `ex`: `ent` is this rank's entity rows [row0, row0 + ent.size(0)). With an exchange of more than one rank the [B, 4]
    row statistics make ONE all-gather (ex.gather_stats) and are merged over the ranks in rank order by the kernel that merged
    the chunks; the finish then takes the global statistics. The rank's loss is the sum of its own positions' terms, so the
    ranks' losses and d x add up to the one-rank step's; d ent and d bias are the rank's rows, complete. A rank without rows
    contributes the empty statistic and joins the all-gather. Without an exchange, or with one of a single rank, there is no
    collective and no second merge. The incoming scalar gradient and `run_split` are handled as in _CandBCEFn."""

    @staticmethod
    def forward(ctx, x, ent, bias, cand, label, eps, row0=0, ex=None, run_split=None):
        _native.check_run_split('_CandCEFn', run_split)       # (before the first launch and the collective)
        B, n = x.size(0), ent.size(0)
        if n:
            z, stat = _native.cand_ce_logits(x, ent, bias, cand, label, ent_row0=row0)
            stat = _native.cand_ce_merge(stat)
        else:
            z = torch.full(tuple(cand.shape), float('-inf'), dtype=torch.float32, device=x.device)
            stat = _native.cand_ce_empty_stat(B, x.device)
        if ex is not None and ex.world > 1:
            stat = _native.cand_ce_merge(ex.gather_stats(stat), part_dim=0)
        loss, g, _ = _native.cand_ce_finish(z, cand, label, stat, eps, n, ent_row0=row0)
        _save_plan(ctx, x, ent, cand, g, row0, run_split)
        return loss

    @staticmethod
    def backward(ctx, gl):
        return _CandBCEFn.backward(ctx, gl)
