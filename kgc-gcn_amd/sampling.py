"""Weighted negative sampling (include/mgcn_hip.h (17)): a static per-entity alias table that the counter-based
candidate draw reads, and the log(N Q) term that the listwise loss subtracts from every candidate's logit.

The table is DATA: it is built once on the CPU in exact integers (mgcn_alias_build_host), stored in checkpoints as it is, and
broadcast once from rank 0 (dist.broadcast_sampler), so that no rank, and no resumed run, depends on its own `pow`. The
distribution it realises is an exact rational, Q(n) = counts()[n] / (N 2^32).

The list BCE takes weighted lists WITHOUT a correction (the word2vec convention); the softmax takes `logq` (sampled softmax)."""
import torch

from . import _native

_TWO32 = 1 << 32


class NegativeSampler(object):
    """sampler = NegativeSampler.from_weights(w) | .uniform(N) | .from_degrees(deg); sampler = sampler.to(device).

    table  int64 [N]: alias << 32 | threshold, what _native.cand_draw(table=...) reads.
    logq   float32 [N]: float32(log(max(cnt, 1) / 2^32)) evaluated in float64 = log(N Q(n)); exactly +0.0 everywhere for the
           uniform table; the clamp keeps it finite for an entity that is never drawn (it is then never a negative either).
    Both tensors are made once per device and keep their addresses (a captured step holds them)."""

    def __init__(self, table):
        table = table.detach()
        if table.dtype != torch.int64 or table.dim() != 1 or table.numel() < 1 or table.numel() > 2 ** 31 - 1:
            raise _native.NativeError('NegativeSampler: the table must be an int64 [N], 1 <= N <= 2^31 - 1')
        self.table = table.contiguous()
        self._check()
        self.logq = self._logq()

    # -- construction -------------------------------------------------------------------------------
    @classmethod
    def from_weights(cls, w):
        """From int64 weights w [N] in [0, 2^32) with a sum >= 1 (any device; the table is built on the CPU and lives there
        until .to())."""
        return cls(_native.alias_build_host(w))

    @classmethod
    def uniform(cls, num_entities):
        """The table of equal weights, n << 32 | 0xffffffff: the draw is mgcn_cand_draw's bit for bit and logq is all +0.0."""
        n = int(num_entities)
        if n < 1 or n > 2 ** 31 - 1:
            raise _native.NativeError('NegativeSampler.uniform: N = %d outside [1, 2^31 - 1]' % n)
        return cls(torch.arange(n, dtype=torch.int64) * _TWO32 + (_TWO32 - 1))

    @classmethod
    def from_degrees(cls, deg=None, power=0.75, shift=1.0, index=None, num_entities=None):
        """Weights floor((deg + shift)^power 2^16), evaluated in float64 on the CPU and clamped below 2^32. deg [N] (any integer
        or float dtype); None: torch.bincount(index.tails, minlength=num_entities), how often the entity is a known tail of
        `index` (a dist.FilterIndex). The weights depend on this machine's pow: ship the TABLE (state_dict, broadcast_sampler),
        not the recipe."""
        if deg is None:
            if index is None or num_entities is None:
                raise _native.NativeError('NegativeSampler.from_degrees: give deg, or index and num_entities')
            deg = torch.bincount(index.tails.detach().to('cpu', torch.int64), minlength=int(num_entities))
        d = deg.detach().to('cpu', torch.float64)
        w = torch.floor(torch.pow(d + float(shift), float(power)) * 65536.0).clamp(min=0.0, max=float(_TWO32 - 1))
        return cls.from_weights(w.to(torch.int64))

    # -- the distribution ---------------------------------------------------------------------------
    def _check(self):
        alias = self.table >> 32
        if bool(((alias < 0) | (alias >= self.table.numel())).any()):
            raise _native.NativeError('NegativeSampler: the table holds an alias outside [0, N)')

    def counts(self):
        """cnt int64 [N] on the table's device: thr[n] plus (2^32 - thr[m]) of every m whose alias is n (m == n included).
        Q(n) = cnt[n] / (N 2^32); the counts sum to N 2^32."""
        thr = self.table & (_TWO32 - 1)
        return thr.clone().index_add_(0, self.table >> 32, _TWO32 - thr)

    def _logq(self):
        cnt = self.counts().to('cpu').clamp(min=1).to(torch.float64)      # (always on the CPU: one libm for every rank's table)
        return torch.log(cnt / float(_TWO32)).to(torch.float32).to(self.table.device)

    @property
    def num_entities(self):
        return self.table.numel()

    @property
    def device(self):
        return self.table.device

    # -- placement and checkpoints ------------------------------------------------------------------
    def to(self, device):
        """A sampler whose table and logq live on `device` (self when they already do). logq is copied, not recomputed: the
        device never evaluates a logarithm."""
        device = torch.device(device)
        if device == self.table.device or (device.type == 'cuda' and device.index is None and self.table.is_cuda):
            return self
        other = object.__new__(NegativeSampler)
        other.table, other.logq = self.table.to(device), self.logq.to(device)
        return other

    def state_dict(self):
        """{'table': the table on the CPU}: a checkpoint stores the table itself, next to draw_seed and the step count."""
        return {'table': self.table.detach().to('cpu').clone()}

    def load_state_dict(self, state):
        """Takes the table of state_dict() IN PLACE when it has this sampler's length (tensor addresses survive: a captured step
        stays valid), otherwise replaces the tensors. logq is recomputed from the table on the CPU."""
        new = NegativeSampler(state['table'].detach().to('cpu', torch.int64))
        if new.table.numel() == self.table.numel():
            self.table.copy_(new.table)
            self.logq.copy_(new.logq)
        else:
            dev = self.table.device
            self.table, self.logq = new.table.to(dev), new.logq.to(dev)
        return self
