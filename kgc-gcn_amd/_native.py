"""ctypes binding of libmgcn_hip.so (include/mgcn_hip.h) — the only way the package reaches the GPU.

There is deliberately NO fallback: if the library is missing or a tensor is not resident on a GPU the
call raises. torch is used here for device memory and the current HIP stream only.

The header is the one description of the C ABI: the restype / argtypes of every entry point and the constants the header
defines are parsed from its text at import (_parse_abi, _abi_defines), the same text the compiler holds every definition
under csrc/ to. Adding an entry point means declaring it in the header and writing its wrapper here, nothing else.
"""
import ctypes
import math
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MGCN_LIB') or os.path.join(_HERE, 'csrc', 'libmgcn_hip.so')   # MGCN_LIB: A/B builds
_HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'mgcn_hip.h')   # the tree's header, also under MGCN_LIB

_lib = None

_i32, _i64, _ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


class NativeError(RuntimeError):
    pass


class FusedUnsupported(NativeError):
    """mgcn_layer_fwd_fused returned MGCN_EUNSUPPORTED (misaligned operand, shape outside the kernel): callers take the
    aggregation + dense launches instead."""


_C_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
              'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double}


def _strip_comments(text):
    return re.sub(r'/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*', ' ', text)     # /* ... */ (the unrolled form of /\*.*?\*/) and // ...


def _abi_defines(text):
    """{macro: value} of the header's `#define MGCN_<NAME> <integer>` lines."""
    return {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(MGCN_\w+)[ \t]+(\d+)[ \t]*$', _strip_comments(text), re.M)}


def _c_type(fn, text, is_param):
    """ctypes type of one parameter (`const float *x_dev`) or return type (`const char *`) of declaration `fn`."""
    # [const] type [stars, `*const` too] [name]: no arrays, no function pointers
    m = re.fullmatch(r'\s*(const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w*)\s*', text)
    const, base, stars, name = m.groups() if m else (None, None, '', '')
    if stars:                                                              # `const char *` is a string, every other pointer an address
        return ctypes.c_char_p if const and (base, stars.strip()) == ('char', '*') else ctypes.c_void_p
    if base == 'void' and not (is_param or const or name):
        return None
    if base in _C_SCALARS and (is_param or not name):
        return _C_SCALARS[base]
    raise NativeError('include/mgcn_hip.h: %s: no ctypes type for `%s`' % (fn, ' '.join(text.split())))


def _parse_abi(text):
    """{name: (restype, [argtypes])} of every `<return type> mgcn_<name>(<params>);` in the text of include/mgcn_hip.h. Strict: a type
    outside the map above, an array or function-pointer parameter, or a declaration this pattern cannot read raises."""
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', _strip_comments(text), flags=re.M)
    table = {}
    for stmt in re.split(r'[;{}]', text):
        m = re.fullmatch(r'\s*([\w\s*]+?)\s*\b(mgcn_\w+)\s*\(([^()]*)\)\s*', stmt)
        if m:
            ret, fn, params = m.groups()
            params = [] if params.strip() == 'void' else params.split(',')
            table[fn] = (_c_type(fn, ret, False), [_c_type(fn, p, True) for p in params])
    skipped = set(re.findall(r'\b(mgcn_\w+)\s*\(', text)) - set(table)
    if skipped:
        raise NativeError('include/mgcn_hip.h: cannot parse the declaration of %s' % ', '.join(sorted(skipped)))
    return table


def _read_header():
    if not os.path.exists(_HEADER_PATH):
        raise NativeError('%s not found: the binding takes the C ABI from it' % _HEADER_PATH)
    with open(_HEADER_PATH) as f:
        return f.read()


_HEADER = _read_header()
_SIGNATURES = _parse_abi(_HEADER)
_DEFINES = _abi_defines(_HEADER)
EXPORTS = tuple(sorted(_SIGNATURES))
ABI_VERSION = _DEFINES['MGCN_ABI_VERSION']


def lib():
    """Load (once) and return the shared library; raise loudly when it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError('%s not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                              '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError = symbol missing from the build
            fn.restype, fn.argtypes = res, args
        if handle.mgcn_abi_version() != ABI_VERSION:
            raise NativeError('libmgcn_hip.so ABI %d, binding expects %d' % (handle.mgcn_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def _check(rc, what):
    if rc != 0:
        raise NativeError('%s failed (%d): %s' % (what, rc, lib().mgcn_last_error().decode()))


def _dev(t, dtype, what, allow_none=False):
    """Borrowed device pointer of tensor `t` (last dimension contiguous)."""
    if t is None:
        if allow_none:
            return None
        raise NativeError('%s: tensor required' % what)
    if not t.is_cuda:
        raise NativeError('%s must live on a GPU (got %s): the M-GCN hot path has no CPU fallback' % (what, t.device))
    if t.dtype != dtype:
        raise NativeError('%s: dtype %s, expected %s' % (what, t.dtype, dtype))
    if t.dim() > 0 and t.numel() > 0 and t.size(-1) > 1 and t.stride(-1) != 1:       # (the stride of a last dimension of size 1 is never used)
        raise NativeError('%s: last dimension must be contiguous' % what)
    return t.data_ptr()


def _ld(t):
    return t.stride(0) if t.dim() == 2 and t.size(0) > 1 else t.size(-1)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _same_device(*ts):
    devs = {t.device for t in ts if t is not None}
    if len(devs) > 1:
        raise NativeError('tensors on different devices: %s' % sorted(map(str, devs)))


def is_ee16(ee):
    """A per-edge table held in bf16 (include/mgcn_hip.h (2e)): the forward launches take their _ee16 entry points, which compute
    what the f32 launch computes from ee.float(), bit for bit; there is no backward (inference only)."""
    return ee is not None and ee.dtype == torch.bfloat16


def _refuse_ee16(ee, what):
    if is_ee16(ee):
        raise NativeError('%s: the per-edge table is bf16, which is inference-only (include/mgcn_hip.h (2e)): the backward '
                          'entry points take f32 tables' % what)


# ------------------------------------------------------------------------------------------------
# slots per (half, destination) above which it is a hub. 32: below a gather group's fair share of an FB15k-237 tile (~42 slots per
# half and stage), so that no single row outlasts its stage; measured on that shape's step: 64 -> 0.323, 48 -> 0.311, 32 -> 0.303, 24 -> 0.314,
# 16 -> 0.331 ms (tools/hub_sweep.sh). WN18RR / uniform graphs have no such rows either way.
HUB_THRESHOLD = int(os.environ.get('MGCN_HUB_THRESHOLD', '32'))
HUB_CHUNK = int(os.environ.get('MGCN_HUB_CHUNK', '64'))             # slots per hub chunk


def csr_build_host(num_nodes, num_rel_rows, edge_index, edge_type, with_backward=True, hub_threshold=None,
                   hub_chunk=None):
    """(1) Feeder. edge_index [2, 2E] int64, edge_type [2E] int64 (any device; copied to host).
    Returns a dict of HOST tensors (see mgcn_csr_build_host); 'chunks' is trimmed to the chunks in use."""
    ei = edge_index.detach().to('cpu', torch.int64).contiguous()
    et = edge_type.detach().to('cpu', torch.int64).contiguous()
    if ei.dim() != 2 or ei.size(0) != 2 or ei.size(1) % 2 or et.numel() != ei.size(1):
        raise NativeError('csr_build: edge_index must be [2, 2E] and edge_type [2E]')
    E2, E, N = ei.size(1), ei.size(1) // 2, int(num_nodes)
    thr = HUB_THRESHOLD if hub_threshold is None else int(hub_threshold)
    chk = HUB_CHUNK if hub_chunk is None else int(hub_chunk)
    max_chunks = (E2 // max(chk, 1) + E2 // max(thr, 1) + 2) if thr > 0 else 0
    out = dict(rowptr=torch.empty((2, N + 1), dtype=torch.int32), rec=torch.empty((E2, 4), dtype=torch.int32),
               perm=torch.empty(E2, dtype=torch.int64), hubinfo=torch.empty((2, N, 2), dtype=torch.int32),
               chunks=torch.empty((max(max_chunks, 1), 4), dtype=torch.int32))
    nch = ctypes.c_int64(0)
    if with_backward:
        out.update(slot_dst=torch.empty(E2, dtype=torch.int32), mirror=torch.empty(E2, dtype=torch.int32),
                   typeptr=torch.empty(num_rel_rows + 1, dtype=torch.int32),
                   typeslots=torch.empty(E2, dtype=torch.int32))
    p = lambda k: out[k].data_ptr() if k in out else None
    _check(lib().mgcn_csr_build_host(N, E, int(num_rel_rows), ei.data_ptr(), et.data_ptr(), thr, chk, p('rowptr'),
                                     p('rec'), p('perm'), p('hubinfo'), p('chunks'), max_chunks, ctypes.byref(nch),
                                     p('slot_dst'), p('mirror'), p('typeptr'), p('typeslots')),
           'mgcn_csr_build_host')
    out['num_chunks'] = int(nch.value)
    out['chunks'] = out['chunks'][:max(int(nch.value), 1)].contiguous()
    return out


def csr_live_view_host(rowptr, rec):
    """(1v) The live view of a canonical layout (host tensors rowptr [2, N+1] int32, rec [2E, 4] int32): the non-hub slots
    whose norm is not exactly zero. Returns None when no slot is dead (nothing is built), else a dict of HOST tensors:
    live_rowptr [2, N+1] int32, live_rec [L, 4] int32 (fourth word: the canonical slot index), num_live, num_dead."""
    if rowptr.dim() != 2 or rowptr.size(0) != 2 or rowptr.size(1) < 1 or rowptr.dtype != torch.int32 or rowptr.is_cuda or \
            not rowptr.is_contiguous() or rec.dtype != torch.int32 or rec.is_cuda or not rec.is_contiguous() or \
            (rec.numel() and (rec.dim() != 2 or rec.size(1) != 4)):
        raise NativeError('csr_live_view: rowptr must be a contiguous host int32 [2, N+1], rec a contiguous host int32 [2E, 4]')
    N = rowptr.size(1) - 1
    if int(rowptr[1, N]) > rec.size(0) or int(rowptr[0, 0]) < 0:
        raise NativeError('csr_live_view: rowptr points past the records')
    live, dead = ctypes.c_int64(0), ctypes.c_int64(0)
    call = lambda lrp, lrec, cap: _check(lib().mgcn_csr_live_view_host(
        N, rowptr.data_ptr(), rec.data_ptr(), lrp, lrec, cap, ctypes.byref(live), ctypes.byref(dead)), 'mgcn_csr_live_view_host')
    L = int(rowptr[1, N]) - int(rowptr[0, 0])                     # capacity: every non-hub slot
    out = dict(live_rowptr=torch.empty((2, N + 1), dtype=torch.int32), live_rec=torch.empty((max(L, 1), 4), dtype=torch.int32))
    call(out['live_rowptr'].data_ptr(), out['live_rec'].data_ptr(), L)
    if dead.value == 0:
        return None
    out['live_rec'] = out['live_rec'][:max(int(live.value), 1)].contiguous()   # (never empty: the launch wants a valid pointer)
    out['num_live'], out['num_dead'] = int(live.value), int(dead.value)
    return out


# MGCN_LIVE_SLOTS=0: fused launches walk the canonical layout even where the graph has a live view (A/B runs). Read once at import.
LIVE_SLOTS = os.environ.get('MGCN_LIVE_SLOTS', '1') != '0'


def _hub_args(csr, d, device, n0, n1):
    """(hubinfo ptr, chunks ptr, chunk_begin, chunk_end, partial tensor) for a launch over destinations [n0, n1). The chunk
    sums and the fold's arrival counters live in a buffer kept on the graph per (width, chunk range): the counters are
    zero when it is made and every launch leaves them zero (include/mgcn_hip.h (2)), and its address is stable for a
    captured launch. Launches that share it must not overlap: a launch on another stream than the last one waits for
    that stream first."""
    c0, c1 = csr.chunk_range(n0, n1)
    if c1 == c0:
        return None, None, 0, 0, None
    cache = csr.__dict__.setdefault('_hub_partials', {})
    key = (int(d), c0, c1, str(device))
    hit = cache.get(key)
    stream = torch.cuda.current_stream(device)
    if hit is None:            # (never evicted: a captured launch keeps the buffer's address; one entry per width and range)
        hit = cache[key] = [torch.zeros(int(lib().mgcn_hub_partial_floats(c1 - c0, int(d))), dtype=torch.float32, device=device),
                            stream]
    elif hit[1] != stream and not torch.cuda.is_current_stream_capturing():
        stream.wait_stream(hit[1])
        hit[1] = stream
    return _dev(csr.hubinfo, torch.int32, 'hubinfo'), _dev(csr.chunks, torch.int32, 'chunks'), c0, c1, hit[0]


def _hub_failed(csr, d, device, n0, n1):
    """A launch that was handed the (width, chunk range) hub buffer returned an error: its fold may have stopped between two
    arrivals and left counters non-zero, which would silently switch the NEXT launch's fold off. Forget the buffer: the next
    launch gets a fresh zeroed one (a captured graph that holds the old address is invalid after a failed launch anyway)."""
    c0, c1 = csr.chunk_range(n0, n1)
    csr.__dict__.get('_hub_partials', {}).pop((int(d), c0, c1, str(device)), None)


def aggregate_fwd(csr, x, rel, ee, ee_in_slot_order, loop_edge, out, loop_rel=None, node_range=None, ee_sub=(0, 0, 0),
                  out_row0=0):
    """(2) out[:, 0:D | D:2D | 2D:3D) = in / out / self-loop aggregates. `csr` is a graph.GraphCSR.
    `rel` is either the whole relation table [num_rel_rows, D] (last row = self-loop row) or, with
    `loop_rel` [D] given separately, its first num_rel_rows-1 rows (no concatenation needed).
    With `node_range` = (n0, n1), `ee` may be that range's shard of the slot-ordered table
    (graph.GraphCSR.edge_table_shard) and `ee_sub` its three slot offsets (GraphCSR.shard_ee_sub). `out_row0`: `out`
    holds rows [out_row0, out_row0 + out.size(0)) of the aggregate (the kernel indexes rows by global node id).
    A bf16 `ee` takes mgcn_aggregate_fwd_ee16: the rows of the f32 launch on ee.float(), bit for bit."""
    N, E, D = csr.num_nodes, csr.num_edges_half, x.size(1)
    _same_device(csr.rowptr, x, rel, ee, loop_edge, out, loop_rel)
    if loop_rel is None:
        if rel.size(0) != csr.num_rel_rows:
            raise NativeError('aggregate_fwd: rel has %d rows, graph expects %d' % (rel.size(0), csr.num_rel_rows))
        loop_rel, rel = rel[-1], rel[:-1]
    if x.size(0) != N or rel.size(0) != csr.num_rel_rows - 1 or rel.size(1) != D or loop_rel.numel() != D:
        raise NativeError('aggregate_fwd: x %s / rel %s do not match graph (N=%d, rel rows=%d)'
                          % (tuple(x.shape), tuple(rel.shape), N, csr.num_rel_rows))
    ee_sub = tuple(int(v) for v in ee_sub)
    sharded = ee_sub != (0, 0, 0) or (ee is not None and ee.size(0) != 2 * E)
    if ee is not None and not sharded and tuple(ee.shape) != (2 * E, D):
        raise NativeError('aggregate_fwd: per-edge table %s, expected (%d, %d)' % (tuple(ee.shape), 2 * E, D))
    if not rel.is_contiguous() or (ee is not None and not ee.is_contiguous()):
        raise NativeError('aggregate_fwd: relation and per-edge tables must be contiguous')
    modes = 3 if loop_edge is not None else 2
    if loop_edge is not None and loop_edge.numel() != D:
        raise NativeError('aggregate_fwd: loop_edge must have %d elements' % D)
    n0, n1 = (0, N) if node_range is None else (int(node_range[0]), int(node_range[1]))
    if not 0 <= n0 <= n1 <= N:
        raise NativeError('aggregate_fwd: node range (%d, %d) outside [0, %d]' % (n0, n1, N))
    out_row0 = int(out_row0)
    if out.size(1) < modes * D or out_row0 > n0 or out_row0 + out.size(0) < n1 or (out_row0 == 0 and node_range is None and out.size(0) != N):
        raise NativeError('aggregate_fwd: out %s (rows from %d) does not cover destinations [%d, %d) x %d columns'
                          % (tuple(out.shape), out_row0, n0, n1, modes * D))
    if sharded:
        rows = csr.shard_slot_counts(n0, n1)
        if ee is None or not ee_in_slot_order or tuple(ee.shape) != (sum(rows), D) or not ee.is_contiguous() or \
                ee_sub != csr.shard_ee_sub(n0, n1):
            raise NativeError('aggregate_fwd: per-edge shard does not match destinations [%d, %d)' % (n0, n1))
        if ee.numel() == 0:
            ee = torch.zeros((1, D), dtype=ee.dtype, device=x.device)
    hub_info, hub_chunks, hub_c0, hub_c1, hub_partial = _hub_args(csr, D, x.device, n0, n1)
    ee16 = is_ee16(ee)
    rc = (lib().mgcn_aggregate_fwd_ee16 if ee16 else lib().mgcn_aggregate_fwd)(
        N, E, D, csr.num_rel_rows, _dev(csr.rowptr, torch.int32, 'rowptr'), _dev(csr.rec, torch.int32, 'rec'),
        _dev(x, torch.float32, 'x'), _ld(x), _dev(rel, torch.float32, 'rel'), _dev(loop_rel, torch.float32, 'loop_rel'),
        _dev(ee, torch.bfloat16 if ee16 else torch.float32, 'ee', True), int(bool(ee_in_slot_order)),
        _dev(loop_edge, torch.float32, 'loop_edge', True), _dev(out, torch.float32, 'out') - out_row0 * _ld(out) * 4, _ld(out), n0, n1, hub_info, hub_chunks, hub_c0, hub_c1,
        _dev(hub_partial, torch.float32, 'partial', True), ee_sub[0], ee_sub[1], ee_sub[2], _stream(x))
    if rc != 0 and hub_partial is not None:
        _hub_failed(csr, D, x.device, n0, n1)
    _check(rc, 'mgcn_aggregate_fwd')
    return out


def _bwd_out(out, i, want, shape, device, what):
    """Output i of a backward: the caller's tensor (`out` = (gx, gee, grel), entries may be None) or a fresh one."""
    given = None if out is None else out[i]
    if not want:
        if given is not None:
            raise NativeError('%s: out[%d] given for a gradient that is not computed' % (what, i))
        return None
    if given is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(given.shape) != tuple(shape) or given.dtype != torch.float32 or given.device != device or not given.is_contiguous():
        raise NativeError('%s: out[%d] must be a contiguous float32 %s on %s' % (what, i, tuple(shape), device))
    return given


def aggregate_bwd(csr, x, rel, ee, g, want_gx=True, want_gee=True, want_grel=True, out=None):
    """(3) Gradients of aggregate_fwd's first 2D columns w.r.t. x, the per-edge table (slot order) and rel. `out` =
    (gx, gee, grel): tensors to write instead of fresh ones (contiguous, entries may be None)."""
    _refuse_ee16(ee, 'aggregate_bwd')
    N, E, D = csr.num_nodes, csr.num_edges_half, x.size(1)
    _same_device(csr.rowptr, x, rel, ee, g)
    if not csr.has_backward:
        raise NativeError('aggregate_bwd: graph was prepared without the backward indices')
    if want_gx and not csr.mirrored:
        raise NativeError('aggregate_bwd: the edge list is not mirror-symmetric (edge e + E is not the reverse of edge e, '
                          'data_loader.py:143-149), so the gradient w.r.t. the layer input cannot be formed from the '
                          'destination runs; forward, per-edge and relation gradients are unaffected')
    if g.size(0) != N or g.size(1) < 2 * D:
        raise NativeError('aggregate_bwd: g %s too small' % (tuple(g.shape),))
    if x.size(0) != N or tuple(rel.shape) != (csr.num_rel_rows, D) or not rel.is_contiguous():
        raise NativeError('aggregate_bwd: x / rel do not match the graph')
    if ee is not None and (tuple(ee.shape) != (2 * E, D) or not ee.is_contiguous()):
        raise NativeError('aggregate_bwd: per-edge table must be contiguous (%d, %d) in slot order' % (2 * E, D))
    if out is not None and len(out) != 3:
        raise NativeError('aggregate_bwd: out must be (gx, gee, grel)')
    gx = _bwd_out(out, 0, want_gx, (N, D), x.device, 'aggregate_bwd')
    gee = _bwd_out(out, 1, want_gee and ee is not None, (2 * E, D), x.device, 'aggregate_bwd')
    grel = _bwd_out(out, 2, want_grel, (csr.num_rel_rows, D), x.device, 'aggregate_bwd')
    need_ws = want_grel or (want_gx and csr.num_chunks > 0)
    ws_bytes = lib().mgcn_aggregate_bwd_workspace(E, D, csr.num_rel_rows, csr.num_chunks) if need_ws else 0
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=x.device) if need_ws else None
    hubs = csr.num_chunks > 0
    _check(lib().mgcn_aggregate_bwd(
        N, E, D, csr.num_rel_rows, _dev(csr.rowptr, torch.int32, 'rowptr'), _dev(csr.rec, torch.int32, 'rec'),
        _dev(csr.slot_dst, torch.int32, 'slot_dst'), _dev(csr.mirror, torch.int32, 'mirror'),
        _dev(csr.hubinfo, torch.int32, 'hubinfo') if hubs else None,
        _dev(csr.chunks, torch.int32, 'chunks') if hubs else None, csr.num_chunks,
        _dev(csr.typeptr, torch.int32, 'typeptr'), _dev(csr.typeslots, torch.int32, 'typeslots'),
        _dev(x, torch.float32, 'x'), _ld(x), _dev(rel, torch.float32, 'rel'), _dev(ee, torch.float32, 'ee', True),
        _dev(g, torch.float32, 'g'), _ld(g), _dev(gx, torch.float32, 'gx', True), _dev(gee, torch.float32, 'gee', True),
        _dev(grel, torch.float32, 'grel', True), _dev(ws, torch.float32, 'ws', True), ws_bytes, _stream(x)),
        'mgcn_aggregate_bwd')
    return gx, gee, grel


def aggregate_bwd_shard(csr, x, rel, ee, g, node_range, want_gx=True, out=None):
    """(3s) aggregate_bwd for the destinations [n0, n1) of one rank from its table shard `ee` (slot order, the rows of
    GraphCSR.edge_table_shard); `g` [n1 - n0, >= 2D] holds the gradient of those rows only. Returns (gx [N, D] partial or None,
    gee [shard rows, D] complete, grel [num_rel_rows, D] partial): summed over the ranks of a partition, gx / grel are
    aggregate_bwd's (bit-identical with one range covering the graph). `out` = (gx, gee, grel): tensors to write instead
    of fresh ones (contiguous, entries may be None)."""
    _refuse_ee16(ee, 'aggregate_bwd_shard')
    N, E, D = csr.num_nodes, csr.num_edges_half, x.size(1)
    n0, n1 = int(node_range[0]), int(node_range[1])
    _same_device(csr.rowptr, x, rel, ee, g)
    if not csr.has_backward:
        raise NativeError('aggregate_bwd_shard: graph was prepared without the backward indices')
    if want_gx and not csr.mirrored:
        raise NativeError('aggregate_bwd_shard: the edge list is not mirror-symmetric: no gradient w.r.t. the layer input')
    if not 0 <= n0 <= n1 <= N:
        raise NativeError('aggregate_bwd_shard: node range (%d, %d) outside [0, %d]' % (n0, n1, N))
    if x.size(0) != N or tuple(rel.shape) != (csr.num_rel_rows, D) or not rel.is_contiguous():
        raise NativeError('aggregate_bwd_shard: x / rel do not match the graph')
    rows = csr.shard_slot_counts(n0, n1)
    if ee is None or tuple(ee.shape) != (sum(rows), D) or not ee.is_contiguous():
        raise NativeError('aggregate_bwd_shard: per-edge shard %s does not match destinations [%d, %d) (%d rows)'
                          % (None if ee is None else tuple(ee.shape), n0, n1, sum(rows)))
    if g.dim() != 2 or g.size(0) != n1 - n0 or g.size(1) < 2 * D:
        raise NativeError('aggregate_bwd_shard: g %s must be [%d, >= %d]' % (tuple(g.shape), n1 - n0, 2 * D))
    idx = csr.shard_backward_index(n0, n1)
    sub = csr.shard_ee_sub(n0, n1)
    if out is not None and len(out) != 3:
        raise NativeError('aggregate_bwd_shard: out must be (gx, gee, grel)')
    gx = _bwd_out(out, 0, want_gx, (N, D), x.device, 'aggregate_bwd_shard')
    gee = _bwd_out(out, 1, True, (sum(rows), D), x.device, 'aggregate_bwd_shard')
    grel = _bwd_out(out, 2, True, (csr.num_rel_rows, D), x.device, 'aggregate_bwd_shard')
    hubs = csr.num_chunks > 0
    ws_bytes = lib().mgcn_aggregate_bwd_shard_workspace(sum(rows), D, csr.num_rel_rows, csr.num_chunks)
    ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device=x.device)
    nz = lambda t, dtype, what: _dev(t, dtype, what) if t.numel() > 0 else None     # (an empty shard: nothing is read or written)
    _check(lib().mgcn_aggregate_bwd_shard(
        N, E, D, csr.num_rel_rows, _dev(csr.rec, torch.int32, 'rec'), _dev(csr.slot_dst, torch.int32, 'slot_dst'), n0, n1,
        rows[0], rows[1], rows[2], sub[0], sub[1], sub[2], _dev(idx['src_ptr'], torch.int32, 'src_ptr'),
        nz(idx['src_rows'], torch.int32, 'src_rows'), _dev(csr.hubinfo, torch.int32, 'hubinfo') if hubs else None,
        _dev(idx['src_chunks'], torch.int32, 'src_chunks') if hubs else None, csr.num_chunks,
        _dev(idx['type_ptr'], torch.int32, 'type_ptr'), nz(idx['type_rows'], torch.int32, 'type_rows'), _dev(x, torch.float32, 'x'), _ld(x),
        _dev(rel, torch.float32, 'rel'), nz(ee, torch.float32, 'ee'), nz(g, torch.float32, 'g'), _ld(g) if g.numel() > 0 else 2 * D,
        _dev(gx, torch.float32, 'gx', True), nz(gee, torch.float32, 'gee'), _dev(grel, torch.float32, 'grel'), _dev(ws, torch.float32, 'ws'),
        ws_bytes, _stream(x)), 'mgcn_aggregate_bwd_shard')
    return gx, gee, grel


def dense_bn_tanh_fwd(a, w_cat, bias, bn_mean, bn_var, bn_gamma, bn_beta, eps, out):
    """(4) out = tanh(BN_eval((A @ w_cat) / 3 + bias)), w_cat [3D, O] = W_in, W_out, W_loop stacked by rows."""
    N, O = a.size(0), w_cat.size(1)
    D = w_cat.size(0) // 3
    _same_device(a, w_cat, bias, bn_mean, bn_var, bn_gamma, bn_beta, out)
    if w_cat.dim() != 2 or w_cat.size(0) != 3 * D or not w_cat.is_contiguous():
        raise NativeError('dense_bn_tanh_fwd: w_cat must be contiguous (3D, O)')
    for v in (bn_mean, bn_var, bn_gamma, bn_beta) + ((bias,) if bias is not None else ()):
        if v.numel() != O:
            raise NativeError('dense_bn_tanh_fwd: per-column vectors must have %d elements' % O)
    if a.size(1) < 3 * D or tuple(out.shape) != (N, O):
        raise NativeError('dense_bn_tanh_fwd: a %s / out %s do not match' % (tuple(a.shape), tuple(out.shape)))
    _check(lib().mgcn_dense_bn_tanh_fwd(
        N, D, O, _dev(a, torch.float32, 'a'), _ld(a), _dev(w_cat, torch.float32, 'w_cat'),
        _dev(bias, torch.float32, 'bias', True), _dev(bn_mean, torch.float32, 'bn_mean'),
        _dev(bn_var, torch.float32, 'bn_var'), _dev(bn_gamma, torch.float32, 'bn_gamma'),
        _dev(bn_beta, torch.float32, 'bn_beta'), float(eps), _dev(out, torch.float32, 'out'), _ld(out), _stream(a)),
        'mgcn_dense_bn_tanh_fwd')
    return out


# `tune` argument of mgcn_layer_fwd_fused (include/mgcn_hip.h): 0 = automatic. Read ONCE at import, for A/B tools only (see
# INTEGRATION.md "Environment switches"): bits 0-3 row tiles per tile, 4-7 staging buffers, 8-9 relation
# table in LDS, 10-11 a forced kernel generation (2 or 3; 1 is reserved), 12-13 columns per slot walk, 14 the legacy column cut.
FUSED_TUNE = int(os.environ.get('MGCN_FUSED_TUNE', '0'), 0)
# `tune` bit 14: the legacy column cut of the fused layer kernels (128-column chunks, idle lanes on the row's head) instead of
# the one that follows the row stride (include/mgcn_hip.h (2b)); same rows either way. MGCN_FUSED_CUT=legacy, read ONCE at
# import, sets it in every launch: for A/B runs.
FUSED_CUT_LEGACY = 1 << 14
FUSED_CUT = FUSED_CUT_LEGACY if os.environ.get('MGCN_FUSED_CUT', '') == 'legacy' else 0


def fused_cut(dim_in, legacy=False):
    """The column cut of a `dim_in`-wide fused layer (mgcn_fused_cut, no device work): ([(first column, columns), ...], modelled
    mean 128-byte lines one input row costs per mode)."""
    col0, ncol, lines = (_i32 * 8)(), (_i32 * 8)(), ctypes.c_double(0.0)
    n = lib().mgcn_fused_cut(int(dim_in), int(bool(legacy)), col0, ncol, 8, ctypes.byref(lines))
    if n < 0:
        raise NativeError('fused_cut: no fused kernel takes %d input columns' % dim_in)
    return [(col0[i], ncol[i]) for i in range(n)], lines.value


def tune_generation(tune=None):
    """Kernel generation a `tune` word forces: 2, 3, or 0 = the shape's own. Raises for the reserved field value 1."""
    tune = FUSED_TUNE if tune is None else int(tune)
    f = (tune >> 10) & 3
    if f == 1:
        raise NativeError('tune %#x: bits 10-11 = 1 is reserved (mgcn_layer_fwd_fused refuses it)' % tune)
    return f


_FUSED_STATUS = {}


def fused_status(device):
    """The device's status word handed to every fused launch (mgcn_layer_fwd_fused status_dev): one int32, zero while no
    bounded spin of the generation-3 kernel has run out."""
    key = str(torch.device(device))
    if key not in _FUSED_STATUS:
        _FUSED_STATUS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _FUSED_STATUS[key]


def check_fused_status(device):
    """Synchronising check of the status word (call where the host waits for results anyway: end of an evaluation, a
    benchmark's timed region, tests): raises if a fused launch since the last check reported a spin timeout, and clears it."""
    key = str(torch.device(device))
    if key in _FUSED_STATUS:
        v = int(_FUSED_STATUS[key].item())
        if v:
            _FUSED_STATUS[key].zero_()
            raise NativeError('a fused layer launch on %s reported status %d: a bounded LDS-counter spin ran out '
                              '(layer_fused3.hip), rows of that launch are invalid' % (key, v))
FUSED_ENABLED = os.environ.get('MGCN_FUSED', '1') != '0'


_CU_COUNT = {}


def _cu_count(device):
    key = str(device)
    if key not in _CU_COUNT:
        _CU_COUNT[key] = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return _CU_COUNT[key]


def fused_supported(d_in, d_out):
    """Shapes the one-launch layer kernel handles (else: aggregate_fwd + dense_bn_tanh_fwd)."""
    return FUSED_ENABLED and d_in % 4 == 0 and d_in <= 1024 and d_out % 4 == 0 and d_out <= 512


def pack_weights(w_cat, out=None, generation=None):
    """Stacked [3D, O] weights -> MFMA fragment order for layer_fwd_fused (re-pack whenever a weight changes).
    `generation`: the kernel generation to pack for: 2, 3, or 0 = the shape's own (None = what MGCN_FUSED_TUNE forces, else the
    shape's own); any other value raises NativeError."""
    D, O = w_cat.size(0) // 3, w_cat.size(1)
    if w_cat.dim() != 2 or w_cat.size(0) != 3 * D or not w_cat.is_contiguous():
        raise NativeError('pack_weights: w_cat must be contiguous (3D, O)')
    gen = tune_generation() if generation is None else int(generation)
    nbytes = lib().mgcn_packed_weights_bytes_gen(gen, D, O)
    if nbytes == 0:
        raise NativeError('pack_weights: there is no kernel generation %d (0, 2 or 3)' % gen)
    if out is None:
        out = torch.empty(nbytes // 4, dtype=torch.float32, device=w_cat.device)
    if out.numel() * 4 < nbytes:
        raise NativeError('pack_weights: out too small')
    _same_device(w_cat, out)
    _check(lib().mgcn_pack_weights_gen(gen, D, O, _dev(w_cat, torch.float32, 'w_cat'), _dev(out, torch.float32, 'wp'),
                                       out.numel() * 4, _stream(w_cat)), 'mgcn_pack_weights')
    return out


MAX_ROW_BOUNDS = 4096     # runs per launch (mgcn_layer_fwd_fused num_row_bounds)


def row_bounds_cap(rows, runs):
    """Longest run a launch over `rows` destinations in `runs` runs sizes its tiles for: per = ceil(rows / runs) rounded up to
    whole 16-row tiles while per <= 80, to whole 80-row tiles past that (fused3_launch, GraphCSR.workgroup_bounds)."""
    per = -(-int(rows) // int(runs))
    return (per + 15) // 16 * 16 if per <= 80 else (per + 79) // 80 * 80


def check_row_bounds(offsets, rows):
    """What the elastic launch assumes of a caller's runs, on the host values `offsets` (a sequence of ints): raises NativeError."""
    b = [int(v) for v in offsets]
    runs = len(b) - 1
    if not 1 <= runs <= MAX_ROW_BOUNDS:
        raise NativeError('layer_fwd_fused: row_bounds must give 1 .. %d runs (got %d offsets)' % (MAX_ROW_BOUNDS, len(b)))
    if b[0] != 0 or b[-1] != int(rows) or any(hi <= lo for lo, hi in zip(b[:-1], b[1:])):
        raise NativeError('layer_fwd_fused: row_bounds must increase strictly from 0 to the %d rows of the launch' % int(rows))
    cap = row_bounds_cap(rows, runs)
    longest = max(hi - lo for lo, hi in zip(b[:-1], b[1:]))
    if longest > cap:
        raise NativeError('layer_fwd_fused: row_bounds has a run of %d rows; %d rows in %d runs allow at most %d'
                          % (longest, int(rows), runs, cap))


def _checked_row_bounds(b, rows, x):
    if not torch.is_tensor(b) or b.dtype != torch.int32 or b.dim() != 1 or not b.is_contiguous() or not b.is_cuda or \
            b.device != x.device:
        raise NativeError('layer_fwd_fused: row_bounds must be a contiguous 1-D int32 tensor on %s' % x.device)
    if b.numel() > MAX_ROW_BOUNDS + 1:
        raise NativeError('layer_fwd_fused: row_bounds must give 1 .. %d runs (got %d offsets)' % (MAX_ROW_BOUNDS, b.numel()))
    check_row_bounds(b.tolist(), rows)
    return b


def layer_fwd_fused(csr, x, rel, loop_rel, ee, ee_in_slot_order, loop_edge, w_packed, d_out, bias, bn_mean, bn_var,
                    bn_gamma, bn_beta, eps, out, node_range=None, ee_sub=(0, 0, 0), rels_weight=None, rel_out=None,
                    tune=None, balance=True, live=None, row_bounds=None):
    """(2)+(4) in one launch: out = tanh(BN_eval((aggregates @ W) / 3 + bias)), aggregates kept in LDS.
    `w_packed` = pack_weights(stacked [3D, O] weights). With `node_range` = (n0, n1) only those destinations are
    computed and `out` is [n1 - n0, O]; `ee` may then be this range's shard of the slot-ordered table (see
    graph.GraphCSR.edge_table_shard) with `ee_sub` its three slot offsets (in-half, out-half, hub region).
    `balance`: hand the launch the graph's work-balanced per-workgroup row runs (GraphCSR.workgroup_bounds, one run per
    CU, None when equal runs are balanced already); results do not depend on it.
    `row_bounds`: the caller's own runs instead (it overrides `balance`): an int32 tensor on the launch's device, row offsets
    from n0, strictly increasing from 0 to n1 - n0, at most 4096 runs, one workgroup each. No run may be longer than the cap the
    launch sizes its tiles by, from per = ceil(rows / runs): per rounded up to whole 16-row tiles while per <= 80, to whole 80-row
    tiles past that (the rule of GraphCSR.workgroup_bounds); anything else raises NativeError before a launch (the check reads
    the tensor back: it synchronises). Read by generation 3 (bounds make a lockstep shape with O > 128 and fewer than two
    tiles per CU take generation 3); generation 2 tiles the range itself. Results do not depend on the runs.
    `live`: walk the graph's live view (GraphCSR.live_rowptr / live_rec: zero-norm slots left out; bit-identical rows for
    finite inputs). None = whenever the graph has one and MGCN_LIVE_SLOTS is not 0; False = the canonical launch; True raises
    where there is no view to walk.
    A bf16 `ee` takes the _ee16 entry points (generations 2 and 3): the rows of the f32 launch on ee.float(), bit for bit."""
    N, E, D, O = csr.num_nodes, csr.num_edges_half, x.size(1), int(d_out)
    n0, n1 = (0, N) if node_range is None else (int(node_range[0]), int(node_range[1]))
    if not 0 <= n0 <= n1 <= N:
        raise NativeError('layer_fwd_fused: node range (%d, %d) outside [0, %d]' % (n0, n1, N))
    ee_sub = tuple(int(v) for v in ee_sub) + (0,) * (3 - len(ee_sub))
    sharded = ee_sub != (0, 0, 0) or (ee is not None and ee.size(0) != 2 * E)
    _same_device(csr.rowptr, x, rel, loop_rel, ee, loop_edge, w_packed, bias, bn_mean, bn_var, bn_gamma, bn_beta, out)
    if x.size(0) != N or tuple(rel.shape) != (csr.num_rel_rows - 1, D) or loop_rel.numel() != D or loop_edge.numel() != D:
        raise NativeError('layer_fwd_fused: x / rel / loop rows do not match the graph')
    if ee is not None and not sharded and (tuple(ee.shape) != (2 * E, D) or not ee.is_contiguous()):
        raise NativeError('layer_fwd_fused: per-edge table must be contiguous (%d, %d)' % (2 * E, D))
    if ee is not None and sharded:
        rows = csr.shard_slot_counts(n0, n1)
        if not ee_in_slot_order or tuple(ee.shape) != (sum(rows), D) or not ee.is_contiguous() or \
                ee_sub != csr.shard_ee_sub(n0, n1):
            raise NativeError('layer_fwd_fused: per-edge shard does not match destinations [%d, %d)' % (n0, n1))
    tune = (FUSED_TUNE if tune is None else int(tune)) | FUSED_CUT
    if not rel.is_contiguous() or w_packed.numel() * 4 < lib().mgcn_packed_weights_bytes_gen(tune_generation(tune), D, O):
        raise NativeError('layer_fwd_fused: rel must be contiguous and w_packed sized by mgcn_packed_weights_bytes')
    for v in (bn_mean, bn_var, bn_gamma, bn_beta) + ((bias,) if bias is not None else ()):
        if v.numel() != O:
            raise NativeError('layer_fwd_fused: per-column vectors must have %d elements' % O)
    if tuple(out.shape) != (n1 - n0, O):
        raise NativeError('layer_fwd_fused: out must be (%d, %d)' % (n1 - n0, O))
    if (rels_weight is None) != (rel_out is None):
        raise NativeError('layer_fwd_fused: give rels_weight and rel_out together')
    if rel_out is not None:
        _same_device(x, rels_weight, rel_out)
        if tuple(rels_weight.shape) != (D, O) or not rels_weight.is_contiguous() or \
                tuple(rel_out.shape) != (csr.num_rel_rows - 1, O) or not rel_out.is_contiguous():
            raise NativeError('layer_fwd_fused: rels_weight must be contiguous (%d, %d) and rel_out (%d, %d)'
                              % (D, O, csr.num_rel_rows - 1, O))
    if row_bounds is not None:
        row_bounds = _checked_row_bounds(row_bounds, n1 - n0, x)
    if n1 == n0 and rel_out is None:
        return out                                   # an empty destination range: nothing to launch
    if ee is not None and ee.numel() == 0:           # a range whose destinations have no slots: the kernel still wants
        ee = torch.zeros((1, D), dtype=ee.dtype, device=x.device)   # a valid (never read) table pointer
    hub_info, hub_chunks, hub_c0, hub_c1, hub_partial = _hub_args(csr, D, x.device, n0, n1)
    bounds = csr.workgroup_bounds(n0, n1, _cu_count(x.device)) if balance and n1 > n0 else None
    if row_bounds is not None:
        bounds = row_bounds
    # the graph's live view (zero-norm slots left out) whenever it has one: same rows for finite inputs, fewer row loads
    has_view = getattr(csr, 'live_rowptr', None) is not None
    if live and not has_view:
        raise NativeError('layer_fwd_fused: live=True, but this graph has no live view (no dead slot)')
    live = has_view and (LIVE_SLOTS if live is None else bool(live))
    ee16 = is_ee16(ee)
    if live:
        fn = lib().mgcn_layer_fwd_fused_live_ee16 if ee16 else lib().mgcn_layer_fwd_fused_live
        head = (_dev(csr.live_rowptr, torch.int32, 'live_rowptr'), _dev(csr.live_rec, torch.int32, 'live_rec'),
                _dev(csr.rec, torch.int32, 'rec'))
    else:
        fn = lib().mgcn_layer_fwd_fused_ee16 if ee16 else lib().mgcn_layer_fwd_fused
        head = (_dev(csr.rowptr, torch.int32, 'rowptr'), _dev(csr.rec, torch.int32, 'rec'))
    rc = fn(
        N, E, D, O, csr.num_rel_rows, *head,
        _dev(x, torch.float32, 'x'), _ld(x), _dev(rel, torch.float32, 'rel'), _dev(loop_rel, torch.float32, 'loop_rel'),
        _dev(ee, torch.bfloat16 if ee16 else torch.float32, 'ee', True), int(bool(ee_in_slot_order)),
        _dev(loop_edge, torch.float32, 'loop_edge'), _dev(w_packed, torch.float32, 'w_packed'), _dev(bias, torch.float32, 'bias', True),
        _dev(bn_mean, torch.float32, 'bn_mean'), _dev(bn_var, torch.float32, 'bn_var'),
        _dev(bn_gamma, torch.float32, 'bn_gamma'), _dev(bn_beta, torch.float32, 'bn_beta'), float(eps),
        _dev(out, torch.float32, 'out'), _ld(out), n0, n1, int(ee_sub[0]), int(ee_sub[1]), int(ee_sub[2]),
        hub_info, hub_chunks, hub_c0, hub_c1,
        _dev(hub_partial, torch.float32, 'partial', True), _dev(rels_weight, torch.float32, 'rels_weight', True),
        _dev(rel_out, torch.float32, 'rel_out', True), _dev(bounds, torch.int32, 'row_bounds', True),
        bounds.numel() - 1 if bounds is not None else 0, tune, _dev(fused_status(x.device), torch.int32, 'status'),
        _stream(x))
    if rc != 0 and hub_partial is not None:
        _hub_failed(csr, D, x.device, n0, n1)
    if rc == 3:
        raise FusedUnsupported('mgcn_layer_fwd_fused: %s' % lib().mgcn_last_error().decode())
    _check(rc, 'mgcn_layer_fwd_fused')
    return out


def matmul(a, b):
    """C = A @ B on the f32 MFMA tile kernel."""
    _same_device(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.size(1) != b.size(0):
        raise NativeError('matmul: shapes %s @ %s' % (tuple(a.shape), tuple(b.shape)))
    c = torch.empty((a.size(0), b.size(1)), dtype=torch.float32, device=a.device)
    _check(lib().mgcn_matmul_f32(a.size(0), a.size(1), b.size(1), _dev(a, torch.float32, 'a'), _ld(a),
                                 _dev(b, torch.float32, 'b'), _ld(b), _dev(c, torch.float32, 'c'), _ld(c), _stream(a)),
           'mgcn_matmul_f32')
    return c


def matmul_tn(a, b):
    """C = A^T @ B for A [K, M], B [K, N] (the weight gradient dW = aggregate^T g): split-K exact-f32 MFMA kernel."""
    _same_device(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.size(0) != b.size(0):
        raise NativeError('matmul_tn: shapes %s^T @ %s' % (tuple(a.shape), tuple(b.shape)))
    K, M, N = a.size(0), a.size(1), b.size(1)
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    nbytes = lib().mgcn_matmul_tn_workspace(K, M, N)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=a.device)
    _check(lib().mgcn_matmul_tn_f32(K, M, N, _dev(a, torch.float32, 'a'), _ld(a), _dev(b, torch.float32, 'b'), _ld(b),
                                    _dev(c, torch.float32, 'c'), _ld(c), _dev(ws, torch.float32, 'ws'), nbytes, _stream(a)),
           'mgcn_matmul_tn_f32')
    return c


def matmul_tn_supported(m, n):
    return m <= 208 and n <= 256


def _bn_block(t, n, O, what, name):
    """z / y of the training epilogue: the kernels index t[r * O + col] and take no leading dimension, so anything but a contiguous
    [n, O] block (a column window of a wider tensor, say) would be read at the wrong stride. Refused, never copied."""
    if t is None or t.dim() != 2 or tuple(t.shape) != (n, O) or not t.is_contiguous():
        raise NativeError('%s: %s must be contiguous [%d, %d], got %s with strides %s'
                          % (what, name, n, O, None if t is None else tuple(t.shape), None if t is None else tuple(t.stride())))


def _bn_grad(gy, n, O, what):
    """gy as autograd hands it over: [n, O] in any layout, made contiguous here."""
    if gy is None or tuple(gy.shape) != (n, O):
        raise NativeError('%s: gy must be [%d, %d], got %s' % (what, n, O, None if gy is None else tuple(gy.shape)))
    return gy.contiguous()


def _bn_vecs(O, what, **vecs):
    """Per-column vectors (None = not given): O contiguous elements each, or the kernels read past their end."""
    for name, v in vecs.items():
        if v is not None and (v.numel() != O or not v.is_contiguous()):
            raise NativeError('%s: %s must be contiguous with %d elements, got %s' % (what, name, O, tuple(v.shape)))


def bn_tanh_train_fwd(u_in, u_out, u_loop, bias, gamma, beta, running_mean, running_var, momentum, eps):
    """(4t) z = (u_in + u_out + u_loop) / 3 (+ bias); y = tanh(BN_batch(z)). Returns (y, z, save_mean, save_rstd); updates
    the running statistics in place when given. The products may be column windows (one common row stride); bias, gamma, beta
    and the running statistics must have O elements: a wrong length is refused before any launch."""
    N, O = u_in.shape
    _same_device(u_in, u_out, u_loop, bias, gamma, beta, running_mean, running_var)
    for t in (u_in, u_out, u_loop):
        if tuple(t.shape) != (N, O) or t.stride(1) != 1 or t.stride(0) != u_in.stride(0):
            raise NativeError('bn_tanh_train_fwd: the three products must be [N, O] with the same row stride')
    _bn_vecs(O, 'bn_tanh_train_fwd', bias=bias, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var)
    z = torch.empty((N, O), dtype=torch.float32, device=u_in.device)
    y = torch.empty_like(z)
    mean = torch.empty(O, dtype=torch.float32, device=u_in.device)
    rstd = torch.empty_like(mean)
    nbytes = lib().mgcn_bn_tanh_train_workspace(N, O)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=u_in.device)
    _check(lib().mgcn_bn_tanh_train_fwd(
        N, O, _dev(u_in, torch.float32, 'u_in'), _dev(u_out, torch.float32, 'u_out'), _dev(u_loop, torch.float32, 'u_loop'),
        u_in.stride(0), _dev(bias, torch.float32, 'bias', True), _dev(gamma, torch.float32, 'gamma'), _dev(beta, torch.float32, 'beta'),
        _dev(running_mean, torch.float32, 'running_mean', True), _dev(running_var, torch.float32, 'running_var', True),
        float(momentum), float(eps), _dev(z, torch.float32, 'z'), _dev(y, torch.float32, 'y'), _dev(mean, torch.float32, 'mean'),
        _dev(rstd, torch.float32, 'rstd'), _dev(ws, torch.float32, 'ws'), nbytes, _stream(u_in)), 'mgcn_bn_tanh_train_fwd')
    return y, z, mean, rstd


def bn_tanh_train_bwd(z, y, gy, mean, rstd, gamma):
    """Backward of bn_tanh_train_fwd: (gz [N, O], gu = gz / 3, ggamma [O], gbeta [O]). z and y are the forward's own outputs:
    contiguous [N, O] (refused otherwise, not copied); gy [N, O] in any layout; mean, rstd, gamma with O elements."""
    N, O = z.shape
    _same_device(z, y, gy, mean, rstd, gamma)
    _bn_block(z, N, O, 'bn_tanh_train_bwd', 'z')
    _bn_block(y, N, O, 'bn_tanh_train_bwd', 'y')
    gy = _bn_grad(gy, N, O, 'bn_tanh_train_bwd')
    _bn_vecs(O, 'bn_tanh_train_bwd', mean=mean, rstd=rstd, gamma=gamma)
    gz, gu = torch.empty_like(z), torch.empty_like(z)
    gg, gb = torch.empty_like(mean), torch.empty_like(mean)
    nbytes = lib().mgcn_bn_tanh_train_workspace(N, O)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=z.device)
    _check(lib().mgcn_bn_tanh_train_bwd(
        N, O, _dev(z, torch.float32, 'z'), _dev(y, torch.float32, 'y'), _dev(gy, torch.float32, 'gy'), _dev(mean, torch.float32, 'mean'),
        _dev(rstd, torch.float32, 'rstd'), _dev(gamma, torch.float32, 'gamma'), _dev(gz, torch.float32, 'gz'), _dev(gu, torch.float32, 'gu'),
        _dev(gg, torch.float32, 'ggamma'), _dev(gb, torch.float32, 'gbeta'), _dev(ws, torch.float32, 'ws'), nbytes, _stream(z)),
        'mgcn_bn_tanh_train_bwd')
    return gz, gu, gg, gb


BN_BLOCK = 128       # rows per partial-sum block of the training epilogue (csrc/train_layer.hip)


def bn_blocks(rows):
    return (int(rows) + BN_BLOCK - 1) // BN_BLOCK


def _bn_parts(parts, O, what):
    if parts.dim() != 2 or parts.size(0) < 1 or parts.size(1) != O or not parts.is_contiguous():
        raise NativeError('%s: block partials must be contiguous [blocks >= 1, %d]' % (what, O))
    return parts.size(0)


# (4s) The split stages below take this rank's rows [n, O] (n may be 0) and ALL ranks' block partials in rank-then-block order.
# Each rank cuts ITS rows into 128-row blocks from its own first row, so at rank boundaries that are not multiples of 128 (the
# ones GraphCSR.balanced_bounds produces) the blocks are not those of bn_tanh_train_fwd / _bwd: every rank still gets the same
# bits for mean, rstd, ggamma, gbeta and the running statistics (same partials, same fold order), and the results meet the
# float64 bars of (4t), but they are not (4t)'s bits. z, y must be contiguous [n, O] and every per-column vector must have O
# elements: anything else is refused before a launch, never copied (gy alone is taken in any layout).
def bn_train_stage_sum(u_in, u_out, u_loop, bias):
    """(4s) stage 1: z = (u_in + u_out + u_loop) / 3 (+ bias) of this rank's rows and its per-block column sums [bn_blocks(n), O]."""
    n, O = u_in.shape
    _same_device(u_in, u_out, u_loop, bias)
    for t in (u_in, u_out, u_loop):
        if tuple(t.shape) != (n, O) or (n > 0 and (t.stride(1) != 1 or t.stride(0) != u_in.stride(0))):
            raise NativeError('bn_train_stage_sum: the three products must be [N, O] with the same row stride')
    _bn_vecs(O, 'bn_train_stage_sum', bias=bias)
    z = torch.empty((n, O), dtype=torch.float32, device=u_in.device)
    part = torch.empty((bn_blocks(n), O), dtype=torch.float32, device=u_in.device)
    if n > 0:
        _check(lib().mgcn_bn_train_stage_sum(n, O, _dev(u_in, torch.float32, 'u_in'), _dev(u_out, torch.float32, 'u_out'),
                                             _dev(u_loop, torch.float32, 'u_loop'), u_in.stride(0), _dev(bias, torch.float32, 'bias', True),
                                             _dev(z, torch.float32, 'z'), _dev(part, torch.float32, 'part'), _stream(u_in)),
               'mgcn_bn_train_stage_sum')
    return z, part


def bn_train_stage_center(z, sum_parts, total_rows):
    """(4s) stage 2: mean [O] from ALL ranks' stage-1 blocks (rank, then block order) and this rank's blocks of (z - mean)^2.
    z: contiguous [n, O] (stage 1's own output)."""
    n, O = z.shape
    _same_device(z, sum_parts)
    _bn_block(z, n, O, 'bn_train_stage_center', 'z')
    nb = _bn_parts(sum_parts, O, 'bn_train_stage_center')
    mean = torch.empty(O, dtype=torch.float32, device=z.device)
    part = torch.empty((bn_blocks(n), O), dtype=torch.float32, device=z.device)
    _check(lib().mgcn_bn_train_stage_center(n, O, _dev(z, torch.float32, 'z', n == 0), _dev(sum_parts, torch.float32, 'sum_parts'), nb,
                                            int(total_rows), _dev(mean, torch.float32, 'mean'),
                                            _dev(part, torch.float32, 'part') if n > 0 else None, _stream(sum_parts)),
           'mgcn_bn_train_stage_center')
    return mean, part


def bn_train_stage_finish(z, sq_parts, total_rows, mean, gamma, beta, running_mean, running_var, momentum, eps):
    """(4s) stage 3: rstd [O] (and the running statistics, in place) from ALL ranks' stage-2 blocks, then y = tanh(BN(z)).
    z: contiguous [n, O]; mean, gamma, beta and the running statistics: O elements."""
    n, O = z.shape
    _same_device(z, sq_parts, mean, gamma, beta, running_mean, running_var)
    _bn_block(z, n, O, 'bn_train_stage_finish', 'z')
    nb = _bn_parts(sq_parts, O, 'bn_train_stage_finish')
    _bn_vecs(O, 'bn_train_stage_finish', mean=mean, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var)
    y = torch.empty_like(z)
    rstd = torch.empty(O, dtype=torch.float32, device=z.device)
    _check(lib().mgcn_bn_train_stage_finish(
        n, O, _dev(z, torch.float32, 'z', n == 0), _dev(sq_parts, torch.float32, 'sq_parts'), nb, int(total_rows),
        _dev(mean, torch.float32, 'mean'), _dev(gamma, torch.float32, 'gamma'), _dev(beta, torch.float32, 'beta'),
        _dev(running_mean, torch.float32, 'running_mean', True), _dev(running_var, torch.float32, 'running_var', True),
        float(momentum), float(eps), _dev(rstd, torch.float32, 'rstd'), _dev(y, torch.float32, 'y') if n > 0 else None,
        _stream(sq_parts)), 'mgcn_bn_train_stage_finish')
    return y, rstd


def bn_train_bwd_stage_sums(z, y, gy, mean, rstd):
    """(4s) backward stage 1: this rank's per-block sums of g_pre and g_pre * xhat, as one [2, bn_blocks(n), O] tensor.
    z, y: contiguous [n, O]; gy [n, O] in any layout; mean, rstd: O elements."""
    n, O = z.shape
    _same_device(z, y, gy, mean, rstd)
    _bn_block(z, n, O, 'bn_train_bwd_stage_sums', 'z')
    _bn_block(y, n, O, 'bn_train_bwd_stage_sums', 'y')
    gy = _bn_grad(gy, n, O, 'bn_train_bwd_stage_sums')
    _bn_vecs(O, 'bn_train_bwd_stage_sums', mean=mean, rstd=rstd)
    part = torch.empty((2, bn_blocks(n), O), dtype=torch.float32, device=z.device)
    if n > 0:
        _check(lib().mgcn_bn_train_bwd_stage_sums(n, O, _dev(z, torch.float32, 'z'), _dev(y, torch.float32, 'y'),
                                                  _dev(gy, torch.float32, 'gy'), _dev(mean, torch.float32, 'mean'),
                                                  _dev(rstd, torch.float32, 'rstd'), _dev(part[0], torch.float32, 'g_part'),
                                                  _dev(part[1], torch.float32, 'gx_part'), _stream(z)), 'mgcn_bn_train_bwd_stage_sums')
    return part


def bn_train_bwd_stage_apply(z, y, gy, mean, rstd, gamma, g_parts, gx_parts, total_rows):
    """(4s) backward stage 2: (gz, gu = gz / 3, ggamma, gbeta) with ggamma / gbeta folded from ALL ranks' blocks.
    z, y: contiguous [n, O]; gy [n, O] in any layout; mean, rstd, gamma: O elements."""
    n, O = z.shape
    _same_device(z, y, gy, mean, rstd, gamma, g_parts, gx_parts)
    _bn_block(z, n, O, 'bn_train_bwd_stage_apply', 'z')
    _bn_block(y, n, O, 'bn_train_bwd_stage_apply', 'y')
    gy = _bn_grad(gy, n, O, 'bn_train_bwd_stage_apply')
    _bn_vecs(O, 'bn_train_bwd_stage_apply', mean=mean, rstd=rstd, gamma=gamma)
    nb = _bn_parts(g_parts, O, 'bn_train_bwd_stage_apply')
    if _bn_parts(gx_parts, O, 'bn_train_bwd_stage_apply') != nb:
        raise NativeError('bn_train_bwd_stage_apply: g / gx partials differ in blocks')
    gz, gu = torch.empty_like(z), torch.empty_like(z)
    gg, gb = torch.empty_like(mean), torch.empty_like(mean)
    live = n > 0
    _check(lib().mgcn_bn_train_bwd_stage_apply(
        n, O, _dev(z, torch.float32, 'z', not live), _dev(y, torch.float32, 'y', not live), _dev(gy, torch.float32, 'gy', not live),
        _dev(mean, torch.float32, 'mean'), _dev(rstd, torch.float32, 'rstd'), _dev(gamma, torch.float32, 'gamma'),
        _dev(g_parts, torch.float32, 'g_parts'), _dev(gx_parts, torch.float32, 'gx_parts'), nb, int(total_rows),
        _dev(gz, torch.float32, 'gz') if live else None, _dev(gu, torch.float32, 'gu') if live else None,
        _dev(gg, torch.float32, 'ggamma'), _dev(gb, torch.float32, 'gbeta'), _stream(mean)), 'mgcn_bn_train_bwd_stage_apply')
    return gz, gu, gg, gb


def _score_args(x, ent, bias):
    _same_device(x, ent, bias)
    if x.dim() != 2 or ent.dim() != 2 or x.size(1) != ent.size(1) or bias.numel() != ent.size(0):
        raise NativeError('score: x %s, ent %s, bias %s do not match' % (tuple(x.shape), tuple(ent.shape), tuple(bias.shape)))
    return x.size(0), ent.size(0), x.size(1)


def score_fwd(x, ent, bias):
    """(5) score [B, n_local] = sigmoid(x @ ent^T + bias)."""
    B, n, O = _score_args(x, ent, bias)
    out = torch.empty((B, n), dtype=torch.float32, device=x.device)
    _check(lib().mgcn_score_fwd(B, n, O, _dev(x, torch.float32, 'x'), _ld(x), _dev(ent, torch.float32, 'ent'), _ld(ent),
                                _dev(bias, torch.float32, 'bias'), _dev(out, torch.float32, 'score'), _ld(out),
                                _stream(x)), 'mgcn_score_fwd')
    return out


def score_target(x, ent, bias, obj, ent_row0=0, out=None):
    """target[b] = score[b, obj[b]] for the queries whose obj is a row of this shard (others keep `out`)."""
    B, n, O = _score_args(x, ent, bias)
    if obj.numel() != B:
        raise NativeError('score_target: obj must have %d elements' % B)
    if out is None:
        out = torch.zeros(B, dtype=torch.float32, device=x.device)
    _check(lib().mgcn_score_target(B, n, int(ent_row0), O, _dev(x, torch.float32, 'x'), _ld(x),
                                   _dev(ent, torch.float32, 'ent'), _ld(ent), _dev(bias, torch.float32, 'bias'),
                                   _dev(obj, torch.int64, 'obj'), _dev(out, torch.float32, 'target'), _stream(x)),
           'mgcn_score_target')
    return out


def score_rank(x, ent, bias, obj, target, label=None, ent_row0=0, counts=None, mask=None):
    """counts [B, 3] int64 += (gt, ties_lower, ties) over this shard's entities. Filter = dense `label` rows [B, n]
    (reference loader) or the bit-packed `mask` [B, ceil(n/32)] int32 from filter_mask()."""
    B, n, O = _score_args(x, ent, bias)
    if (label is None) == (mask is None):
        raise NativeError('score_rank: give exactly one of label / mask')
    if obj.numel() != B or target.numel() != B:
        raise NativeError('score_rank: obj/target do not match batch %d' % B)
    if label is not None and (label.dim() != 2 or label.size(0) != B or label.size(1) != n):
        raise NativeError('score_rank: label must be (%d, %d)' % (B, n))
    if mask is not None and (mask.dim() != 2 or mask.size(0) != B or mask.size(1) < (n + 31) // 32 or not mask.is_contiguous()):
        raise NativeError('score_rank: mask must be contiguous (%d, >= %d)' % (B, (n + 31) // 32))
    if counts is None:
        counts = torch.zeros((B, 3), dtype=torch.int64, device=x.device)
    _same_device(x, ent, bias, obj, target, label, mask, counts)
    _check(lib().mgcn_score_rank(B, n, int(ent_row0), O, _dev(x, torch.float32, 'x'), _ld(x),
                                 _dev(ent, torch.float32, 'ent'), _ld(ent), _dev(bias, torch.float32, 'bias'),
                                 _dev(obj, torch.int64, 'obj'), _dev(target, torch.float32, 'target'),
                                 _dev(label, torch.float32, 'label', True), _ld(label) if label is not None else 0,
                                 _dev(mask, torch.int32, 'mask', True), mask.size(1) if mask is not None else 0,
                                 _dev(counts, torch.int64, 'counts'), _stream(x)), 'mgcn_score_rank')
    return counts


TOPK_MAX = 1024


def _check_k(k, what):
    if not 1 <= int(k) <= TOPK_MAX:
        raise NativeError('%s: k = %d outside [1, %d]' % (what, int(k), TOPK_MAX))
    return int(k)


def _topk_out(out, B, k, device, what, contiguous):
    """The (scores [B, k] f32, ids [B, k] int64) pair a top-k call writes: fresh, or the caller's `out` views."""
    if out is None:
        return (torch.empty((B, k), dtype=torch.float32, device=device),
                torch.empty((B, k), dtype=torch.int64, device=device))
    scores, ids = out
    for t, name in ((scores, 'scores'), (ids, 'ids')):
        if t.dim() != 2 or tuple(t.shape) != (B, k):
            raise NativeError('%s: out %s %s must be (%d, %d)' % (what, name, tuple(t.shape), B, k))
        if contiguous and not t.is_contiguous():
            raise NativeError('%s: out %s must be contiguous' % (what, name))
        if B > 1 and t.stride(0) < k:
            raise NativeError('%s: out %s rows overlap (stride %d < %d)' % (what, name, t.stride(0), k))
    return scores, ids


def score_topk(x, ent, bias, k, mask=None, ent_row0=0, out=None):
    """(7) The k best entities of this shard per query: (scores [B, k] f32, ids [B, k] int64 global ids), score
    descending then id ascending, each score the f32 value of score_fwd; entities whose bit is set in the bit-packed
    `mask` [B, >= ceil(n/32)] int32 of filter_mask() are excluded; a row with fewer than k entities left ends in
    (-inf, -1) padding (see mgcn_score_topk). out = (scores, ids): 2-d [B, k] views to write into, their row strides
    are the ABI's ldo / ldi (columns outside the views are left alone)."""
    B, n, O = _score_args(x, ent, bias)
    k = _check_k(k, 'score_topk')
    if mask is not None and (mask.dim() != 2 or mask.size(0) != B or mask.size(1) < (n + 31) // 32 or not mask.is_contiguous()):
        raise NativeError('score_topk: mask must be contiguous (%d, >= %d)' % (B, (n + 31) // 32))
    scores, ids = _topk_out(out, B, k, x.device, 'score_topk', False)
    _same_device(x, ent, bias, mask, scores, ids)
    nbytes = lib().mgcn_score_topk_workspace(B, n, k)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)    # the caching allocator's memory
    _check(lib().mgcn_score_topk(B, n, int(ent_row0), O, _dev(x, torch.float32, 'x'), _ld(x),
                                 _dev(ent, torch.float32, 'ent'), _ld(ent), _dev(bias, torch.float32, 'bias'),
                                 _dev(mask, torch.int32, 'mask', True), mask.size(1) if mask is not None else 0, k,
                                 _dev(scores, torch.float32, 'scores'), _ld(scores),
                                 _dev(ids, torch.int64, 'ids'), _ld(ids),
                                 _dev(ws, torch.uint8, 'workspace'), nbytes, _stream(x)), 'mgcn_score_topk')
    return scores, ids


def topk_merge(scores, ids, k, out=None):
    """(7) The top-k of candidate lists laid side by side: scores [B, L] f32, ids [B, L] int64 with L a multiple of k
    (L / k lists of k, id -1 = padding) -> (scores [B, k], ids [B, k]) in the order of score_topk (see mgcn_topk_merge).
    out = (scores, ids): contiguous [B, k] tensors to write into (the ABI has no output stride)."""
    k = _check_k(k, 'topk_merge')
    _same_device(scores, ids)
    if scores.dim() != 2 or ids.shape != scores.shape or scores.size(1) % k != 0:
        raise NativeError('topk_merge: scores %s / ids %s must be equal [B, lists * %d]' % (tuple(scores.shape), tuple(ids.shape), k))
    B, lists = scores.size(0), scores.size(1) // k
    scores, ids = scores.contiguous(), ids.contiguous()
    out_s, out_i = _topk_out(out, B, k, scores.device, 'topk_merge', True)
    _same_device(scores, out_s, out_i)
    _check(lib().mgcn_topk_merge(B, lists, _dev(scores, torch.float32, 'scores'), _dev(ids, torch.int64, 'ids'),
                                 scores.size(1), k, _dev(out_s, torch.float32, 'out scores'),
                                 _dev(out_i, torch.int64, 'out ids'), _stream(scores)), 'mgcn_topk_merge')
    return out_s, out_i


def score_candidates(x, ent, bias, cand, mask=None, ent_row0=0, out=None):
    """(13) Scores [B, K] f32 of the per-query candidate lists cand [B, K] int64 (global entity ids; its row stride is the
    ABI's ldc): element (b, j) is the f32 value score_fwd gives (b, cand[b, j]) when the id is a row of this shard
    [ent_row0, ent_row0 + n), -inf when its bit is set in the bit-packed `mask` [B, >= ceil(n/32)] int32 of filter_mask(), and
    is left as it is for every other id (-1 padding, another shard's id, any int64). out: a 2-d [B, K] f32 view to write into
    (its row stride is ldo; columns outside the view are left alone); None allocates a block filled with -inf, so that padding
    and foreign ids read -inf, the padding convention of score_topk."""
    B, n, O = _score_args(x, ent, bias)
    if cand.dim() != 2 or cand.size(0) != B:
        raise NativeError('score_candidates: cand %s must be (%d, K)' % (tuple(cand.shape), B))
    K = cand.size(1)
    if B > 1 and K > 0 and cand.stride(0) < K:
        raise NativeError('score_candidates: cand rows overlap (stride %d < %d)' % (cand.stride(0), K))
    if mask is not None and (mask.dim() != 2 or mask.size(0) != B or mask.size(1) < (n + 31) // 32 or not mask.is_contiguous()):
        raise NativeError('score_candidates: mask must be contiguous (%d, >= %d)' % (B, (n + 31) // 32))
    if out is None:
        out = torch.full((B, K), float('-inf'), dtype=torch.float32, device=x.device)
    elif out.dim() != 2 or tuple(out.shape) != (B, K) or (B > 1 and K > 0 and out.stride(0) < K):
        raise NativeError('score_candidates: out %s must be (%d, %d) with rows that do not overlap' % (tuple(out.shape), B, K))
    _same_device(x, ent, bias, cand, mask, out)
    if K == 0 or B == 0 or n == 0:         # nothing to write (an empty shard owns no id)
        return out
    _check(lib().mgcn_score_candidates(B, K, n, int(ent_row0), O, _dev(x, torch.float32, 'x'), _ld(x),
                                       _dev(ent, torch.float32, 'ent'), _ld(ent), _dev(bias, torch.float32, 'bias'),
                                       _dev(cand, torch.int64, 'cand'), _ld(cand), _dev(mask, torch.int32, 'mask', True),
                                       mask.size(1) if mask is not None else 0, _dev(out, torch.float32, 'out'), _ld(out),
                                       _stream(x)), 'mgcn_score_candidates')
    return out


# ------------------------------------------------------------------------------------------------
# (14) Training on per-query candidate lists
def _cand_block(cand, B, what):
    if cand.dim() != 2 or cand.size(0) != B or cand.dtype != torch.int64:
        raise NativeError('%s: cand must be int64 (%d, K), got %s %s' % (what, B, cand.dtype, tuple(cand.shape)))
    K = cand.size(1)
    if B > 1 and K > 0 and cand.stride(0) < K:
        raise NativeError('%s: cand rows overlap (stride %d < %d)' % (what, cand.stride(0), K))
    return K


def _cand_rows(t, B, K, dtype, what, name):
    """(pointer, row stride) of the [B, K] block `t` of `dtype` (uint8 also takes bool) whose rows do not overlap."""
    if t.dim() != 2 or tuple(t.shape) != (B, K) or (B > 1 and K > 0 and t.stride(0) < K):
        raise NativeError('%s: %s %s must be (%d, %d) with rows that do not overlap' % (what, name, tuple(t.shape), B, K))
    if dtype == torch.uint8 and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return _dev(t, dtype, name), _ld(t)


def cand_labels(qkey, keys, ptr, tails, cand, n_local, ent_row0=0, out=None):
    """(14) label [B, K] uint8: 1 where cand[b, j] is a row of the shard [ent_row0, ent_row0 + n_local) and a known tail of
    qkey[b] in the index arrays of filter_mask(), else 0 (see mgcn_cand_labels). No [B, N/32] mask is built."""
    B = qkey.numel()
    K = _cand_block(cand, B, 'cand_labels')
    if ptr.numel() != keys.numel() + 1:
        raise NativeError('cand_labels: ptr must have len(keys) + 1 entries')
    if out is None:
        out = torch.zeros((B, K), dtype=torch.uint8, device=cand.device)
    _same_device(qkey, keys, ptr, tails, cand, out)
    op, ldl = _cand_rows(out, B, K, torch.uint8, 'cand_labels', 'out')
    if B == 0 or K == 0 or int(n_local) == 0:
        return out
    _check(lib().mgcn_cand_labels(B, K, _dev(qkey, torch.int64, 'qkey'), keys.numel(), _dev(keys, torch.int64, 'keys'),
                                  _dev(ptr, torch.int64, 'ptr'), _dev(tails, torch.int32, 'tails'), int(ent_row0), int(n_local),
                                  _dev(cand, torch.int64, 'cand'), _ld(cand), op, ldl, _stream(cand)), 'mgcn_cand_labels')
    return out


def cand_bce_fwd(x, ent, bias, cand, label, hot, cold, inv_count=None, ent_row0=0):
    """(14) One launch: (loss [] f32, g [B, K] f32 = d loss / d logit per list position) of the mean BCE of
    sigmoid(x[b] . ent[o] + bias[o]) over the lists cand [B, K] int64 against `hot` where label [B, K] (uint8 / bool) is set,
    `cold` elsewhere. inv_count: the mean's weight, default 1 / (B K): EVERY list position counts, dead ones (ids outside the
    shard) contribute zero and get g = 0. For a live position g has the bits of score_bce_fwd's G[o, b] under the same
    inv_count."""
    B, n, O = _score_args(x, ent, bias)
    K = _cand_block(cand, B, 'cand_bce_fwd')
    _same_device(x, ent, bias, cand, label)
    lp, ldl = _cand_rows(label, B, K, torch.uint8, 'cand_bce_fwd', 'label')
    inv = 1.0 / (float(B) * float(K)) if inv_count is None else float(inv_count)
    g = torch.zeros((B, K), dtype=torch.float32, device=x.device)
    parts = torch.zeros(int(lib().mgcn_cand_bce_partials(B, K)), dtype=torch.float32, device=x.device)
    if B and K and n:
        _check(lib().mgcn_cand_bce_fwd(B, K, n, int(ent_row0), O, _dev(x, torch.float32, 'x'), _ld(x), _dev(ent, torch.float32, 'ent'),
                                       _ld(ent), _dev(bias, torch.float32, 'bias'), _dev(cand, torch.int64, 'cand'), _ld(cand), lp, ldl,
                                       float(hot), float(cold), inv, _dev(g, torch.float32, 'g'), K,
                                       _dev(parts, torch.float32, 'loss_partial'), _stream(x)), 'mgcn_cand_bce_fwd')
    return parts.sum() * inv, g


def cand_bce_bwd_x(g, cand, ent, ent_row0=0):
    """(14) dx [B, dim] = sum over the live list positions of g[b, j] ent[o_j], in the fixed chunked order of
    mgcn_cand_bce_bwd_x."""
    B = g.size(0)
    K = _cand_block(cand, B, 'cand_bce_bwd_x')
    _same_device(g, cand, ent)
    if ent.dim() != 2:
        raise NativeError('cand_bce_bwd_x: ent %s must be (n, dim)' % (tuple(ent.shape),))
    gp, ldg = _cand_rows(g, B, K, torch.float32, 'cand_bce_bwd_x', 'g')
    n, O = ent.size(0), ent.size(1)
    ep = _dev(ent, torch.float32, 'ent')
    dx = torch.zeros((B, O), dtype=torch.float32, device=g.device)
    if B and K and n:
        _check(lib().mgcn_cand_bce_bwd_x(B, K, n, int(ent_row0), O, gp, ldg, _dev(cand, torch.int64, 'cand'), _ld(cand),
                                         ep, _ld(ent), _dev(dx, torch.float32, 'dx'), O, _stream(g)),
               'mgcn_cand_bce_bwd_x')
    return dx


def cand_plan(cand, n_local, ent_row0=0, count=True, keys=False):
    """(perm [B K] int64, n_live): the flat positions b K + j of the live entries of cand [B, K] (ids in
    [ent_row0, ent_row0 + n_local)) ordered by (shard row, flat position), then the dead ones by flat position: the plan
    mgcn_cand_bce_bwd_ent takes. One torch.sort of the UNIQUE keys row * (B K) + pos (dead entries: row = n_local), so the plan is a
    function of cand alone whatever the sort does with ties. Integer work in torch, on any device. Counting the live entries
    reads one integer back from the device; count=False skips that and returns n_live = B K, which mgcn_cand_bce_bwd_ent takes
    as well: the dead entries sort last, and the kernel re-checks every entry and skips a dead one.
    keys=True: (perm, n_live, keys) with the sorted keys themselves, keys[i] the key of perm[i]: what
    cand_bce_bwd_ent(run_split=...) finds a run's first entry by. The plan is the same either way."""
    if cand.dim() != 2 or cand.dtype != torch.int64:
        raise NativeError('cand_plan: cand must be int64 [B, K], got %s %s' % (cand.dtype, tuple(cand.shape)))
    n_local, row0, total = int(n_local), int(ent_row0), cand.numel()
    if n_local < 0 or row0 < 0:
        raise NativeError('cand_plan: n_local and ent_row0 must be >= 0')
    if (n_local + 1) * total >= 2 ** 63:
        raise NativeError('cand_plan: the sort key row * (B K) + position overflows int64 (n_local = %d, B K = %d)' % (n_local, total))
    flat = cand.reshape(-1)
    live = flat >= row0                            # with ent_row0 >= 0 and n_local < 2^63 this pair of signed comparisons is the
    if row0 + n_local <= 2 ** 63 - 1:              # kernels' one unsigned comparison of id - ent_row0 against n_local
        live = live & (flat < row0 + n_local)
    row = torch.where(live, flat - row0, torch.full_like(flat, n_local))     # (a wrapped difference of a dead id is never used)
    key = row * total + torch.arange(total, dtype=torch.int64, device=cand.device)
    sorted_keys, perm = torch.sort(key)
    n_live = int(live.sum()) if count else total
    return (perm, n_live, sorted_keys) if keys else (perm, n_live)


RUN_SPLIT_MIN, RUN_SPLIT_MAX = 16, 65536


def check_run_split(what, run_split):
    """run_split is None (the one-wave-per-run backward) or an int in [16, 65536]; anything else is refused."""
    if run_split is None:
        return None
    if isinstance(run_split, bool) or not isinstance(run_split, int) or not RUN_SPLIT_MIN <= run_split <= RUN_SPLIT_MAX:
        raise NativeError('%s: run_split must be None or an int in [%d, %d], got %r' % (what, RUN_SPLIT_MIN, RUN_SPLIT_MAX, run_split))
    return run_split       # (16.0 and True are refused like 15: the value is a count that also keys a captured graph)


def cand_bce_bwd_ent(g, cand, x, perm, n_live, n_local, ent_row0=0, d_ent=None, d_bias=None, want=('ent', 'bias'), run_split=None,
                     keys=None):
    """(14) (d_ent [n_local, dim], d_bias [n_local]): the rows that live list positions name receive their fixed-order sums of
    g[pos] x[b(pos)] and of g[pos] (plan order, see mgcn_cand_bce_bwd_ent); every other row is LEFT AS IT IS. d_ent / d_bias:
    blocks to write into (d_ent may be a column window); None allocates zeros for what `want` names.
    run_split = S (None: the above, unchanged), an int in [16, 65536], with keys = the sorted keys of cand_plan(keys=True): (18),
    a run of more than S plan entries is cut into pieces of S counted from its own first entry, the pieces are summed by
    different waves and folded in piece order (mgcn_cand_bce_bwd_ent_split). A run of at most S entries keeps its bits; a longer
    one has another, equally fixed, summation order. The workspace (about 2 B K / S rows of dim + 1 floats, plus a byte per list
    position) is allocated here per call."""
    check_run_split('cand_bce_bwd_ent', run_split)
    B = g.size(0)
    K = _cand_block(cand, B, 'cand_bce_bwd_ent')
    _same_device(g, cand, x, perm, d_ent, d_bias, keys)
    if x.dim() != 2 or x.size(0) != B or perm.dim() != 1 or perm.numel() != B * K or not 0 <= int(n_live) <= B * K:
        raise NativeError('cand_bce_bwd_ent: x must be (%d, dim), perm [%d] and 0 <= n_live <= %d' % (B, B * K, B * K))
    if run_split is not None and (keys is None or keys.dim() != 1 or keys.numel() != B * K):
        raise NativeError('cand_bce_bwd_ent: run_split needs keys [%d], the sorted keys of cand_plan(keys=True)' % (B * K))
    gp, ldg = _cand_rows(g, B, K, torch.float32, 'cand_bce_bwd_ent', 'g')
    n, O = int(n_local), x.size(1)
    if d_ent is None and 'ent' in want:
        d_ent = torch.zeros((n, O), dtype=torch.float32, device=g.device)
    if d_bias is None and 'bias' in want:
        d_bias = torch.zeros(n, dtype=torch.float32, device=g.device)
    if d_ent is not None and (d_ent.dim() != 2 or tuple(d_ent.shape) != (n, O)):
        raise NativeError('cand_bce_bwd_ent: d_ent must be (%d, %d)' % (n, O))
    if d_bias is not None and (d_bias.numel() != n or not d_bias.is_contiguous()):
        raise NativeError('cand_bce_bwd_ent: d_bias must be contiguous [%d]' % n)
    if run_split is not None:
        if B and K and n and int(n_live):
            need = int(lib().mgcn_cand_bwd_ent_split_workspace(B, K, O, run_split))
            if need == 0:
                raise NativeError('cand_bce_bwd_ent: no workspace for batch = %d, n_cand = %d, dim = %d, run_split = %d'
                                  % (B, K, O, run_split))
            ws = torch.empty(need, dtype=torch.uint8, device=g.device)
            _check(lib().mgcn_cand_bce_bwd_ent_split(B, K, n, int(ent_row0), O, gp, ldg, _dev(cand, torch.int64, 'cand'), _ld(cand),
                                                     _dev(perm, torch.int64, 'perm'), int(n_live), _dev(x, torch.float32, 'x'), _ld(x),
                                                     _dev(d_ent, torch.float32, 'd_ent', True), _ld(d_ent) if d_ent is not None else 0,
                                                     _dev(d_bias, torch.float32, 'd_bias', True), _dev(keys, torch.int64, 'keys'),
                                                     run_split, _dev(ws, torch.uint8, 'workspace'), need, _stream(g)),
                   'mgcn_cand_bce_bwd_ent_split')
        return d_ent, d_bias
    if B and K and n and int(n_live):
        _check(lib().mgcn_cand_bce_bwd_ent(B, K, n, int(ent_row0), O, gp, ldg, _dev(cand, torch.int64, 'cand'), _ld(cand),
                                           _dev(perm, torch.int64, 'perm'), int(n_live), _dev(x, torch.float32, 'x'), _ld(x),
                                           _dev(d_ent, torch.float32, 'd_ent', True), _ld(d_ent) if d_ent is not None else 0,
                                           _dev(d_bias, torch.float32, 'd_bias', True), _stream(g)), 'mgcn_cand_bce_bwd_ent')
    return d_ent, d_bias


# ------------------------------------------------------------------------------------------------
# (16) Softmax cross-entropy over per-query candidate lists. A statistic is a row of four 32-bit words held in a float32 tensor
# [..., 4]: m, s as f32, n_live, n_pos as int32 (cand_ce_stat_fields reads them).
def cand_ce_empty_stat(rows, device):
    """[rows, 4]: the statistic (-inf, 0, 0, 0) of a row without a live position (a rank without entity rows passes it on)."""
    stat = torch.zeros((int(rows), 4), dtype=torch.float32, device=device)
    stat[:, 0] = float('-inf')
    return stat


def cand_ce_stat_fields(stat):
    """(m, s, n_live, n_pos) of a statistics tensor [..., 4]: two float32 and two int32 views."""
    words = stat.view(torch.int32)
    return stat[..., 0], stat[..., 1], words[..., 2], words[..., 3]


def cand_ce_logits(x, ent, bias, cand, label, ent_row0=0):
    """(16) One launch: (z [B, K] f32, stat [B, ceil(K / 64), 4]): the logits x[b] . ent[o] + bias[o] of the lists cand [B, K]
    int64 (-inf at positions whose id is outside [ent_row0, ent_row0 + n_local)) and per (query, 64 list positions) the
    statistic (max, sum of exp(z - max), live positions, live positions with label set). See mgcn_cand_ce_logits."""
    B, n, O = _score_args(x, ent, bias)
    K = _cand_block(cand, B, 'cand_ce_logits')
    _same_device(x, ent, bias, cand, label)
    lp, ldl = _cand_rows(label, B, K, torch.uint8, 'cand_ce_logits', 'label')
    chunks = int(lib().mgcn_cand_ce_partials(B, K)) // B if B and K else 0
    if not (B and K and n):
        return (torch.full((B, K), float('-inf'), dtype=torch.float32, device=x.device),
                cand_ce_empty_stat(B * chunks, x.device).view(B, chunks, 4))
    z = torch.empty((B, K), dtype=torch.float32, device=x.device)
    stat = torch.empty((B, chunks, 4), dtype=torch.float32, device=x.device)
    _check(lib().mgcn_cand_ce_logits(B, K, n, int(ent_row0), O, _dev(x, torch.float32, 'x'), _ld(x), _dev(ent, torch.float32, 'ent'),
                                     _ld(ent), _dev(bias, torch.float32, 'bias'), _dev(cand, torch.int64, 'cand'), _ld(cand), lp, ldl,
                                     _dev(z, torch.float32, 'z'), K, _dev(stat, torch.float32, 'stat'), _stream(x)),
           'mgcn_cand_ce_logits')
    return z, stat


def cand_ce_merge(stat, part_dim=1):
    """(16) [B, 4]: the statistics of `stat` folded over its parts in part order (see mgcn_cand_ce_merge). stat is contiguous
    float32 [B, P, 4] (part_dim = 1: the chunks of cand_ce_logits) or [P, B, 4] (part_dim = 0: the ranks' blocks of an
    all-gather). One part gives the same bits back."""
    if stat.dim() != 3 or stat.size(2) != 4 or part_dim not in (0, 1) or not stat.is_contiguous():
        raise NativeError('cand_ce_merge: stat %s must be contiguous [B, P, 4] (part_dim 1) or [P, B, 4] (part_dim 0)' % (tuple(stat.shape),))
    B, P = stat.size(1 - part_dim), stat.size(part_dim)
    if P < 1:
        if B == 0:
            return cand_ce_empty_stat(0, stat.device)
        raise NativeError('cand_ce_merge: no part to merge')
    out = torch.empty((B, 4), dtype=torch.float32, device=stat.device)
    if B:
        row_stride, part_stride = (P, 1) if part_dim == 1 else (1, B)
        _check(lib().mgcn_cand_ce_merge(B, P, _dev(stat, torch.float32, 'stat'), row_stride, part_stride,
                                        _dev(out, torch.float32, 'out'), _stream(stat)), 'mgcn_cand_ce_merge')
    return out


def cand_ce_finish(z, cand, label, stat, lbl_smooth, n_local, ent_row0=0, inv_batch=None):
    """(16) One launch: (loss [] f32, g [B, K] f32 = d loss / d logit, loss_partial [B ceil(K / 64)]) of the softmax
    cross-entropy over the lists, from the logits z of cand_ce_logits and the rows' statistics stat [B, 4] (of the whole row:
    merged over chunks and, sharded, over ranks). inv_batch: the weight of a query, default 1 / B. Positions whose id is outside
    [ent_row0, ent_row0 + n_local) and rows without a positive get g = 0 and add nothing. See mgcn_cand_ce_finish."""
    B = z.size(0)
    K = _cand_block(cand, B, 'cand_ce_finish')
    _same_device(z, cand, label, stat)
    if tuple(stat.shape) != (B, 4) or not stat.is_contiguous():
        raise NativeError('cand_ce_finish: stat %s must be contiguous (%d, 4)' % (tuple(stat.shape), B))
    zp, ldz = _cand_rows(z, B, K, torch.float32, 'cand_ce_finish', 'z')
    lp, ldl = _cand_rows(label, B, K, torch.uint8, 'cand_ce_finish', 'label')
    inv = 1.0 / float(B) if inv_batch is None else float(inv_batch)
    n_parts = int(lib().mgcn_cand_ce_partials(B, K))
    if not (B and K and int(n_local)):
        g = torch.zeros((B, K), dtype=torch.float32, device=z.device)
        parts = torch.zeros(n_parts, dtype=torch.float32, device=z.device)
        return parts.sum() * inv, g, parts
    g = torch.empty((B, K), dtype=torch.float32, device=z.device)
    parts = torch.empty(n_parts, dtype=torch.float32, device=z.device)
    _check(lib().mgcn_cand_ce_finish(B, K, int(n_local), int(ent_row0), zp, ldz, _dev(cand, torch.int64, 'cand'), _ld(cand), lp, ldl,
                                     _dev(stat, torch.float32, 'stat'), float(lbl_smooth), inv, _dev(g, torch.float32, 'g'), K,
                                     _dev(parts, torch.float32, 'loss_partial'), _stream(z)), 'mgcn_cand_ce_finish')
    return parts.sum() * inv, g, parts


# ------------------------------------------------------------------------------------------------
# (8) ConvE query trunk. geom = (k_w, k_h, kernel_size, num_filter, O)
def conve_supported(k_w, k_h, kernel_size, num_filter, dim_out):
    """Geometries mgcn_conve_trunk_fwd takes (k_w k_h == O <= 512, 1 <= kernel <= min(2 k_w, k_h), a pack below 2^31 floats)."""
    geom = tuple(int(v) for v in (k_w, k_h, kernel_size, num_filter, dim_out))
    return min(geom) >= 1 and lib().mgcn_conve_packed_bytes(*geom) > 0


def conve_pack(geom, conv_w, conv_b, fc_w, fc_b, bn0, bn1, bn2, out=None):
    """Fold and pack the trunk's weights (see mgcn_conve_pack): bn* = (running_mean, running_var, weight, bias, eps) with
    weight / bias None for a BN without affine pair. `out`: a pack to refresh in place (same geometry and device)."""
    geom = tuple(int(v) for v in geom)
    nbytes = lib().mgcn_conve_packed_bytes(*geom)
    if nbytes == 0:
        raise NativeError('conve_pack: geometry %s is not supported' % (geom,))
    if not conv_w.is_contiguous() or fc_w.dim() != 2:
        raise NativeError('conve_pack: conv weight must be contiguous, fc weight 2-d')
    if out is None or out.numel() * 4 < nbytes or out.device != fc_w.device:
        out = torch.empty(nbytes // 4, dtype=torch.float32, device=fc_w.device)
    args = []
    for mean, var, gamma, beta, eps in (bn0, bn1, bn2):
        _same_device(fc_w, mean, var, gamma, beta)
        args += [_dev(mean, torch.float32, 'bn mean'), _dev(var, torch.float32, 'bn var'), _dev(gamma, torch.float32, 'bn weight', True),
                 _dev(beta, torch.float32, 'bn bias', True), float(eps)]
    _same_device(fc_w, conv_w, conv_b, fc_b, out)
    _check(lib().mgcn_conve_pack(*geom, _dev(conv_w, torch.float32, 'conv weight'), _dev(conv_b, torch.float32, 'conv bias', True),
                                 _dev(fc_w, torch.float32, 'fc weight'), _ld(fc_w), _dev(fc_b, torch.float32, 'fc bias', True),
                                 *args, _dev(out, torch.float32, 'pack'), out.numel() * 4, _stream(fc_w)), 'mgcn_conve_pack')
    return out


def conve_trunk(geom, packed, ent, src, rel, rel_idx, out=None):
    """x [B, O] = trunk(ent[src], rel[rel_idx]) on the HIP kernel; src / rel_idx int64 [B] or None (rows 0 .. B-1 of both
    tables, which then have the same number of rows). `out`: an f32 [B, >= O] view to fill (row stride = its ldo)."""
    geom = tuple(int(v) for v in geom)
    O = geom[4]
    if ent.dim() != 2 or rel.dim() != 2 or ent.size(1) != O or rel.size(1) != O:
        raise NativeError('conve_trunk: tables must be [rows, %d], got %s and %s' % (O, tuple(ent.shape), tuple(rel.shape)))
    if (src is None) != (rel_idx is None):
        raise NativeError('conve_trunk: give both index vectors or neither')
    B = int(src.numel()) if src is not None else int(ent.size(0))
    if src is not None and (rel_idx.numel() != B or not src.is_contiguous() or not rel_idx.is_contiguous()):
        raise NativeError('conve_trunk: index vectors must be contiguous and of equal length')
    if src is None and rel.size(0) != B:
        raise NativeError('conve_trunk: without index vectors both tables need the same number of rows')
    _same_device(ent, rel, src, rel_idx, packed, out)
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=ent.device)
    elif out.dim() != 2 or out.size(0) != B or out.size(1) != O:
        raise NativeError('conve_trunk: out must be [%d, %d]' % (B, O))
    if B == 0:
        return out
    nbytes = lib().mgcn_conve_trunk_workspace(B, *geom)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ent.device) if nbytes else None    # the caching allocator's memory
    _check(lib().mgcn_conve_trunk_fwd(B, *geom, _dev(ent, torch.float32, 'ent'), _ld(ent), ent.size(0),
                                      _dev(src, torch.int64, 'src', True), _dev(rel, torch.float32, 'rel'), _ld(rel), rel.size(0),
                                      _dev(rel_idx, torch.int64, 'rel index', True), _dev(packed, torch.float32, 'pack'),
                                      _dev(out, torch.float32, 'out'), _ld(out) if B > 1 else max(out.stride(0), O),
                                      _dev(ws, torch.uint8, 'workspace', True), nbytes, _stream(ent)), 'mgcn_conve_trunk_fwd')
    return out


# ------------------------------------------------------------------------------------------------
# (9) ConvE query trunk, training mode. geom = (k_w, k_h, kernel_size, num_filter, O)
def conve_train_supported(batch, geom):
    """Batches and geometries mgcn_conve_train_fwd takes (those of (8), 1 <= B <= 4096, B H W >= 2, B F H W < 2^31)."""
    geom = tuple(int(v) for v in geom)
    return min(geom) >= 1 and int(batch) >= 1 and lib().mgcn_conve_train_workspace(int(batch), *geom) > 0


def _rows(t, O, what):
    if t.dim() != 2 or t.size(1) != O:
        raise NativeError('%s must be [B, %d], got %s' % (what, O, tuple(t.shape)))
    return _dev(t, torch.float32, what), (_ld(t) if t.size(0) > 1 else max(t.stride(0), O))


def conve_train_fwd(geom, s, r, conv_w, conv_b, fc_w, fc_b, bn0, bn1, keep, inv_keep):
    """z [B, O], saved statistics [2 + 2 F] (mu0, rstd0, mu1, rstd1) and the workspace that holds c for the backward.
    bn* = (weight, bias, running_mean, running_var, momentum, eps); the running statistics are updated in place.
    keep: bool / uint8 [B, F H W] contiguous or None (keep all)."""
    geom = tuple(int(v) for v in geom)
    O, B = geom[4], int(s.size(0))
    nbytes = lib().mgcn_conve_train_workspace(B, *geom)
    if nbytes == 0:
        raise NativeError('conve_train_fwd: batch %d of geometry %s is not supported' % (B, geom))
    if not conv_w.is_contiguous() or fc_w.dim() != 2 or (keep is not None and not keep.is_contiguous()):
        raise NativeError('conve_train_fwd: conv weight and mask must be contiguous, fc weight 2-d')
    _same_device(s, r, conv_w, conv_b, fc_w, fc_b, keep, *bn0[:4], *bn1[:4])
    sp, lds = _rows(s, O, 's')
    rp, ldr = _rows(r, O, 'r')
    z = torch.empty((B, O), dtype=torch.float32, device=s.device)
    saved = torch.empty(2 + 2 * geom[3], dtype=torch.float32, device=s.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    bn_args = []
    for gamma, beta, rm, rv, mom, eps in (bn0, bn1):
        bn_args += [_dev(gamma, torch.float32, 'bn weight'), _dev(beta, torch.float32, 'bn bias'), _dev(rm, torch.float32, 'running mean'),
                    _dev(rv, torch.float32, 'running var'), float(mom), float(eps)]
    _check(lib().mgcn_conve_train_fwd(B, *geom, sp, lds, rp, ldr, _dev(conv_w, torch.float32, 'conv weight'),
                                      _dev(conv_b, torch.float32, 'conv bias', True), _dev(fc_w, torch.float32, 'fc weight'), _ld(fc_w),
                                      _dev(fc_b, torch.float32, 'fc bias', True), *bn_args,
                                      None if keep is None else keep.data_ptr(), float(inv_keep), _dev(z, torch.float32, 'z'), O,
                                      _dev(saved, torch.float32, 'saved'), ws.data_ptr(), nbytes, _stream(s)), 'mgcn_conve_train_fwd')
    return z, saved, ws


def conve_train_bwd(geom, s, r, conv_w, fc_w, bn0_weight, bn0_bias, bn1_weight, bn1_bias, keep, inv_keep, saved, ws, gz, want):
    """The gradients named in `want` (a set of 's', 'r', 'conv_w', 'conv_b', 'g0', 'b0', 'g1', 'b1', 'fc_w', 'fc_b') as a
    dict; `ws` is the forward's workspace: its first section c [B, F H W] is read and keeps its bits, every later section is this
    call's scratch and is overwritten (include/mgcn_hip.h (9)), with the same bits whenever the call is repeated on the same inputs."""
    geom = tuple(int(v) for v in geom)
    k_w, k_h, ks, F, O = geom
    B = int(s.size(0))
    sp, lds = _rows(s, O, 's')
    rp, ldr = _rows(r, O, 'r')
    gp, ldg = _rows(gz, O, 'gz')
    _same_device(s, r, conv_w, fc_w, keep, saved, ws, gz)
    shapes = {'s': (B, O), 'r': (B, O), 'conv_w': tuple(conv_w.shape), 'conv_b': (F,), 'g0': (1,), 'b0': (1,), 'g1': (F,), 'b1': (F,),
              'fc_w': (O, fc_w.size(1)), 'fc_b': (O,)}
    out = {k: torch.empty(shapes[k], dtype=torch.float32, device=s.device) for k in shapes if k in want}
    ptr = lambda k: out[k].data_ptr() if k in out else None
    _check(lib().mgcn_conve_train_bwd(B, *geom, sp, lds, rp, ldr, _dev(conv_w, torch.float32, 'conv weight'),
                                      _dev(fc_w, torch.float32, 'fc weight'), _ld(fc_w), _dev(bn0_weight, torch.float32, 'bn0 weight'),
                                      _dev(bn0_bias, torch.float32, 'bn0 bias'), _dev(bn1_weight, torch.float32, 'bn1 weight'),
                                      _dev(bn1_bias, torch.float32, 'bn1 bias'), None if keep is None else keep.data_ptr(),
                                      float(inv_keep), _dev(saved, torch.float32, 'saved'), gp, ldg, ptr('s'), O, ptr('r'), O,
                                      ptr('conv_w'), ptr('conv_b'), ptr('g0'), ptr('b0'), ptr('g1'), ptr('b1'), ptr('fc_w'),
                                      fc_w.size(1), ptr('fc_b'), ws.data_ptr(), ws.numel(), _stream(s)), 'mgcn_conve_train_bwd')
    return out


# ------------------------------------------------------------------------------------------------
# (11) the training step's query path: the row gathers' backward and the trunk's tail
QUERY_MAX_BATCH = _DEFINES['MGCN_QUERY_MAX_BATCH']


def query_rows_supported(batch):
    return 1 <= int(batch) <= QUERY_MAX_BATCH


def query_rows_bwd(idx, d, num_rows, out=None):
    """out [num_rows, dim] with out[idx[b]] += d[b] added in ascending b (bit for bit the sequential f32 loop), rows that no
    b names zero. idx: int64 [B], d: f32 [B, dim]; `out` may be a column window of a wider tensor (its other columns stay)."""
    if idx.dim() != 1 or d.dim() != 2 or d.size(0) != idx.numel():
        raise NativeError('query_rows_bwd: idx must be [B] and d [B, dim], got %s and %s' % (tuple(idx.shape), tuple(d.shape)))
    B, dim = int(d.size(0)), int(d.size(1))
    if out is None:
        out = torch.empty((int(num_rows), dim), dtype=torch.float32, device=d.device)
    elif out.dim() != 2 or tuple(out.shape) != (int(num_rows), dim):
        raise NativeError('query_rows_bwd: out must be [%d, %d]' % (num_rows, dim))
    _same_device(idx, d, out)
    dp, ldd = _rows(d, dim, 'd')
    op, ldo = _rows(out, dim, 'out')
    nbytes = lib().mgcn_query_rows_bwd_workspace(B)
    if nbytes == 0:
        raise NativeError('query_rows_bwd: a batch of %d is not supported' % B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d.device)
    _check(lib().mgcn_query_rows_bwd(B, int(num_rows), dim, _dev(idx.contiguous(), torch.int64, 'idx'), dp, ldd, op, ldo, ws.data_ptr(),
                                     nbytes, _stream(d)), 'mgcn_query_rows_bwd')
    return out


def conve_tail_supported(batch, dim):
    """Shapes mgcn_conve_tail_fwd takes: batch statistics need 2 <= B (<= 4096)."""
    return 2 <= int(batch) <= QUERY_MAX_BATCH and int(dim) >= 1


def _keep_rows(keep, B, O):
    if keep is None:
        return None, O
    if keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (B, O) or (O > 1 and keep.stride(1) != 1):
        raise NativeError('conve tail: keep must be bool / uint8 [%d, %d] with a contiguous last dimension' % (B, O))
    return keep.data_ptr(), max(keep.stride(0), O)


def conve_tail_fwd(z, keep, inv_keep, gamma, beta, running_mean, running_var, momentum, eps):
    """x = relu(bn2_batch(z keep inv_keep)) [B, O] and saved [2, O] (mean, rstd); the running statistics are updated in
    place. keep: bool / uint8 [B, O] or None (keep all)."""
    B, O = int(z.size(0)), int(z.size(1))
    _same_device(z, keep, gamma, beta, running_mean, running_var)
    zp, ldz = _rows(z, O, 'z')
    kp, ldk = _keep_rows(keep, B, O)
    x = torch.empty((B, O), dtype=torch.float32, device=z.device)
    saved = torch.empty((2, O), dtype=torch.float32, device=z.device)
    _check(lib().mgcn_conve_tail_fwd(B, O, zp, ldz, kp, ldk, float(inv_keep), _dev(gamma, torch.float32, 'bn weight'),
                                     _dev(beta, torch.float32, 'bn bias'), _dev(running_mean, torch.float32, 'running mean'),
                                     _dev(running_var, torch.float32, 'running var'), float(momentum), float(eps), x.data_ptr(), O,
                                     saved.data_ptr(), O, _stream(z)), 'mgcn_conve_tail_fwd')
    return x, saved


def conve_tail_bwd(z, keep, inv_keep, x, saved, gamma, gx, want=('z', 'gamma', 'beta')):
    """(gz [B, O], d gamma [O], d beta [O]) of the forward's (z, keep, x, saved) for gx; None for what `want` leaves out."""
    B, O = int(z.size(0)), int(z.size(1))
    _same_device(z, keep, x, saved, gamma, gx)
    zp, ldz = _rows(z, O, 'z')
    kp, ldk = _keep_rows(keep, B, O)
    xp, ldx = _rows(x, O, 'x')
    gp, ldg = _rows(gx, O, 'gx')
    if tuple(saved.shape) != (2, O) or not saved.is_contiguous():
        raise NativeError('conve_tail_bwd: saved must be contiguous [2, %d]' % O)
    new = lambda name, shape: torch.empty(shape, dtype=torch.float32, device=z.device) if name in want else None
    gz, dg, db = new('z', (B, O)), new('gamma', (O,)), new('beta', (O,))
    ptr = lambda t: None if t is None else t.data_ptr()
    _check(lib().mgcn_conve_tail_bwd(B, O, zp, ldz, kp, ldk, float(inv_keep), xp, ldx, _dev(saved, torch.float32, 'saved'), O,
                                     _dev(gamma, torch.float32, 'bn weight'), gp, ldg, ptr(gz), O, ptr(dg), ptr(db), _stream(z)),
           'mgcn_conve_tail_bwd')
    return gz, dg, db


def filter_mask(qkey, keys, ptr, tails, n_local, ent_row0=0, out=None):
    """Bit-packed filter rows [B, ceil(n_local/32)] int32 for queries with keys `qkey` (see mgcn_filter_mask)."""
    B, words = qkey.numel(), (int(n_local) + 31) // 32
    if out is None:
        out = torch.empty((B, words), dtype=torch.int32, device=qkey.device)
    if out.size(0) != B or out.size(1) < words or not out.is_contiguous():
        raise NativeError('filter_mask: out must be contiguous (%d, >= %d)' % (B, words))
    if ptr.numel() != keys.numel() + 1:
        raise NativeError('filter_mask: ptr must have len(keys) + 1 entries')
    _same_device(qkey, keys, ptr, tails, out)
    _check(lib().mgcn_filter_mask(B, _dev(qkey, torch.int64, 'qkey'), keys.numel(), _dev(keys, torch.int64, 'keys'),
                                  _dev(ptr, torch.int64, 'ptr'), _dev(tails, torch.int32, 'tails'), int(ent_row0),
                                  int(n_local), _dev(out, torch.int32, 'mask'), out.size(1), _stream(qkey)),
           'mgcn_filter_mask')
    return out


def smoothed_targets(lbl_smooth, num_entities):
    """(hot, cold) = (1 - eps) * y + 1/N for y = 1, 0, evaluated in f32 as numpy does (data_loader.py:41-43)."""
    import numpy as np
    y = np.array([1.0, 0.0], dtype=np.float32)
    if lbl_smooth != 0.0:
        y = (1.0 - lbl_smooth) * y + (1.0 / int(num_entities))
    return float(y[0]), float(y[1])


def score_bce_supported(x, ent):
    return (x.size(0) % 4 == 0 and x.size(1) % 4 == 0 and x.is_contiguous() and ent.is_contiguous()
            and x.data_ptr() % 16 == 0 and ent.data_ptr() % 16 == 0)


def score_bce_fwd(x, ent, bias, mask, hot, cold, num_entities=None):
    """(N3) One launch: returns (loss [] f32, G [n, B] f32 = d loss / d logits, entity-major) for the mean BCE of
    sigmoid(x @ ent^T + bias) against targets `hot` at the mask's bits, `cold` elsewhere (see mgcn_score_bce_fwd).
    `num_entities`: the mean's count of entities when `ent` is one rank's row shard of a larger table (default: its rows);
    the ranks' losses and gradients then add up to the whole table's."""
    B, n, O = _score_args(x, ent, bias)
    if mask.dim() != 2 or mask.size(0) != B or mask.size(1) < (n + 31) // 32 or not mask.is_contiguous():
        raise NativeError('score_bce_fwd: mask must be contiguous (%d, >= %d)' % (B, (n + 31) // 32))
    _same_device(x, ent, bias, mask)
    g = torch.empty((n, B), dtype=torch.float32, device=x.device)
    parts = torch.empty(int(lib().mgcn_score_bce_partials(B, n)), dtype=torch.float32, device=x.device)
    inv = 1.0 / (float(B) * float(n if num_entities is None else int(num_entities)))
    _check(lib().mgcn_score_bce_fwd(B, n, O, _dev(x, torch.float32, 'x'), _ld(x), _dev(ent, torch.float32, 'ent'), _ld(ent),
                                    _dev(bias, torch.float32, 'bias'), _dev(mask, torch.int32, 'mask'), mask.size(1),
                                    float(hot), float(cold), inv, _dev(g, torch.float32, 'grad_logit'), g.stride(0),
                                    _dev(parts, torch.float32, 'loss_partial'), _stream(x)), 'mgcn_score_bce_fwd')
    return parts.sum() * inv, g


# ------------------------------------------------------------------------------------------------
# (20) Softmax cross-entropy over the full entity table: (16)'s loss with every entity a live position. Statistics are (16)'s
# records; z and g are entity-major [n, B] like score_bce_fwd's G.
def _table_mask(mask, B, n, what):
    if mask.dim() != 2 or mask.size(0) != B or mask.size(1) < (n + 31) // 32 or not mask.is_contiguous():
        raise NativeError('%s: mask must be contiguous (%d, >= %d)' % (what, B, (n + 31) // 32))


def score_ce_supported(x, ent):
    """Whether mgcn_score_ce_logits takes the batch: score_bce_fwd's rule."""
    return score_bce_supported(x, ent)


def score_ce_fold_shape(n):
    """(tiles, G, P) of a table of n rows: its tiles of 32 entities fold in one level (G = 1, P = tiles) up to 64 tiles, beyond in
    two: G = ceil(sqrt(tiles)) groups of P = ceil(tiles / G) tiles, group g holding the tiles g, g + G, g + 2 G, ... A function
    of n alone, so the order of every sum is fixed."""
    tiles = (int(n) + 31) // 32
    G = 1 if tiles <= 64 else math.isqrt(tiles - 1) + 1
    return tiles, G, (tiles + G - 1) // G if tiles else 0


def score_ce_logits(x, ent, bias, mask):
    """(20) One launch: (z [n, B] f32 entity-major, stat [G P, B, 4]): the logits ent[n] . x[b] + bias[n] and per (tile of 32
    entities, query) the statistic (max, sum of exp(z - max), rows of the tile, set mask bits of the tile); (tiles, G, P) =
    score_ce_fold_shape(n), the records past `tiles` hold the empty statistic. Fold the tiles with score_ce_fold(stat, n). See
    mgcn_score_ce_logits; raises for a batch score_ce_supported refuses."""
    B, n, O = _score_args(x, ent, bias)
    _table_mask(mask, B, n, 'score_ce_logits')
    _same_device(x, ent, bias, mask)
    tiles, G, P = score_ce_fold_shape(n)
    z = torch.empty((n, B), dtype=torch.float32, device=x.device)
    stat = torch.empty((G * P, B, 4), dtype=torch.float32, device=x.device)
    if G * P > tiles:
        stat[tiles:] = cand_ce_empty_stat(1, x.device)
    if B and n:
        _check(lib().mgcn_score_ce_logits(B, n, O, _dev(x, torch.float32, 'x'), _ld(x), _dev(ent, torch.float32, 'ent'), _ld(ent),
                                          _dev(bias, torch.float32, 'bias'), _dev(mask, torch.int32, 'mask'), mask.size(1),
                                          _dev(z, torch.float32, 'z'), B, _dev(stat, torch.float32, 'stat'), B, _stream(x)),
               'mgcn_score_ce_logits')
    return z, stat


def score_ce_fold(stat, n):
    """(20) [B, 4]: the rows' statistics from the tile records stat [G P, B, 4] of score_ce_logits for a table of n rows, by
    mgcn_cand_ce_merge through its strides. Up to 64 tiles: ONE sequential fold in tile order. Beyond, one thread per query
    walking every tile would be the stage's longest launch (62 500 dependent steps at n = 2 000 000), so two folds: (group g,
    query b) folds its tiles g, g + G, ... in that order (B G rows, P parts, part_stride = G B records), then query b folds its
    G groups in group order. Empty records are skipped by the merge."""
    tiles, G, P = score_ce_fold_shape(n)
    if stat.dim() != 3 or stat.size(0) != G * P or stat.size(2) != 4 or not stat.is_contiguous():
        raise NativeError('score_ce_fold: stat %s must be contiguous (%d, B, 4) for %d rows' % (tuple(stat.shape), G * P, n))
    B = stat.size(1)
    if G <= 1:
        return cand_ce_merge(stat, part_dim=0)
    return cand_ce_merge(cand_ce_merge(stat.view(P, G * B, 4), part_dim=0).view(G, B, 4), part_dim=0)


def score_ce_finish(z, mask, stat, lbl_smooth, num_entities, inv_batch=None):
    """(20) One launch, IN PLACE: z [n, B] (contiguous f32, the logits) becomes g = d loss / d logit; returns (loss [] f32, g = z,
    loss_partial). stat [B, 4]: the rows' statistics over the WHOLE table (merged over tiles and, sharded, over ranks);
    num_entities: the global entity count the smoothing mass lbl_smooth is spread over; inv_batch: the weight of a query, default
    1 / B. Any batch and alignment. See mgcn_score_ce_finish."""
    if z.dim() != 2 or z.dtype != torch.float32 or not z.is_contiguous():
        raise NativeError('score_ce_finish: z must be contiguous f32 [n, B]')
    n, B = z.shape
    _table_mask(mask, B, n, 'score_ce_finish')
    _same_device(z, mask, stat)
    if tuple(stat.shape) != (B, 4) or stat.dtype != torch.float32 or not stat.is_contiguous():
        raise NativeError('score_ce_finish: stat %s must be contiguous f32 (%d, 4)' % (tuple(stat.shape), B))
    inv = (1.0 / float(B) if B else 0.0) if inv_batch is None else float(inv_batch)
    parts = torch.empty(int(lib().mgcn_score_ce_partials(B, n)), dtype=torch.float32, device=z.device)
    if B and n:
        _check(lib().mgcn_score_ce_finish(B, n, _dev(z, torch.float32, 'z'), B, _dev(mask, torch.int32, 'mask'), mask.size(1),
                                          _dev(stat, torch.float32, 'stat'), float(lbl_smooth), inv, int(num_entities),
                                          _dev(parts, torch.float32, 'loss_partial'), _stream(z)), 'mgcn_score_ce_finish')
    return parts.sum() * inv, z, parts


def mask_popcount(mask, n=None):
    """[B] int32: the set bits of each row of a bit-packed mask [B, words] int32 (integer ops on the device, no host read). `n`:
    only the bits of entities below n count, as in the EPI_CE epilogue (mgcn_filter_mask sets none past them; this does not rely
    on it)."""
    v = mask.to(torch.int64) & 0xffffffff
    if n is not None:
        words = (int(n) + 31) // 32
        v = v[:, :words]
        if int(n) % 32:
            v = torch.cat([v[:, :-1], v[:, -1:] & ((1 << (int(n) % 32)) - 1)], 1)
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    v = (v + (v >> 4)) & 0x0f0f0f0f
    return (((v * 0x01010101) >> 24) & 0xff).sum(1).to(torch.int32)


def label_rows(qkey, keys, ptr, tails, n_local, lbl_smooth=0.0, num_entities=None, ent_row0=0, out=None):
    """Dense training targets [B, n_local] f32 for queries with keys `qkey` (see mgcn_label_rows): 1 at the known
    tails, 0 elsewhere, then (1 - eps) * y + 1/N when eps != 0 (data_loader.py:41-43, evaluated in f32 as numpy does)."""
    B = qkey.numel()
    y = smoothed_targets(lbl_smooth, int(n_local if num_entities is None else num_entities))
    if out is None:
        out = torch.empty((B, int(n_local)), dtype=torch.float32, device=qkey.device)
    if out.size(0) != B or out.size(1) < n_local or out.stride(1) != 1:
        raise NativeError('label_rows: out must be (%d, >= %d) with unit column stride' % (B, n_local))
    if ptr.numel() != keys.numel() + 1:
        raise NativeError('label_rows: ptr must have len(keys) + 1 entries')
    _same_device(qkey, keys, ptr, tails, out)
    _check(lib().mgcn_label_rows(B, _dev(qkey, torch.int64, 'qkey'), keys.numel(), _dev(keys, torch.int64, 'keys'),
                                 _dev(ptr, torch.int64, 'ptr'), _dev(tails, torch.int32, 'tails'), int(ent_row0),
                                 int(n_local), float(y[0]), float(y[1]), _dev(out, torch.float32, 'labels'),
                                 out.stride(0), _stream(qkey)), 'mgcn_label_rows')
    return out


ADAM_CHUNK = _DEFINES['MGCN_ADAM_CHUNK']     # elements per workgroup of the optimizer kernels (csrc/optim.hip)
ADAM_BATCH = _DEFINES['MGCN_ADAM_BATCH']     # tensors per launch


def _ptr_array(tensors):
    """Host array of the tensors' device pointers (None -> NULL)."""
    return (_ptr * max(len(tensors), 1))(*[None if t is None else t.data_ptr() for t in tensors])


def _adam_list(what, lists):
    """Check a list of f32 device tensors per role (contiguous, same device, same element counts as the first role)."""
    first = lists[0]
    for ts in lists:
        if len(ts) != len(first):
            raise NativeError('%s: the tensor lists differ in length' % what)
        for t, ref in zip(ts, first):
            if t is None:
                continue
            _dev(t, torch.float32, what)
            if not t.is_contiguous() or (ref is not None and t.numel() != ref.numel()):
                raise NativeError('%s: tensors must be contiguous with matching element counts' % what)
    _same_device(*[t for ts in lists for t in ts])


def adam_sq_norms(grads, out=None):
    """(10) sq [n] f32: the sum of squares of every gradient of the list (0 for a None or empty one), in a fixed order."""
    _adam_list('adam_sq_norms', [grads])
    live = [g for g in grads if g is not None]
    if not live:
        raise NativeError('adam_sq_norms: no gradient to take the device from')
    dev, n = live[0].device, len(grads)
    numel = (_i64 * max(n, 1))(*[0 if g is None else g.numel() for g in grads])
    sq = torch.empty(n, dtype=torch.float32, device=dev) if out is None else out
    if sq.numel() != n or not sq.is_contiguous():
        raise NativeError('adam_sq_norms: out must be contiguous [%d]' % n)
    nbytes = lib().mgcn_adam_sq_norms_workspace(n, numel)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    _check(lib().mgcn_adam_sq_norms(n, _ptr_array(grads), numel, _dev(sq, torch.float32, 'sq'), _dev(ws, torch.float32, 'ws'),
                                    nbytes, _stream(sq)), 'mgcn_adam_sq_norms')
    return sq


def adam_clip_coef(sq, max_norm, out=None):
    """(10) [2] f32 = (total norm, clip coefficient) from the per-tensor sums of squares; stays on the device."""
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=sq.device)
    _same_device(sq, out)
    if not sq.is_contiguous() or out.numel() != 2 or not out.is_contiguous():
        raise NativeError('adam_clip_coef: sq must be contiguous and out [2]')
    _check(lib().mgcn_adam_clip_coef(sq.numel(), _dev(sq, torch.float32, 'sq'), float(max_norm), _dev(out, torch.float32, 'out'),
                                     _stream(sq)), 'mgcn_adam_clip_coef')
    return out


def adam_step(grads, params, exp_avgs, exp_avg_sqs, coef, step_size, bc2_sqrt, beta1, beta2, eps, weight_decay, hyper_dev=None):
    """(10) One Adam update of the listed tensors in place; `coef`: a 1-element device tensor (None = no clipping). A None
    or empty gradient skips its tensor. `hyper_dev`: a contiguous f32 device tensor of two elements that holds (step_size,
    bc2_sqrt); the kernels then read the pair from it when they RUN (mgcn_adam_step_dev: what a captured launch needs), and the two
    by-value arguments are not used."""
    _adam_list('adam_step', [params, grads, exp_avgs, exp_avg_sqs])
    _same_device(coef, hyper_dev, *params)
    n = len(params)
    if n == 0:
        return
    numel = (_i64 * n)(*[p.numel() for p in params])
    if hyper_dev is not None:
        if hyper_dev.numel() != 2 or not hyper_dev.is_contiguous():
            raise NativeError('adam_step: hyper_dev must be a contiguous tensor of two floats (step_size, bc2_sqrt)')
        _check(lib().mgcn_adam_step_dev(n, _ptr_array(grads), _ptr_array(params), _ptr_array(exp_avgs), _ptr_array(exp_avg_sqs), numel,
                                        _dev(coef, torch.float32, 'coef', True), _dev(hyper_dev, torch.float32, 'hyper_dev'), float(beta1),
                                        float(beta2), float(eps), float(weight_decay), _stream(params[0])), 'mgcn_adam_step_dev')
        return
    _check(lib().mgcn_adam_step(n, _ptr_array(grads), _ptr_array(params), _ptr_array(exp_avgs), _ptr_array(exp_avg_sqs), numel,
                                _dev(coef, torch.float32, 'coef', True), float(step_size), float(bc2_sqrt), float(beta1),
                                float(beta2), float(eps), float(weight_decay), _stream(params[0])), 'mgcn_adam_step')


# ------------------------------------------------------------------------------------------------
# (12) counter-based dropout (csrc/dropout.hip)
_M64 = (1 << 64) - 1
DROPOUT_SITE_FEATURE, DROPOUT_SITE_HIDDEN = 0x1000, 0x1001


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def dropout_key(seed, step, site):
    """key(seed, step, site) = sm(sm(sm(seed) ^ step) ^ site), sm = one SplitMix64 step: the 64-bit key of one site's masks."""
    return _splitmix64(_splitmix64(_splitmix64(int(seed) & _M64) ^ (int(step) & _M64)) ^ (int(site) & _M64))


def dropout_step_key(seed, step):
    """sm(sm(seed) ^ step): the 64-bit word of one step, all that the kernels' device-key form needs of (seed, step). Every site's
    key follows from it: dropout_key(seed, step, site) == sm(dropout_step_key(seed, step) ^ site)."""
    return _splitmix64(_splitmix64(int(seed) & _M64) ^ (int(step) & _M64))


class DeviceKey(object):
    """A site's key in the device form: `word` is a one-element int64 device tensor that holds dropout_step_key(seed, step) (the
    64 bits, two's complement) at the time the kernel RUNS, `site` the site id. dropout_apply / dropout_apply_pair / dropout_mask
    take one wherever they take an integer key and then launch the _dev entry points, whose lanes form sm(word ^ site)."""
    __slots__ = ('word', 'site')

    def __init__(self, word, site):
        if not torch.is_tensor(word) or word.dtype != torch.int64 or word.numel() != 1 or not word.is_cuda:
            raise NativeError('DeviceKey: the step word must be a one-element int64 tensor on a GPU')
        self.word, self.site = word, int(site) & _M64


def dropout_layer_site(li, which):
    """Site id of layer `li`: which = 0 (in), 1 (out), 2 (gcn_drop)."""
    return 4 * int(li) + int(which)


def dropout_threshold(p):
    """T = min(2^32 - 1, floor((1 - p) * 2^32)) in Python doubles: an element is kept iff its 32-bit word is below T."""
    return max(0, min((1 << 32) - 1, int(math.floor((1.0 - float(p)) * 4294967296.0))))


def dropout_scale(p):
    """(threshold, inv_keep) of a site with 0 < p: p >= 1 keeps nothing (T = 0) and scales by 0, as F.dropout(p=1) gives zeros."""
    return (0, 0.0) if p >= 1 else (dropout_threshold(p), 1.0 / (1.0 - p))


def dropout_supported(*tensors):
    """f32 GPU matrices (1-D or 2-D, last dimension contiguous, rows at least cols apart) the dropout kernels take."""
    for t in tensors:
        if t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() not in (1, 2) or t.numel() == 0:
            return False
        if t.size(-1) >= (1 << 31) or (t.size(-1) > 1 and t.stride(-1) != 1) or (t.dim() == 2 and t.size(0) > 1 and t.stride(0) < t.size(1)):
            return False
    return True


def _drop_block(t, what):
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.size(0) > 1 and t.stride(0) < t.size(1)):
        raise NativeError('%s: a matrix [rows, cols] with rows at least cols apart is required, got %s strides %s'
                          % (what, tuple(t.shape), t.stride()))
    return (1, t.size(0)) if t.dim() == 1 else (t.size(0), t.size(1))


def dropout_apply(x, key, row0, p, out=None):
    """(12) Dropout of x [rows, cols] under `key` with global first row `row0`; `out`: the tensor to write (x itself = in place;
    None = a fresh one). p in (0, 1]; p >= 1 gives zeros."""
    rows, cols = _drop_block(x, 'dropout_apply')
    if out is None:
        out = torch.empty((rows, cols) if x.dim() == 2 else (cols,), dtype=torch.float32, device=x.device)
    _same_device(x, out)
    if _drop_block(out, 'dropout_apply') != (rows, cols):
        raise NativeError('dropout_apply: out %s does not match x %s' % (tuple(out.shape), tuple(x.shape)))
    if rows == 0 or cols == 0:
        return out
    thr, inv_keep = dropout_scale(p)
    if isinstance(key, DeviceKey):
        _same_device(x, key.word)
        _check(lib().mgcn_dropout_apply_dev(rows, cols, _dev(x, torch.float32, 'x'), _ld(x), _dev(out, torch.float32, 'out'), _ld(out),
                                            key.word.data_ptr(), key.site, int(row0) & _M64, thr, inv_keep, _stream(x)),
               'mgcn_dropout_apply_dev')
        return out
    _check(lib().mgcn_dropout_apply(rows, cols, _dev(x, torch.float32, 'x'), _ld(x), _dev(out, torch.float32, 'out'), _ld(out),
                                    int(key) & _M64, int(row0) & _M64, thr, inv_keep, _stream(x)), 'mgcn_dropout_apply')
    return out


def dropout_apply_pair(xa, key_a, xb, key_b, row0, p, out_a=None, out_b=None):
    """(12) Two sites over one block in one launch (the layer's in / out pair). xa and xb may be one tensor; an output may be its
    input (in place); None = a fresh tensor. Returns (out_a, out_b)."""
    rows, cols = _drop_block(xa, 'dropout_apply_pair')
    new = lambda: torch.empty((rows, cols), dtype=torch.float32, device=xa.device)
    out_a, out_b = new() if out_a is None else out_a, new() if out_b is None else out_b
    _same_device(xa, xb, out_a, out_b)
    if any(t.dim() != 2 or _drop_block(t, 'dropout_apply_pair') != (rows, cols) for t in (xa, xb, out_a, out_b)):
        raise NativeError('dropout_apply_pair: the four matrices must be [%d, %d]' % (rows, cols))
    if rows == 0 or cols == 0:
        return out_a, out_b
    thr, inv_keep = dropout_scale(p)
    if isinstance(key_a, DeviceKey) or isinstance(key_b, DeviceKey):
        if not (isinstance(key_a, DeviceKey) and isinstance(key_b, DeviceKey)) or key_a.word.data_ptr() != key_b.word.data_ptr():
            raise NativeError('dropout_apply_pair: the two sites of a pair share one device step word')
        _same_device(xa, key_a.word)
        _check(lib().mgcn_dropout_apply_pair_dev(
            rows, cols, _dev(xa, torch.float32, 'x_a'), _ld(xa), _dev(out_a, torch.float32, 'out_a'), _ld(out_a), key_a.site,
            _dev(xb, torch.float32, 'x_b'), _ld(xb), _dev(out_b, torch.float32, 'out_b'), _ld(out_b), key_b.site,
            key_a.word.data_ptr(), int(row0) & _M64, thr, inv_keep, _stream(xa)), 'mgcn_dropout_apply_pair_dev')
        return out_a, out_b
    _check(lib().mgcn_dropout_apply_pair(
        rows, cols, _dev(xa, torch.float32, 'x_a'), _ld(xa), _dev(out_a, torch.float32, 'out_a'), _ld(out_a), int(key_a) & _M64,
        _dev(xb, torch.float32, 'x_b'), _ld(xb), _dev(out_b, torch.float32, 'out_b'), _ld(out_b), int(key_b) & _M64,
        int(row0) & _M64, thr, inv_keep, _stream(xa)), 'mgcn_dropout_apply_pair')
    return out_a, out_b


def dropout_mask(rows, cols, key, row0, p, device=None, out=None):
    """(12) The bool keep-mask [rows, cols] of a site: what (9) and (11) take in place of a bernoulli_ draw. `out`: a bool or uint8
    matrix to write (may be a padded view)."""
    if out is None:
        out = torch.empty((int(rows), int(cols)), dtype=torch.bool, device=device)
    if out.dtype not in (torch.bool, torch.uint8) or out.dim() != 2 or tuple(out.shape) != (int(rows), int(cols)):
        raise NativeError('dropout_mask: out must be a bool / uint8 [%d, %d]' % (rows, cols))
    _drop_block(out, 'dropout_mask')
    if out.numel() == 0:
        return out
    if isinstance(key, DeviceKey):
        _same_device(out, key.word)
        _check(lib().mgcn_dropout_mask_dev(int(rows), int(cols), _dev(out, out.dtype, 'mask'), _ld(out), key.word.data_ptr(), key.site,
                                           int(row0) & _M64, dropout_scale(p)[0], _stream(out)), 'mgcn_dropout_mask_dev')
        return out
    _check(lib().mgcn_dropout_mask(int(rows), int(cols), _dev(out, out.dtype, 'mask'), _ld(out), int(key) & _M64, int(row0) & _M64,
                                   dropout_scale(p)[0], _stream(out)), 'mgcn_dropout_mask')
    return out


def dropout_mask_host(rows, cols, key, row0, p):
    """(12) dropout_mask on the CPU (uint8 host tensor), from the same inline function the kernels call: test infrastructure."""
    out = torch.empty((int(rows), int(cols)), dtype=torch.uint8)
    if out.numel() == 0:
        return out
    _check(lib().mgcn_dropout_mask_host(int(rows), int(cols), out.data_ptr(), int(cols),
                                        int(key) & _M64, int(row0) & _M64, dropout_scale(p)[0]), 'mgcn_dropout_mask_host')
    return out


# ------------------------------------------------------------------------------------------------
# (19) edge dropout and own-triple removal: this step's slot records (csrc/dropout.hip)
EDGE_DROP_SITE = 0x3000


def edge_drop_threshold(p):
    """The threshold of the edge site: T(p) of the dropout sites for p < 1 (p <= 0 included: T(0) = 2^32 - 1), 0 for p >= 1."""
    return 0 if p >= 1 else dropout_threshold(max(float(p), 0.0))


def edge_drop_table_host(length):
    """(19) T[d] = deg^-1/2 as the feeder forms it, d = 0 .. length - 1: a host f32 tensor."""
    out = torch.empty(int(length), dtype=torch.float32)
    _check(lib().mgcn_edge_drop_table_host(int(length), out.data_ptr()), 'mgcn_edge_drop_table_host')
    return out


def max_run_host(rowptr, hubinfo, chunks, num_chunks):
    """The longest destination run of a layout (host tensors of csr_build_host), hub segments included."""
    longest = int((rowptr[:, 1:] - rowptr[:, :-1]).max()) if rowptr.size(1) > 1 else 0
    if num_chunks:
        first, cnt = hubinfo[:, :, 0].reshape(-1).long(), hubinfo[:, :, 1].reshape(-1).long()
        hub = cnt > 0
        if bool(hub.any()):
            seg = chunks[(first + cnt - 1)[hub], 1] - chunks[first[hub], 0]
            longest = max(longest, int(seg.max()))
    return longest


def _refuse_edge_drop_graph(csr, what):
    if not csr.has_backward:
        raise NativeError('%s: graph was prepared without the backward indices' % what)
    if not csr.mirrored:
        raise NativeError('%s: the edge list is not mirror-symmetric (edge e + E is not the reverse of edge e), so an edge and its '
                          'reverse cannot be dropped together and the degrees of the kept graph do not follow from the destination runs'
                          % what)


def edge_drop_records(csr, state, key, p, forced=None, out=None):
    """(19) rec' [2E, 4] int32 of `csr` under `key` (an int, or a DeviceKey: the _dev entry point) and drop probability `p`, with
    the undirected edges marked in `forced` [E] uint8 (None: none) removed as well. `state` is csr.edge_drop_state(). p <= 0
    without `forced`: nothing is launched and csr.rec itself is returned. `out`: the tensor to write (None: a fresh one)."""
    what = 'edge_drop_records'
    _refuse_edge_drop_graph(csr, what)
    if p <= 0 and forced is None:
        return csr.rec
    N, E = csr.num_nodes, csr.num_edges_half
    if out is None:
        out = torch.empty_like(csr.rec)
    if out.dtype != torch.int32 or tuple(out.shape) != tuple(csr.rec.shape) or not out.is_contiguous() or out.data_ptr() == csr.rec.data_ptr():
        raise NativeError('%s: out must be a contiguous int32 %s that is not csr.rec' % (what, tuple(csr.rec.shape)))
    if forced is not None and (forced.dtype != torch.uint8 or forced.numel() != E or not forced.is_contiguous()):
        raise NativeError('%s: forced must be a contiguous uint8 [%d]' % (what, E))
    _same_device(csr.rec, state.table, state.cinv, forced, out)
    hubs = csr.num_chunks > 0
    head = (N, E, _dev(csr.rowptr, torch.int32, 'rowptr'), _dev(csr.rec, torch.int32, 'rec'), _dev(csr.slot_dst, torch.int32, 'slot_dst'),
            _dev(csr.hubinfo, torch.int32, 'hubinfo') if hubs else None, _dev(csr.chunks, torch.int32, 'chunks') if hubs else None,
            csr.num_chunks, _dev(state.table, torch.float32, 'table'), state.table.numel(), state.max_run,
            _dev(forced, torch.uint8, 'forced', True))
    tail = (edge_drop_threshold(p), _dev(state.cinv, torch.float32, 'cinv'), _dev(out, torch.int32, 'rec_out'), _stream(out))
    if isinstance(key, DeviceKey):
        _same_device(out, key.word)
        _check(lib().mgcn_edge_drop_records_dev(*(head + (key.word.data_ptr(), key.site) + tail)), 'mgcn_edge_drop_records_dev')
    else:
        _check(lib().mgcn_edge_drop_records(*(head + (int(key) & _M64,) + tail)), 'mgcn_edge_drop_records')
    return out


def edge_drop_records_host(host, table, key, p, forced=None):
    """(19) on the CPU from the same inline functions: `host` is csr_build_host's dict (with the backward index), `table` a host
    f32 tensor, `forced` a host uint8 [E] or None. Returns (rec' [2E, 4] int32, cinv [2, N] f32). Test infrastructure."""
    rowptr, rec = host['rowptr'], host['rec']
    N, E = rowptr.size(1) - 1, rec.size(0) // 2
    out, cinv = torch.empty_like(rec), torch.empty((2, max(N, 1)), dtype=torch.float32)
    nch = int(host['num_chunks'])
    if forced is not None and (forced.dtype != torch.uint8 or forced.numel() != E or forced.is_cuda or not forced.is_contiguous()):
        raise NativeError('edge_drop_records_host: forced must be a contiguous host uint8 [%d]' % E)
    _check(lib().mgcn_edge_drop_records_host(
        N, E, rowptr.data_ptr(), rec.data_ptr(), host['slot_dst'].data_ptr(), host['hubinfo'].data_ptr() if nch else None,
        host['chunks'].data_ptr() if nch else None, nch, table.data_ptr(), table.numel(), None if forced is None else forced.data_ptr(),
        int(key) & _M64, edge_drop_threshold(p), cinv.data_ptr(), out.data_ptr()), 'mgcn_edge_drop_records_host')
    return out, cinv[:, :N]


def edge_flags_from_queries(qkey, state, num_edges_half, out=None):
    """(19) forced [E] uint8: 1 for every undirected edge one of whose directions (src, type) is a query of `qkey` [B] int64
    (src * 2R + type, FilterIndex.query_keys), 0 elsewhere. `out` (None: state.forced) is zero-filled first."""
    out = state.forced if out is None else out
    E = int(num_edges_half)
    if out.dtype != torch.uint8 or out.numel() != E or not out.is_contiguous():
        raise NativeError('edge_flags_from_queries: out must be a contiguous uint8 [%d]' % E)
    if state.ekeys.numel() != 2 * E or state.eund.numel() != 2 * E:
        raise NativeError('edge_flags_from_queries: ekeys / eund must hold %d entries' % (2 * E))
    qkey = qkey.reshape(-1).contiguous()
    _same_device(qkey, state.ekeys, state.eund, out)
    out.zero_()
    if qkey.numel() == 0 or E == 0:
        return out
    _check(lib().mgcn_edge_flags_from_queries(qkey.numel(), _dev(qkey, torch.int64, 'qkey'), E, _dev(state.ekeys, torch.int64, 'ekeys'),
                                              _dev(state.eund, torch.int32, 'eund'), _dev(out, torch.uint8, 'forced'), _stream(out)),
           'mgcn_edge_flags_from_queries')
    return out


# ------------------------------------------------------------------------------------------------
# (15) counter-drawn candidate lists (csrc/dropout.hip)
CAND_DRAW_SITE = 0x2000


def _cand_draw(fn, what, on_gpu, qkey, keys, ptr, tails, num_entities, n_cand, key, row0, labels, out, table=None):
    B, K = qkey.numel(), int(n_cand)
    dev = qkey.device
    if dev.type != ('cuda' if on_gpu else 'cpu'):
        raise NativeError('%s: the tensors must live on %s (got %s)' % (what, 'a GPU' if on_gpu else 'the CPU', dev))
    if qkey.dim() != 1 or ptr.numel() != keys.numel() + 1:
        raise NativeError('%s: qkey must be [B] and ptr must have len(keys) + 1 entries' % what)
    cand, label = out if isinstance(out, (tuple, list)) else (out, None)
    if cand is None:
        cand = torch.empty((B, max(K, 0)), dtype=torch.int64, device=dev)
    if label is None and labels:
        label = torch.empty((B, max(K, 0)), dtype=torch.uint8, device=dev)
    if not labels:
        label = None
    dev_key = isinstance(key, DeviceKey)
    if dev_key and not on_gpu:
        raise NativeError('%s: a DeviceKey is for the GPU launch' % what)
    _same_device(qkey, keys, ptr, tails, cand, label, key.word if dev_key else None, table)
    if table is not None and (table.dtype != torch.int64 or table.dim() != 1 or table.numel() != int(num_entities) or not table.is_contiguous()):
        raise NativeError('%s: table must be a contiguous int64 [%d] (sampling.NegativeSampler.table)' % (what, int(num_entities)))

    def block(t, dtype, name):
        if t.dim() != 2 or tuple(t.shape) != (B, K) or (t.dtype != dtype and not (dtype == torch.uint8 and t.dtype == torch.bool)) \
                or (K > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < K):
            raise NativeError('%s: %s must be %s (%d, %d) with unit column stride and rows that do not overlap, got %s %s strides %s'
                              % (what, name, dtype, B, K, t.dtype, tuple(t.shape), t.stride()))
        return t.data_ptr(), _ld(t)

    def arr(t, dtype, name):
        if t.dtype != dtype or (t.numel() > 1 and not t.is_contiguous()):
            raise NativeError('%s: %s must be a contiguous %s array' % (what, name, dtype))
        return t.data_ptr() if t.numel() else None

    cp, ldc = block(cand, torch.int64, 'cand') if K >= 1 else (cand.data_ptr(), 0)
    lp, ldl = (block(label, torch.uint8, 'label') if K >= 1 else (label.data_ptr(), 0)) if label is not None else (None, 0)
    args = [B, K, int(num_entities), arr(qkey, torch.int64, 'qkey') if B else qkey.new_zeros(1).data_ptr(), keys.numel(),
            arr(keys, torch.int64, 'keys'), arr(ptr, torch.int64, 'ptr'), arr(tails, torch.int32, 'tails'), tails.numel(),
            ] + ([table.data_ptr()] if table is not None else []) + ([key.word.data_ptr(), key.site] if dev_key else [int(key) & _M64]) + [int(row0) & _M64, cp, ldc, lp, ldl]
    _check(fn(*(args + ([_stream(cand)] if on_gpu else []))), what)
    return cand, label


def cand_draw(qkey, keys, ptr, tails, num_entities, n_cand, key, row0=0, labels=True, out=None, table=None):
    """(15) (cand [B, n_cand] int64, label [B, n_cand] uint8 or None): the candidate lists of the queries with keys qkey [B] under
    `key` (dropout_key(seed, step, CAND_DRAW_SITE); or a DeviceKey(word, CAND_DRAW_SITE), whose word on the tensors' device holds
    dropout_step_key(seed, step) when the kernel RUNS: mgcn_cand_draw_dev, what a captured launch needs), row b being global batch row row0 + b. Column 0 is one known tail of the query
    drawn from its run in the keys / ptr / tails arrays of filter_mask() (-1 for a query without one), the other columns are ids
    in [0, num_entities); label is cand_labels() of the drawn list against the whole table. One launch (see mgcn_cand_draw).
    out: a cand tensor, or (cand, label), to write into (padded row views are fine).
    table (None: the uniform draw above, unchanged): an alias table [num_entities] int64 on the tensors' device
    (sampling.NegativeSampler.table): (17), the negatives follow the table's distribution (mgcn_cand_draw_alias / _alias_dev);
    an alias outside the table is written as -1."""
    tag = '' if table is None else '_alias'
    if isinstance(key, DeviceKey):
        what = 'mgcn_cand_draw%s_dev' % tag
    else:
        what = 'mgcn_cand_draw%s' % tag
    return _cand_draw(getattr(lib(), what), what, True, qkey, keys, ptr, tails, num_entities, n_cand, key, row0, labels, out, table)


def cand_draw_host(qkey, keys, ptr, tails, num_entities, n_cand, key, row0=0, labels=True, out=None, table=None):
    """(15) / (17) cand_draw on CPU tensors, from the same inline function the kernel calls: test infrastructure."""
    what = 'mgcn_cand_draw_host' if table is None else 'mgcn_cand_draw_alias_host'
    return _cand_draw(getattr(lib(), what), what, False, qkey, keys, ptr, tails, num_entities, n_cand, key, row0, labels, out, table)


def alias_build_host(w):
    """(17) The alias table [N] int64 (alias << 32 | threshold) of the int64 weights w [N] in [0, 2^32), built on the CPU in exact
    integers (mgcn_alias_build_host). A host tensor; what sampling.NegativeSampler wraps."""
    w = w.detach().to('cpu', torch.int64).contiguous()
    if w.dim() != 1:
        raise NativeError('alias_build_host: w must be an int64 [N]')
    table = torch.empty(w.numel(), dtype=torch.int64)
    _check(lib().mgcn_alias_build_host(w.numel(), w.data_ptr() if w.numel() else None, table.data_ptr() if w.numel() else None),
           'mgcn_alias_build_host')
    return table


class IngestUnsupported(NativeError):
    """The native reader declined the files (non-ASCII names): use the Python reader."""


def ingest(train_path, valid_path, test_path):
    """(0) Native reader of the three split files. Returns (entity_names, relation_names, {split: [n, 3] int64 ids}):
    names in id order (first-seen over train, valid, test; lower-cased), ids as data_loader.py:84-86 assigns them.
    Raises ValueError / KeyError where the reference's reader does, IngestUnsupported for non-ASCII names."""
    handle = _ptr()
    rc = lib().mgcn_ingest_open(os.fsencode(train_path), os.fsencode(valid_path), os.fsencode(test_path),
                                ctypes.byref(handle))
    if rc != 0:
        msg = (lib().mgcn_last_error() or b'').decode('utf-8', 'replace')
        if rc == 3:
            raise IngestUnsupported(msg)
        if 'KeyError' in msg:
            raise KeyError(msg.split("'")[1] if "'" in msg else msg)
        if 'ValueError' in msg:
            raise ValueError(msg)
        if 'cannot open' in msg:
            raise FileNotFoundError(msg)
        raise NativeError('mgcn_ingest_open failed (%d): %s' % (rc, msg))
    try:
        names = []
        for kind in (0, 1):
            n, nbytes = lib().mgcn_ingest_count(handle, kind), lib().mgcn_ingest_names_bytes(handle, kind)
            buf = ctypes.create_string_buffer(max(int(nbytes), 1))
            offs = torch.empty(n + 1, dtype=torch.int64)
            _check(lib().mgcn_ingest_names(handle, kind, ctypes.cast(buf, _ptr), offs.data_ptr()), 'mgcn_ingest_names')
            raw, o = buf.raw, offs.tolist()
            names.append([raw[o[i]:o[i + 1]].decode('ascii') for i in range(n)])
        ids = {}
        for k, split in enumerate(('train', 'valid', 'test')):
            t = torch.empty((int(lib().mgcn_ingest_count(handle, 2 + k)), 3), dtype=torch.int64)
            _check(lib().mgcn_ingest_triples(handle, k, t.data_ptr() if t.numel() else None), 'mgcn_ingest_triples')
            ids[split] = t
        return names[0], names[1], ids
    finally:
        lib().mgcn_ingest_close(handle)


def filter_index_build(triples, num_relations):
    """Known-answer index of [n, 3] int64 id triples, both directions: (keys [K] int64, ptr [K+1] int64, tails int32),
    all host tensors (see mgcn_filter_index_build)."""
    t = triples.detach().to('cpu', torch.int64).contiguous().reshape(-1, 3)
    nk, nt = _i64(0), _i64(0)
    tp = t.data_ptr() if t.numel() else None
    _check(lib().mgcn_filter_index_build(t.size(0), tp, int(num_relations), None, None, None, ctypes.byref(nk),
                                         ctypes.byref(nt)), 'mgcn_filter_index_build')
    keys = torch.empty(nk.value, dtype=torch.int64)
    ptr = torch.empty(nk.value + 1, dtype=torch.int64)
    tails = torch.empty(nt.value, dtype=torch.int32)
    _check(lib().mgcn_filter_index_build(t.size(0), tp, int(num_relations), keys.data_ptr(), ptr.data_ptr(),
                                         tails.data_ptr() if nt.value else None, ctypes.byref(nk), ctypes.byref(nt)),
           'mgcn_filter_index_build')
    return keys, ptr, tails
