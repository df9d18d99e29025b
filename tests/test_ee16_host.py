"""The bf16 per-edge table (include/mgcn_hip.h (2e)) without a GPU: the widening the kernels apply is torch's own
bf16 -> f32 conversion, the model switch builds bf16 tables without gradients that load and save like the f32 ones, the three
entry points are declared and exported, and everything that would train such a model refuses before it touches a device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from .conftest import ROOT
from .live_graphs import edge_list, random_halves


def _params(**kw):
    base = dict(gcn_in_dim=8, gcn_out_dim=12, gcn_drop=0.0, hidden_drop=0.0, feat_drop=0.0, k_w=3, k_h=4, num_filter=2,
                kernel_size=3, bias=False, lbl_smooth=0.1, gcn_layers=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _widen(h):
    """The definition: the f32 whose bit pattern is uint32(h) << 16, h the bf16's 16 bits."""
    bits = h.view(torch.int16).numpy().view(np.uint16).astype(np.uint32) << 16
    return torch.from_numpy(bits.view(np.float32).copy())


def test_widen_is_torch_bf16_to_float():
    vals = [0.0, -0.0, 1.0, -1.0, 2.0 ** 120, -2.0 ** 120, 2.0 ** -126, 2.0 ** -133, -2.0 ** -130, 3.0 * 2.0 ** -133,   # denormals
            1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20,  # ties
            -(1.0 + 2.0 ** -8), 0.1, -0.3, 3.3895313892515355e38, 65504.0, 1e-40, float('inf'), float('-inf')]
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.tensor(vals, dtype=torch.float32), torch.randn(4096, generator=g),
                   torch.randn(4096, generator=g) * 1e-38, torch.randn(4096, generator=g) * 1e30])
    h = v.to(torch.bfloat16)
    assert torch.equal(_widen(h).view(torch.int32), h.float().view(torch.int32))               # bit for bit, signs of zero too
    # round to nearest even: the ties of the grid go to the even neighbour
    assert float(torch.tensor(1.0 + 2.0 ** -8).to(torch.bfloat16)) == 1.0
    assert float(torch.tensor(1.0 + 3 * 2.0 ** -8).to(torch.bfloat16)) == 1.0 + 2.0 ** -6
    assert float(torch.tensor(1.0 + 2.0 ** -8 + 2.0 ** -20).to(torch.bfloat16)) == 1.0 + 2.0 ** -7
    # the lanes of an 8-byte load: element 0 is the low half of the first dword
    words = h[:4].view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
    lo, hi = words[0] | (words[1] << 16), words[2] | (words[3] << 16)
    lanes = np.array([lo << 16, lo & 0xffff0000, hi << 16, hi & 0xffff0000], dtype=np.uint32).view(np.float32)
    assert np.array_equal(lanes.view(np.uint32), h[:4].float().numpy().view(np.uint32))


def test_switch_builds_bf16_tables_without_gradients(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_EE', raising=False)
    torch.manual_seed(3)
    ref = pkg.MGCN(9, 2, 11, _params())
    torch.manual_seed(3)
    m = pkg.MGCN(9, 2, 11, _params(edge_table_dtype='bf16'))
    assert ref.edge_embeddings.dtype == torch.float32 and ref.edge_embeddings.requires_grad
    tables = [m.edge_embeddings] + list(m.edge_embeddings_extra)
    assert len(tables) == 2
    for t, r in zip(tables, [ref.edge_embeddings] + list(ref.edge_embeddings_extra)):
        assert isinstance(t, torch.nn.Parameter) and t.dtype == torch.bfloat16 and not t.requires_grad
        assert torch.equal(t.data, r.data.to(torch.bfloat16))                                  # the same draws, rounded
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    for (k, a), (_, b) in zip(m.named_parameters(), ref.named_parameters()):                   # seeding of the rest is unchanged
        if 'edge_embeddings' not in k:
            assert torch.equal(a, b), k
    # a sharded model's tables too
    ms = pkg.MGCN(9, 2, 11, _params(edge_table_dtype='bf16', edge_table_rows=5))
    assert ms.edge_embeddings.dtype == torch.bfloat16 and tuple(ms.edge_embeddings.shape) == (5, 8) and not ms.edge_embeddings.requires_grad
    # MGCN_EE overrides in both directions
    monkeypatch.setenv('MGCN_EE', 'bf16')
    assert pkg.MGCN(9, 2, 11, _params()).edge_embeddings.dtype == torch.bfloat16
    monkeypatch.setenv('MGCN_EE', 'f32')
    assert pkg.MGCN(9, 2, 11, _params(edge_table_dtype='bf16')).edge_embeddings.dtype == torch.float32
    monkeypatch.setenv('MGCN_EE', 'fp8')
    with pytest.raises(pkg._native.NativeError):
        pkg.MGCN(9, 2, 11, _params())


def test_f32_checkpoint_loads_rounded_and_round_trips_in_reference_order(pkg, monkeypatch):
    monkeypatch.delenv('MGCN_EE', raising=False)
    N, R = 12, 2
    ei, et = edge_list(*random_halves(N, R, 0.3, 4))
    E = ei.size(1) // 2
    torch.manual_seed(5)
    ref = pkg.MGCN(N, R, E, _params())
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    m = pkg.MGCN(N, R, E, _params(edge_table_dtype='bf16'))
    m.load_state_dict(sd)
    names = ['edge_embeddings', 'edge_embeddings_extra.0']
    for n in names:
        assert m.state_dict()[n].dtype == torch.bfloat16 and torch.equal(m.state_dict()[n], sd[n].to(torch.bfloat16))
    assert torch.equal(m.entity_embedding, ref.entity_embedding)
    # slot order in memory, reference order in the state dict (the hooks of the f32 model, on bf16 rows)
    csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, torch.device('cpu'), hub_threshold=4, hub_chunk=4)
    assert not torch.equal(csr.perm, torch.arange(2 * E))
    m._use_slot_order(csr)
    for n, p in m._edge_tables():
        assert p.dtype == torch.bfloat16 and not p.requires_grad
        assert torch.equal(p.data, sd[n].to(torch.bfloat16).index_select(0, csr.perm))
    out = m.state_dict()
    for n in names:
        assert out[n].dtype == torch.bfloat16 and torch.equal(out[n], sd[n].to(torch.bfloat16))
    # a bf16 state dict loads back unchanged and forgets the slot layout; an f32 one loaded over a slot layout is rounded
    m2 = pkg.MGCN(N, R, E, _params(edge_table_dtype='bf16'))
    m2.load_state_dict(out)
    assert all(torch.equal(m2.state_dict()[n], out[n]) for n in names)
    m.load_state_dict(sd)
    assert m._slot_csr is None and all(torch.equal(p.data, sd[n].to(torch.bfloat16)) for n, p in m._edge_tables())
    # and the bf16 state dict loads into an f32 model as the widened values
    ref.load_state_dict(out)
    assert ref.edge_embeddings.dtype == torch.float32 and torch.equal(ref.edge_embeddings.data, out[names[0]].float())


def test_entry_points_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, 'include', 'mgcn_hip.h')).read()
    handle = ctypes.CDLL(pkg._native.LIB_PATH)
    for name in ('mgcn_aggregate_fwd_ee16', 'mgcn_layer_fwd_fused_ee16', 'mgcn_layer_fwd_fused_live_ee16'):
        assert name in pkg._native.EXPORTS and name + '(' in header and hasattr(handle, name), name
    assert 'const uint16_t *ee_dev' in header
    assert pkg._native.ABI_VERSION == 4 and pkg._native.lib().mgcn_abi_version() == 4          # additive: the version stays
    # a null table is refused by argument validation, before anything is launched
    lib = pkg._native.lib()
    rc = lib.mgcn_aggregate_fwd_ee16(4, 2, 8, 3, None, None, None, 8, None, None, None, 1, None, None, 24, 0, 4, None, None, 0, 0,
                                     None, 0, 0, 0, None)
    assert rc == 1 and b'null per-edge table' in lib.mgcn_last_error()


def test_refusals_come_before_any_device_work(pkg, monkeypatch):
    """Everything here runs on CPU tensors: a refusal that came after a launch (or after the `must live on a GPU` check of
    the binding) would raise something else."""
    monkeypatch.delenv('MGCN_EE', raising=False)
    nat = pkg._native
    N, R = 12, 2
    ei, et = edge_list(*random_halves(N, R, 0.3, 4))
    E = ei.size(1) // 2
    csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, torch.device('cpu'))
    D = 8
    x, rel, g = torch.zeros(N, D), torch.zeros(2 * R + 1, D), torch.zeros(N, 2 * D)
    ee = torch.zeros(2 * E, D, dtype=torch.bfloat16)
    with pytest.raises(nat.NativeError, match='inference-only'):
        nat.aggregate_bwd(csr, x, rel, ee, g)
    with pytest.raises(nat.NativeError, match='inference-only'):
        nat.aggregate_bwd_shard(csr, x, rel, ee[:3], g[:2], (0, 2))
    with pytest.raises(nat.NativeError, match='must live on a GPU'):                            # the f32 table gets as far as the binding
        nat.aggregate_bwd(csr, x, rel, ee.float(), g, want_gx=False)

    graph = pkg.Graph(edge_index=ei.clone(), edge_attr=torch.stack((et, torch.arange(2 * E))))
    graph.entity, graph.num_nodes, graph.edge_norm = torch.arange(N), N, None
    m = pkg.MGCN(N, R, E, _params(edge_table_dtype='bf16'))
    src, r = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    m.train()
    with pytest.raises(nat.NativeError, match='inference-only'):
        m.encode(graph)
    with pytest.raises(nat.NativeError, match='inference-only'):
        m(src, r, graph)
    with pytest.raises(nat.NativeError, match='inference-only'):
        m.forward_loss(src, r, graph, None)
    assert m._slot_csr is None and getattr(graph, '_mgcn_facts', None) is None                  # nothing was laid out or looked at
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    step = pkg.captured.CapturedTrainStep(m, graph, None, opt)
    with pytest.raises(nat.NativeError, match='inference-only'):
        step(src, r)
    with pytest.raises(nat.NativeError, match='inference-only'):
        pkg.dist.train_step_sharded(m, graph, src, r, None, opt)
    assert m.training                                                                           # (the refusal did not switch modes)
    # the f32 model is not refused on these grounds: it fails later, for what a CPU model on this graph cannot do
    mf = pkg.MGCN(N, R, E, _params()).train()
    with pytest.raises(nat.NativeError) as err:
        mf.encode(graph)
    assert 'inference-only' not in str(err.value)


def test_shard_model_tables_rounds_f32_rows_into_the_bf16_shard(pkg, monkeypatch):
    """A model that holds nothing but its table shard (params.edge_table_rows): dist.shard_model_tables copies the source's f32
    rows into the bf16 shard in slot order, rounded to nearest even by copy_."""
    monkeypatch.delenv('MGCN_EE', raising=False)
    N, R = 12, 2
    ei, et = edge_list(*random_halves(N, R, 0.3, 4))
    E = ei.size(1) // 2
    csr = pkg.GraphCSR(N, 2 * R + 1, ei, et, torch.device('cpu'), hub_threshold=4, hub_chunk=4)
    g = torch.Generator().manual_seed(6)
    src = [torch.randn(2 * E, 8, generator=g), torch.randn(2 * E, 12, generator=g)]
    m = pkg.MGCN(N, R, E, _params(edge_table_dtype='bf16', edge_table_rows=2 * E))
    pkg.dist.shard_model_tables(m, csr, 0, N, lambda li, ids: src[li].index_select(0, ids))
    assert m._edge_shard[1:] == (0, N)
    for li, (_, t) in enumerate(m._edge_tables()):
        assert t.dtype == torch.bfloat16 and not t.requires_grad
        assert torch.equal(t.data, src[li].index_select(0, csr.perm).to(torch.bfloat16))
