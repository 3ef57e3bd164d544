"""The fused fp32 conv layer (conv_x3.hip: rg_conv_proj_x3_for + rg_conv_layer_x3_for) under
both term schemes -- 'h2', the engine's default (two fp16 terms, three products, one
power-of-two scale per image) and 'b3' (three bf16 terms, six products) -- set through
engine.X3_TERMS.

Criteria.  f32-class: the layer's error against the oracle's conv block in float64 within T of
the float32 oracle's, rms and max (tests/test_chain_error_budget.py's error_ratios); T = T_CONV
of tests/test_gpu_chain_x3.py except where tests/test_conv_terms_emulation.py shows a mutant
below 3 T_CONV and sets its own (T_CASE).  Tile shapes: against the float32 oracle at FP32_TOL.
Every reference is computed once per module (_case).
"""
import json

import numpy as np
import pytest
import torch

from test_chain_error_budget import dense_inputs, error_ratios
from test_conv_terms_emulation import T_CASE, conv_model, oracle_conv
from test_gpu_chain_x3 import FP32_TOL, T_CONV
from test_gpu_f32 import _conv_plan, _graph, _x3_slabs

pytestmark = pytest.mark.gpu

terms_p = pytest.mark.parametrize('terms', ['h2', 'b3'])


@pytest.fixture(autouse=True)
def _x3(monkeypatch):
    from graph_neural_network_for_radar_perception_amd import engine
    monkeypatch.setattr(engine, 'F32_ARITH', 'x3')


def _set(monkeypatch, terms):
    from graph_neural_network_for_radar_perception_amd import engine
    monkeypatch.setattr(engine, 'X3_TERMS', terms)


def _scheme_used(cv, terms):
    """The plan's images are those of `terms` (no test here passes on the other scheme)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    flag = nat.RG_PACK_H2 if terms == 'h2' else nat.RG_PACK_X3
    assert all(f & flag for f in cv.fused_fmts) and cv.fused_ok
    assert all(bool(d.flags & nat.RG_LAYER_H2) == (terms == 'h2') for d in cv._layers())


_CASES = {}


def _case(dev, aggr, scaling, blocks=1):
    """Model, batched kNN graph [700, 1, 33, 1500, 64] (k = 10), dense inputs and the float64 /
    float32 oracle outputs of `blocks` conv blocks -- built once."""
    key = (aggr, scaling, blocks)
    if key not in _CASES:
        m, cfg = conv_model(aggr, scaling, blocks, dev)
        batch, gb = _graph(dev, [700, 1, 33, 1500, 64], 10, 90, cfg)
        g, N, E = gb.graph, batch.n_nodes, int(gb.n_edges_dev.item())
        x = dense_inputs(N, 64, 1).to(dev)
        e = dense_inputs(gb.capacity, 64, 2).to(dev)
        # the h2 residues of values below 0.125 are fp16 subnormals
        assert bool((x.abs() < 0.125).any()) and bool((e[:E].abs() < 0.125).any())
        ei = torch.stack((g.src[:E], g.dst[:E])).long().cpu()
        ref = {dt: oracle_conv(m, cfg, x, e[:E], ei, dt, blocks)
               for dt in (torch.float64, torch.float32)}
        _CASES[key] = (m, cfg, g, N, E, x, e, ref)
    return _CASES[key]


def _f32_class(out, ref, T, **rec):
    rms, mx = error_ratios(out.cpu(), ref[torch.float32], ref[torch.float64])
    print(json.dumps(dict(rec, rms_ratio=round(rms, 4), max_ratio=round(mx, 4), T=T)))
    assert rms <= T and mx <= T, (rms, mx)


@terms_p
@pytest.mark.parametrize('aggr,scaling', [('add', 'equal'), ('mean', 'equal'),
                                          ('add', 'x_down_e_up'), ('add', 'x_up_e_down')])
def test_conv_layer_f32_class(cuda_device, monkeypatch, terms, aggr, scaling):
    """One layer at f32-class error, 'add' and 'mean'; and with msg0's x columns times 2^-9 and
    its edge columns times 2^7 (and the reverse), so that under h2 the scale of the P | Q image
    and of the W_e image differ by many powers of two: the P | Q rows must reach the edge
    launch in W_e's units."""
    _set(monkeypatch, terms)
    m, cfg, g, N, E, x, e, ref = _case(cuda_device, aggr, scaling)
    cv = _conv_plan(m, 'x3')
    out = torch.full((N, 64), float('nan'), device=cuda_device)
    assert cv.run_fused(x, e, g, out)
    _scheme_used(cv, terms)
    if terms == 'h2' and scaling != 'equal':
        from graph_neural_network_for_radar_perception_amd import engine
        W = m.pred.pass_messages.conv_blk[0].msg[0].block[0].weight.detach().float()
        Wc = W - W.mean(0, keepdim=True)
        s_pq = engine.h2_scale_exp(float(Wc[:, :128].abs().max()))
        s_e = engine.h2_scale_exp(float(Wc[:, 128:].abs().max()))
        assert abs(s_pq - s_e) >= 12, (s_pq, s_e)
    assert T_CASE[scaling] <= T_CONV
    _f32_class(out, ref, T_CASE[scaling], test='conv_layer_f32_class', terms=terms, aggr=aggr,
               scaling=scaling)


@terms_p
def test_two_stacked_layers(cuda_device, monkeypatch, terms):
    """Layer 0's node launch writes layer 1's P | Q from its registers (under h2 in the units of
    layer 1's W_e image); the other route runs layer 1 alone on layer 0's output, its P | Q from
    rg_conv_proj_x3_for.  Both routes f32-class against the float64 oracle of the two blocks.
    Not bit-identical to each other, under 'b3' in the parent build either: the register route
    reads W_pq as a FAST_CHAIN image and the projection launch as a FAST_IN one, whose k-steps
    hold the 64 inputs in different orders (measured: profiles/conv_h2_b3_identity.json)."""
    _set(monkeypatch, terms)
    dev = cuda_device
    m, cfg, g, N, E, x, e, ref = _case(dev, 'add', 'equal', 2)
    cv0, cv1 = _conv_plan(m, 'x3', 0), _conv_plan(m, 'x3', 1)
    pq0 = torch.empty((N, 256), device=dev)
    pq1 = torch.full((N, 256), float('nan'), device=dev)
    x1 = torch.full((N, 64), float('nan'), device=dev)
    x2 = torch.full((N, 64), float('nan'), device=dev)
    assert cv0.project_x3(x, pq0)
    assert cv0.run_x3(x, e, g, x1, pq0, cv1, pq1)
    assert cv1.run_x3(x1, e, g, x2, pq1)
    _scheme_used(cv1, terms)
    x2b = torch.full((N, 64), float('nan'), device=dev)
    assert cv1.run_fused(x1, e, g, x2b)
    print(json.dumps(dict(test='two_stacked_layers', terms=terms,
                          routes_bit_identical=bool(torch.equal(x2, x2b)))))
    _f32_class(x2, ref, T_CONV, test='two_stacked_layers', terms=terms, route='registers')
    _f32_class(x2b, ref, T_CONV, test='two_stacked_layers', terms=terms, route='projection')


def _long_segment_graph(dev):
    """300 nodes; node 7 has in-degree 130 (its running sum crosses four 32-edge tiles), every
    other node three incoming edges."""
    from graph_neural_network_for_radar_perception_amd import engine
    N = 300
    gen = torch.Generator(device='cpu').manual_seed(21)
    dst = torch.cat((torch.full((130,), 7), torch.arange(N).repeat_interleave(3)))
    src = (dst + 1 + torch.randint(0, N - 1, dst.shape, generator=gen)) % N
    ei = torch.stack((src, dst)).to(dev)
    g = engine.DeviceGraph.from_edge_index(ei, N)
    seg = g.seg_ptr.cpu()
    assert int(seg[8] - seg[7]) >= 100
    return g, N, ei.shape[1]


@terms_p
@pytest.mark.parametrize('shape', ['slow_path', 'long_segment', 'ragged_end', 'tiny'])
def test_edge_launch_tile_shapes(cuda_device, monkeypatch, terms, shape):
    """Where the one-wave edge launch can go wrong: tiles with more than four new destinations
    (k = 2: the P rows' slow path), a running sum across four tiles, a partial last tile, and
    waves without tiles -- against the float32 oracle at FP32_TOL."""
    from oracle import gnn_forward_ref
    _set(monkeypatch, terms)
    dev = cuda_device
    m, cfg = conv_model('add', 'equal', 1, dev)
    if shape == 'long_segment':
        g, N, E = _long_segment_graph(dev)
        cap = E
    else:
        sizes, k = {'slow_path': ([300, 47], 2), 'ragged_end': ([33, 64], 10), 'tiny': ([3], 10)}[shape]
        batch, gb = _graph(dev, sizes, k, 93, cfg)
        g, N, E, cap = gb.graph, batch.n_nodes, int(gb.n_edges_dev.item()), gb.capacity
    seg = g.seg_ptr.cpu().numpy()
    if shape == 'slow_path':     # some tile of 32 edges starts more than four destinations
        assert max(np.searchsorted(seg, t + 32, 'left') - np.searchsorted(seg, t, 'right')
                   for t in range(0, E - 32, 32)) > 4
    if shape == 'ragged_end':
        assert E % 32 != 0 and E > 64
    x = dense_inputs(N, 64, 5).to(dev)
    e = dense_inputs(cap, 64, 6).to(dev)
    cv = _conv_plan(m, 'x3')
    out = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out)
    _scheme_used(cv, terms)
    sd = {k_: v.float().cpu() for k_, v in m.state_dict().items()}
    ei = torch.stack((g.src[:E], g.dst[:E])).long().cpu()
    with torch.no_grad():
        ref = gnn_forward_ref.conv_block(gnn_forward_ref._Ctx(sd, cfg), 'pass_messages.conv_blk.0',
                                         x.cpu(), e[:E].cpu(), ei)
    torch.testing.assert_close(out.cpu(), ref, **FP32_TOL)


def test_b3_slabs_and_wave_table_bit_identical(cuda_device, monkeypatch):
    """Under 'b3' (the existing tests of tests/test_gpu_f32.py now run 'h2'), at the smallest
    size with more than one slab: the launch over the graph's table, the launch that builds the
    table into its workspace, and the launch over one contiguous range per wave (pieces
    1 .. S - 1 empty) give the same bits."""
    from graph_neural_network_for_radar_perception_amd import engine
    _set(monkeypatch, 'b3')
    dev = cuda_device
    m, cfg = conv_model('add', 'equal', 1, dev)
    batch, gb = _graph(dev, [3000] * 24, 10, 92, cfg)
    g, N = gb.graph, batch.n_nodes
    S = _x3_slabs(N)
    assert S > 1
    G = min(max((N // 128 + 7) // 8 * 8, 8), 256)
    WX = G // 8 * 4
    W = 8 * WX
    gen = torch.Generator(device='cpu').manual_seed(5)
    x = (torch.randn(N, 64, generator=gen) * 1.5).to(dev)
    e = (torch.randn(gb.capacity, 64, generator=gen) * 1.5).to(dev)
    cv = _conv_plan(m, 'x3')
    out_s = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_s)
    _scheme_used(cv, 'b3')
    assert bool(torch.isfinite(out_s).all())
    tbl = g.conv_x3_blocks()
    seg = g.seg_ptr.cpu().numpy().astype(np.int64)
    E = int(seg[N])
    one = np.searchsorted(seg, (E * np.arange(W + 1)) // W, side='left')
    one[W] = N
    t2 = np.empty(W * S + 1, np.int32)
    for xcd in range(8):
        for k in range(S):
            for j in range(WX):
                t2[(xcd * S + k) * WX + j] = one[xcd * WX + j] if k == 0 else one[(xcd + 1) * WX]
    t2[W * S] = N
    g._conv_x3_blocks = torch.from_numpy(t2).to(dev)
    out_c = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_c)
    g._conv_x3_blocks = tbl
    assert torch.equal(out_s, out_c)
    monkeypatch.setattr(engine, 'CONV_X3_TABLE', False)
    g2 = engine.DeviceGraph(g.n_nodes, g.n_edges_cap, g.seg_ptr, g.dst, g.src, g.perm,
                            g.pair_src, g.pair_dst, g.n_pairs_dev)
    assert g2.conv_x3_blocks() is None
    out_p = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g2, out_p)
    assert torch.equal(out_s, out_p)


def test_h2_domain(cuda_device, monkeypatch):
    """One x value of 1e6 (past the h2 domain, |a| < 2^15): under 'h2' that node's output row is
    non-finite and every other row has the bits of the run without it; under 'b3' the same
    input is finite and within FP32_TOL of the oracle.  The node is the graph's last and only a
    destination: its P row enters the edge launch (messages to it), its Q row no message, and
    no destination follows it in its wave's range -- a non-finite running sum is carried into
    the destinations after it in the same range (non-finite, never finite and wrong; so does a
    non-finite input under 'b3')."""
    from oracle import gnn_forward_ref
    from graph_neural_network_for_radar_perception_amd import engine
    dev = cuda_device
    m, cfg = conv_model('add', 'equal', 1, dev)
    N = 200
    gen = torch.Generator(device='cpu').manual_seed(22)
    dst = torch.arange(N).repeat_interleave(5)
    src = (dst + 1 + torch.randint(0, N - 2, dst.shape, generator=gen)) % (N - 1)   # never N - 1
    src = torch.where(src == dst, (src + 1) % (N - 1), src)
    assert bool((src != N - 1).all())
    ei = torch.stack((src, dst)).to(dev)
    g = engine.DeviceGraph.from_edge_index(ei, N)
    E = ei.shape[1]
    x = dense_inputs(N, 64, 7).to(dev)
    e = dense_inputs(E, 64, 8).to(dev)
    xb = x.clone()
    xb[N - 1, 17] = 1e6
    outs = {}
    for terms in ('h2', 'b3'):
        _set(monkeypatch, terms)
        cv = _conv_plan(m, 'x3')
        for name, xin in (('in', x), ('past', xb)):
            o = torch.full((N, 64), float('nan'), device=dev)
            assert cv.run_fused(xin, e, g, o)
            outs[terms, name] = o
        _scheme_used(cv, terms)
    assert bool(torch.isfinite(outs['h2', 'in']).all())
    assert not bool(torch.isfinite(outs['h2', 'past'][N - 1]).any())
    assert torch.equal(outs['h2', 'past'][:N - 1], outs['h2', 'in'][:N - 1])
    assert bool(torch.isfinite(outs['b3', 'past']).all())
    sd = {k_: v.float().cpu() for k_, v in m.state_dict().items()}
    eic = torch.stack((g.src[:E], g.dst[:E])).long().cpu()
    with torch.no_grad():
        ref = gnn_forward_ref.conv_block(gnn_forward_ref._Ctx(sd, cfg), 'pass_messages.conv_blk.0',
                                         xb.cpu(), e.cpu(), eic)
    torch.testing.assert_close(outs['b3', 'past'].cpu(), ref, **FP32_TOL)
