"""GPU parity of the register-resident float32 kernels (the reference precision):
rg_mlp_chain_f32 (chain_f32.hip) and the fused float32 conv layer rg_conv_layer_f32
(conv_f32.hip), against the generic f32 chain kernel, a float64 torch evaluation of the
same weights and the oracle's residual_graph_conv_block (gnn_blocks.py:96-113).

Tolerances: f32 kernels vs float64 evaluation of the same f32 weights / inputs
|d| <= 1e-4 + 1e-4 |ref| (north_star's fp32 bound); fused vs unfused f32 conv layer
|d| <= 2e-5 + 2e-5 |ref| (same arithmetic up to summation order inside the GEMMs).
"""
import os

import numpy as np
import pytest
import torch

from oracle import gnn_forward_ref

pytestmark = pytest.mark.gpu

FP32_TOL = dict(rtol=1e-4, atol=1e-4)


def _torch_chain64(plan, x):
    """float64 evaluation of a ChainPlan's ffn_blocks (common.py:185-220)."""
    h = x.double()
    for s in plan.specs:
        h = torch.nn.functional.linear(h, s.weight.double(),
                                       None if s.bias is None else s.bias.double())
        if s.mu is not None:
            h = (h - h.mean(1, keepdim=True)) / (h.std(1, keepdim=True) + 1e-5) * s.std.double() \
                + s.mu.double()
        if s.act == 'leakyrelu':
            h = torch.nn.functional.leaky_relu(h, 0.01)
    return h


@pytest.mark.parametrize('arith', ['x3', 'mfma_f32'])
def test_f32_fast_chains_used_and_exact(cuda_device, arith, monkeypatch):
    """Every chain of the yml architecture in fp32 runs on its register-resident kernel --
    rg_mlp_chain_x3 (f32 products from split operands: the engine's default scheme, 'h2', two
    fp16 terms and three products; 'b3' is held to the same in test_gpu_chain_x3.py) or rg_mlp_chain_f32
    (v_mfma_f32_32x32x2_f32) -- and agrees with the generic f32 kernel and with a float64
    evaluation (1e-4)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd import engine
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    monkeypatch.setattr(engine, 'F32_ARITH', arith)
    used = 'x3_ok' if arith == 'x3' else 'fast_ok'
    dev = cuda_device
    torch.manual_seed(5)
    cfg = default_config()
    m = Model_Training(cfg, dev).to(dev).eval().requires_grad_(False)
    plans = m.pred.plans('fp32')
    g = torch.Generator(device='cpu').manual_seed(0)
    R = 3001   # not a multiple of 32: a partial last tile

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) * 2).to(dev)

    idx0 = torch.randint(0, R, (R,), generator=g).to(torch.int32).to(dev)
    idx1 = torch.randint(0, R, (R,), generator=g).to(torch.int32).to(dev)
    x64 = rnd(R, 64)
    cases = [
        (plans.node_enc, dict(in0=rnd(R, 6), w0=6)),
        (plans.edge_enc, dict(in0=rnd(R, 7), w0=7)),
        (plans.node_head, dict(in0=x64, w0=64)),
        (plans.offset_head, dict(in0=x64, w0=64)),
        (plans.link_node, dict(in0=x64, w0=64)),
        (plans.link_pair, dict(in0=x64, w0=64, mode=nat.IN_PAIRADD, idx0=idx0, idx1=idx1)),
        (plans.cls_stem, dict(in0=x64, w0=64)),
        (plans.cls_head, dict(in0=x64, w0=64)),
    ]
    for plan, kw in cases:
        outs = []
        for use_fast in (True, False):
            plan.use_fast = use_fast
            plan.fast_ok = {}
            plan.x3_ok = {}
            out = torch.full((R, plan.out_dim), float('nan'), device=dev)
            plan(R, out, **kw)
            outs.append(out)
            if use_fast:
                assert getattr(plan, used).get(kw.get('mode', nat.IN_DENSE)), \
                    f'{arith} chain kernel not used'
        plan.use_fast = True
        if kw.get('mode') == nat.IN_PAIRADD:
            xin = kw['in0'][idx0.long()] + kw['in0'][idx1.long()]
        else:
            xin = kw['in0']
        ref = _torch_chain64(plan, xin).float()
        assert torch.isfinite(outs[0]).all()
        torch.testing.assert_close(outs[0], ref, **FP32_TOL)
        torch.testing.assert_close(outs[0], outs[1], **FP32_TOL)


def test_f32_chain_rows_dev_and_empty(cuda_device):
    """rows_dev bounds the rows written (edge encoder over a capacity); rows = 0 is a no-op."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    torch.manual_seed(6)
    m = Model_Training(default_config(), dev).to(dev).eval().requires_grad_(False)
    plan = m.pred.plans('fp32').edge_enc
    x = torch.randn(500, 7, device=dev)
    out = torch.full((500, 64), 7.0, device=dev)
    n = torch.tensor([123], dtype=torch.int32, device=dev)
    plan(500, out, x, 7, rows_dev=n)
    assert plan.fast_ok.get(0) or plan.x3_ok.get(0)
    ref = _torch_chain64(plan, x[:123]).float()
    torch.testing.assert_close(out[:123], ref, **FP32_TOL)
    assert bool((out[123:] == 7.0).all())
    plan(0, out[:0], x[:0], 7)


@pytest.mark.parametrize('R', [1, 3001, 140_000])
def test_x3_encoders_rows(cuda_device, R):
    """The x3 encoders (chain_x3 under the engine's default scheme, 'h2': two-term fp16 splits,
    three products; both schemes per shape in test_gpu_chain_x3.py) over one row,
    a partial pass and several passes per workgroup: every sampled row at 1e-4 of a float64
    evaluation, deterministic across calls, and rows_dev bounds the rows written."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    torch.manual_seed(11)
    m = Model_Training(default_config(), dev).to(dev).eval().requires_grad_(False)
    plans = m.pred.plans('fp32')
    g = torch.Generator(device='cpu').manual_seed(R)
    for plan, w in ((plans.node_enc, 6), (plans.edge_enc, 7)):
        x = (torch.randn(R, w, generator=g) * 2).to(dev)
        outs = []
        for _ in range(2):
            out = torch.full((R, plan.out_dim), float('nan'), device=dev)
            plan(R, out, x, w)
            assert plan.x3_ok.get(0), 'x3 encoder not used'
            outs.append(out)
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1])
        sel = torch.arange(0, R, max(1, R // 4000), device=dev)
        torch.testing.assert_close(outs[0][sel], _torch_chain64(plan, x[sel]).float(), **FP32_TOL)
        if R > 1:
            n = torch.tensor([R // 2 + 5], dtype=torch.int32, device=dev)
            out = torch.full((R, plan.out_dim), 7.0, device=dev)
            plan(R, out, x, w, rows_dev=n)
            assert torch.equal(out[:R // 2 + 5], outs[0][:R // 2 + 5])
            assert bool((out[R // 2 + 5:] == 7.0).all())


def _graph(dev, sizes, k, seed0, cfg):
    from graph_neural_network_for_radar_perception_amd import synthetic
    from graph_neural_network_for_radar_perception_amd import graph_features as gf
    frames = [synthetic.make_frame(n, seed0 + i) for i, n in enumerate(sizes)]
    batch = gf.FrameBatch.from_frames(frames, device=dev)
    return batch, gf.build_graph_batch(batch, cfg, k=k)


def _conv_plan(m, arith, li=0):
    """A fresh fp32 ConvPlan of block li with the given f32 arithmetic ('x3' | 'mfma_f32')."""
    from graph_neural_network_for_radar_perception_amd import engine
    old = engine.F32_ARITH
    engine.F32_ARITH = arith
    try:
        cv = engine.ConvPlan(m.pred.pass_messages.conv_blk[li], 'fp32', next(m.parameters()).device)
    finally:
        engine.F32_ARITH = old
    assert cv.f32_arith == arith
    return cv


@pytest.mark.parametrize('arith', ['x3', 'mfma_f32'])
@pytest.mark.parametrize('aggr', ['add', 'mean'])
def test_f32_fused_conv_matches_unfused_and_oracle(cuda_device, aggr, arith):
    """The fused float32 conv layer -- rg_conv_layer_x3 (f32 products from exact three-term
    bf16 splits, one launch) and rg_conv_layer_f32 (v_mfma_f32_32x32x2_f32, two launches) --
    against the unfused f32 path (generic chain + rg_segment_reduce + chain) and the
    oracle's residual_graph_conv_block, on a batched kNN graph with an isolated-size frame
    (N = 1: no edges) and frames whose nodes straddle work blocks."""
    from graph_neural_network_for_radar_perception_amd import engine
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    cfg = default_config(graph_convolution_stem_channels=[64], aggregation=aggr,
                         k_number_nearest_points=10)
    torch.manual_seed(12)
    m = Model_Training(cfg, dev).to(dev).eval().requires_grad_(False)
    cv = _conv_plan(m, arith)
    assert cv.fused
    batch, gb = _graph(dev, [700, 1, 33, 1500, 64], 10, 90, cfg)
    g = gb.graph
    N = batch.n_nodes
    E = int(gb.n_edges_dev.item())
    gen = torch.Generator(device='cpu').manual_seed(1)
    x = (torch.randn(N, 64, generator=gen) * 1.5).to(dev)
    e = (torch.randn(gb.capacity, 64, generator=gen) * 1.5).to(dev)
    out_f = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_f)
    assert cv.fused_ok
    msg = torch.empty(gb.capacity, 64, device=dev)
    cv.msg(gb.capacity, msg, x, 64, mode=2, in2=e, w2=64, idx0=g.dst, idx1=g.src,
           rows_dev=gb.n_edges_dev)
    agg = torch.empty(N, 64, device=dev)
    engine.segment_reduce(msg, g.seg_ptr, N, aggr, agg)
    out_u = torch.empty(N, 64, device=dev)
    cv.upd(N, out_u, x, 64, mode=1, in1=agg, w1=64, residual=x)
    torch.testing.assert_close(out_f, out_u, rtol=2e-5, atol=2e-5)
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    ei = torch.stack((g.src[:E], g.dst[:E])).long().cpu()
    with torch.no_grad():
        ctx = gnn_forward_ref._Ctx(sd, cfg)
        ref = gnn_forward_ref.conv_block(ctx, 'pass_messages.conv_blk.0', x.cpu(), e[:E].cpu(), ei)
    torch.testing.assert_close(out_f.cpu(), ref, **FP32_TOL)
    # a second launch on the same workspace (counters reset by the launch itself (x3) or by
    # the projection launch (mfma_f32))
    out_2 = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_2)
    assert torch.equal(out_f, out_2)


@pytest.mark.parametrize('sizes', [[700, 1, 33, 1500, 64], [3], [3000] * 8])
def test_x3_conv_wave_table_bit_identical(cuda_device, sizes):
    """rg_conv_x3_blocks: the edge launch's per-wave node ranges -- wave w (XCD-major rank)
    owns the destinations [wtab[w], wtab[w + 1]) whose CSR starts reach E w / W: ranges
    ascending and covering every node once, edge counts within one destination's degree of
    an equal share.  rg_conv_layer_x3_blocks over it is bit-identical to rg_conv_layer_x3,
    which builds the same table in its workspace (every destination's messages summed in CSR
    order by one wave)."""
    from graph_neural_network_for_radar_perception_amd import engine
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    cfg = default_config(graph_convolution_stem_channels=[64], k_number_nearest_points=10)
    torch.manual_seed(14)
    m = Model_Training(cfg, dev).to(dev).eval().requires_grad_(False)
    cv = _conv_plan(m, 'x3')
    batch, gb = _graph(dev, sizes, 10, 91, cfg)
    g = gb.graph
    N = batch.n_nodes
    tbl = g.conv_x3_blocks()
    assert tbl is not None and tbl.numel() * 4 >= nat.lib().rg_conv_x3_blocks_bytes(N)
    G = min(max((N // 128 + 7) // 8 * 8, 8), 256)      # workgroups (x3_sp_groups)
    W = 4 * G * _x3_slabs(N)                             # pieces: waves x slabs
    wt = tbl[:W + 1].cpu().numpy()
    seg = g.seg_ptr.cpu().numpy()
    E = int(seg[N])
    assert wt[0] == 0 and wt[W] == N and np.all(np.diff(wt) >= 0)
    per = seg[wt[1:]] - seg[wt[:-1]]
    assert per.sum() == E
    maxdeg = int(np.diff(seg).max())
    assert np.all(per <= -(-E // W) + maxdeg), (per.max(), E / W, maxdeg)
    gen = torch.Generator(device='cpu').manual_seed(4)
    x = (torch.randn(N, 64, generator=gen) * 1.5).to(dev)
    e = (torch.randn(gb.capacity, 64, generator=gen) * 1.5).to(dev)
    out_t = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_t)
    old = engine.CONV_X3_TABLE
    engine.CONV_X3_TABLE = False
    try:
        g2 = engine.DeviceGraph(g.n_nodes, g.n_edges_cap, g.seg_ptr, g.dst, g.src, g.perm,
                                g.pair_src, g.pair_dst, g.n_pairs_dev)
        assert g2.conv_x3_blocks() is None
        out_p = torch.full((N, 64), float('nan'), device=dev)
        assert cv.run_fused(x, e, g2, out_p)
    finally:
        engine.CONV_X3_TABLE = old
    assert torch.equal(out_t, out_p)


def _x3_slabs(N):
    """conv_x3.hip x3_slabs: slabs per XCD node range of ~6000 nodes, 1 .. 8."""
    return min(max((N // 8 + 3000) // 6000, 1), 8)


@pytest.mark.parametrize('sizes', [[3000] * 24, [2999, 1, 40] * 24 + [500] * 2])
def test_x3_conv_slab_schedule_bit_identical(cuda_device, sizes):
    """The one-wave edge launch's slab schedule: each wave walks S pieces of whole
    destinations (one per slab of its XCD's node range, so the XCD's waves gather Q rows from
    one slab at a time) as one virtual edge sequence.  Bit-identical to one contiguous range
    per wave -- the same launch over a table whose pieces 1 .. S - 1 are empty -- and the
    table's pieces cover every node once with equal edge shares; the output also against
    the oracle's residual_graph_conv_block."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    cfg = default_config(graph_convolution_stem_channels=[64], k_number_nearest_points=10)
    torch.manual_seed(15)
    m = Model_Training(cfg, dev).to(dev).eval().requires_grad_(False)
    cv = _conv_plan(m, 'x3')
    batch, gb = _graph(dev, sizes, 10, 92, cfg)
    g = gb.graph
    N = batch.n_nodes
    S = _x3_slabs(N)
    assert S > 1
    G = min(max((N // 128 + 7) // 8 * 8, 8), 256)
    WX = G // 8 * 4                                      # waves per XCD
    W = 8 * WX
    tbl = g.conv_x3_blocks()
    seg = g.seg_ptr.cpu().numpy().astype(np.int64)
    E = int(seg[N])
    wt = tbl[:W * S + 1].cpu().numpy()
    assert wt[0] == 0 and wt[W * S] == N and np.all(np.diff(wt) >= 0)
    per = seg[wt[1:]] - seg[wt[:-1]]
    assert per.sum() == E and np.all(per <= -(-E // (W * S)) + int(np.diff(seg).max()))
    gen = torch.Generator(device='cpu').manual_seed(5)
    x = (torch.randn(N, 64, generator=gen) * 1.5).to(dev)
    e = (torch.randn(gb.capacity, 64, generator=gen) * 1.5).to(dev)
    out_s = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_s)
    # one contiguous range per wave: wave (x, j) = the single-slab table's range, as piece 0;
    # its pieces 1 .. S - 1 empty at the end of the XCD's range
    one = np.searchsorted(seg, (E * np.arange(W + 1)) // W, side='left')
    one[W] = N
    t2 = np.empty(W * S + 1, np.int32)
    for xcd in range(8):
        for k in range(S):
            for j in range(WX):
                q = (xcd * S + k) * WX + j
                t2[q] = one[xcd * WX + j] if k == 0 else one[(xcd + 1) * WX]
    t2[W * S] = N
    assert np.all(np.diff(t2.astype(np.int64)) >= 0)
    g._conv_x3_blocks = torch.from_numpy(t2).to(dev)
    out_c = torch.full((N, 64), float('nan'), device=dev)
    assert cv.run_fused(x, e, g, out_c)
    g._conv_x3_blocks = tbl
    assert torch.equal(out_s, out_c)
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    ei = torch.stack((g.src[:E], g.dst[:E])).long().cpu()
    with torch.no_grad():
        ctx = gnn_forward_ref._Ctx(sd, cfg)
        ref = gnn_forward_ref.conv_block(ctx, 'pass_messages.conv_blk.0', x.cpu(), e[:E].cpu(), ei)
    torch.testing.assert_close(out_s.cpu(), ref, **FP32_TOL)


def test_f32_fused_conv_deterministic_and_isolated_nodes(cuda_device):
    """Bit-reproducible across launches; nodes without incoming edges get agg = 0 (PyG)."""
    from graph_neural_network_for_radar_perception_amd import engine
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    cfg = default_config(graph_convolution_stem_channels=[64])
    torch.manual_seed(13)
    m = Model_Training(cfg, dev).to(dev).eval().requires_grad_(False)
    cv = m.pred.plans('fp32').convs[0]
    # a hand-made graph: node 0 <- 1, 2; node 3 <- 0; nodes 1, 2, 4..69 isolated
    N = 70
    ei = torch.tensor([[1, 2, 0], [0, 0, 3]], dtype=torch.int64, device=dev)
    g = engine.DeviceGraph.from_edge_index(ei, N)
    gen = torch.Generator(device='cpu').manual_seed(2)
    x = torch.randn(N, 64, generator=gen).to(dev)
    e = torch.randn(3, 64, generator=gen).to(dev)
    e_dst = e[g.perm[:3].long()].contiguous()
    outs = []
    for _ in range(3):
        o = torch.empty(N, 64, device=dev)
        assert cv.run_fused(x, e_dst, g, o)
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ctx = gnn_forward_ref._Ctx(sd, cfg)
        ref = gnn_forward_ref.conv_block(ctx, 'pass_messages.conv_blk.0', x.cpu(), e.cpu(),
                                         ei.cpu())
    torch.testing.assert_close(outs[0].cpu(), ref, **FP32_TOL)


@pytest.mark.timeout(600)
def test_m_config_full_batch_fp32_matches_oracle(cuda_device):
    """The metric configuration M at full size (64 frames x 3000 nodes, k = 10, L = 7,
    trained weights, the bench's own pipeline): every frame's edge count and four outputs
    against the oracle, with the worst error over all 64 frames reported as a fraction of
    the 1e-4 bound and held to <= 0.5 of it; the fused conv and the f32 fast chains are the
    ones used."""
    from graph_neural_network_for_radar_perception_amd import synthetic
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    from graph_neural_network_for_radar_perception_amd.graph_features import FrameBatch
    from graph_neural_network_for_radar_perception_amd.pipeline import RadarGNNPipeline
    from oracle import graph_features_ref as gref
    dev = cuda_device
    cfg = default_config()
    d = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'model_trained_N50.npz'))
    sd = {k[2:]: torch.from_numpy(np.array(d[k])) for k in d.files if k.startswith('w/')}
    m = Model_Training(cfg, 'cpu')
    m.load_state_dict(sd)
    pred = m.to(dev).pred.eval().requires_grad_(False)
    B, N = 64, 3000
    frames = [synthetic.make_frame(N, synthetic.SEED0 + f) for f in range(B)]
    clusters = [synthetic.cluster_lists(N) for _ in range(B)]
    batch = FrameBatch.from_frames(frames, clusters, device=dev)
    pipe = RadarGNNPipeline(pred, cfg, 'fp32')
    with torch.no_grad():
        gb, out = pipe.step(batch)
        torch.cuda.synchronize()
    plans = pipe.plans
    assert all(cv.fused_ok for cv in plans.convs), 'fused f32 conv not used'
    for c in (plans.node_enc, plans.edge_enc, plans.node_head, plans.offset_head,
              plans.link_pair, plans.cls_head):
        assert any(c.fast_ok.values()) or any(c.x3_ok.values()), 'f32 fast chain not used'
    rp = gb.row_ptr.cpu().numpy()
    fptr = np.arange(0, B + 1) * N
    U = int(gb.graph.n_pairs_dev.item())
    link = out.link_cls[:U].cpu().numpy()
    pair_src = gb.graph.pair_src[:U].cpu().numpy()
    got = {'node_cls': out.node_cls.cpu().numpy(), 'node_reg': out.node_reg.cpu().numpy(),
           'obj_cls': out.obj_cls.cpu().numpy()}
    gmax = float(np.sqrt(np.float64(100 ** 2 + 50 ** 2)))
    sdc = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    keys = ('node_cls', 'node_reg', 'link_cls', 'obj_cls')
    # worst |d| / (atol + rtol |ref|) per output over ALL 64 frames (1.0 = the 1e-4 bound)
    worst = {k: 0.0 for k in keys}
    maxabs = {k: 0.0 for k in keys}
    for f in range(B):
        g = gref.build_frame_graph(frames[f], 25.0, 10, gmax)
        assert rp[fptr[f + 1]] - rp[fptr[f]] == g['edge_index'].shape[1]
        with torch.no_grad():
            ref = gnn_forward_ref.forward(sdc, cfg, torch.from_numpy(g['node_features']),
                                          torch.from_numpy(g['edge_features']),
                                          torch.from_numpy(g['edge_index']), None,
                                          [torch.from_numpy(c) for c in clusters[f]])
        sl = slice(f * N, (f + 1) * N)
        ncl = len(clusters[f])
        sel = (pair_src >= f * N) & (pair_src < (f + 1) * N)
        pairs = {'node_cls': got['node_cls'][sl], 'node_reg': got['node_reg'][sl],
                 'link_cls': link[sel], 'obj_cls': got['obj_cls'][f * ncl:(f + 1) * ncl]}
        for k, r in zip(keys, ref):
            r = r.numpy()
            assert pairs[k].shape == r.shape, (f, k)
            d = np.abs(pairs[k].astype(np.float64) - r)
            worst[k] = max(worst[k], float((d / (1e-4 + 1e-4 * np.abs(r))).max()))
            maxabs[k] = max(maxabs[k], float(d.max()))
    report = {'frames': B, 'nodes': N, 'worst_over_bound': worst, 'max_abs_err': maxabs}
    print('M parity headroom (1.0 = the 1e-4 bound):', report)
    path = os.environ.get('RG_PARITY_REPORT')
    if path:
        import json
        with open(path, 'w') as fh:
            json.dump(report, fh, indent=1)
    # headroom: a regression has to double the error before it reaches the 1e-4 bound
    assert all(v <= 0.5 for v in worst.values()), report


@pytest.mark.parametrize('over', [dict(node_feat_enc_stem_channels=[256, 128, 96],
                                       graph_convolution_stem_channels=[96, 96]),
                                  dict(graph_convolution_stem_channels=[64, 64],
                                       msg_mlp_hidden_dim=96)])
def test_f32_non_yml_conv_widths_match_oracle(cuda_device, over):
    """fp32 models whose conv blocks are NOT the compiled fused shape (C = 64, hidden 128):
    96-wide blocks without a residual projection, and a 96-wide message hidden layer
    (widths above 256, e.g. 128-wide conv blocks with their 320-wide message input, are
    outside the chain kernels and raise).
    The fused f32 conv is not planned for them (ConvPlan.fused is None), the unfused chains
    run, and the forward equals the oracle at 1e-4 (these raised before)."""
    from graph_neural_network_for_radar_perception_amd import synthetic
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    from oracle import graph_features_ref as gref
    dev = cuda_device
    cfg = default_config(**over)
    torch.manual_seed(31)
    m = Model_Training(cfg, 'cpu')
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pred = m.to(dev).pred.eval().requires_grad_(False)
    gmax = float(np.sqrt(np.float64(100 ** 2 + 50 ** 2)))
    fr = synthetic.make_frame(400, 4242)
    g = gref.build_frame_graph(fr, 25.0, 10, gmax)
    cl = [torch.from_numpy(c) for c in synthetic.cluster_lists(400)]
    args = (torch.from_numpy(g['node_features']), torch.from_numpy(g['edge_features']),
            torch.from_numpy(g['edge_index']))
    with torch.no_grad():
        out = pred(*(a.to(dev) for a in args), None, [c.to(dev) for c in cl])
        ref = gnn_forward_ref.forward(sd, cfg, *args, None, cl)
    for cv in pred.plans('fp32').convs:
        if cv.c_out != 64 or cv.msg.specs[0].out_dim != 128:
            assert not cv.fused
    for o, r in zip(out, ref):
        np.testing.assert_allclose(o.cpu().numpy(), r.numpy(), **FP32_TOL)


def test_generic_chain_f32x3_matches_f32(cuda_device):
    """rg_mlp_chain RG_F32X3 (layers packed RG_BF16 | RG_PACK_X3: three exact bf16 planes,
    products from exact activation splits, f32 accumulation) against the same chain on the
    exact f32 MFMA (RG_F32), GATHER3 input, norm + LeakyReLU, training tapes on: outputs and
    both tapes agree to 2e-5 of their scale; the backward's transposed x3 packing (dX = dZ W)
    likewise."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    lib = nat.lib()
    dev = cuda_device
    st = nat.stream_ptr(dev)
    g = torch.Generator().manual_seed(5)
    N, E, C = 900, 5000, 64
    dims = [(3 * C, 128), (128, 64)]
    ws = [(torch.randn(o, i, generator=g) / i ** 0.5).to(dev) for i, o in dims]
    bs = [(0.1 * torch.randn(o, generator=g)).to(dev) for _, o in dims]
    mus = [torch.tensor([0.2], device=dev), torch.tensor([-0.1], device=dev)]
    sds = [torch.tensor([1.3], device=dev), torch.tensor([0.7], device=dev)]
    x = torch.randn(N, C, generator=g).to(dev)
    e = torch.randn(E, C, generator=g).to(dev)
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32).to(dev)
    dst = torch.randint(0, N, (E,), generator=g, dtype=torch.int32).to(dev)

    def run(dtype, fmt):
        bufs, arr = [], (nat.rg_layer * 2)()
        tapes = []
        for l, ((i, o), w, b) in enumerate(zip(dims, ws, bs)):
            buf = torch.empty(lib.rg_packed_linear_bytes(i, o, fmt), dtype=torch.uint8, device=dev)
            nat.check(lib.rg_pack_linear(w.data_ptr(), b.data_ptr(), i, o, fmt, buf.data_ptr(), st),
                      'rg_pack_linear')
            bufs.append(buf)
            z = torch.empty(E, o, device=dev)
            a = torch.empty(E, o, device=dev)
            tapes.append((z, a))
            arr[l].w_packed = buf.data_ptr()
            arr[l].norm_mu = mus[l].data_ptr()
            arr[l].norm_std = sds[l].data_ptr()
            arr[l].in_dim, arr[l].out_dim = i, o
            arr[l].act = nat.ACT['leakyrelu']
            arr[l].save_pre, arr[l].save_out = z.data_ptr(), a.data_ptr()
        out = torch.empty(E, 64, device=dev)
        nat.check(lib.rg_mlp_chain(dtype, arr, 2, E, None, nat.IN_GATHER3, nat.RG_F32,
                                   x.data_ptr(), x.stride(0), C, None, 0, 0, e.data_ptr(),
                                   e.stride(0), C, dst.data_ptr(), src.data_ptr(), None, 0,
                                   nat.RG_F32, out.data_ptr(), out.stride(0), nat.RG_F32, st),
                  'rg_mlp_chain')
        torch.cuda.synchronize()
        return out, tapes

    o32, t32 = run(nat.RG_F32, nat.RG_F32)
    ox3, tx3 = run(nat.RG_F32X3, nat.RG_BF16 | nat.RG_PACK_X3)
    for a, b in [(o32, ox3)] + [p for pair in zip(t32, tx3) for p in zip(*pair)]:
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 2e-5 * max(scale, 1.0)
    # dX = dZ W with transposed packing, as the training backward runs it
    dz = torch.randn(E, 128, generator=g).to(dev)
    outs = []
    for dtype, fmt in ((nat.RG_F32, nat.RG_F32), (nat.RG_F32X3, nat.RG_BF16 | nat.RG_PACK_X3)):
        buf = torch.empty(lib.rg_packed_linear_bytes(128, 3 * C, fmt), dtype=torch.uint8, device=dev)
        nat.check(lib.rg_pack_linear(ws[0].data_ptr(), None, 128, 3 * C, fmt | nat.RG_PACK_TRANSPOSE,
                                     buf.data_ptr(), st), 'rg_pack_linear')
        arr = (nat.rg_layer * 1)()
        arr[0].w_packed = buf.data_ptr()
        arr[0].in_dim, arr[0].out_dim = 128, 3 * C
        arr[0].act = nat.ACT['none']
        dx = torch.empty(E, 3 * C, device=dev)
        nat.check(lib.rg_mlp_chain(dtype, arr, 1, E, None, nat.IN_DENSE, nat.RG_F32, dz.data_ptr(),
                                   dz.stride(0), 128, None, 0, 0, None, 0, 0, None, None, None,
                                   0, nat.RG_F32, dx.data_ptr(), dx.stride(0), nat.RG_F32, st),
                  'rg_mlp_chain')
        outs.append(dx)
    torch.cuda.synchronize()
    ref = (dz.double() @ ws[0].double()).float()
    for dx in outs:
        assert float((dx - ref).abs().max()) <= 2e-5 * float(ref.abs().max())


def test_link_head_per_node_first_layer(cuda_device, monkeypatch):
    """fp32 link head through RG_IN_PAIRPRE (ModelPlans.link_pairs_pre: the pair chain's first
    Linear applied per node, W0 (s_i + s_j) + b0 = W0 s_i + W0 s_j + b0) against the per-pair
    chain (RG_IN_PAIRADD) on the trained model at M-frame size: the link logits agree at the
    fp32 bound, and the per-node path is the one that ran."""
    from graph_neural_network_for_radar_perception_amd import engine, synthetic
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.graph_features import FrameBatch
    from graph_neural_network_for_radar_perception_amd.pipeline import RadarGNNPipeline
    import bench
    dev = cuda_device
    cfg = default_config()
    frames = [synthetic.make_frame(3000, 700 + i) for i in range(3)]
    clusters = [synthetic.cluster_lists(3000) for _ in range(3)]
    batch = FrameBatch.from_frames(frames, clusters, device=dev)
    outs = {}
    for pre in (True, False):
        monkeypatch.setattr(engine, 'LINK_PRE', pre)
        model = bench.make_model(cfg, dev, bench.model_state(cfg, 'trained'))
        with torch.no_grad():
            gb, out = RadarGNNPipeline(model, cfg, 'fp32').step(batch)
        plans = model.plans('fp32')
        if pre:
            assert plans.link_pre is not None and plans.link_pre.x3_ok.get('pre') is not False
        else:
            assert plans.link_pre is None
        outs[pre] = RadarGNNPipeline.trim(gb, out)[2]
    torch.testing.assert_close(outs[True], outs[False], **FP32_TOL)
