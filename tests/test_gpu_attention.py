"""Graph attention on the GPU: the fused GATv2 layer (rg_gat_v2_layer), the composed path,
the residual attention block and Model_Inference_v2 against the float64 oracle
(tests/attention_ref.py) at the project's fp32 bound |d| <= 1e-4 + 1e-4 |ref|, and the
bit-equalities the kernel promises (run to run, batch independence, capacity padding).

Layer shape: yml (in = Ce = 64, H = 8, C = 64), 15 destinations with segment lengths
0, 1, 2, 5, 31, 32, 33, 63, 64, 65, 130, 0, 7, 200, 3 (636 edges): empty segments, lengths
around the 32-edge tile and the 64-lane wave, segments that span several tiles.
Every reading is printed, and appended as a JSON line to $RG_GAT_REPORT when set (the committed
readings: profiles/gat_v2_parity.json)."""
import json
import os

import pytest
import torch

import attention_ref as aref

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(case, seed=0):
    """(inputs, float64 oracle) of one layer case, computed once."""
    key = (case, seed)
    if key not in _CASES:
        c = aref.layer_case(case, seed)
        sd64 = {'.' + k: v.double() for k, v in c['sd'].items()}
        want = aref.gat_v2(sd64, '', c['x'].double(), c['e'].double(),
                           torch.stack((c['src'], c['dst'])))
        _CASES[key] = (c, want)
    return _CASES[key]


def _record(rec):
    print(json.dumps(rec))
    path = os.environ.get('RG_GAT_REPORT')
    if path:
        with open(path, 'a') as fh:
            fh.write(json.dumps(rec) + '\n')


def _gat(sd, dev):
    from graph_neural_network_for_radar_perception_amd.gnn_attention import GATv2Conv
    gat = GATv2Conv(64, 64, heads=8, edge_dim=64, add_self_loops=False)
    gat.load_state_dict(sd)
    return gat.to(dev).eval().requires_grad_(False)


def _graph(seg_ptr, src, dst, dev, cap=None, n_edges='given'):
    """A DeviceGraph from destination-major arrays; cap > E: positions past the edges hold
    index 0 (and the edge count stays on the device: n_edges None)."""
    from graph_neural_network_for_radar_perception_amd import engine
    E = int(src.numel())
    cap = E if cap is None else cap
    s = torch.zeros(max(cap, 1), dtype=torch.int32)
    d = torch.zeros(max(cap, 1), dtype=torch.int32)
    s[:E], d[:E] = src.int(), dst.int()
    return engine.DeviceGraph(int(seg_ptr.numel()) - 1, cap, seg_ptr.int().to(dev), d.to(dev),
                              s.to(dev), None, None, None, None,
                              n_edges=E if n_edges == 'given' else None)


def _run(c, dev, fused, cap=None):
    from graph_neural_network_for_radar_perception_amd import engine
    gat = _gat(c['sd'], dev)
    E = int(c['src'].numel())
    g = _graph(c['seg_ptr'], c['src'], c['dst'], dev, cap, 'given' if cap is None else None)
    e = c['e']
    if cap is not None:   # the padding: NaN rows
        e = torch.cat((e, torch.full((cap - E, e.shape[1]), float('nan'))))
    out = engine.gat_v2_conv(gat, c['x'].to(dev), e.to(dev).contiguous(), g, fused=fused)
    assert not out.requires_grad
    return out


@pytest.mark.parametrize('path', ['fused', 'composed'])
@pytest.mark.parametrize('case', [1, 2, 3])
def test_layer_matches_float64_oracle(cuda_device, case, path):
    """Case 1: randn inputs; 2: inputs x 12 (logits +- 36); 3: b_r = 25 sign(att), flipped on
    odd heads (logits + 100 .. + 180 / - 85 .. - 165: no softmax without the max subtraction
    survives float32).  Float32 torch on the CPU reads 0.003 / 0.15 / 0.11 of the bound."""
    c, want = _case(case)
    out = _run(c, cuda_device, path == 'fused')
    r = aref.worst_ratio(out, want)
    _record({'test': 'layer', 'case': case, 'path': path, 'of_bound': r})
    assert r <= 1.0, r
    empty = [i for i, n in enumerate(aref.SEG_LENGTHS) if n == 0]
    assert torch.equal(out[empty].cpu(), c['sd']['bias'].expand(len(empty), -1))


def test_layer_bit_equal_run_to_run(cuda_device):
    c, _ = _case(1)
    a, b = _run(c, cuda_device, True), _run(c, cuda_device, True)
    assert torch.equal(a, b)


def test_layer_bit_equal_in_twice_the_capacity(cuda_device):
    """Edges at positions from seg_ptr[N] up to the capacity are never read: NaN rows in e
    and index 0 in src / dst there change nothing, bit for bit -- on both paths."""
    c, _ = _case(1)
    E = int(c['src'].numel())
    for fused in (True, False):
        tight, padded = _run(c, cuda_device, fused), _run(c, cuda_device, fused, cap=2 * E)
        assert torch.isfinite(padded).all()
        assert torch.equal(tight, padded), fused


def test_layer_bit_equal_alone_and_in_a_batch(cuda_device):
    """A frame alone equals the same frame as the middle one of a batch of three (other
    tile boundaries, other workgroups)."""
    from graph_neural_network_for_radar_perception_amd import engine
    dev = cuda_device
    # other segment lengths in the first frame, so that the middle one starts inside a tile
    first = aref.layer_case(1, 1, lengths=(3, 0, 40, 7, 1, 0, 9, 2, 2, 2, 11, 5, 0, 1, 6))
    frames = [first, _case(1)[0], aref.layer_case(1, 2)]
    gat = _gat(frames[1]['sd'], dev)
    n = len(aref.SEG_LENGTHS)
    alone = engine.gat_v2_conv(
        gat, frames[1]['x'].to(dev), frames[1]['e'].to(dev),
        _graph(frames[1]['seg_ptr'], frames[1]['src'], frames[1]['dst'], dev), fused=True)
    x = torch.cat([f['x'] for f in frames])
    e = torch.cat([f['e'] for f in frames])
    src = torch.cat([f['src'] + n * k for k, f in enumerate(frames)])
    dst = torch.cat([f['dst'] + n * k for k, f in enumerate(frames)])
    lens = torch.cat([f['seg_ptr'][1:] - f['seg_ptr'][:-1] for f in frames])
    seg_ptr = torch.cat((torch.zeros(1, dtype=torch.int64), lens.cumsum(0)))
    assert int(first['src'].numel()) % 32 != 0
    batch = engine.gat_v2_conv(gat, x.to(dev), e.to(dev), _graph(seg_ptr, src, dst, dev),
                               fused=True)
    assert torch.equal(alone, batch[n:2 * n])


def _knn_edges(n, k, gen):
    """A symmetric k-NN graph on random points, edges in np.where (row-major) order."""
    p = torch.rand((n, 2), generator=gen)
    d = torch.cdist(p, p) + torch.eye(n) * 1e9
    nb = d.topk(k, largest=False).indices
    adj = torch.zeros((n, n), dtype=torch.bool)
    adj[torch.arange(n).repeat_interleave(k), nb.reshape(-1)] = True
    adj |= adj.T.clone()
    return torch.stack(torch.nonzero(adj, as_tuple=True))


def _randomise(module, gen):
    """Biases 0.1 randn everywhere and O(1) rows in the heads (whose 0.01 init would hide the
    backbone behind the bias)."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith('weight') and float(p.std()) < 0.02:
                p.copy_(torch.randn(p.shape, generator=gen) / p.shape[1] ** 0.5)


def test_block_with_extra_features(cuda_device):
    """residual_graph_attn_block built with in_extra_feature_dim = 3: the update runs on
    cat(x, extra, attention output), 579 wide (not a multiple of 4: the wide linear's
    unaligned path), edges in the caller's order, fused and composed."""
    from graph_neural_network_for_radar_perception_amd.gnn_attention import \
        residual_graph_attn_block
    from graph_neural_network_for_radar_perception_amd import engine
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(12)
    blk = residual_graph_attn_block(64, 512, 64, 8, [256, 128, 64], 'leakyrelu',
                                    in_extra_feature_dim=3)
    _randomise(blk, gen)
    N = 37
    ei = _knn_edges(N, 4, gen)
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    x = torch.randn((N, 64), generator=gen)
    ef = torch.randn((ei.shape[1], 64), generator=gen)
    extra = torch.randn((N, 3), generator=gen)
    want = aref.attn_block(aref.to64({'b.' + k: v for k, v in blk.state_dict().items()}), 'b',
                           x.double(), ef.double(), ei, 'leakyrelu', extra.double())
    blk = blk.to(cuda_device).eval().requires_grad_(False)
    dev = cuda_device
    out = blk(x.to(dev), ef.to(dev), ei.to(dev), extra.to(dev))
    assert not out.requires_grad
    r = aref.worst_ratio(out, want)
    rc = aref.worst_ratio(engine.run_attn_block(blk, x.to(dev), ef.to(dev), ei.to(dev),
                                                extra_features=extra.to(dev), fused=False), want)
    _record({'test': 'block_extra', 'of_bound': r, 'of_bound_composed': rc})
    assert r <= 1.0 and rc <= 1.0, (r, rc)
    with pytest.raises(TypeError):
        blk(x.to(dev), ef.to(dev), ei.to(dev))


def test_block_with_residual_projection_over_two_frames(cuda_device):
    """Widths 64 -> 32: identity = Linear + layer_normalization, whose statistics run over
    one frame's rows -- two frames of 29 and 18 nodes in one batch."""
    from graph_neural_network_for_radar_perception_amd.gnn_attention import \
        residual_graph_attn_block
    from graph_neural_network_for_radar_perception_amd import engine
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(22)
    blk = residual_graph_attn_block(64, 512, 64, 8, [256, 128, 32], 'leakyrelu')
    _randomise(blk, gen)
    with torch.no_grad():
        blk.residual_connection[1].mu.fill_(0.3)
        blk.residual_connection[1].std.fill_(1.7)
    sd64 = aref.to64({'b.' + k: v for k, v in blk.state_dict().items()})
    sizes = (29, 18)
    xs, efs, eis, wants = [], [], [], []
    for n in sizes:
        ei = _knn_edges(n, 4, gen)
        x = torch.randn((n, 64), generator=gen)
        ef = torch.randn((ei.shape[1], 64), generator=gen)
        wants.append(aref.attn_block(sd64, 'b', x.double(), ef.double(), ei, 'leakyrelu'))
        xs.append(x), efs.append(ef), eis.append(ei)
    dev = cuda_device
    blk = blk.to(dev).eval().requires_grad_(False)
    ap = engine.AttnPlan(blk, 'fp32', dev)
    N = sum(sizes)
    ei = torch.cat((eis[0], eis[1] + sizes[0]), 1).to(dev)
    g = engine.DeviceGraph.from_edge_index(ei, N, count_pairs=False)
    g.set_frames(torch.tensor([0, sizes[0], N], device=dev), 2)
    e = engine._edges_by_destination(torch.cat(efs).to(dev), g)
    out = torch.empty((N, 32), dtype=torch.float32, device=dev)
    ap.run(torch.cat(xs).to(dev), e, g, out, segs=g.segs('node'))
    r = aref.worst_ratio(out, torch.cat(wants))
    _record({'test': 'block_residual_projection', 'of_bound': r})
    assert r <= 1.0, r
    # a frame alone through the module: the same rows
    alone = blk(xs[1].to(dev), efs[1].to(dev), eis[1].to(dev))
    assert aref.worst_ratio(alone, wants[1]) <= 1.0


@pytest.mark.parametrize('name,overrides', [
    ('yml_fused', dict(graph_convolution_stem_channels=[64, 64])),
    ('h128_composed', dict(hidden_node_channels_GAT=128, num_heads_GAT=4,
                           graph_convolution_stem_channels=[64, 32])),
])
def test_model_v2_matches_oracle(cuda_device, name, overrides):
    """Model_Inference_v2 on two frames of 40 and 23 nodes (k-NN, k = 4, object clusters
    given) against the float64 oracle per frame; forward per frame and forward_frames agree
    bit for bit."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Inference_v2
    from graph_neural_network_for_radar_perception_amd import engine
    cfg = default_config(**overrides)
    gen = torch.Generator().manual_seed(31)
    torch.manual_seed(32)
    m = Model_Inference_v2(cfg)
    _randomise(m, gen)
    sd64 = aref.to64(m.state_dict())
    frames = []
    for n in (40, 23):
        ei = _knn_edges(n, 4, gen)
        nf = torch.randn((n, cfg.input_node_feat_dim), generator=gen)
        ef = torch.randn((ei.shape[1], cfg.input_edge_feat_dim), generator=gen)
        perm = torch.randperm(n, generator=gen)
        clusters = [perm[:5], perm[5:6], perm[6:17], perm[17:]]
        want = aref.forward(sd64, cfg, nf.double(), ef.double(), ei, clusters)
        frames.append((nf, ef, ei, clusters, want))
    dev = cuda_device
    m = m.to(dev).eval()
    fused = engine.gat_fused_shape(m.pass_messages.conv_blk[0].GATblk)
    assert fused == (name == 'yml_fused')
    per_frame = [m(nf.to(dev), ef.to(dev), ei.to(dev), None, [c.to(dev) for c in cl])
                 for nf, ef, ei, cl, _ in frames]
    worst = 0.0
    for outs, (_, _, _, _, want) in zip(per_frame, frames):
        for o, w in zip(outs, want):
            assert not o.requires_grad and o.shape == w.shape
            worst = max(worst, aref.worst_ratio(o, w))
    _record({'test': 'model_v2', 'case': name, 'of_bound': worst})
    assert worst <= 1.0, worst
    batch = m.forward_frames([f[0].to(dev) for f in frames], [f[1].to(dev) for f in frames],
                             [f[2].to(dev) for f in frames],
                             [[c.to(dev) for c in f[3]] for f in frames])
    for k in range(4):
        assert torch.equal(batch[k], torch.cat([p[k] for p in per_frame])), k
    with pytest.raises(NotImplementedError):
        m.compute_dtype = 'bf16'
        m.forward_frames([frames[0][0].to(dev)], [frames[0][1].to(dev)], [frames[0][2].to(dev)],
                         [[c.to(dev) for c in frames[0][3]]])
