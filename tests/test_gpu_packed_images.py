"""Every packed image of a chain follows the weights: each kind of image engine.PackedImages
holds is made by running its consumer once, the parameters are changed through torch and
behind its version counters, and every consumer must then compute, bit for bit, what freshly
built plans over the same parameters compute."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

R = 70          # rows of the chains = nodes of the graph (three 32-row tiles, the last partial)
K = 4           # neighbours per node


def _kinds(images):
    from graph_neural_network_for_radar_perception_amd import _native as nat
    out = set()
    for fmts, transpose, block in images.held():
        if block is not None:
            out.add('column-block')
        elif transpose:
            out.add('transposed')
        elif fmts[0] & nat.RG_PACK_H2:
            out.add('x3-h2')
        elif fmts[0] & nat.RG_PACK_X3:
            out.add('x3-b3')
        elif fmts[0] == nat.RG_PACK_F32_FAST:
            out.add('f32-fast')
        elif fmts[0] == nat.RG_F32:
            out.add('generic')
    return out


def _consume(o, d, monkeypatch):
    """Run every consumer of o's images once; returns their outputs by name."""
    from graph_neural_network_for_radar_perception_amd import engine
    dev = d.x.device
    out = {}
    plan = o.head.plan

    def call():
        y = torch.full((R, plan.out_dim), float('nan'), device=dev)
        plan(R, y, d.x, 64)
        return y

    for terms in ('h2', 'b3'):                      # rg_mlp_chain_x3 under either scheme
        monkeypatch.setattr(engine, 'X3_TERMS', terms)
        out[terms] = call()
        assert plan.x3_ok.get(0), 'x3 chain kernel not used'
    monkeypatch.setattr(engine, 'F32_ARITH', 'mfma_f32')    # rg_mlp_chain_f32: exact products
    out['f32-fast'] = call()
    assert plan.fast_ok.get(0), 'f32 chain kernel not used'
    monkeypatch.setattr(engine, 'F32_ARITH', 'x3')
    plan.use_fast = False                           # the generic chain kernel
    out['generic'] = call()
    plan.use_fast = True
    # the training tape and the backward: transposes, rg_dx_norm_backward
    grads = {id(p): torch.zeros_like(p) for p in d.head_params}
    y = torch.full((R, plan.out_dim), float('nan'), device=dev)
    tape = o.head.forward(R, y, d.x, 64)
    assert o.head._fast_ok.get(0), 'fast tape not used'
    din = torch.full((R, 64), float('nan'), device=dev)
    o.head.backward(tape, d.dout.clone(), grads, din=din)
    out['tape'], out['din'] = y, din
    out['grads'] = torch.cat([grads[id(p)].flatten() for p in d.head_params])
    # dX over one column block of the message chain's 192-wide first layer
    dxb = torch.full((R, 64), float('nan'), device=dev)
    o.msg._dx(0, R, d.dz, dxb, None, block=(64, 64))
    out['dx-block'] = dxb
    # the fused conv layer (rg_conv_proj_x3 + rg_conv_layer_x3)
    xo = torch.full((R, 64), float('nan'), device=dev)
    assert o.conv.run_fused(d.x, d.e, d.g, xo) and o.conv.x3, 'fused x3 conv not used'
    out['conv'] = xo
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in out.values())
    return out


def test_every_image_follows_the_weights(cuda_device, monkeypatch):
    from graph_neural_network_for_radar_perception_amd import engine, training
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    torch.manual_seed(31)
    pred = Model_Training(default_config(), dev).to(dev).pred
    # the node head (3-block stem, ffn, Linear -> 7): the chain with compiled x3, f32 and
    # generic kernels ([64 -> 128 -> 64 -> 7] has no rg_mlp_chain_x3 instantiation)
    pn = pred.predict_node
    head_mods = list(pn.stem) + [pn.pred_cls.head[0], pn.pred_cls.head[1]]
    blk = pred.pass_messages.conv_blk[0]

    def build():
        ws = training.Workspaces(dev)
        return types.SimpleNamespace(head=training.TrainChain(head_mods, dev, ws),
                                     msg=training.TrainChain(list(blk.msg), dev, ws),
                                     conv=engine.ConvPlan(blk, 'fp32', dev))

    g = torch.Generator().manual_seed(5)
    dst = torch.arange(R).repeat_interleave(K)
    src = (dst + torch.arange(1, K + 1).repeat(R)) % R
    d = types.SimpleNamespace(
        x=torch.randn(R, 64, generator=g).to(dev), e=torch.randn(R * K, 64, generator=g).to(dev),
        dout=torch.randn(R, 7, generator=g).to(dev), dz=torch.randn(R, 128, generator=g).to(dev),
        g=engine.DeviceGraph.from_edge_index(torch.stack((src, dst)).to(dev), R, count_pairs=False),
        head_params=[p for m in head_mods for p in m.parameters()])
    params = d.head_params + list(blk.parameters())

    o = build()
    before = _consume(o, d, monkeypatch)
    held = _kinds(o.head.plan.images) | _kinds(o.msg.plan.images)
    assert held >= {'generic', 'f32-fast', 'x3-h2', 'x3-b3', 'transposed', 'column-block'}, held
    assert o.conv.images.held(), 'no fused conv image held'

    def through_torch():
        with torch.no_grad():
            for p in params:
                p.add_(0.05 * torch.randn_like(p))

    def behind_the_counters():
        for p in params:
            p.data.add_(0.05 * torch.randn_like(p))
        for c in (o.head, o.msg, o.conv):
            c.invalidate()

    for update in (through_torch, behind_the_counters):
        update()
        for c in (o.head, o.msg, o.conv):       # as every forward does
            c.refresh()
        got = _consume(o, d, monkeypatch)
        want = _consume(build(), d, monkeypatch)
        for name in want:
            assert torch.equal(got[name], want[name]), (update.__name__, name)
            assert not torch.equal(got[name], before[name]), (update.__name__, name)
        before = got
