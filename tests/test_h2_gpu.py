"""The 'h2' term scheme of the fp32 MLP chains on the GPU (chain_x3.hip with RG_PACK_H2
images: two-term IEEE fp16 splits, three MFMA products per f32 product): the hardware fact
it rests on, the packed image, every chain of the shipped architecture, inputs of mixed
magnitude and past the domain, and the whole model against the reference's fixtures.

Tolerances: a chain against a float64 evaluation of the same float32 weights and inputs,
|d| <= 1e-4 + 1e-4 |ref| (the fp32 bound of the other float32 kernels); the packed planes
against the weights, 2^-21 |w| + 2^-24 2^-s (two 11-bit planes; the second plane's quantum
after the descale).
"""
import types

import numpy as np
import pytest
import torch

from conftest import cluster_lists, golden, model_cfg, model_state_dict

pytestmark = pytest.mark.gpu

FP32_TOL = dict(rtol=1e-4, atol=1e-4)


@pytest.fixture(autouse=True)
def _h2(monkeypatch):
    from graph_neural_network_for_radar_perception_amd import engine
    monkeypatch.setattr(engine, 'F32_ARITH', 'x3')
    monkeypatch.setattr(engine, 'X3_TERMS', 'h2')


# ------------------------------------------------------------------ the hardware fact
def _probe(dev, a, b):
    """rg_h2_mfma_probe: c[m][n] = sum_k a[m][k] b[n][k], a / b float16 [32][16]."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    ta = torch.from_numpy(a.view(np.int16).copy()).to(dev)
    tb = torch.from_numpy(b.view(np.int16).copy()).to(dev)
    c = torch.full((32, 32), float('nan'), dtype=torch.float32, device=dev)
    nat.check(nat.lib().rg_h2_mfma_probe(ta.data_ptr(), tb.data_ptr(), c.data_ptr(),
                                         nat.stream_ptr(dev)), 'rg_h2_mfma_probe')
    return c.cpu().numpy()


def test_mfma_honours_fp16_subnormal_operands(cuda_device):
    """v_mfma_f32_32x32x16_f16 as the kernels run it takes SUBNORMAL fp16 inputs at their
    value, in A and in B: with subnormals (2^-24, 2^-20, 2^-15, 1023 2^-24 and their
    negatives) in one operand and normal values in the other, every accumulator equals the
    exact sum of products.  The h2 arithmetic keeps the low half of every activation in such
    values; were they flushed, it would need a prescaled variant."""
    subs = np.float16([2.0 ** -24, 2.0 ** -20, 2.0 ** -15, 1023 * 2.0 ** -24])
    assert np.all(np.abs(subs.astype(np.float64)) < 2.0 ** -14)        # all subnormal
    rng = np.random.default_rng(3)
    sub = np.zeros((32, 16), np.float16)
    for m in range(32):
        for k in range(16):
            sub[m, k] = subs[(m + k) % 4] * (-1 if (m * 7 + k) % 3 == 0 else 1)
    sub[5] = 0
    sub[5, 9] = np.float16(-2.0 ** -24)                                # a lone smallest value
    # normal values whose products and 16-term sums are exact in float32: small integers
    # times powers of two
    nrm = (rng.integers(-8, 9, (32, 16)) * np.exp2(rng.integers(0, 4, (32, 16)))).astype(np.float16)
    nrm[nrm == 0] = 1
    for a, b in ((sub, nrm), (nrm, sub)):
        want = a.astype(np.float64) @ b.astype(np.float64).T
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        got = _probe(cuda_device, a, b)
        assert np.count_nonzero(want) > 900
        assert np.array_equal(got.astype(np.float64), want)


# ------------------------------------------------------------------ the packed image
def _unpack_h2(buf, K, N, chain_fmt):
    """(plane0, plane1 as float64 [N][K], bias float32 [N], (ds, sc, s)) of an RG_PACK_H2 image
    (x3_common.h: [m][s][lane][8] fragments, lane = (row r, half h))."""
    NT, KS = (N + 31) // 32, (K + 15) // 16
    pl = NT * KS * 1024
    raw = buf.cpu().numpy()
    planes = []
    m, s, lane, j = np.meshgrid(np.arange(NT), np.arange(KS), np.arange(64), np.arange(8),
                                indexing='ij')
    r, h = lane & 31, lane >> 5
    o = 32 * m + r
    k = (32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3)) if chain_fmt \
        else 16 * s + 8 * h + j
    for p in range(2):
        frag = raw[p * pl:(p + 1) * pl].view(np.float16).reshape(NT, KS, 64, 8).astype(np.float64)
        W = np.zeros((32 * NT, 16 * KS))
        W[o, k] = frag
        assert not W[N:].any() and not W[:, K:].any()                  # zero padding
        planes.append(W[:N, :K])
    tail = raw[2 * pl:2 * pl + 32 * NT * 4 + 16]
    bacc = tail[:32 * NT * 4].view(np.float32)
    t = np.arange(32 * NT)
    f = 32 * (t >> 5) + 8 * ((t >> 2) & 3) + 4 * ((t >> 4) & 1) + (t & 3)
    bias = np.zeros(32 * NT, np.float32)
    bias[f] = bacc
    tr = tail[32 * NT * 4:]
    return planes[0], planes[1], bias[:N], (float(tr[:4].view(np.float32)[0]),
                                            float(tr[4:8].view(np.float32)[0]),
                                            int(tr[8:12].view(np.int32)[0]))


@pytest.mark.parametrize('K,N,chain_fmt,top,centre', [
    (7, 256, False, 0.4, False), (64, 64, True, 1.19, True), (128, 64, True, 1e-6, False),
    (64, 32, True, 1e3, True), (16, 40, False, 0.0, False)])
def test_h2_pack_round_trip(cuda_device, K, N, chain_fmt, top, centre):
    """rg_pack_linear with RG_PACK_H2: the stored exponent follows the scale rule (tiny, huge
    and all-zero layers included), the two planes times 2^-s reproduce the (centred) weights
    to 2^-21 |w| + 2^-24 2^-s, the bias is b 2^s exactly, the padding is zero."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd.engine import h2_scale_exp
    dev = cuda_device
    rng = np.random.default_rng(K * 1000 + N)
    w = (rng.uniform(-1.0, 1.0, (N, K)) * top).astype(np.float32)
    b = rng.normal(0.0, 1.0, N).astype(np.float32)
    fmt = (nat.RG_PACK_FAST_CHAIN if chain_fmt else nat.RG_PACK_FAST_IN) | nat.RG_PACK_H2 \
        | (nat.RG_PACK_CENTERED if centre else 0)
    lib = nat.lib()
    size = lib.rg_packed_linear_bytes(K, N, fmt)
    assert size == 2 * ((N + 31) // 32) * ((K + 15) // 16) * 1024 + (N + 31) // 32 * 128 + 16
    buf = torch.zeros(size, dtype=torch.uint8, device=dev)
    tw, tb = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    nat.check(lib.rg_pack_linear(tw.data_ptr(), tb.data_ptr(), K, N, fmt, buf.data_ptr(),
                                 nat.stream_ptr(dev)), 'rg_pack_linear')
    torch.cuda.synchronize()
    p0, p1, bias, (ds, sc, s) = _unpack_h2(buf, K, N, chain_fmt)
    wc, bc = w, b
    if centre:   # the pack's float32 centring: a sequential sum over the outputs
        cs = np.zeros(K, np.float32)
        for o in range(N):
            cs = cs + w[o]
        wc = w - cs / np.float32(N)
        bs = np.float32(0)
        for o in range(N):
            bs = bs + b[o]
        bc = b - bs / np.float32(N)
    m = float(np.abs(wc).max())
    assert s == h2_scale_exp(m) and ds == 2.0 ** -s and sc == 2.0 ** s
    if m > 0:
        assert 2.0 ** 12 <= m * 2.0 ** s < 2.0 ** 13
    back = (p0 + p1) * 2.0 ** -s
    tol = 2.0 ** -21 * np.abs(wc.astype(np.float64)) + 2.0 ** -24 * 2.0 ** -s
    assert np.all(np.abs(back - wc.astype(np.float64)) <= tol)
    assert np.array_equal(bias.astype(np.float64), bc.astype(np.float64) * 2.0 ** s)


# ------------------------------------------------------------------ the chains
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


@pytest.fixture(scope='module')
def trained(cuda_device):
    """The trained checkpoint's fp32 plans (packed once for the module)."""
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    name = 'model_trained_N50'
    m = Model_Training(model_cfg(name), cuda_device)
    m.load_state_dict(model_state_dict(name))
    pred = m.to(cuda_device).pred.eval().requires_grad_(False)
    return pred, pred.plans('fp32')


def _is_h2(plan):
    from graph_neural_network_for_radar_perception_amd import _native as nat
    return all(plan._x3[i].flags & nat.RG_LAYER_H2 for i in range(len(plan.specs)))


@pytest.mark.parametrize('R', [1, 33, 3001])
def test_h2_every_chain(cuda_device, trained, R):
    """Every chain of the shipped architecture under 'h2' over a single row, a partial second
    tile and many tiles: against a float64 evaluation at the fp32 bound, two calls
    bit-identical, rows_dev < rows leaves the tail untouched; and the link head's per-node
    first layer (RG_IN_PAIRPRE) against the same float64 pair chain."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    dev = cuda_device
    pred, plans = trained
    g = torch.Generator(device='cpu').manual_seed(100 + R)

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
    keep = R // 2
    for plan, kw in cases:
        mode = kw.get('mode', nat.IN_DENSE)
        outs = []
        for _ in range(2):
            out = torch.full((R, plan.out_dim), float('nan'), device=dev)
            plan(R, out, **kw)
            assert plan.x3_ok.get(mode), 'x3 chain kernel not used'
            outs.append(out)
        assert _is_h2(plan)
        xin = kw['in0'][idx0.long()] + kw['in0'][idx1.long()] if mode == nat.IN_PAIRADD else kw['in0']
        assert torch.isfinite(outs[0]).all()
        torch.testing.assert_close(outs[0], _torch_chain64(plan, xin).float(), **FP32_TOL)
        assert torch.equal(outs[0], outs[1])
        out = torch.full((R, plan.out_dim), 7.0, device=dev)
        plan(R, out, rows_dev=torch.tensor([keep], dtype=torch.int32, device=dev), **kw)
        assert torch.equal(out[:keep], outs[0][:keep])
        assert bool((out[keep:] == 7.0).all())
    # RG_IN_PAIRPRE: t = stem -> W0 per node, the pairs from t_i + t_j + b0
    link = torch.full((R, plans.link_pair.out_dim), float('nan'), device=dev)
    graph = types.SimpleNamespace(n_pairs_dev=torch.tensor([R], dtype=torch.int32, device=dev),
                                  pair_src=idx0, pair_dst=idx1)
    assert plans.link_pairs_pre(R, x64, 64, R, link, graph)
    stem = _torch_chain64(plans.link_node, x64).float() if plans.link_node is not None else x64
    ref = _torch_chain64(plans.link_pair, stem[idx0.long()].double() + stem[idx1.long()].double())
    torch.testing.assert_close(link, ref.float(), **FP32_TOL)


def test_h2_terms_switch_repacks(cuda_device, trained, monkeypatch):
    """engine.X3_TERMS selects the scheme of a chain already packed: 'b3' repacks it as
    RG_PACK_X3, both schemes agree at the fp32 bound, another value is an error."""
    from graph_neural_network_for_radar_perception_amd import engine
    dev = cuda_device
    plan = trained[1].node_head
    x = torch.randn(70, 64, device=dev)
    outs = {}
    for terms in ('h2', 'b3', 'h2'):
        monkeypatch.setattr(engine, 'X3_TERMS', terms)
        out = torch.empty(70, plan.out_dim, device=dev)
        plan(70, out, x, 64)
        assert plan.x3_ok.get(0) and _is_h2(plan) == (terms == 'h2')
        outs.setdefault(terms, out)
        assert torch.equal(outs[terms], out)
    torch.testing.assert_close(outs['h2'], outs['b3'], **FP32_TOL)
    monkeypatch.setattr(engine, 'X3_TERMS', 'f8')
    with pytest.raises(ValueError):
        plan(70, out, x, 64)


def test_h2_mixed_magnitudes_and_overflow(cuda_device, trained):
    """Columns of 1e-4, 1 and 3e3 in one row: the encoders (un-normalised first layer) and a
    bare Linear against float64 at the fp32 bound.  A row holding only the 1e-4 columns keeps
    them: its bare-Linear output is right to the arithmetic's absolute floor, 2^-24 sum |w|
    (a residue below fp16's normal range rounds to a 2^-24 quantum; dropping the columns
    would miss by ~1e-4 |w|).  A row with an input of 1e6 -- past the fp16 domain -- comes back
    non-finite, and its neighbours are untouched."""
    from graph_neural_network_for_radar_perception_amd import engine
    dev = cuda_device
    _, plans = trained
    g = torch.Generator(device='cpu').manual_seed(9)
    R = 40
    for plan, w in ((plans.node_enc, 6), (plans.edge_enc, 7)):
        x = torch.randn(R, w, generator=g)
        x[:, 0:2] *= 1e-4
        x[:, 4:w] *= 3e3
        x = x.to(dev)
        out = torch.full((R, plan.out_dim), float('nan'), device=dev)
        plan(R, out, x, w)
        assert plan.x3_ok.get(0) and _is_h2(plan)
        torch.testing.assert_close(out, _torch_chain64(plan, x).float(), **FP32_TOL)
        xb = x.clone()
        xb[17, 1] = 1e6
        outb = torch.full((R, plan.out_dim), float('nan'), device=dev)
        plan(R, outb, xb, w)
        assert not torch.isfinite(outb[17]).any()
        keep = torch.arange(R, device=dev) != 17
        assert torch.equal(outb[keep], out[keep])
    W = (torch.randn(64, 64, generator=g) * 0.2).to(dev)
    bare = engine.ChainPlan([engine.LayerSpec(W, None, None, None, 'none')], 'fp32', dev)
    x = torch.randn(R, 64, generator=g)
    x[:, 0:20] *= 1e-4
    x[:, 40:64] *= 3e3
    x[3, 20:] = 0          # rows of tiny values only
    x[4, 20:] = 0
    x = x.to(dev)
    out = torch.full((R, 64), float('nan'), device=dev)
    bare(R, out, x, 64)
    assert bare.x3_ok.get(0) and _is_h2(bare)
    ref = _torch_chain64(bare, x)
    torch.testing.assert_close(out, ref.float(), **FP32_TOL)
    floor = 2.0 ** -24 * float(W.abs().sum(1).max())
    tiny = (out[3:5].double() - ref[3:5]).abs().max()
    assert float(ref[3:5].abs().max()) > 100 * floor      # the signal stands far above the floor
    assert float(tiny) <= floor
    xb = x.clone()
    xb[8, 50] = 1e6
    outb = torch.full((R, 64), float('nan'), device=dev)
    bare(R, outb, xb, 64)
    assert not torch.isfinite(outb[8]).any()
    keep = torch.arange(R, device=dev) != 8
    assert torch.equal(outb[keep], out[keep])


# ------------------------------------------------------------------ the whole model
@pytest.mark.parametrize('name', ['model_trained_N50', 'model_trained_N500'])
def test_h2_full_model_matches_reference(cuda_device, name):
    """The trained model with its chains under 'h2' against the reference's own outputs
    (tests/golden) at 1e-4."""
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    d = golden(name)
    m = Model_Training(model_cfg(name), dev)
    m.load_state_dict(model_state_dict(name))
    pred = m.to(dev).pred.eval().requires_grad_(False)
    pred.compute_dtype = 'fp32'
    ei = torch.from_numpy(d['edge_index'].astype(np.int64)).to(dev)
    n = int(d['n'])
    adj = torch.zeros((n, n), dtype=torch.bool, device=dev)
    adj[ei[0], ei[1]] = True
    with torch.no_grad():
        out = pred(torch.from_numpy(d['node_features']).to(dev),
                   torch.from_numpy(d['edge_features']).to(dev), ei, adj,
                   [c.to(dev) for c in cluster_lists(d)])
    for got, key in zip(out, ('node_cls', 'node_reg', 'link_cls', 'obj_cls')):
        np.testing.assert_allclose(got.cpu().numpy(), d[key], err_msg=key, **FP32_TOL)
    plans = pred.plans('fp32')
    for c in (plans.node_enc, plans.edge_enc, plans.node_head, plans.offset_head, plans.cls_head):
        assert any(c.x3_ok.values()) and _is_h2(c), 'h2 chain not used'
    assert plans.link_pair._x3 is not None and _is_h2(plans.link_pair)
