"""The fused fp32 conv layer under the 'h2' term scheme (conv_x3.hip), emulated on the CPU in
the structure the kernels compute it in, and the host's refusal of mixed schemes.  No GPU.

The emulation: msg0 centred over its outputs and cut into P | Q (the x_i / x_j columns, with
the bias) and W_e (the edge columns), each Linear in the h2 arithmetic with its OWN power-of-two
scale (tests/test_h2_emulation.py's _H2Linear); layer 1's accumulator starts as P[dst] + Q[src]
in the units of W_e's scale (exact) and W_e e's three products accumulate onto it; msg1; the sum
in edge order; upd on cat(x, agg); the residual.  Its error against the float64 oracle conv
block reads <= T_CONV of the float32 oracle's, and each mutant -- P | Q one power of two off
against W_e e, a1 w0 dropped, residues flushed -- >= 3 T_CONV: the figure the GPU tests of
tests/test_gpu_conv_terms.py hold the kernels to separates right from wrong.

One case needs a threshold of its own.  With msg0's x columns times 2^7 and its edge columns
times 2^-9 ('x_up_e_down'), P + Q is 2^16 times W_e e and the channel normalisation that
follows is invariant to the scale of its input: P | Q doubled changes the layer's output by
only 8.0 (rms) / 6.4 (max) times the float32 oracle's error, where every other case and mutant
reads 29 or more (the correct arithmetic: 0.77 .. 1.05).  That case is therefore held to
T = 2.5 <= 8.0 / 3 here and on the GPU (T_CASE).
"""
import ctypes
import functools

import pytest
import torch

from oracle import gnn_forward_ref
from test_chain_error_budget import T_DEFAULT, _MutantH2, dense_inputs, error_ratios

T_CONV = T_DEFAULT
C = 64
P0 = 'pass_messages.conv_blk.0'
MUTANTS = ('pq_shift', 'drop_a1w0', 'flush')
# msg0's (x columns, edge columns) factors of the unequal-scale cases
SCALINGS = {'equal': (0, 0), 'x_down_e_up': (-9, 7), 'x_up_e_down': (7, -9)}
# the threshold of a scaling whose mildest mutant reads below 3 T_CONV (the module docstring)
T_CASE = {'equal': T_CONV, 'x_down_e_up': T_CONV, 'x_up_e_down': 2.5}


def conv_model(aggr, scaling='equal', blocks=1, device='cpu'):
    """The model of the conv-layer tests (one or two 64-channel blocks, freshly initialised,
    seed 12); msg0's x and edge columns of every block times 2^(SCALINGS[scaling])."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    cfg = default_config(graph_convolution_stem_channels=[64] * blocks, aggregation=aggr,
                         k_number_nearest_points=10)
    torch.manual_seed(12)
    m = Model_Training(cfg, device).to(device).eval().requires_grad_(False)
    sx, se = SCALINGS[scaling]
    with torch.no_grad():
        for blk in m.pred.pass_messages.conv_blk:
            w = blk.msg[0].block[0].weight
            w[:, :2 * C] *= 2.0 ** sx
            w[:, 2 * C:] *= 2.0 ** se
    return m, cfg


def oracle_conv(m, cfg, x, e, ei, dtype, blocks=1):
    sd = {k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items()}
    ctx = gnn_forward_ref._Ctx(sd, cfg)
    h = x.cpu().to(dtype)
    with torch.no_grad():
        for b in range(blocks):
            h = gnn_forward_ref.conv_block(ctx, f'pass_messages.conv_blk.{b}', h, e.cpu().to(dtype), ei)
    return h


def _norm_act(h, mu, std):
    h = (h - h.mean(1, keepdim=True)) / (h.std(1, keepdim=True) + 1e-5) * std + mu
    return torch.nn.functional.leaky_relu(h, 0.01)


def emulated_conv(m, x, e, ei, aggr, mutant=None):
    """One conv block as conv_x3.hip computes it under h2 (float32 tensors, CPU)."""
    sd = {k[len('pred.' + P0) + 1:]: v.detach().cpu().float() for k, v in m.state_dict().items()
          if k.startswith('pred.' + P0)}
    emu = _MutantH2(None if mutant in (None, 'pq_shift') else mutant)
    W, b = sd['msg.0.block.0.weight'], sd['msg.0.block.0.bias']
    Wc, bc = W - W.mean(0, keepdim=True), b - b.mean()
    src, dst = ei[0], ei[1]
    P = emu.linear(x, Wc[:, :C], bc)
    Q = emu.linear(x, Wc[:, C:2 * C])
    pq = P[dst] + Q[src]
    if mutant == 'pq_shift':
        pq = pq * 2.0
    # _H2Linear.linear starts its accumulator at `bias` times the image's scale: here a row
    # per edge, (P + Q) 2^(s_e)
    h = _norm_act(emu.linear(e, Wc[:, 2 * C:], pq), sd['msg.0.block.1.mu'], sd['msg.0.block.1.std'])
    msg = _norm_act(emu.linear(h, sd['msg.1.block.0.weight'], sd['msg.1.block.0.bias']),
                    sd['msg.1.block.1.mu'], sd['msg.1.block.1.std'])
    agg = torch.zeros(x.shape[0], C).index_add_(0, dst, msg)
    if aggr == 'mean':
        deg = torch.zeros(x.shape[0]).index_add_(0, dst, torch.ones(dst.shape[0]))
        agg = agg / deg.clamp(min=1)[:, None]
    u = _norm_act(emu.linear(torch.cat((x, agg), 1), sd['upd.0.block.0.weight'],
                             sd['upd.0.block.0.bias']),
                  sd['upd.0.block.1.mu'], sd['upd.0.block.1.std'])
    return x + u, emu.max_act


def _inputs(n=600, k=10):
    g = torch.Generator(device='cpu').manual_seed(3)
    dst = torch.arange(n).repeat_interleave(k)
    src = (dst + 1 + torch.randint(0, n - 1, (n * k,), generator=g)) % n
    return dense_inputs(n, C, 1), dense_inputs(n * k, C, 2), torch.stack((src, dst))


@functools.lru_cache(maxsize=None)
def emulated_ratios(aggr, scaling):
    """{None | mutant: (rms, max)} of the emulated layer's error over the float32 oracle's."""
    m, cfg = conv_model(aggr, scaling)
    x, e, ei = _inputs()
    ref64 = oracle_conv(m, cfg, x, e, ei, torch.float64)
    f32 = oracle_conv(m, cfg, x, e, ei, torch.float32)
    out = {}
    with torch.no_grad():
        for mu in (None,) + MUTANTS:
            y, top = emulated_conv(m, x, e, ei, aggr, mu)
            if mu is None:
                assert top < 2.0 ** 15      # the h2 domain, the aggregate included
            out[mu] = error_ratios(y, f32, ref64)
    # the float32 oracle itself, in units of the project's fp32 bound
    out['f32'] = float(((f32.double() - ref64).abs() / (1e-4 + 1e-4 * ref64.abs())).max())
    return out


cases = pytest.mark.parametrize('aggr,scaling', [('add', 'equal'), ('mean', 'equal'),
                                                 ('add', 'x_down_e_up'), ('add', 'x_up_e_down')])


@cases
def test_emulated_h2_conv_is_f32_class(aggr, scaling):
    r = emulated_ratios(aggr, scaling)
    print(f'{aggr} / {scaling}: h2 conv / f32 error  rms {r[None][0]:.3f}  max {r[None][1]:.3f}')
    assert max(r[None]) <= T_CASE[scaling]


@cases
def test_f32_oracle_stays_f32_class_on_these_weights(aggr, scaling):
    """The float32 oracle against the float64 one within half the 1e-4 bound -- also with
    msg0's x and edge columns 2^16 apart, the GPU file's unequal-scale cases."""
    r = emulated_ratios(aggr, scaling)
    print(f'{aggr} / {scaling}: f32 oracle error / (1e-4 + 1e-4 |ref|) = {r["f32"]:.4f}')
    assert r['f32'] <= 0.5


@pytest.mark.parametrize('mutant', MUTANTS)
@cases
def test_conv_mutant_is_caught(aggr, scaling, mutant):
    rms, mx = emulated_ratios(aggr, scaling)[mutant]
    print(f'{aggr} / {scaling} / {mutant}: error over f32  rms {rms:.1f}  max {mx:.1f}')
    assert max(rms, mx) >= 3 * T_CASE[scaling]


# ------------------------------------------------------------------ the host's refusal
_FAKE = ctypes.create_string_buffer(256)   # host memory: never read, a launch would fault


def _layers(nat, h2_flags):
    """rg_conv_layer_x3_for descriptors of the right shapes over fake images: W_e, msg1, upd,
    then next_pq and next_we; RG_LAYER_H2 where h2_flags says."""
    dims = ((64, 128), (128, 64), (128, 64), (64, 256), (64, 128))
    arr = (nat.rg_layer * 5)()
    fake = ctypes.addressof(_FAKE)
    for d, (i, o), h2 in zip(arr, dims, h2_flags):
        d.w_packed, d.in_dim, d.out_dim = fake, i, o
        d.flags = nat.RG_LAYER_CENTERED | (nat.RG_LAYER_H2 if h2 else 0)
        if o != 256:
            d.norm_mu = d.norm_std = fake
            d.act = nat.ACT['leakyrelu']
    return arr, fake


@pytest.mark.parametrize('h2_flags', [(1, 0, 0, 0, 0), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1),
                                      (1, 1, 1, 1, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)])
def test_mixed_schemes_are_refused_before_any_launch(h2_flags):
    """A conv layer whose images (next_pq and next_we included) mix RG_PACK_H2 and RG_PACK_X3
    is RG_ERR_ARG; the pointers are not device memory, so a launch would not come back."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    lib = nat.lib()
    arr, fake = _layers(nat, h2_flags)
    ws = lib.rg_conv_layer_x3_workspace_size(64)
    rc = lib.rg_conv_layer_x3_for(arr, ctypes.byref(arr[3]), ctypes.byref(arr[4]), nat.REDUCE['add'],
                                  fake, 64, fake, 64, fake, fake, fake, fake, 64, fake + 64, 64,
                                  fake + 128, None, fake, ws, None)
    assert rc == 1, rc      # RG_ERR_ARG
    assert b'RG_LAYER_H2' in lib.rg_last_error()


def test_h2_projection_needs_its_w_e_image():
    """rg_conv_proj_x3 (no W_e image) refuses an h2 projection, and rg_conv_proj_x3_for a W_e
    image of the other scheme, with RG_ERR_ARG; an h2 next_pq without next_we likewise."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    lib = nat.lib()
    arr, fake = _layers(nat, (1, 1, 1, 1, 1))
    assert lib.rg_conv_proj_x3(ctypes.byref(arr[3]), fake, 64, 64, fake, None) == 1
    b3, _ = _layers(nat, (0, 0, 0, 0, 0))
    assert lib.rg_conv_proj_x3_for(ctypes.byref(arr[3]), b3, fake, 64, 64, fake, None) == 1
    assert lib.rg_conv_proj_x3_for(ctypes.byref(b3[3]), arr, fake, 64, 64, fake, None) == 1
    ws = lib.rg_conv_layer_x3_workspace_size(64)
    rc = lib.rg_conv_layer_x3_for(arr, ctypes.byref(arr[3]), None, nat.REDUCE['add'], fake, 64,
                                  fake, 64, fake, fake, fake, fake, 64, fake + 64, 64, fake + 128,
                                  None, fake, ws, None)
    assert rc == 1, rc


def test_conv_plan_follows_x3_terms(monkeypatch):
    """ConvPlan.fused_fmts: the five images all RG_PACK_H2 under 'h2', all RG_PACK_X3 under 'b3',
    centred alike; any other engine.X3_TERMS is the chains' ValueError."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd import engine
    cv = engine.ConvPlan.__new__(engine.ConvPlan)
    cv.f32_arith = 'x3'
    X3, H2, CEN = nat.RG_PACK_X3, nat.RG_PACK_H2, nat.RG_PACK_CENTERED
    cv._fused_fmts = (nat.RG_PACK_FAST_IN | X3, nat.RG_PACK_FAST_CHAIN | X3 | CEN,
                      nat.RG_PACK_FAST_IN | X3 | CEN, nat.RG_PACK_FAST_IN | X3,
                      nat.RG_PACK_FAST_CHAIN | X3)
    monkeypatch.setattr(engine, 'X3_TERMS', 'b3')
    assert cv.fused_fmts == cv._fused_fmts
    monkeypatch.setattr(engine, 'X3_TERMS', 'h2')
    assert cv.fused_fmts == tuple((f ^ X3) | H2 for f in cv._fused_fmts)
    monkeypatch.setattr(engine, 'X3_TERMS', 'x4')
    with pytest.raises(ValueError, match="engine.X3_TERMS must be 'h2' or 'b3'"):
        cv.fused_fmts
