"""The 16-bit kernels' discriminating check, on the CPU: a rounding-point emulation.  No GPU.

The bf16 / fp16 chain kernels (chain_fast_impl.h, the 16-bit path of mlp_chain.hip) and the
fused conv layer (conv_fused_impl.h) are nearly deterministic functions of the places where they
round to 16 bits.  emulate_chain / emulate_conv round (to nearest even) exactly there and sum in
`acc_dtype`; tests/test_gpu_half_kernels.py compares every kernel with them.  This file holds
the emulation, the input recipes, the metrics, the bounds of the GPU check and the mutants, and
proves on the CPU that the bounds separate a right kernel from a subtly wrong one.

Rounding points, as read from the kernels
  fast chains (chain_fast_impl.h)
    * weights: a normalised layer is packed RG_PACK_CENTERED -- W - mean_o(W) per input column
      (pack.hip column_mean: one sequential f32 sum over the outputs, one division), THEN
      rounded; its bias is centred the same way and stays f32.  Other layers: W rounded.
    * a float32 dense input (the encoders, <= 8 features) whose un-normalised LeakyReLU first
      layer is tile-fused (run_chain01, pre_scaled_l0) is multiplied by LEAKY_PRE = 0.505f and
      then rounded, round(0.505 x); the layer's bias is multiplied by 0.505f in f32.
    * 16-bit inputs are used as they are; GATHER3 and CONCAT2 concatenate 16-bit rows; a
      PAIRADD input is never rounded as a sum -- the MFMAs add W x_i + W x_j (RG_PAIR_SPLIT).
    * a centred normalised layer takes no mean: ss = sum y^2, inv = 1 / (sqrt(ss (1/(N-1)))
      + 1e-5), and with LeakyReLU y' = fma(y, 0.505 (std inv), 0.505 mu), out = fma(|y'|,
      0.495/0.505, y') (channel_norm_leaky_centered); an un-normalised LeakyReLU is
      max(y, 0.01 y); the last layer of the heads is a bare Linear.
    * activations are rounded after normalisation and LeakyReLU, between layers (pack_next).
    * fp16 only: where a LeakyReLU's |y'| C + y' (or the input's 0.505 x) feeds nothing but the
      conversion, the compiler emits ONE v_fma_mixlo_f16 / v_fma_mixhi_f16 -- the exact
      multiply-add rounded once to fp16, not first to f32.  That is every rounding between
      layers, the prescaled input and the encoders' plain output epilogue; the general
      store_out (f32 value, then v_cvt) and every bf16 conversion round twice.  pack_once
      emulates the single rounding.  (Found by the first GPU measurement: 5 of 100 003
      edge-encoder rows stood 3.5 .. 15 spacings off in 34 .. 51 channels although 61 valid
      evaluations of the emulation agreed on them; in each, f32(0.505 x) of one input was an
      exact fp16 tie, and flipping that one rounding reproduced the kernel's row bit for bit.
      The emulation was corrected, not the kernel: the single rounding is the more exact.)
      This rounding point is a choice of the compiler's code generation, not of the source:
      a compiler that keeps the f32 multiply-add and a separate v_cvt_f16_f32 rounds twice,
      and the 100 003-row fp16 edge encoder then reads ~15 spacings (bound 12.6) with no kernel
      fault.  A failure of that shape points at code generation: count v_fma_mixlo_f16 /
      v_fma_mixhi_f16 in the fp16 kernels' assembly before suspecting the kernel.
    * the residual is added in f32 before the last rounding; the output is f32 or 16-bit.
  generic 16-bit chain (mlp_chain.hip)
    * weights rounded as they are (no centring), bias f32; every input is rounded into the
      slab -- a float32 input as x, a PAIRADD input as round(x_i + x_j) of an f32 sum.
    * channel_normalization with its mean pass: mean = sum / N, std = sqrt(sum (y - mean)^2 /
      (N - 1)), std_p ((y - mean) (1 / (std + 1e-5))) + mu, LeakyReLU max(y, 0.01 y).
    * the same roundings between layers, residual in f32, output f32 or 16-bit.
  fused conv layer (conv_fused_impl.h), all three layers centred
    * P = W0[:, :64] x[node] + b0 per node, kept in f32 (LDS).
    * per edge P[dst] + W0[:, 64:] [x[src], e], normalisation + LeakyReLU, rounded; the second
      message layer, normalisation + LeakyReLU, rounded: the message (fp16: both single
      roundings of the LeakyReLU's multiply-add, as above).
    * messages summed in f32 per destination (CSR order; an MFMA against a one-hot matrix);
      'mean' divides by max(deg, 1) in f32 (correctly rounded); rounded.
    * the update layer on [x, agg], normalisation + LeakyReLU; + x in f32; rounded.

Metrics (readings) of `out` against the emulation `emu`, per element in spacings of the 16-bit
type at max(|emu[i, c]|, rms of emu row i) -- the row rms keeps cancelled outputs near zero
from inflating the count: the share of elements that differ, the largest number of differing
channels in one row, the largest distance; and as a drift check error_ratios(out, emu, ref64),
ref64 the same operations in float64 with no rounding between layers.  An element of a 16-bit
output differs when it is not equal; an element of a float32 output (the heads' logits) when
it is more than 1/16 of a spacing away (the f32 summation orders of two right evaluations differ
by 2^-13 spacings or less; a flipped rounding one layer up moves a logit by a weight times a
spacing).

Noise floor (printed by test_chain_noise_floor / test_conv_noise_floor): two valid evaluations
of the emulation -- float32 against float64 sums, and float32 with every Linear's K sum permuted
(conftest.permuted_linear_sums) -- over 3001 rows of every chain and both weight sets, and on
the hub graph.  Worst readings (share / channels in a row / distance):

    chain bf16  0.0027 / 42 / 2.0      chain fp16  0.029 / 46 / 6.0
    conv  bf16  0.0004 /  2 / 0.12     conv  fp16  0.0059 / 8 / 1.0

(the conv layer and the one-layer chains are well under 1 %; the four- and five-layer chains in
fp16 reach 1 .. 3 %: a flipped rounding in an early layer moves every channel of that row a
little, and each later rounding may follow it -- hence few rows with many channels, each 1 to a
few spacings away).

Bounds.  BOUNDS holds, per kind (chain / conv) and type, 1.5 x the worst reading of the MI355X
kernels against the emulation (float32 sums) over three input seeds, both weight sets, fast and
generic kernels and every conv schedule (profiles/half_emulation.jsonl); the 1.5 covers what
the kernels' own f32 arithmetic does differently from the emulation's (v_rcp / v_sqrt in
inv_std_bf16, fused multiply-adds, the MFMA summation order), which flips a rounding only
rarely.  Measured worst (share / channels in a row / distance / drift ratio; the share over the
runs of SMALL_NUMEL = 4096 elements or more -- the 3001- and 100 003-row chains, the conv
graphs -- rows and distance over every run):

    chain bf16  0.0030 / 40 / 4.19 / 1.034     chain fp16  0.0263 / 45 / 8.42 / 1.129
    conv  bf16  0.0013 /  4 / 1.0  / 1.002     conv  fp16  0.0040 / 11 / 1.0  / 1.000

-- the kernels stand at the CPU noise floor, and no kernel fault was found.  (Before the fp16
single roundings were emulated the fp16 readings were 0.0273 / 51 / 15.0 for the chains and
0.0064 / 11 / 1.0 for the conv layer.)  The fp16 chains' row bound (67 of 64 channels) decides
nothing: share and distance do.  A valid evaluation must never read as a mutant: the noise floor
stays below 3 x every bound (asserted).

Small outputs.  A share is a rate, and the 1- and 33-row runs have 2 .. 2112 elements: there the
nominal share bound is a handful of elements or less than one, while one flipped early rounding
takes a row's channels with it.  Below SMALL_NUMEL elements `within` therefore holds the NUMBER
of differing elements to ceil(share bound x elements) + min(row bound, output width): the
bound's own expectation plus one more row's worth, nothing kind-wide.  Readings of the
committed profile above the nominal share, all inside that count: offset_head / random / fp16 /
33 rows 3 of 66 elements (0.045, allowed 5), edge_enc / random / fp16 / 1 row 5 of 64 (0.078),
cls_stem / trained / bf16 / 33 rows 15 of 2112 (0.0071); edge_enc / random / fp16 / 33 rows
reads 0.034, above the measured worst of the large runs but inside the nominal bound.  That
count is NOT a third of any mutant's share (at 33 rows of a 2-wide head it is 5 of 66): on the
small runs the distance bound separates, and the sentinels, rows_dev and window checks are what
those sizes are for.  At SMALL_NUMEL elements and above, and for the conv layer's isolated rows
at any size, the nominal share holds with no allowance, and the GPU tests assert that share
against mutant_floor / 3.

Every mutant must read >= 3 x the bound on at least one of the first three metrics
(test_chain_mutant_is_caught: on at least half of the chain x weight-set cases;
test_conv_mutant_is_caught: on at least one aggregation x weight set); mutant_floor gives the
mildest caught reading per metric, and the GPU tests assert bound <= mutant_floor / 3 before
they assert a reading.  As the floor is taken over the readings that are already >= 3 x the
bound, that assertion holds by construction whenever any mutant is caught on the metric (it
fails only where a bound is raised past every mutant): it documents the margin, it does not
guard it.  The safeguard is the pair of mutant_is_caught tests, which fail when a bound is
raised until a listed fault passes.  mean by deg with no clamp is caught by finiteness.

Faults this check does not see.  Every listed mutant is caught somewhere, but not on every case
the GPU test runs (the tests print the whole table, "NOT SEEN" where a case misses):
  * random weights, node_head / link_pair / cls_head: the output layer of a freshly initialised
    classification head (w ~ 0.01, b = -log 99) scales every upstream fault to a few hundredths
    of a spacing of a logit that is all bias -- truncating packs, the k-step rounding, packed
    statistics and, in bf16, the biased std (on cls_head also the zero slope) pass there; the
    trained weights catch all of them.
  * packed statistics on the one-layer chains conv_upd and link_node in fp16 (3 .. 8 % of the
    elements, bound 3.9 %) and the k-step rounding on conv_upd / trained / fp16 (11 %): one
    normalisation only; caught on every deeper chain.
  * one dropped edge under 'mean' (hub: 1 of 200 messages, 0.5 % of the aggregate; 2 .. 3
    spacings of at most 10 channels), and at the hub with random weights under 'add'; one
    dropped edge of a degree-65 node with trained weights in bf16.  The same kernel code is
    caught under 'add' with trained weights (hub: 21 spacings, 33 channels) and with random weights
    (degree 65: 14 spacings, 38 channels).
  * aggregates packed per tile and P packed to 16 bits under 'mean' with trained weights in
    fp16: 0.9 and 1.1 % of the elements at 1 spacing, 3 x the bound is 1.8 %; caught under 'add'
    and with random weights (2.7 .. 12 %).
What the metrics cannot see by construction: a fault below one rounding of the last stored value
that also leaves every earlier rounding in place.
"""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import model_state_dict, permuted_linear_sums
from oracle import gnn_forward_ref as _ref
from test_chain_error_budget import dense_inputs, encoder_inputs, error_ratios

HALVES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
_MANT = {torch.bfloat16: 7, torch.float16: 10}       # explicit significand bits
_EMIN = {torch.bfloat16: -126, torch.float16: -14}   # exponent of the smallest normal
LEAKY_PRE = float(np.float32(0.505))
LEAKY_C = float(np.float32(0.495) / np.float32(0.505))
SLOPE = float(np.float32(0.01))
EPS = float(np.float32(1e-5))
F32_DIFF = 1.0 / 16     # a float32 output differs beyond this many spacings
R = 3001

METRICS = ('share', 'row', 'dist')
# 1.5 x the worst MI355X reading against the emulation (profiles/half_emulation.jsonl); 'T':
# the drift check's threshold, 1.5 x the worst error ratio (rms or max)
BOUNDS = {
    ('chain', 'bf16'): dict(share=0.00449, row=60, dist=6.27, T=1.55),
    ('chain', 'fp16'): dict(share=0.0394, row=67, dist=12.6, T=1.69),
    ('conv', 'bf16'): dict(share=0.00198, row=6, dist=1.5, T=1.50),
    ('conv', 'fp16'): dict(share=0.00594, row=16, dist=1.5, T=1.50),
}

# the fast chain kernel against the generic one, largest distance per chain (1.5 x measured):
# their weights are rounded differently (centred or not), so most elements differ at all --
# share 0.3 .. 0.97, up to 61 channels of a row -- and only how far they part is a property
# of the chain: least after one normalised layer, most where two outputs nearly cancel
FAST_GENERIC = {
    'bf16': dict(node_enc=52.5, edge_enc=37.3, conv_msg=78.0, conv_upd=4.5, node_head=8.03,
                 offset_head=310.0, link_node=10.5, link_pair=56.3, cls_stem=15.0, cls_head=3.96),
    'fp16': dict(node_enc=46.0, edge_enc=41.2, conv_msg=142.0, conv_upd=3.0, node_head=11.1,
                 offset_head=728.0, link_node=10.5, link_pair=33.0, cls_stem=13.5, cls_head=3.40),
}
SMALL_NUMEL = 4096      # below: the share is held as a count (within)

CHAIN_MUTANTS = ('trunc', 'kstep', 'stats_packed', 'biased', 'relu')
CONV_MUTANTS = ('drop_straddle', 'drop_hub', 'drop_small', 'agg_tile_packed', 'p_packed',
                'p_tile_first', 'mean_plus1')
# (mean by deg with no clamp is not a reading: it must make an isolated node non-finite,
# test_mean_without_clamp_is_not_finite)


# ------------------------------------------------------------------ rounding
def pack(t, half, trunc=False):
    """t rounded to `half` (to nearest even; trunc: toward zero), in t's dtype."""
    h = t.to(half)
    if trunc:
        over = h.to(t.dtype).abs() > t.abs()
        bits = h.view(torch.int16)
        h = torch.where(over, bits - 1, bits).view(half)     # one step toward zero
    return h.to(t.dtype)


def pack_once(v, half):
    """A float64 v rounded ONCE to `half` (torch converts float64 through float32, a second
    rounding): float32 rounded to odd first, which a following round to nearest even cannot
    tell from v.  Returns `half`."""
    assert v.dtype == torch.float64
    f = v.float()
    err = v - f.double()
    g = torch.nextafter(f, torch.where(err > 0, torch.full_like(f, math.inf),
                                       torch.full_like(f, -math.inf)))
    odd = (f.view(torch.int32) & 1) == 1
    return torch.where((err != 0) & ~odd, g, f).to(half)


def _fma(a, b, c):
    """a b + c with one rounding when the operands are float32 (through float64: the product
    is exact there); plain a b + c in float64."""
    if a.dtype == torch.float32:
        f = lambda v: v.double() if torch.is_tensor(v) else v     # noqa: E731
        return (f(a) * f(b) + f(c)).float()
    return a * b + c


def _linear(h, w, b):
    """oracle.gnn_forward_ref's F.linear, so conftest.permuted_linear_sums reorders the K sum."""
    return _ref.F.linear(h, w, b)


def half_weights(s, half, centred):
    """(W, b) of a layer as the pack writes them: float32 tensors, W of `half` values;
    centred: W - mean over the outputs per column and b - mean(b) first (sequential f32 sums)."""
    cache = s.__dict__.setdefault('_half_weights', {})
    key = (half, centred)
    if key not in cache:
        w = s.weight.detach().float().cpu()
        b = (s.bias.detach().float().cpu() if s.bias is not None
             else torch.zeros(w.shape[0]))
        if centred:
            cs, cb = torch.zeros_like(w[0]), torch.zeros(())
            for o in range(w.shape[0]):
                cs = cs + w[o]
                cb = cb + b[o]
            w = w - cs / float(w.shape[0])
            if s.bias is not None:
                b = b - cb / float(w.shape[0])
        cache[key] = (w.to(half).float(), b)
    return cache[key]


class _Ops:
    """The normalisation + activation of one kernel family in `acc`; mutant: a fault."""

    def __init__(self, half, acc, mutant=None, exact=False):
        self.half, self.acc, self.mutant, self.exact = half, acc, mutant, exact
        # fp16: a multiply-add whose only use is a conversion to fp16 is ONE instruction with
        # one rounding (v_fma_mixlo_f16 / v_fma_mixhi_f16); bf16 has none
        self.mix = half == torch.float16 and not exact and mutant != 'trunc'

    def pack(self, t):
        if self.exact:
            return t
        return pack(t, self.half, trunc=self.mutant == 'trunc')

    def _inv(self, y, n):
        ys = pack(y, self.half) if self.mutant == 'stats_packed' else y
        ss = (ys * ys).sum(1, keepdim=True)
        n1 = n if self.mutant == 'biased' else n - 1
        rn = torch.ones((), dtype=self.acc) / float(n1)
        return 1.0 / (torch.sqrt(ss * rn) + EPS)

    def leaky_pre(self, yp, fuse=False):
        """LeakyReLU of a prescaled y' = 0.505 y: |y'| C + y'; fuse: the result only feeds a
        pack, which in fp16 rounds |y'| C + y' once (returned already packed)."""
        if fuse and self.mix:
            out = pack_once(yp.double().abs() * LEAKY_C + yp.double(), self.half).to(self.acc)
        else:
            out = _fma(yp.abs(), LEAKY_C, yp)
        if self.mutant == 'relu':
            out = torch.where(yp > 0, out, torch.zeros_like(out))
        return out

    def leaky(self, y):
        if self.mutant == 'relu':
            return torch.where(y > 0, y, torch.zeros_like(y))
        return torch.maximum(y, y * SLOPE)

    def norm_centred(self, y, s, fuse=False):
        """A centred layer's channel_normalization (+ LeakyReLU) as the fast kernels run it."""
        mu, sd = s.mu.detach().cpu().to(self.acc), s.std.detach().cpu().to(self.acc)
        inv = self._inv(y, y.shape[1])
        if s.act == 'leakyrelu':
            return self.leaky_pre(_fma(y, LEAKY_PRE * (sd * inv), LEAKY_PRE * mu), fuse)
        assert s.act == 'none'
        return _fma(y, sd * inv, mu)

    def norm_generic(self, y, s):
        mu, sd = s.mu.detach().cpu().to(self.acc), s.std.detach().cpu().to(self.acc)
        n = y.shape[1]
        d = y - y.sum(1, keepdim=True) / float(n)
        ds = pack(d, self.half) if self.mutant == 'stats_packed' else d
        n1 = n if self.mutant == 'biased' else n - 1
        inv = 1.0 / (torch.sqrt((ds * ds).sum(1, keepdim=True) / float(n1)) + EPS)
        out = sd * (d * inv) + mu
        return self.leaky(out) if s.act == 'leakyrelu' else out


# ------------------------------------------------------------------ chains
def emulate_chain(specs, x, half, acc_dtype, mode='dense', idx0=None, idx1=None, in1=None,
                  in2=None, residual=None, out_half=True, kernel='fast', mutant=None,
                  exact=False):
    """eval_chain as the `kernel` ('fast' | 'generic') 16-bit chain computes it, on the CPU.

    x: float32 rows (a float32 dense input) or rows of `half`; mode 'dense' | 'gather3'
    (cat(x[idx0], x[idx1], in2)) | 'concat2' (cat(x, in1)) | 'pairadd' (x[idx0] + x[idx1]);
    residual: rows added in f32 before the last rounding; out_half: the output is rounded.
    Sums run in acc_dtype.  exact: no rounding between layers (ref64 with acc_dtype float64).
    Returns acc_dtype."""
    assert kernel in ('fast', 'generic') and (mutant is None or mutant in CHAIN_MUTANTS)
    fast = kernel == 'fast'
    op = _Ops(half, acc_dtype, mutant, exact)
    in_f32 = x.dtype == torch.float32
    assert in_f32 or x.dtype == half
    assert not in_f32 or mode == 'dense'
    xa = x.to(acc_dtype)
    L = len(specs)
    pre0 = (fast and in_f32 and L >= 2 and specs[0].mu is None and specs[0].act == 'leakyrelu')
    pair_split = fast and mode == 'pairadd'
    i0 = None if idx0 is None else idx0.long()
    i1 = None if idx1 is None else idx1.long()
    # the encoders' 16-bit rows leave through the plain epilogue (SPEC_PLAIN_OUT)
    plain_out = fast and in_f32 and out_half and residual is None and L >= 3
    if mode == 'dense':
        # (the input's rounding is the kernel's own: a mutant of the pack leaves it alone)
        if pre0 and half == torch.float16 and not exact:
            h = pack_once(x.double() * LEAKY_PRE, half).to(acc_dtype)    # v_fma_mixlo_f16
        else:
            h = pack(xa * LEAKY_PRE if pre0 else xa, half) if in_f32 else xa
    elif mode == 'gather3':
        h = torch.cat((xa[i0], xa[i1], in2.to(acc_dtype)), 1)
    elif mode == 'concat2':
        h = torch.cat((xa, in1.to(acc_dtype)), 1)
    else:
        assert mode == 'pairadd'
        h = torch.cat((xa[i0], xa[i1]), 1) if pair_split else pack(xa[i0] + xa[i1], half)
    kstep_layer = min(1, L - 1)
    for l, s in enumerate(specs):
        norm = s.mu is not None
        w, b = half_weights(s, half, fast and (norm or getattr(s, 'center', False)))
        w, b = w.to(acc_dtype), b.to(acc_dtype)
        if l == 0 and pair_split:
            w = torch.cat((w, w), 1)
        if l == 0 and pre0:
            b = b * LEAKY_PRE
        if mutant == 'kstep' and l == kstep_layer:
            y = b.expand(h.shape[0], -1)
            for k0 in range(0, w.shape[1], 16):
                y = pack(y + _linear(h[:, k0:k0 + 16], w[:, k0:k0 + 16], None), half)
        else:
            y = _linear(h, w, b)
        fuse = l + 1 < L or plain_out     # the activation's only use is a pack
        if norm:
            y = op.norm_centred(y, s, fuse) if fast else op.norm_generic(y, s)
        elif s.act == 'leakyrelu':
            y = op.leaky_pre(y, fuse) if (l == 0 and pre0) else op.leaky(y)
        else:
            assert s.act == 'none'
        if l + 1 < L:
            h = op.pack(y)
    if residual is not None:
        y = residual.to(acc_dtype) + y
    return op.pack(y) if out_half else y


def ref64_chain(specs, x, half, **kw):
    """The same operations in float64 on the same 16-bit-valued inputs and weights, with no
    rounding between layers."""
    kw.pop('mutant', None)
    return emulate_chain(specs, x, half, torch.float64, exact=True, **kw)


# ------------------------------------------------------------------ the fused conv layer
def conv_tiles(dst, seg_ptr):
    """(block, tile) of every CSR position under the plain schedule: 8-node runs, 32-edge tiles
    from the run's first edge."""
    blk = dst.long() // 8
    e0 = seg_ptr.long()[torch.clamp(blk * 8, max=seg_ptr.numel() - 1)]
    return blk, (torch.arange(dst.numel()) - e0) // 32


def emulate_conv(specs, x, e, src, dst, seg_ptr, aggr, half, acc_dtype, mutant=None,
                 exact=False):
    """One residual_graph_conv_block as rg_conv_layer_fused computes it.  specs: msg0, msg1, upd
    (LayerSpec-like); x [N, 64], e [E, 64] of `half`; src, dst [E] in destination-major order,
    seg_ptr [N + 1].  Returns acc_dtype [N, 64] (of `half` values unless exact)."""
    assert aggr in ('add', 'sum', 'mean') and (mutant is None or mutant in CONV_MUTANTS
                                               or mutant == 'mean_noclamp')
    op = _Ops(half, acc_dtype, None, exact)
    m0, m1, u = specs
    N, E, C = x.shape[0], src.numel(), 64
    src, dst, seg = src.long(), dst.long(), seg_ptr.long()
    deg = seg[1:] - seg[:-1]
    xa, ea = x.to(acc_dtype), e[:E].to(acc_dtype)
    (w0, b0), (w1, b1), (wu, bu) = [tuple(t.to(acc_dtype) for t in half_weights(s, half, True))
                                    for s in (m0, m1, u)]
    P = _linear(xa, w0[:, :C], b0)
    if mutant == 'p_packed':
        P = pack(P, half)
    blk, tile = conv_tiles(dst, seg)
    pdst = dst
    if mutant == 'p_tile_first' and E:
        key = blk * (E + 1) + tile
        first = torch.ones(E, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]
        start = torch.where(first, torch.arange(E), torch.zeros(E, dtype=torch.long))
        pdst = dst[torch.cummax(start, 0)[0]]     # the destination of the tile's first edge
    y = P[pdst] + _linear(torch.cat((xa[src], ea), 1), w0[:, C:], None)
    y = _linear(op.pack(op.norm_centred(y, m0, True)), w1, b1)
    msg = op.pack(op.norm_centred(y, m1, True))
    keep = torch.ones(E, dtype=torch.bool)
    if mutant == 'drop_straddle':
        for n in range(N):
            if deg[n] > 0 and tile[seg[n]] != tile[seg[n + 1] - 1]:
                keep[seg[n + 1] - 1] = False
    elif mutant in ('drop_hub', 'drop_small'):
        cand = deg if mutant == 'drop_hub' else torch.where(deg <= 65, deg, torch.zeros_like(deg))
        n = int(cand.argmax())
        keep[seg[n] + int(deg[n]) // 2] = False
    agg = torch.zeros(N, C, dtype=acc_dtype)
    if mutant == 'agg_tile_packed':
        key = blk * (E + 1) + tile
        for k in torch.unique_consecutive(key):
            part = torch.zeros(N, C, dtype=acc_dtype).index_add_(0, dst[key == k], msg[key == k])
            agg = pack(agg + part, half)
    else:
        agg.index_add_(0, dst[keep], msg[keep])
    if aggr == 'mean':
        cnt = deg if mutant == 'mean_noclamp' else torch.clamp(deg, min=1)
        if mutant == 'mean_plus1':
            cnt = deg + 1
        agg = agg / cnt.to(acc_dtype)[:, None]
    return update_rows(u, xa, op.pack(agg), half, acc_dtype, exact)


def update_rows(u, x, agg, half, acc_dtype, exact=False):
    """The update layer of the fused conv on [x, agg] (agg already of `half` values), + x."""
    op = _Ops(half, acc_dtype, None, exact)
    wu, bu = (t.to(acc_dtype) for t in half_weights(u, half, True))
    xa = x.to(acc_dtype)
    y = op.norm_centred(_linear(torch.cat((xa, agg.to(acc_dtype)), 1), wu, bu), u)
    return op.pack(xa + y)


def ref64_conv(specs, x, e, src, dst, seg_ptr, aggr, half):
    return emulate_conv(specs, x, e, src, dst, seg_ptr, aggr, half, torch.float64, exact=True)


# ------------------------------------------------------------------ metrics
def spacing(v, half):
    """The spacing of `half` at |v| (float64)."""
    a = v.double().abs()
    _, ex = torch.frexp(a)                              # |v| = m 2^ex, m in [0.5, 1)
    ex = torch.clamp(torch.where(a > 0, ex - 1, torch.full_like(ex, _EMIN[half])), min=_EMIN[half])
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - _MANT[half])


def distances(out, emu, half):
    """|out - emu| per element in spacings of `half` at max(|emu|, the row's rms)."""
    o, m = out.double(), emu.double()
    scale = torch.maximum(m.abs(), m.pow(2).mean(1, keepdim=True).sqrt())
    return (o - m).abs() / spacing(scale, half)


def readings(out, emu, half, out_half=True):
    """dict(share, row, dist) of out against emu; a non-finite element counts as infinitely far."""
    d = distances(out, emu, half)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    diff = d > (0.0 if out_half else F32_DIFF)
    return dict(share=float(diff.double().mean()), row=int(diff.sum(1).max()),
                dist=float(d.max()))


def share_bound(bound, numel, width, small=True):
    """The share `within` holds an output of numel elements, `width` channels wide, to: the
    nominal bound from SMALL_NUMEL elements on (and always with small=False); below, the count
    ceil(share bound x numel) + min(row bound, width) as a share (module docstring)."""
    if numel >= SMALL_NUMEL or not small:
        return bound['share']
    return (math.ceil(bound['share'] * numel) + min(bound['row'], width)) / numel


def within(rd, bound, numel, width, small=True):
    """Whether readings rd of an output of numel elements hold `bound`."""
    share = share_bound(bound, numel, width, small)
    return (rd['share'] * numel <= share * numel + 1e-6 and rd['row'] <= bound['row']
            and rd['dist'] <= bound['dist'])


# ------------------------------------------------------------------ models, chains, inputs
@functools.lru_cache(maxsize=None)
def cpu_model(weights, aggr='add'):
    """The yml architecture on the CPU: 'trained' (the checkpoint of model_trained_N50) or
    'random' (a fresh initialisation with its norm parameters moved off (0, 1)), as
    test_gpu_chain_x3.py's models."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    torch.manual_seed(77)
    m = Model_Training(default_config(aggregation=aggr), 'cpu')
    if weights == 'trained':
        m.load_state_dict(model_state_dict('model_trained_N50'))
    else:
        assert weights == 'random'
        g = torch.Generator(device='cpu').manual_seed(78)
        with torch.no_grad():
            for k, p in m.named_parameters():
                if k.endswith('.mu') or k.endswith('.std'):
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m.eval().requires_grad_(False)


# chain -> (input mode, float32 input, 16-bit output, residual = in0): how engine.forward_batched
# calls each ChainPlan of ModelPlans
CHAINS = {
    'node_enc': ('dense', True, True, False), 'edge_enc': ('dense', True, True, False),
    'conv_msg': ('gather3', False, True, False), 'conv_upd': ('concat2', False, True, True),
    'node_head': ('dense', False, False, False), 'offset_head': ('dense', False, False, False),
    'link_node': ('dense', False, True, False), 'link_pair': ('pairadd', False, False, False),
    'cls_stem': ('dense', False, True, False), 'cls_head': ('dense', False, False, False),
}


def chain_specs(pred):
    """{chain: LayerSpecs} of a Model_Inference, the lists engine.ModelPlans builds."""
    from graph_neural_network_for_radar_perception_amd.engine import specs_from_modules as sp
    pn, po, pl, pc = pred.predict_node, pred.predict_offset, pred.predict_link, pred.predict_class
    blk = pred.pass_messages.conv_blk[0]
    return {
        'node_enc': sp(list(pred.encode_node_feat.encoder)),
        'edge_enc': sp(list(pred.encode_edge_feat.encoder)),
        'conv_msg': sp(list(blk.msg)), 'conv_upd': sp(list(blk.upd)),
        'node_head': sp(list(pn.stem) + [pn.pred_cls.head[0], pn.pred_cls.head[1]]),
        'offset_head': sp(list(po.stem) + [po.pred_offsets.head[0], po.pred_offsets.head[1]]),
        'link_node': sp(list(pl.compute_edge.stem)),
        'link_pair': sp(list(pl.stem) + [pl.pred_cls.head[0], pl.pred_cls.head[1]]),
        'cls_stem': sp(list(pc.stem)),
        'cls_head': sp([pc.pred_cls.head[0], pc.pred_cls.head[1]]),
    }


def chain_inputs(chain, specs, rows, seed, half):
    """kwargs of emulate_chain / the kernel call for `rows` rows: x (float32 encoder_inputs for
    the encoders, else dense_inputs rounded to `half`), in1 / in2, idx0 / idx1 (int32, into the
    rows), residual.  fp16: |x| stays far below 2^15 (test_h2_domain_at_physical_limits)."""
    mode, in_f32, _, res = CHAINS[chain]
    g = torch.Generator(device='cpu').manual_seed(seed + 1000)
    idx = lambda: torch.randint(0, rows, (rows,), generator=g).to(torch.int32)   # noqa: E731
    kw = dict(mode=mode)
    if in_f32:
        kw['x'] = encoder_inputs(rows, specs[0].in_dim, seed)
    else:
        kw['x'] = dense_inputs(rows, 64, seed).to(half)
    if mode == 'gather3':
        kw.update(in2=dense_inputs(rows, 64, seed + 500).to(half), idx0=idx(), idx1=idx())
    elif mode == 'concat2':
        kw['in1'] = dense_inputs(rows, 64, seed + 500).to(half)
    elif mode == 'pairadd':
        kw.update(idx0=idx(), idx1=idx())
    if res:
        kw['residual'] = kw['x']
    assert float(kw['x'].abs().max()) < 2.0 ** 15
    return kw


def hub_graph(seed=0):
    """(edge_index int64 [2, E] in a shuffled order, N): 71 nodes with in-degrees 0, 1, 31, 32,
    33, 64, 65 and a hub of 200 (nodes 0..7), one whole 8-node run without edges (8..15), random
    degrees below 45, the last node isolated; sources uniform (a multigraph)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    N = 71
    deg = [0, 1, 31, 32, 33, 64, 65, 200] + [0] * 8 + \
        torch.randint(0, 45, (N - 17,), generator=g).tolist() + [0]
    if sum(deg) % 32 == 0:
        deg[16] += 1
    dst = torch.cat([torch.full((d,), n, dtype=torch.int64) for n, d in enumerate(deg)])
    src = torch.randint(0, N, (dst.numel(),), generator=g)
    p = torch.randperm(dst.numel(), generator=g)
    return torch.stack((src[p], dst[p])), N


def csr_by_dst(edge_index, n_nodes):
    """(src, dst, seg_ptr) destination-major, sources ascending per segment (DeviceGraph)."""
    src, dst = edge_index[0], edge_index[1]
    order = torch.argsort(dst * (n_nodes + 1) + src, stable=True)
    seg = torch.zeros(n_nodes + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.bincount(dst, minlength=n_nodes), 0)
    return src[order], dst[order], seg


def assert_hub_graph(seg_ptr, n_nodes):
    """The properties the conv tests rely on."""
    seg = seg_ptr.long().cpu()
    deg = (seg[1:] - seg[:-1]).tolist()
    E = int(seg[-1])
    assert 70 <= n_nodes <= 100 and n_nodes % 8 != 0 and E % 32 != 0
    assert {0, 1, 31, 32, 33, 64, 65, 200} <= set(deg)
    assert any(all(d == 0 for d in deg[8 * b:8 * b + 8]) for b in range(n_nodes // 8))
    assert deg[-1] == 0
    blk, tile = conv_tiles(torch.repeat_interleave(torch.arange(n_nodes), torch.tensor(deg)), seg)
    straddle = [n for n in range(n_nodes) if deg[n] and tile[seg[n]] != tile[seg[n + 1] - 1]]
    assert len(straddle) >= 8


def conv_inputs(n_nodes, n_edge_rows, seed, half):
    return (dense_inputs(n_nodes, 64, seed).to(half),
            dense_inputs(n_edge_rows, 64, seed + 500).to(half))


# ------------------------------------------------------------------ emulated readings
def _max_readings(rs):
    return {k: max(r[k] for r in rs) for k in METRICS}


@functools.lru_cache(maxsize=None)
def chain_readings(chain, weights, dtype):
    """{'noise': mutual readings of two valid evaluations, mutant: readings against the
    emulation} of the fast kernel's emulation on R rows."""
    half = HALVES[dtype]
    specs = chain_specs(cpu_model(weights).pred)[chain]
    oh = CHAINS[chain][2]
    kw = chain_inputs(chain, specs, R, 0, half)
    with torch.no_grad():
        emu = emulate_chain(specs, half=half, acc_dtype=torch.float32, out_half=oh, **kw)
        e64 = emulate_chain(specs, half=half, acc_dtype=torch.float64, out_half=oh, **kw)
        with permuted_linear_sums(3):
            per = emulate_chain(specs, half=half, acc_dtype=torch.float32, out_half=oh, **kw)
        out = {'noise': _max_readings([readings(e64, emu, half, oh), readings(per, emu, half, oh)])}
        for m in CHAIN_MUTANTS:
            out[m] = readings(emulate_chain(specs, half=half, acc_dtype=torch.float32,
                                            out_half=oh, mutant=m, **kw), emu, half, oh)
    return out


def _conv_case(weights, aggr, dtype):
    half = HALVES[dtype]
    blk = cpu_model(weights, aggr).pred.pass_messages.conv_blk[0]
    from graph_neural_network_for_radar_perception_amd.engine import specs_from_modules as sp
    specs = sp(list(blk.msg)) + sp(list(blk.upd))
    ei, N = hub_graph()
    src, dst, seg = csr_by_dst(ei, N)
    assert_hub_graph(seg, N)
    x, e = conv_inputs(N, src.numel(), 0, half)
    return specs, (x, e, src, dst, seg, aggr, half)


@functools.lru_cache(maxsize=None)
def conv_readings(weights, aggr, dtype):
    half = HALVES[dtype]
    specs, args = _conv_case(weights, aggr, dtype)
    with torch.no_grad():
        emu = emulate_conv(specs, *args, torch.float32)
        e64 = emulate_conv(specs, *args, torch.float64)
        with permuted_linear_sums(3):
            per = emulate_conv(specs, *args, torch.float32)
        out = {'noise': _max_readings([readings(e64, emu, half), readings(per, emu, half)])}
        for m in CONV_MUTANTS:
            if m == 'mean_plus1' and aggr != 'mean':
                continue
            out[m] = readings(emulate_conv(specs, *args, torch.float32, mutant=m), emu, half)
    return out


def _caught(rd, bound):
    return [k for k in METRICS if rd[k] >= 3 * bound[k] and rd[k] > 0]


@functools.lru_cache(maxsize=None)
def mutant_floor(kind, dtype):
    """{metric: the mildest reading among the mutants caught on that metric (>= 3 x its bound)}
    over both weight sets and every chain (kind 'chain') or both aggregations ('conv'); inf
    where no mutant is caught on the metric.  bound <= floor / 3 therefore holds by
    construction: the figure shows the margin, the mutant_is_caught tests guard it."""
    bound = BOUNDS[kind, dtype]
    if kind == 'chain':
        cases = [chain_readings(c, w, dtype) for c in CHAINS for w in ('trained', 'random')]
    else:
        cases = [conv_readings(w, a, dtype) for a in ('add', 'mean') for w in ('trained', 'random')]
    floor = {k: math.inf for k in METRICS}
    for case in cases:
        for m, rd in case.items():
            if m != 'noise':
                for k in _caught(rd, bound):
                    floor[k] = min(floor[k], rd[k])
    return floor


def _fmt(rd):
    return f"share {rd['share']:.5f}  row {rd['row']}  dist {rd['dist']:.2f}"


# ------------------------------------------------------------------ the tests
dtype_p = pytest.mark.parametrize('dtype', list(HALVES))
weights_p = pytest.mark.parametrize('weights', ['trained', 'random'])


def test_pack_rounds_to_nearest_even_and_truncates():
    for half in HALVES.values():
        one, sp1 = 1.0, 2.0 ** -_MANT[half]
        t = torch.tensor([one + 0.5 * sp1, one + 1.5 * sp1, -(one + 0.75 * sp1), one + sp1],
                         dtype=torch.float64)
        assert pack(t, half).tolist() == [one, one + 2 * sp1, -(one + sp1), one + sp1]
        assert pack(t, half, trunc=True).tolist() == [one, one + sp1, -one, one + sp1]
        assert float(spacing(torch.tensor(1.5), half)) == sp1
        assert float(spacing(torch.tensor(0.0), half)) == 2.0 ** (_EMIN[half] - _MANT[half])


@dtype_p
@weights_p
@pytest.mark.parametrize('chain', list(CHAINS))
def test_chain_noise_floor(chain, weights, dtype):
    """Two valid evaluations of the emulation (float64 sums; permuted K sums) against the
    float32 one never read as a mutant: below 3 x the bound on every metric."""
    rd = chain_readings(chain, weights, dtype)['noise']
    print(f'{chain} / {weights} / {dtype}: noise floor  {_fmt(rd)}')
    assert not _caught(rd, BOUNDS['chain', dtype]), rd


def _table(cases, mutant, bound):
    """Print a mutant's readings case by case; the cases that catch it."""
    hit = []
    for name, case in cases:
        if mutant in case:
            on = _caught(case[mutant], bound)
            print(f"{name} / {mutant}: {_fmt(case[mutant])}  ->  "
                  f"{'caught on ' + ', '.join(on) if on else 'NOT SEEN'}")
            if on:
                hit.append(name)
    return hit


@dtype_p
@pytest.mark.parametrize('mutant', CHAIN_MUTANTS)
def test_chain_mutant_is_caught(mutant, dtype):
    """One fault in the emulation reads >= 3 x the GPU bound on at least one metric, on at
    least half of the chain x weight-set cases the GPU test runs (the table of every case is
    printed; the module docstring names the cases that do not see it)."""
    cases = [(f'{c} / {w} / {dtype}', chain_readings(c, w, dtype))
             for c in CHAINS for w in ('trained', 'random')]
    hit = _table(cases, mutant, BOUNDS['chain', dtype])
    assert len(hit) >= len(cases) // 2, hit


def test_generic_emulation_differs_only_by_its_rounding_points():
    """The generic kernel's emulation against the fast one's on a 16-bit chain: other weights
    (uncentred) and another normalisation, the same function -- both within 16-bit rounding of
    one float64 evaluation, neither equal to the other."""
    half = torch.bfloat16
    specs = chain_specs(cpu_model('trained').pred)['node_head']
    kw = chain_inputs('node_head', specs, 257, 1, half)
    with torch.no_grad():
        a = emulate_chain(specs, half=half, acc_dtype=torch.float32, out_half=False, **kw)
        b = emulate_chain(specs, half=half, acc_dtype=torch.float32, out_half=False,
                          kernel='generic', **kw)
        from test_chain_error_budget import eval_chain
        ref = eval_chain(specs, kw['x'].double(), torch.float64)
    assert not torch.equal(a, b)
    for o in (a, b):
        err = (o.double() - ref).abs()
        assert float((err <= 0.05 + 0.05 * ref.abs()).double().mean()) >= 0.995


@dtype_p
@weights_p
@pytest.mark.parametrize('aggr', ['add', 'mean'])
def test_conv_noise_floor(aggr, weights, dtype):
    rd = conv_readings(weights, aggr, dtype)['noise']
    print(f'conv {aggr} / {weights} / {dtype}: noise floor  {_fmt(rd)}')
    assert not _caught(rd, BOUNDS['conv', dtype]), rd


@dtype_p
@pytest.mark.parametrize('mutant', CONV_MUTANTS)
def test_conv_mutant_is_caught(mutant, dtype):
    """One fault in the emulated conv layer reads >= 3 x the GPU bound on at least one metric
    in at least ONE of the four aggregation x weight-set cases of the hub graph -- no more is
    asserted: one dropped edge is caught only under 'add', at the hub with trained weights and
    at the degree-65 node with random ones (module docstring)."""
    cases = [(f'conv {a} / {w} / {dtype}', conv_readings(w, a, dtype))
             for a in ('add', 'mean') for w in ('trained', 'random')]
    hit = _table(cases, mutant, BOUNDS['conv', dtype])
    assert hit, 'no case catches it'


@dtype_p
def test_mean_without_clamp_is_not_finite(dtype):
    """mean by deg with no clamp: every isolated node's row is non-finite (0 / 0), which the
    GPU test's finiteness assertion and its infinite distance both see."""
    specs, args = _conv_case('trained', 'mean', dtype)
    seg = args[4]
    iso = (seg[1:] - seg[:-1]) == 0
    with torch.no_grad():
        bad = emulate_conv(specs, *args, torch.float32, mutant='mean_noclamp')
        emu = emulate_conv(specs, *args, torch.float32)
    assert int(iso.sum()) >= 10 and not torch.isfinite(bad[iso]).any()
    assert torch.isfinite(bad[~iso]).all() and torch.isfinite(emu).all()
    assert readings(bad, emu, HALVES[dtype])['dist'] == math.inf


@dtype_p
def test_isolated_rows_are_the_update_of_a_zero_aggregate(dtype):
    specs, args = _conv_case('trained', 'mean', dtype)
    x, seg, half = args[0], args[4], args[6]
    iso = (seg[1:] - seg[:-1]) == 0
    with torch.no_grad():
        emu = emulate_conv(specs, *args, torch.float32)
        want = update_rows(specs[2], x[iso], torch.zeros(int(iso.sum()), 64), half, torch.float32)
    assert torch.equal(emu[iso], want)


@pytest.mark.parametrize('kind', ['chain', 'conv'])
@dtype_p
def test_bounds_are_a_third_of_the_mutant_floor(kind, dtype):
    floor, bound = mutant_floor(kind, dtype), BOUNDS[kind, dtype]
    print(f'{kind} / {dtype}: bounds {bound}  mutant floor {floor}')
    assert any(math.isfinite(v) for v in floor.values())
    for k in METRICS:
        assert bound[k] <= floor[k] / 3


@dtype_p
def test_drift_reading_of_the_emulation_itself(dtype):
    """error_ratios(out, emu, ref64) of a valid evaluation is ~1 (both are one 16-bit rounding
    per layer from ref64); with truncating packs it is not."""
    half = HALVES[dtype]
    specs = chain_specs(cpu_model('trained').pred)['cls_stem']
    kw = chain_inputs('cls_stem', specs, R, 0, half)
    with torch.no_grad():
        emu = emulate_chain(specs, half=half, acc_dtype=torch.float32, **kw)
        r64 = ref64_chain(specs, half=half, **kw)
        with permuted_linear_sums(3):
            per = emulate_chain(specs, half=half, acc_dtype=torch.float32, **kw)
        bad = emulate_chain(specs, half=half, acc_dtype=torch.float32, mutant='trunc', **kw)
    ok, worse = error_ratios(per, emu, r64), error_ratios(bad, emu, r64)
    print(f'{dtype}: drift of a valid evaluation {ok}, of truncating packs {worse}')
    assert max(ok) <= 1.05 and worse[0] >= 1.5
