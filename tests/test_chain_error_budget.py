"""The error budget of the fp32 chain kernels' discriminating check, on the CPU.  No GPU.

tests/test_gpu_chain_x3.py holds every chain kernel to `T` times the error of a plain float32
evaluation, both against float64, in two metrics over a 3001-row batch:

    rms(out - ref64) <= T rms(f32 - ref64)    and    max|out - ref64| <= T max|f32 - ref64|

(rms: a scheme-wide loss; max: one lane, tile or k-step).  This file proves that the check
separates a right kernel from a subtly wrong one: the h2 arithmetic emulated with
tests/test_h2_emulation.py's _H2Linear reads <= 1.5 on both metrics, and the same arithmetic
with one fault in every layer -- subnormal fp16 planes flushed, one cross product dropped, the
residue dropped in a single 16-wide k-step, the weights' residue dropped in a single 32-wide
M-tile -- reads >= 3 T on at least one.  The input recipes, the metrics and the mutant ratios
(mutant_floor: the cap on any per-chain T) are shared with the GPU file.
"""
import functools
import math
from unittest import mock

import pytest
import torch

import test_h2_emulation as emu
from test_h2_emulation import _H2Linear

T_DEFAULT = 4.0          # the GPU check's threshold unless a chain's measured ratio sets its own
MUTANTS = ('flush', 'drop_a0w1', 'drop_a1w0', 'kstep', 'mtile')
R = 3001


# ------------------------------------------------------------------ shared with the GPU file
def dense_inputs(rows, width, seed):
    """randn * 2: about 5 % of the values below 0.125, where the h2 residue plane is an fp16
    subnormal (|a - f16(a)| <= 2^-11 |a| < 2^-14)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(rows, width, generator=g) * 2


def encoder_inputs(rows, width, seed):
    """Raw-feature rows with columns at scales 0.05, 1 and 30 (inside the physical limits of
    test_h2_domain_at_physical_limits): the 0.05 columns' residues are all subnormal."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    scale = torch.tensor([(0.05, 1.0, 30.0)[j % 3] for j in range(width)])
    return torch.randn(rows, width, generator=g) * scale


def eval_chain(specs, x, dtype, linear=torch.nn.functional.linear, linear_out=None):
    """The chain's ffn_blocks (Linear, channel_normalization, LeakyReLU) in `dtype` on the
    tensors' device; specs: objects with weight, bias, mu, std, act (engine.LayerSpec).
    linear_out: the Linear of an un-normalised last layer (default: `linear`)."""
    h = x.to(dtype)
    for s in specs:
        f = linear_out if (linear_out and s is specs[-1] and s.mu is None) else linear
        h = f(h, s.weight.detach().to(dtype), None if s.bias is None else s.bias.detach().to(dtype))
        if s.mu is not None:
            h = (h - h.mean(1, keepdim=True)) / (h.std(1, keepdim=True) + 1e-5) \
                * s.std.detach().to(dtype) + s.mu.detach().to(dtype)
        if s.act == 'leakyrelu':
            h = torch.nn.functional.leaky_relu(h, 0.01)
    return h


def error_ratios(out, f32, ref64):
    """(rms, max) of out's error over the float32 evaluation's, both against ref64."""
    e = out.double() - ref64
    e32 = f32.double() - ref64
    return (float(e.pow(2).mean().sqrt() / e32.pow(2).mean().sqrt()),
            float(e.abs().max() / e32.abs().max()))


# ------------------------------------------------------------------ chains of random weights
class _Spec:
    def __init__(self, weight, bias, mu, std, act):
        self.weight, self.bias, self.mu, self.std, self.act = weight, bias, mu, std, act


def random_chain(widths, norm_from, last_bare, seed):
    """Linear layers of nn.Linear's initialisation; layers >= norm_from normalised (mu ~ 0.1 N,
    std ~ 1 + 0.1 N) and activated, the last one a bare Linear when last_bare."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    specs = []
    for l, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
        b = 1.0 / math.sqrt(k)
        w = (torch.rand(n, k, generator=g) * 2 - 1) * b
        bias = (torch.rand(n, generator=g) * 2 - 1) * b
        bare = last_bare and l == len(widths) - 2
        norm = l >= norm_from and not bare
        specs.append(_Spec(w, bias, 0.1 * torch.randn(1, generator=g) if norm else None,
                           1 + 0.1 * torch.randn(1, generator=g) if norm else None,
                           'none' if bare else 'leakyrelu'))
    return specs


def prior_head():
    """The head chain with the output layer of a freshly initialised classification head:
    weights ~ 0.01 N, every bias -log(99) (a prior of 0.01).  |b| is ~100 x |W x|: a float32
    evaluation's error is the rounding of the final sum at the bias's magnitude, which hides
    more of a mutant's error than on the other chains (its readings are the smallest)."""
    specs = random_chain([64, 64, 64, 64, 64, 7], 0, True, 4)
    g = torch.Generator(device='cpu').manual_seed(5)
    specs[-1].weight = 0.01 * torch.randn(7, 64, generator=g)
    specs[-1].bias = torch.full((7,), -math.log(99.0))
    return specs


CHAINS = {
    'prior_head': (prior_head, dense_inputs, 64),
    'head': (lambda: random_chain([64, 64, 64, 64, 64, 7], 0, True, 1), dense_inputs, 64),
    'edge_enc': (lambda: random_chain([7, 256, 128, 128, 64], 1, False, 2), encoder_inputs, 7),
    'bare': (lambda: random_chain([64, 64], 0, True, 3), dense_inputs, 64),
}


# ------------------------------------------------------------------ the arithmetic and its mutants
class _MutantH2(_H2Linear):
    """_H2Linear with one fault in every Linear.  Every fault is a change of the fp16 planes
    (dropping a0 w1 is an all-zero w1; dropping a1 w0 an all-zero a1), so the arithmetic itself
    stays _H2Linear.linear's: only its _planes is wrapped for the call."""

    def __init__(self, mutant=None):
        super().__init__()
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def linear(self, x, w, b=None):
        if self.mutant is None:
            return super().linear(x, w, b)
        calls = []
        split = emu._planes

        def planes(v):
            p0, p1 = split(v)
            weights = not calls           # _H2Linear.linear splits the weights, then x
            calls.append(v.shape)
            assert v.shape == (w.shape if weights else x.shape)
            m = self.mutant
            if m == 'flush':              # what an MFMA that flushed fp16 subnormals would read
                p0 = torch.where(p0.abs() < 2.0 ** -14, torch.zeros_like(p0), p0)
                p1 = torch.where(p1.abs() < 2.0 ** -14, torch.zeros_like(p1), p1)
            elif (m == 'drop_a0w1' and weights) or (m == 'drop_a1w0' and not weights):
                p1 = torch.zeros_like(p1)
            elif m == 'kstep' and not weights:
                k0 = 16 if v.shape[-1] >= 32 else 0
                p1 = p1.clone()
                p1[..., k0:k0 + 16] = 0
            elif m == 'mtile' and weights:
                m0 = 32 if v.shape[0] >= 64 else 0
                p1 = p1.clone()
                p1[m0:m0 + 32] = 0
            return p0, p1

        with mock.patch.object(emu, '_planes', planes):
            out = super().linear(x, w, b)
        assert len(calls) == 2
        return out

    def linear_out(self, x, w, b=None):
        """An un-normalised output layer as chain_x3.hip runs it: the bias after the products
        (one rounding at the bias's magnitude; the descale before it is exact)."""
        y = self.linear(x, w, None)
        return y if b is None else y + b.to(torch.float32)


@functools.lru_cache(maxsize=None)
def emulated_ratios(chain):
    """{None | mutant: (rms ratio, max ratio)} of the emulated h2 arithmetic on `chain`."""
    make, inputs, width = CHAINS[chain]
    specs = make()
    x = inputs(R, width, 0)
    with torch.no_grad():
        ref64 = eval_chain(specs, x, torch.float64)
        f32 = eval_chain(specs, x, torch.float32)
        out = {}
        for m in (None,) + MUTANTS:
            e = _MutantH2(m)
            out[m] = error_ratios(eval_chain(specs, x, torch.float32, e.linear, e.linear_out),
                                  f32, ref64)
        return out


def mutant_floor(chain):
    """The mildest mutant's reading on `chain` (its larger metric): the check catches every
    mutant while T stays below this; the GPU file keeps every T at a third of it or less."""
    r = emulated_ratios(chain)
    return min(max(r[m]) for m in MUTANTS)


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize('chain', list(CHAINS))
def test_correct_h2_is_f32_class(chain):
    """The h2 arithmetic reads <= 1.5 of a plain float32 evaluation's error on both metrics."""
    rms, mx = emulated_ratios(chain)[None]
    print(f'{chain}: h2 / f32 error  rms {rms:.3f}  max {mx:.3f}')
    assert rms <= 1.5 and mx <= 1.5


@pytest.mark.parametrize('mutant', MUTANTS)
@pytest.mark.parametrize('chain', list(CHAINS))
def test_mutant_is_caught(chain, mutant):
    """One fault in every layer reads >= 3 T on at least one metric."""
    rms, mx = emulated_ratios(chain)[mutant]
    print(f'{chain} / {mutant}: error over f32  rms {rms:.1f}  max {mx:.1f}')
    assert max(rms, mx) >= 3 * T_DEFAULT
