"""Training through the fused classifier conv layer on the GPU: rg_cls_conv_aggregate_x3,
rg_cls_conv_backward_x3, ClassifierTrainEngine.forward_objects and Model_Training.forward_objects.

One block: the seven gradients (dx, dW0, db0, dW1, db1, dWu, dbu) are held to the float32
class -- their error against float64 autograd through the edge-list oracle is at most
T_GPU_BWD (tests/test_cls_fused_backward_emulation.py) times float32 autograd's, in rms and in
max.  Bit-equality wherever the kernels promise it: run to run, an object alone or in a batch,
across the chunk cuts of the destination pass (test_more_than_one_chunk).  At a LeakyReLU kink
that float32 cannot resolve, either derivative is accepted and nothing else
(test_tile_shape_at_a_kink).
Whole model: the reference fixtures' loss and autograd through the oracle at the bar of
tests/test_gpu_classifier.py.  Memory: the fused step keeps nothing sized by the edge count.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import classifier_cfg, classifier_samples, golden
from oracle import classifier_ref
from test_cls_fused_backward_emulation import (NAMES, T_GPU_BWD, TILE_CASES, ambiguous_kinks,
                                               autograd_grads, backward_ratios, d_out_of,
                                               kink_tolerant_residual)
from test_cls_fused_emulation import C, fresh_block, layer_inputs, yml_block
from test_gpu_cls_fused import LAYER_SIZES

pytestmark = pytest.mark.gpu

PARAMS = ('msg.0.block.0.weight', 'msg.0.block.0.bias', 'msg.1.block.0.weight',
          'msg.1.block.0.bias', 'upd.0.block.0.weight', 'upd.0.block.0.bias')


class _Block:
    """One yml conv block of a 'blk.' state dict under the training engine's block methods."""

    def __init__(self, sd, aggr, dev):
        from graph_neural_network_for_radar_perception_amd.classifier import training as ct
        from graph_neural_network_for_radar_perception_amd.classifier.blocks import \
            residual_graph_conv_block
        from graph_neural_network_for_radar_perception_amd.training import Workspaces
        blk = residual_graph_conv_block(C, [C, C], [C], aggr, 'leakyrelu')
        blk.load_state_dict({k[4:]: v.float() for k, v in sd.items()})
        self.blk = blk.to(dev)
        self.dev = dev
        self.eng = object.__new__(ct.ClassifierTrainEngine)   # the block methods' state only
        self.eng.device = torch.device(dev)
        self.eng.ws = Workspaces(self.eng.device)
        self.cv = ct._ClsConv(self.blk, self.eng.device, self.eng.ws)
        named = dict(self.blk.named_parameters())
        self.params = [named[k] for k in PARAMS]
        self.G = {id(p): torch.zeros_like(p, requires_grad=False) for p in self.params}

    def _grads(self, dx, extra):
        out = {'dx': dx}
        out.update({n: self.G[id(p)].clone() for n, p in zip(NAMES[1:], self.params)})
        out.update(extra)
        return out

    def fused(self, x, sizes, d_out, max_size=None):
        """Gradients of sum(block(x) d_out) through the fused path; asserts the kernels took it."""
        from graph_neural_network_for_radar_perception_amd.classifier import engine as ce
        sizes = [int(n) for n in sizes]
        osz = torch.tensor(sizes, dtype=torch.int64, device=self.dev)
        N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
        T = {'table': None, 'E': E, 'max_degree': (max_size or max(sizes)) - 1}
        xd = x.to(self.dev).float().contiguous()
        ct = self.eng._fused_block_forward(self.cv, xd, T, osz)
        assert ct is not None and ce.fused_plan(self.blk, self.dev).fused_ok is True
        for g in self.G.values():
            g.zero_()
        dx, d_pq = self.eng._fused_block_backward(self.cv, ct, T,
                                                  d_out.to(self.dev).float().clone(), self.G)
        return self._grads(dx, dict(d_pq=d_pq, out=ct['out']))

    def unfused(self, x, sizes, d_out):
        from graph_neural_network_for_radar_perception_amd.classifier import engine as ce
        sizes = [int(n) for n in sizes]
        osz = torch.tensor(sizes, dtype=torch.int64, device=self.dev)
        N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
        g = ce.object_graph(osz, N, E)
        xd = x.to(self.dev).float().contiguous()
        ct, _ = self.eng._block_forward(self.cv, xd, g)
        for gr in self.G.values():
            gr.zero_()
        dx = self.eng._block_backward(self.cv, ct, g, self.eng._graph_incidence(g), C,
                                      d_out.to(self.dev).float().clone(), self.G)
        return self._grads(dx, {})


def _record(rec):
    """One JSON line per reading to $RG_CLS_FUSED_BWD_REPORT when set (the committed readings:
    profiles/cls_fused_backward_error_ratio.jsonl)."""
    path = os.environ.get('RG_CLS_FUSED_BWD_REPORT')
    if path:
        with open(path, 'a') as fh:
            fh.write(json.dumps(rec) + '\n')


_REF = {}


def _refs(weights, aggr):
    """(sd, x, d_out, float32 autograd, float64 autograd) of one case, computed once."""
    key = (weights, aggr)
    if key not in _REF:
        sd = fresh_block(5) if weights == 'fresh' else yml_block()
        x = layer_inputs(LAYER_SIZES, 7)
        d_out = d_out_of(LAYER_SIZES, 8)
        f32 = autograd_grads(sd, x, LAYER_SIZES, aggr, d_out)
        ref64 = autograd_grads({k: v.double() for k, v in sd.items()}, x.double(), LAYER_SIZES,
                               aggr, d_out.double())
        _REF[key] = (sd, x, d_out, f32, ref64)
    return _REF[key]


@pytest.mark.parametrize('weights', ['fresh', 'yml'])
@pytest.mark.parametrize('aggr', ['sum', 'mean'])
def test_layer_gradients_are_f32_class(cuda_device, weights, aggr):
    sd, x, d_out, f32, ref64 = _refs(weights, aggr)
    g = _Block(sd, aggr, cuda_device).fused(x, LAYER_SIZES, d_out)
    r = backward_ratios({n: g[n].cpu() for n in NAMES}, f32, ref64)
    for n in NAMES:
        print(f'cls fused backward {weights} {aggr} {n}: rms {r[n][0]:.3f} max {r[n][1]:.3f} '
              f'(T = {T_GPU_BWD})')
        _record(dict(test='layer_gradients_are_f32_class', weights=weights, aggr=aggr, grad=n,
                     rms=r[n][0], max=r[n][1], T=T_GPU_BWD))
    for n in NAMES:
        assert r[n][0] <= T_GPU_BWD and r[n][1] <= T_GPU_BWD, (n, r[n])


@pytest.mark.parametrize('sizes,seed', TILE_CASES, ids=lambda v: str(v) if isinstance(v, int)
                         else f'{len(v)}x{max(v)}')
def test_tile_shapes(cuda_device, sizes, seed):
    """Tiles that end inside, at and past an owner, pieces without edges, one-member objects
    between others.  x: the seed that keeps the float64 pre-activations clear of LeakyReLU's kink
    (TILE_CASES in tests/test_cls_fused_backward_emulation.py)."""
    sd = fresh_block(5)
    x = layer_inputs(sizes, seed)
    d_out = d_out_of(sizes, 10)
    blk = _Block(sd, 'sum', cuda_device)
    g = blk.fused(x, sizes, d_out)
    ref = autograd_grads({k: v.double() for k, v in sd.items()}, x.double(), sizes, 'sum',
                         d_out.double())
    for n in NAMES:
        scale = float(ref[n].abs().max())
        if scale == 0.0:   # no edges: the message MLP has no gradient
            assert not bool(g[n].any()), n
            continue
        err = (g[n].cpu().double() - ref[n]).abs() / scale
        assert bool((err <= 1e-4 + 1e-4 * ref[n].abs() / scale).all()), (n, float(err.max()))
    # a one-member object's dx row: as the kernels compute it with that object alone
    dx = g['dx'].clone()
    b = 0
    for n in sizes:
        if n == 1:
            alone = blk.fused(x[b:b + 1], [1], d_out[b:b + 1])
            assert torch.equal(dx[b:b + 1], alone['dx']), b
        b += n


def test_tile_shape_at_a_kink(cuda_device):
    """The 7x130 case with x of seed 9, which TILE_CASES passes over: some float64
    pre-activations lie within float32's error of zero (z1 = -1.7e-7 on edge 157 <- 176), where
    either LeakyReLU derivative is a float32-class answer.  The gradients meet test_tile_shapes'
    tolerance against the float64 closed form with each of those derivatives on the side that
    fits (kink_tolerant_residual): nothing but those few elements may differ."""
    sizes = TILE_CASES[6][0]
    sd = fresh_block(5)
    x, d_out = layer_inputs(sizes, 9), d_out_of(sizes, 10)
    assert ambiguous_kinks(sd, x, sizes)
    g = _Block(sd, 'sum', cuda_device).fused(x, sizes, d_out)
    res, ref, taken = kink_tolerant_residual({n: g[n].cpu() for n in NAMES}, sd, x, sizes, 'sum',
                                             d_out)
    print('derivatives taken on the other side:', taken)
    for n in NAMES:
        scale = float(ref[n].abs().max())
        err = res[n].abs() / scale
        assert bool((err <= 1e-4 + 1e-4 * ref[n].abs() / scale).all()), (n, float(err.max()))


def test_reproducibility_and_independence(cuda_device):
    rng = np.random.default_rng(3)
    sizes = [int(n) for n in rng.integers(2, 7, 500)]
    sizes.insert(137, 300)
    sd = fresh_block(5)
    x = layer_inputs(sizes, 13)
    d_out = d_out_of(sizes, 14)
    blk = _Block(sd, 'sum', cuda_device)
    g = {k: v.clone() for k, v in blk.fused(x, sizes, d_out).items()}
    again = blk.fused(x, sizes, d_out)
    for n in NAMES + ('d_pq',):
        assert torch.equal(g[n], again[n]), n
    # an object's d agg rows depend on its own rows only, so its [dP | dQ] rows are those of
    # the object run alone with the same x and d_out rows
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for o in (137, 0, 250, 500):
        b, e = int(starts[o]), int(starts[o + 1])
        alone = blk.fused(x[b:e], [sizes[o]], d_out[b:e])
        assert torch.equal(g['d_pq'][b:e], alone['d_pq']), o


def test_more_work_than_one_pass(cuda_device):
    """3000 objects of 2 .. 6: every wave walks several tiles; against the unfused engine."""
    rng = np.random.default_rng(5)
    sizes = [int(n) for n in rng.integers(2, 7, 3000)]
    sd = fresh_block(5)
    x = layer_inputs(sizes, 21)
    d_out = d_out_of(sizes, 22)
    blk = _Block(sd, 'mean', cuda_device)
    g = {k: v.clone() for k, v in blk.fused(x, sizes, d_out).items()}
    ref = blk.unfused(x, sizes, d_out)
    for n in NAMES:
        scale = float(ref[n].abs().max()) + 1e-12
        rel_max = float((g[n] - ref[n]).abs().max()) / scale
        rel_l2 = float((g[n] - ref[n]).norm()) / (float(ref[n].norm()) + 1e-12)
        assert rel_max <= 2e-3 or rel_l2 <= 1e-2, (n, rel_max, rel_l2)


def test_more_than_one_chunk(cuda_device):
    """The destination pass writes dm and h in chunks of 2^17 edge rows (CHUNK of
    cls_conv_bwd_x3.hip) for rg_linear_grad.  One object of 400 members (159 600 edges) after
    fifty of 3: its edges lie at [300, 159 900) of the edge sequence, across the chunk cut at
    131 072, which falls inside the object and inside one of its destinations.  Alone, the same
    object is cut at another destination.
     * Run to run every gradient is bit-equal; against the unfused engine at the bar of
       test_more_work_than_one_pass (a lost chunk or a wrong cut of the owners).
     * [dP | dQ] of the straddling object: bit-equal to the object run alone.
     * The tapes: the kernels compute the same dm and h bits per edge whatever the batch and
       the cut, and d_agg's rows depend on their own rows only, so dW_1 and db_1 of the batch are
       those of the big object alone plus those of the small objects alone, and do not depend on
       the degree bound (which moves the tapes' zeroed tail and rg_linear_grad's row count), up to
       float32 summation order: rg_linear_grad sums <= ~600 rows per partial and 512 partials, a
       relative 6e-8 * sqrt(600) = 1.5e-6 on an incoherent sum.  Bound 1e-5; one lost, doubled or
       stale row of the 160 000 moves dW_1 by 2.5e-3 of an incoherent sum's norm (2.5e-4 of one ten
       times as coherent as the 7x130 case's)."""
    small_a, small_b = [3] * 50, [5] * 20
    sizes = small_a + [400] + small_b
    E = sum(n * (n - 1) for n in sizes)
    assert 300 < (1 << 17) < 300 + 400 * 399 and (1 << 17) < E < (1 << 18)
    assert ((1 << 17) - 300) % 399 != 0 and (1 << 17) % 399 != 0   # neither cut at an owner's start
    sd = fresh_block(5)
    x = layer_inputs(sizes, 31)
    d_out = d_out_of(sizes, 32)
    rest = torch.cat((torch.arange(0, 150), torch.arange(550, 650)))

    def rel_l2(a, b):
        return float((a - b).norm()) / float(b.norm())

    for aggr in ('sum', 'mean'):
        blk = _Block(sd, aggr, cuda_device)
        g = {k: v.clone() for k, v in blk.fused(x, sizes, d_out).items()}
        again = blk.fused(x, sizes, d_out)
        for n in NAMES + ('d_pq',):
            assert torch.equal(g[n], again[n]), (aggr, n)
        ref = blk.unfused(x, sizes, d_out)
        for n in NAMES:
            rel_max = float((g[n] - ref[n]).abs().max()) / float(ref[n].abs().max())
            print(f'two chunks {aggr} {n}: rel max {rel_max:.2e} rel l2 {rel_l2(g[n], ref[n]):.2e}')
            assert rel_max <= 2e-3 or rel_l2(g[n], ref[n]) <= 1e-2, (aggr, n)
        big = {k: v.clone() for k, v in blk.fused(x[150:550], [400], d_out[150:550]).items()}
        assert torch.equal(g['d_pq'][150:550], big['d_pq']), aggr
        small = blk.fused(x[rest], small_a + small_b, d_out[rest])
        assert torch.equal(g['d_pq'][rest.to(cuda_device)], small['d_pq']), aggr
        loose = blk.fused(x, sizes, d_out, max_size=sum(sizes))
        for n in ('dW1', 'db1'):
            parts, bound = rel_l2(big[n] + small[n], g[n]), rel_l2(loose[n], g[n])
            print(f'two chunks {aggr} {n}: big + small {parts:.2e}, loose degree bound {bound:.2e}')
            assert parts <= 1e-5 and bound <= 1e-5, (aggr, n, parts, bound)
        for n in ('dx', 'dW0', 'db0', 'dWu', 'dbu', 'd_pq'):   # nothing else sees the tapes
            assert torch.equal(g[n], loose[n]), (aggr, n)


# ------------------------------------------------------------------ whole model
def _training_model(name, dev):
    from graph_neural_network_for_radar_perception_amd.classifier import Model_Training
    d = golden(name)
    sd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith('w/')}
    m = Model_Training(classifier_cfg(name))
    m.load_state_dict(sd)
    return m.to(dev).train(), d, sd


def _oracle_loss(ref_sd, cfg, ss):
    logits = torch.cat([classifier_ref.forward(ref_sd, cfg, s['nf'], s['ei'], s['osz'])
                        for s in ss], 0)
    return classifier_ref.focal_loss(logits, torch.cat([s['gt'] for s in ss]), cfg.num_classes)


def _object_args(ss, dev):
    return ([s['nf'].to(dev) for s in ss], [s['osz'].to(dev) for s in ss],
            [s['gt'].to(dev) for s in ss])


@pytest.mark.parametrize('name', ['classifier_yml', 'classifier_mean'])
def test_forward_objects_gradients_match_oracle(cuda_device, name):
    from graph_neural_network_for_radar_perception_amd.classifier import engine as ce
    dev = cuda_device
    m, d, sd = _training_model(name, dev)
    cfg = classifier_cfg(name)
    ss = classifier_samples(d)
    plans = [ce.fused_plan(blk, dev) for blk in m.pred.pass_messages.conv_blk]
    for p in plans:
        p.fused_ok = None
    loss = m.forward_objects(*_object_args(ss, dev))
    assert loss.requires_grad
    loss.backward()
    assert abs(float(loss.detach()) - float(d['loss'])) <= 1e-4 + 1e-4 * abs(float(d['loss']))
    assert all(p.fused_ok is True for p in plans)
    with torch.no_grad():   # without gradients: the inference path from the sizes, the same loss
        plain = m.forward_objects(*_object_args(ss, dev))
    assert not plain.requires_grad
    assert abs(float(plain) - float(d['loss'])) <= 1e-4 + 1e-4 * abs(float(d['loss']))
    ref_sd = {k[len('pred.'):]: v.clone().float().requires_grad_(True)
              for k, v in sd.items() if k.startswith('pred.')}
    _oracle_loss(ref_sd, cfg, ss).backward()
    for k, p in m.named_parameters():
        r = ref_sd[k[len('pred.'):]].grad
        assert p.grad is not None, k
        gg = p.grad.detach().cpu()
        rel_max = float((gg - r).abs().max()) / (float(r.abs().max()) + 1e-12)
        rel_l2 = float((gg - r).norm()) / (float(r.norm()) + 1e-12)
        assert rel_max <= 2e-3 or rel_l2 <= 1e-2, (k, rel_max, rel_l2)


def test_forward_objects_max_falls_back_bit_equal(cuda_device):
    """aggr = 'max' has no fused backward: the blocks run the unfused tape over object_graph's
    CSR, the edges compute_edge_index lists -- loss and gradients are Model_Training.forward's."""
    dev = cuda_device
    m, d, _ = _training_model('classifier_max', dev)
    ss = classifier_samples(d)
    loss = m.forward_objects(*_object_args(ss, dev))
    loss.backward()
    got = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    ref = m([s['nf'].to(dev) for s in ss], [s['ei'].to(dev) for s in ss],
            [s['osz'].to(dev) for s in ss], [s['gt'].to(dev) for s in ss])
    ref.backward()
    assert torch.equal(loss.detach(), ref.detach())
    for k, p in m.named_parameters():
        assert torch.equal(got[k], p.grad), k


def test_two_sgd_steps_match_oracle(cuda_device):
    """Two torch.optim.SGD steps (lr 0.005, momentum 0.9) through forward_objects against two
    oracle steps: the second step runs on images (W_1^T and W_pq^T among them) that must have
    followed the first update."""
    dev = cuda_device
    m, d, sd = _training_model('classifier_yml', dev)
    cfg = classifier_cfg('classifier_yml')
    ss = classifier_samples(d)
    args = _object_args(ss, dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.005, momentum=0.9)
    ref_sd = {k[len('pred.'):]: v.clone().float().requires_grad_(True)
              for k, v in sd.items() if k.startswith('pred.')}
    ropt = torch.optim.SGD(list(ref_sd.values()), lr=0.005, momentum=0.9)
    for _ in range(2):
        opt.zero_grad()
        m.forward_objects(*args).backward()
        opt.step()
        ropt.zero_grad()
        _oracle_loss(ref_sd, cfg, ss).backward()
        ropt.step()
    for k, p in m.named_parameters():
        r = ref_sd[k[len('pred.'):]].detach()
        torch.testing.assert_close(p.detach().cpu(), r, rtol=1e-4, atol=1e-5, msg=k)


def test_memory_does_not_grow_with_edges(cuda_device):
    """4096 nodes as 2048 objects of 2 (E = 4096) and as 16 objects of 256 (E = 1 044 480): the
    fused step's peak allocation differs by less than one [E][128] float32 buffer of the larger
    batch (535 MB); the unfused step on the larger batch exceeds the fused one by more."""
    from graph_neural_network_for_radar_perception_amd import synthetic
    from graph_neural_network_for_radar_perception_amd.classifier import engine as ce
    from graph_neural_network_for_radar_perception_amd.classifier import training as ct
    dev = cuda_device
    m, _, _ = _training_model('classifier_yml', dev)
    eng = ct.ClassifierTrainEngine(m, dev)
    one_buffer = 1044480 * 128 * 4

    def batches(n_obj, size):
        smp = synthetic.make_objects(n_obj, 5, min_size=size, max_size=size)
        nf = [torch.from_numpy(smp['node_features']).to(dev)]
        osz = [torch.from_numpy(smp['object_size'])]
        gt = [torch.from_numpy(smp['object_class']).to(dev)]
        n, e = n_obj * size, n_obj * size * (size - 1)

        def with_graph():
            _, _, ei = ce.object_complete_graph(osz[0].to(dev), n, e)
            return ct.prepare_batch(nf, [ei], osz, gt)
        return ct.prepare_batch_objects(nf, osz, gt), with_graph

    def peak(step):
        step()   # warm-up: plans, images, workspaces
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        step()
        torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev)

    small, _ = batches(2048, 2)
    large, large_graph = batches(16, 256)
    assert small[6] == 4096 and large[6] == 1044480
    p_small = peak(lambda: ct.train_step_loss_objects(eng, small).backward())
    p_large = peak(lambda: ct.train_step_loss_objects(eng, large).backward())
    print(f'fused peak: E = 4096 {p_small / 2**20:.0f} MiB, E = 1044480 {p_large / 2**20:.0f} MiB')
    assert abs(p_large - p_small) < one_buffer, (p_small, p_large)
    gb = large_graph()
    p_unfused = peak(lambda: ct.train_step_loss(eng, gb).backward())
    print(f'unfused peak: E = 1044480 {p_unfused / 2**20:.0f} MiB')
    assert p_unfused - p_large > one_buffer, (p_unfused, p_large)
