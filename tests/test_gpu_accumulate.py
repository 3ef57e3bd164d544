"""Gradient accumulation on the GPU (training.GradAccumulator; RadarGNNTrainer.accumulate /
accumulate_frames / apply_accumulated; ClassifierTrainer.accumulate_objects / accumulate_inputs
/ apply_accumulated; grad_accumulation_steps of train_sequence, train_dataset and
train_classifier_sequence).

Reference: modules/neural_net/gnn/training.py:189-333 and classifier/training.py:138-236
(train_model_accumulate_grad): K micro-batches of ``(loss / K).backward()``, then one
``optimizer.step()`` / ``lr_scheduler.step()``; an empty batch contributes nothing; a NaN loss
skips the step.

Every oracle is existing calls composed by hand in this file -- engine.forward, engine.backward
with ones / K, clones of engine.flat_grad summed in order by torch, opt.step -- or autograd
through train_step_losses.  Two runs of the same launches on the same values are bit-equal in
this project and a float32 sum taken in the same order is the same sum, so
every comparison of weights, optimizer state and gradients is torch.equal.  The one tolerance
is on the learning rate read back from an SGD update, w_before - w_after = lr * momentum
buffer: both sides round once in float32 (the kernel's w - lr * buf, the test's subtraction),
each within 2^-24 max|w|, and the test's product lr * buf a third time, so 2^-22 max|w| is asked.
A rate wrong by the decay factor 10 leaves an error of at least 0.9 max|lr * buf|, so the check
also asks max|lr * buf| > 10 times the bound: such a rate then misses it ninefold."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sequence_ref as sref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = [14, 3, 9, 0, 20, 7, 7, 11, 1, 18, 5, 16, 2]        # the caller's order, a repeat
_CACHE = {}


def _pkg():
    from graph_neural_network_for_radar_perception_amd import frontend, sequence, training
    return frontend, sequence, training


def _cfg():
    from graph_neural_network_for_radar_perception_amd.config import default_config
    return default_config(graph_convolution_stem_channels=[64, 64])


def _trainer(dev, cfg, seed=31, **kw):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    from graph_neural_network_for_radar_perception_amd.training import RadarGNNTrainer
    torch.manual_seed(seed)
    m = Model_Training(cfg, 'cpu').to(dev).train()
    return RadarGNNTrainer(m, cfg, world=kw.pop('world', 1), **kw)


def _frames_labels(cfg, dev, seed, sizes=(230, 57), nan=False):
    """test_gpu_optim._frames_labels restated: synthetic frames and their host-made labels as
    the (batch, labels) ``step`` takes; nan: one corrupted return in the last frame."""
    from graph_neural_network_for_radar_perception_amd import synthetic
    from graph_neural_network_for_radar_perception_amd.graph_features import (FrameBatch,
                                                                                build_graph_batch)
    frames = [synthetic.make_frame(n, seed + i) for i, n in enumerate(sizes)]
    if nan:
        frames[-1]['meas_rcs'] = frames[-1]['meas_rcs'].copy()
        frames[-1]['meas_rcs'][7] = np.float32('nan')
    gb = build_graph_batch(FrameBatch.from_frames(frames, device=dev), cfg)
    rp = gb.row_ptr.cpu().numpy().astype(np.int64)
    col = gb.col[:int(rp[-1])].cpu().numpy().astype(np.int64)
    lab_np, clusters = synthetic.batch_labels(frames, rp, col, cfg.num_classes)
    lab = {k: torch.from_numpy(v).to(dev) for k, v in lab_np.items()}
    lab['class_weights'] = torch.tensor(cfg.class_weights_dyn, device=dev)
    return FrameBatch.from_frames(frames, clusters, device=dev), lab


# frame sizes per batch: 40 .. 400 nodes, odd sizes, one or several frames
_SIZES = {0: (230, 57), 1: (400,), 2: (40, 131, 77), 3: (95, 203), 4: (64, 65), 5: (301, 40)}


def _batches(dev, which, nan=()):
    """Batches ``which`` of the shared pool (made once, never written to); ``nan``: those whose
    last frame holds a NaN radar cross-section."""
    cfg = _cfg()
    out = []
    for b in which:
        key = ('batch', b, b in nan)
        if key not in _CACHE:
            _CACHE[key] = _frames_labels(cfg, dev, 9100 + 10 * b, _SIZES[b], nan=b in nan)
        out.append(_CACHE[key])
    return out


def _engine_batch(tr, batch, labels):
    """The tuple ``step`` passes to engine.forward."""
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
    gb = build_graph_batch(batch, tr.cfg, ws_cache=tr.ws_cache)
    g = gb.graph
    g.n_edges = int(gb.n_edges_dev.item())
    g.n_pairs = int(g.n_pairs_dev.item())
    return (gb.node_features, gb.edge_features, g, batch.cluster_ptr, batch.cluster_idx,
            batch.n_clusters, labels)


def _frames_engine_batch(tr, fb):
    """The tuple ``step_frames`` passes to engine.forward for a frame_batch."""
    from graph_neural_network_for_radar_perception_amd import training
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
    gb = build_graph_batch(fb, tr.cfg, ws_cache=tr.ws_cache)
    g = gb.graph
    lab = training.training_labels(fb, gb, tr.cfg, tr.ws_cache)
    g.n_edges, g.n_pairs = int(gb.n_edges_dev.item()), int(g.n_pairs_dev.item())
    return (gb.node_features, gb.edge_features, g, lab['cluster_ptr'], lab['cluster_idx'],
            int(lab['n_clusters_dev'].item()), lab)


def _micro_gradients(tr, tuples, K):
    """engine.forward and engine.backward(tape, ones / K) as ``step`` calls them, per tuple:
    (clones of engine.flat_grad, the losses)."""
    eng = tr.engine
    g = torch.ones(4, dtype=torch.float32, device=eng.device) / K
    grads, losses = [], []
    for t in tuples:
        lo, _, tape = eng.forward(*t)
        eng.backward(tape, g)
        grads.append(eng.flat_grad.clone())
        losses.append(lo)
    return grads, losses, g


def _sum(ts):
    total = ts[0]
    for t in ts[1:]:
        total = total + t
    return total


def _hand_iteration(tr, tuples, K, scale=1.0):
    """One outer iteration composed by hand: the micro-gradients summed in order, the slots
    sum_j losses_j * g, one opt.step."""
    grads, losses, g = _micro_gradients(tr, tuples, K)
    tr.opt.step(_sum(grads), grad_scale=scale, losses=_sum([lo * g for lo in losses]))
    return losses


def _state(tr):
    torch.cuda.synchronize()
    return [tr.opt.flat.clone()] + [b.clone() for b in tr.opt.state_bufs]


def _same_state(a, b, what=''):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f'{what}: {"weights" if i == 0 else f"optimizer state {i - 1}"}'


# ------------------------------------------------------------------ 1. K = 1 is step
def test_k1_is_step(cuda_device):
    dev = cuda_device
    cfg = _cfg()
    a, b = _trainer(dev, cfg), _trainer(dev, cfg)
    for it, (batch, lab) in enumerate(_batches(dev, (0, 1))):
        la, aa, _ = a.accumulate(batch, lab, 1)
        assert a.apply_accumulated() == 1
        lb, ab, _ = b.step(batch, lab)
        assert bool(torch.isfinite(la).all()) and float(la.sum()) > 0
        assert torch.equal(la, lb) and torch.equal(aa, ab), it
        _same_state(_state(a), _state(b), f'iteration {it}')
    assert a.opt.applied_steps() == b.opt.applied_steps() == 2
    assert torch.equal(a.opt.buf, b.opt.buf) and bool(a.opt.buf.any())


# ------------------------------------------------------------------ 2. K = 3, hand-composed
@pytest.mark.parametrize('optim', ['sgd', 'adamw'])
def test_k3_equals_the_hand_composed_iteration(cuda_device, optim):
    dev = cuda_device
    cfg = _cfg()
    tr, tw = _trainer(dev, cfg, optim=optim), _trainer(dev, cfg, optim=optim)
    w0 = tr.opt.flat.clone()
    for it, which in enumerate(((0, 1, 2), (3, 4, 5))):      # the second exercises the state
        group = _batches(dev, which)
        got = [tr.accumulate(batch, lab, 3)[0] for batch, lab in group]
        assert torch.equal(tr.opt.flat, w0 if it == 0 else before[0]), \
            'a micro-batch changed the weights'
        assert tr.apply_accumulated() == 3
        want = _hand_iteration(tw, [_engine_batch(tw, *b) for b in group], 3)
        for x, y in zip(got, want):
            assert torch.equal(x, y) and bool(torch.isfinite(x).all())   # unscaled
        before = _state(tr)
        _same_state(before, _state(tw), f'{optim} iteration {it}')
    assert tr.opt.applied_steps() == tw.opt.applied_steps() == 2 and tr.opt.steps == 2
    assert not torch.equal(tr.opt.flat, w0)


# ------------------------------------------------------------------ 3. autograd's gradient
@pytest.mark.parametrize('K', [2, 3])
def test_accumulated_gradient_is_autograds(cuda_device, K):
    from graph_neural_network_for_radar_perception_amd import training
    dev = cuda_device
    cfg = _cfg()
    tr = _trainer(dev, cfg)
    group = _batches(dev, (0, 1, 2)[:K])
    for batch, lab in group:
        tr.accumulate(batch, lab, K)
    got = tr.accum.grad.clone()
    slots = tr.accum.slots.clone()
    # the loop a caller writes without the trainer (no weight changed in between)
    eng = tr.engine
    totals = []
    for batch, lab in group:
        losses = training.train_step_losses(eng, _engine_batch(tr, batch, lab))
        totals.append(losses.detach())
        (training.total_loss(losses) / K).backward()
    o = 0
    for i, p in enumerate(eng.params):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        assert torch.equal(got[o:o + p.numel()].view_as(p), p.grad), f'parameter {i}'
        o += p.numel()
    assert o == got.numel() and float(got.abs().max()) > 0
    g = torch.ones(4, dtype=torch.float32, device=dev) / K
    assert torch.equal(slots, _sum([t * g for t in totals]))
    for p in eng.params:
        p.grad = None


# ------------------------------------------------------------------ 4. NaN micro-batch
def test_nan_micro_batch_skips_the_outer_iteration(cuda_device):
    dev = cuda_device
    cfg = _cfg()
    tr = _trainer(dev, cfg, milestones=[1])
    tw = _trainer(dev, cfg, milestones=[1])                  # never sees the NaN iteration
    before = _state(tr)
    losses = [tr.accumulate(batch, lab, 3)[0] for batch, lab in _batches(dev, (0, 1, 2), nan=(1,))]
    assert tr.apply_accumulated() == 3
    assert bool(torch.isnan(losses[1]).any())
    assert bool(torch.isfinite(losses[0]).all()) and bool(torch.isfinite(losses[2]).all())
    _same_state(_state(tr), before, 'the skipped iteration')
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 1
    lr0, lr1 = tr.opt.lr_at(0), tr.opt.lr_at(1)
    assert lr1 == lr0 * 0.1
    for it, (which, lr) in enumerate((((0, 1, 2), lr0), ((3, 4, 5), lr1))):
        group = _batches(dev, which)
        w_before = tr.opt.flat.clone()
        for batch, lab in group:
            tr.accumulate(batch, lab, 3)
        assert tr.apply_accumulated() == 3
        _hand_iteration(tw, [_engine_batch(tw, *b) for b in group], 3)
        _same_state(_state(tr), _state(tw), f'clean iteration {it}')
        # the rate, read from the update itself: w_before - w_after = lr * momentum buffer
        step = lr * tr.opt.buf
        err = float((w_before - tr.opt.flat - step).abs().max())
        bound = 2.0 ** -22 * float(w_before.abs().max())
        print('clean iteration', it, 'lr', lr, 'error', err, 'bound', bound,
              'max |lr * buf|', float(step.abs().max()))
        assert err <= bound and float(step.abs().max()) > 10 * bound
    assert tr.opt.applied_steps() == 2 and tr.opt.steps == 3


# ------------------------------------------------------------------ 5. empty micro-batches
def _static_store(dev):
    """test_gpu_training_feed._static_store restated: six small scenes; the windows of 2 scans
    at 0 and 1 hold no / one dynamic node, so a batch of them has no frame."""
    if 'static' not in _CACHE:
        _, sequence, _ = _pkg()
        sizes = (30, 20, 25, 40, 45, 33)
        kinds = ('static', 'static', 'static+1', 'mixed', 'mixed', 'mixed')
        radar, odo, lists, sensors = sref.make_sequence(11, sizes, kinds)
        _CACHE['static'] = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    return _CACHE['static']


def _adversarial_store(dev):
    if 'adv' not in _CACHE:
        _, sequence, _ = _pkg()
        radar, odo, lists, sensors = sref.adversarial_sequence()
        _CACHE['adv'] = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    return _CACHE['adv']


def _empty_fb(dev):
    frontend = _pkg()[0]
    dd, gd = frontend.dynamic_frame(_static_store(dev).windows([0, 0], 2), with_keys=True,
                                    flip=[0, 1])
    fb = frontend.frame_batch(dd, gd)
    assert fb.n_frames == 0
    return fb


def _real_fb(dev, pos, flags=None):
    frontend = _pkg()[0]
    dd, gd = frontend.dynamic_frame(_adversarial_store(dev).windows(pos, 4), False,
                                    with_keys=True, flip=flags, numpy_mean=True)
    fb = frontend.frame_batch(dd, gd)
    assert fb.n_frames > 0
    return fb


def test_empty_micro_batches_contribute_nothing(cuda_device):
    dev = cuda_device
    cfg = _cfg()
    tr, tw = _trainer(dev, cfg), _trainer(dev, cfg)
    empty, real = _empty_fb(dev), _real_fb(dev, ORDER[:3])
    assert tr.accumulate_frames(empty, 3) is None
    out = tr.accumulate_frames(real, 3)
    assert tr.accumulate_frames(empty, 3) is None
    assert tr.apply_accumulated() == 1
    want = _hand_iteration(tw, [_frames_engine_batch(tw, real)], 3)     # g = 1/3: K stays 3
    assert torch.equal(out[0], want[0]) and bool(torch.isfinite(out[0]).all())
    _same_state(_state(tr), _state(tw), '[empty, real, empty]')
    assert tr.opt.applied_steps() == 1
    # nothing but empty batches on one rank: nothing is launched
    before, steps = _state(tr), tr.opt.steps
    for _ in range(3):
        assert tr.accumulate_frames(empty, 3) is None
    assert tr.apply_accumulated() == 0
    _same_state(_state(tr), before, '[empty] * 3')
    assert tr.opt.steps == steps and tr.opt.applied_steps() == 1


def test_one_allreduce_per_outer_iteration(cuda_device, monkeypatch):
    """world = 2 with the all-reduce stubbed, as
    test_step_frames_empty_batch_on_one_of_several_ranks stubs it."""
    from graph_neural_network_for_radar_perception_amd import training
    dev = cuda_device
    cfg = _cfg()
    tr = _trainer(dev, cfg)
    tr.world = 2
    calls = []

    def peer_sum(bucket, world):
        assert world == 2
        calls.append((bucket, bucket.clone()))
        return 0.5

    monkeypatch.setattr(training, 'allreduce_gradients', peer_sum)
    empty = _empty_fb(dev)
    tr.accumulate_frames(_real_fb(dev, ORDER[:3]), 1)        # stale values in both buckets
    tr.apply_accumulated()
    del calls[:]
    before, steps = _state(tr), tr.opt.steps
    for _ in range(3):
        assert tr.accumulate_frames(empty, 3) is None
    assert tr.apply_accumulated() == 0
    assert len(calls) == 1 and calls[0][0] is tr.accum.bucket
    sent = calls[0][1]
    n = tr.opt.flat.numel()
    assert sent.numel() == n + 4
    assert not bool(sent[:n].any()) and bool(torch.isnan(sent[n:]).all())
    _same_state(_state(tr), before, 'every rank skips')
    assert tr.opt.steps == steps + 1 and tr.opt.applied_steps() == 1
    # three real micro-batches: still one call, after the third
    del calls[:]
    for j, pos in enumerate((ORDER[:3], ORDER[3:6], ORDER[6:9])):
        assert tr.accumulate_frames(_real_fb(dev, pos), 3) is not None
        assert calls == [], f'an all-reduce after micro-batch {j}'
    assert tr.apply_accumulated() == 3
    assert len(calls) == 1 and calls[0][0] is tr.accum.bucket
    assert bool(torch.isfinite(calls[0][1]).all()) and tr.opt.applied_steps() == 2


# ------------------------------------------------------------------ 6. two ranks on one card
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _rank_batches(cfg, dev, rank, it, nan=False):
    """The two micro-batches of rank ``rank`` in iteration ``it``: different on every rank and
    micro-batch; nan: the rank's second one holds a NaN."""
    sizes = ((150, 61), (233,))
    return [_frames_labels(cfg, dev, 7000 + 1000 * it + 100 * rank + 10 * j, sizes[j],
                           nan=(nan and j == 1)) for j in range(2)]


def _two_rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world),
                      RANK=str(rank), LOCAL_RANK=str(rank))
    sys.path.insert(0, REPO)
    dist.init_process_group('gloo')          # both ranks share the test box's one card
    dev = torch.device('cuda', 0)
    cfg = _cfg()
    tr = _trainer(dev, cfg, seed=100 + rank, world=world)    # the broadcast unifies the inits
    w0 = tr.opt.flat.clone()
    for batch, lab in _rank_batches(cfg, dev, rank, 0):
        tr.accumulate(batch, lab, 2)
    n_contrib = tr.apply_accumulated()
    torch.cuda.synchronize()
    w1, b1, n1 = tr.opt.flat.clone(), tr.opt.buf.clone(), tr.opt.applied_steps()
    for batch, lab in _rank_batches(cfg, dev, rank, 1, nan=(rank == 1)):
        tr.accumulate(batch, lab, 2)
    tr.apply_accumulated()
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f'acc{rank}.npz'), w0=w0.cpu().numpy(), w1=w1.cpu().numpy(),
             b1=b1.cpu().numpy(), n1=n1, contrib=n_contrib, w2=tr.opt.flat.cpu().numpy(),
             b2=tr.opt.buf.cpu().numpy(), n2=tr.opt.applied_steps(), steps=tr.opt.steps)
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_accumulate_and_reduce_once(tmp_path, cuda_device):
    """K = 2 on two data-parallel ranks: both end with the weights and momentum this process
    computes from the four hand-composed micro-gradients, (rank 0's sum + rank 1's sum) with
    grad_scale 0.5; a second iteration with a NaN in rank 1's second micro-batch leaves both
    ranks unchanged."""
    world = 2
    mp.spawn(_two_rank_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world,
             join=True)
    r = [np.load(tmp_path / f'acc{k}.npz') for k in range(world)]
    dev = cuda_device
    cfg = _cfg()
    tw = _trainer(dev, cfg, seed=100)                        # rank 0's initialisation
    np.testing.assert_array_equal(r[0]['w0'], tw.opt.flat.cpu().numpy())
    sums, slots = [], []
    for rank in range(world):
        tuples = [_engine_batch(tw, *b) for b in _rank_batches(cfg, dev, rank, 0)]
        grads, losses, g = _micro_gradients(tw, tuples, 2)
        sums.append(_sum(grads))
        slots.append(_sum([lo * g for lo in losses]))
    tw.opt.step(sums[0] + sums[1], grad_scale=0.5, losses=slots[0] + slots[1])
    torch.cuda.synchronize()
    assert tw.opt.applied_steps() == 1
    for k in range(world):
        np.testing.assert_array_equal(r[k]['w0'], r[0]['w0'])           # broadcast from rank 0
        assert int(r[k]['contrib']) == 2 and int(r[k]['n1']) == 1
        np.testing.assert_array_equal(r[k]['w1'], tw.opt.flat.cpu().numpy())
        np.testing.assert_array_equal(r[k]['b1'], tw.opt.buf.cpu().numpy())
        np.testing.assert_array_equal(r[k]['w2'], r[k]['w1'])           # skipped on every rank
        np.testing.assert_array_equal(r[k]['b2'], r[k]['b1'])
        assert int(r[k]['n2']) == 1 and int(r[k]['steps']) == 2
    assert not np.array_equal(r[0]['w1'], r[0]['w0']) and np.isfinite(r[0]['w1']).all()


# ------------------------------------------------------------------ 7. classifier
CLS_SIZES = (2, 3, 5, 33, 70)       # across the fused layer's tile boundaries (32, 64)


def _cls_cfg(aggr):
    from graph_neural_network_for_radar_perception_amd.config import default_classifier_config
    return default_classifier_config(**({} if aggr is None else
                                        {'classifier_aggregation': aggr}))


def _cls_trainer(dev, aggr, optim='sgd', **kw):
    from graph_neural_network_for_radar_perception_amd.classifier import Model_Training
    from graph_neural_network_for_radar_perception_amd.classifier import training as ct
    cfg = _cls_cfg(aggr)
    torch.manual_seed(41)
    m = Model_Training(cfg).to(dev).train()
    return ct.ClassifierTrainer(m, cfg, lr=0.005, weight_decay=1e-4, optim=optim, **kw)


def _cls_batch(dev, seed, nan=False):
    """prepare_batch_objects of two samples of objects of CLS_SIZES members (synthetic
    make_objects' features restated for given sizes: centred positions, range, angle, rcs)."""
    from graph_neural_network_for_radar_perception_amd.classifier import training as ct
    key = ('cls', seed, nan)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    ncls = int(_cls_cfg(None).num_classes)
    nf, osz, gt = [], [], []
    for _ in range(2):
        sizes = rng.permutation(CLS_SIZES).astype(np.int64)
        feats = []
        for n in sizes:
            xy = rng.normal(0.0, 1.0, (int(n), 2)) * rng.uniform(0.3, 2.5, 2)
            xy -= xy.mean(0)
            feats.append(np.stack((xy[:, 0], xy[:, 1], np.hypot(xy[:, 0], xy[:, 1]),
                                   np.arctan2(xy[:, 1], xy[:, 0]),
                                   rng.normal(0.0, 10.0, int(n))), -1))
        nf.append(torch.from_numpy(np.concatenate(feats, 0).astype(np.float32)).to(dev))
        osz.append(torch.from_numpy(sizes).to(dev))
        gt.append(torch.from_numpy(rng.integers(0, ncls, len(sizes)).astype(np.int64)).to(dev))
    if nan:
        # the rcs of every member of the first object: the max reductions (aggregation 'max',
        # the pooling) are fmaxf folds, which drop a NaN beside a number, so one NaN row does
        # not reach the loss under 'max'; an object whose every row is NaN does, in both cases
        nf[0][:int(osz[0][0]), 4] = float('nan')
    _CACHE[key] = ct.prepare_batch_objects(nf, osz, gt)
    return _CACHE[key]


def _cls_hand_iteration(tr, batches, K):
    eng = tr.engine
    g = torch.ones(1, dtype=torch.float32, device=eng.device) / K
    grads, losses = [], []
    for b in batches:
        loss, tape = eng.forward_objects(*b)
        eng.backward(tape, g)
        grads.append(eng.flat_grad.clone())
        losses.append(loss)
    tr.opt.step(_sum(grads), grad_scale=1.0, losses=_sum([lo * g for lo in losses]))
    return losses


def _cls_empty_inputs(dev):
    """test_gpu_classifier_trainer._empty_inputs restated: no object has enough members."""
    from conftest import golden
    from graph_neural_network_for_radar_perception_amd import objects
    d = golden('objects_batch4')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    xy = up(np.stack((d['px'], d['py']), axis=-1))
    inp = objects.classifier_inputs(xy, up(d['rcs']), up(d['cluster_ptr']), up(d['cluster_idx']),
                                    up(d['frame_ptr']), d['noise'],
                                    min_meas=int(d['size'].max()) + 1, node_labels=up(d['labels']))
    assert inp.n_objects == 0
    return inp


@pytest.mark.parametrize('aggr,optim', [(None, 'sgd'), (None, 'adamw'), ('max', 'sgd')])
def test_classifier_k3_equals_the_hand_composed_iteration(cuda_device, aggr, optim):
    dev = cuda_device
    tr, tw = _cls_trainer(dev, aggr, optim), _cls_trainer(dev, aggr, optim)
    w0 = tr.opt.flat.clone()
    fused = [ct_.get('fused') is not None
             for ct_ in tr.engine.forward_objects(*_cls_batch(dev, 1))[1]['conv']]
    assert all(fused) if aggr is None else not any(fused)    # the path the case is about
    for it, seeds in enumerate(((1, 2, 3), (4, 5, 6))):
        group = [_cls_batch(dev, s) for s in seeds]
        got = [tr.accumulate_objects(*b, 3) for b in group]
        assert tr.apply_accumulated() == 3
        want = _cls_hand_iteration(tw, group, 3)
        for x, y in zip(got, want):
            assert x.shape == (1,) and torch.equal(x, y) and bool(torch.isfinite(x).all())
        _same_state(_state(tr), _state(tw), f'{aggr} {optim} iteration {it}')
    assert tr.opt.applied_steps() == 2 and tr.opt.steps == 2
    assert not torch.equal(tr.opt.flat, w0)


@pytest.mark.parametrize('aggr', [None, 'max'])
def test_classifier_nan_micro_batch_skips_the_outer_iteration(cuda_device, aggr):
    dev = cuda_device
    tr = _cls_trainer(dev, aggr, milestones=[1])
    tw = _cls_trainer(dev, aggr, milestones=[1])
    before = _state(tr)
    group = [_cls_batch(dev, 1), _cls_batch(dev, 2, nan=True), _cls_batch(dev, 3)]
    losses = [tr.accumulate_objects(*b, 3) for b in group]
    assert tr.apply_accumulated() == 3
    assert bool(torch.isnan(losses[1]).all())
    assert bool(torch.isfinite(losses[0]).all()) and bool(torch.isfinite(losses[2]).all())
    _same_state(_state(tr), before, 'the skipped iteration')
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 1
    lr0, lr1 = tr.opt.lr_at(0), tr.opt.lr_at(1)
    assert lr1 == lr0 * 0.1
    for it, (seeds, lr) in enumerate((((1, 2, 3), lr0), ((4, 5, 6), lr1))):
        group = [_cls_batch(dev, s) for s in seeds]
        w_before = tr.opt.flat.clone()
        for b in group:
            tr.accumulate_objects(*b, 3)
        assert tr.apply_accumulated() == 3
        _cls_hand_iteration(tw, group, 3)
        _same_state(_state(tr), _state(tw), f'clean iteration {it}')
        step = lr * tr.opt.buf
        err = float((w_before - tr.opt.flat - step).abs().max())
        bound = 2.0 ** -22 * float(w_before.abs().max())
        print(aggr, 'clean iteration', it, 'lr', lr, 'error', err, 'bound', bound,
              'max |lr * buf|', float(step.abs().max()))
        assert err <= bound and float(step.abs().max()) > 10 * bound
    assert tr.opt.applied_steps() == 2 and tr.opt.steps == 3


@pytest.mark.parametrize('aggr', [None, 'max'])
def test_classifier_empty_micro_batches(cuda_device, monkeypatch, aggr):
    from graph_neural_network_for_radar_perception_amd import training
    dev = cuda_device
    tr, tw = _cls_trainer(dev, aggr), _cls_trainer(dev, aggr)
    empty, real = _cls_empty_inputs(dev), _cls_batch(dev, 1)
    # nothing but empty batches on one rank: nothing is launched, no engine is built
    before = _state(tr)
    for inp in (empty, None, empty):
        assert tr.accumulate_inputs(inp, 3) is None
    assert tr.apply_accumulated() == 0
    assert getattr(tr.model, '_train_engine', None) is None
    _same_state(_state(tr), before, '[empty] * 3')
    assert tr.opt.steps == 0 and tr.opt.applied_steps() == 0
    # [empty, real, empty]: the one real gradient at g = 1/3
    assert tr.accumulate_inputs(empty, 3) is None
    loss = tr.accumulate_objects(*real, 3)
    assert tr.accumulate_inputs(None, 3) is None
    assert tr.apply_accumulated() == 1
    want = _cls_hand_iteration(tw, [real], 3)
    assert torch.equal(loss, want[0])
    _same_state(_state(tr), _state(tw), '[empty, real, empty]')
    assert tr.opt.applied_steps() == 1
    # world = 2, the all-reduce stubbed: one call per outer iteration
    tr.world = 2
    calls = []

    def peer_sum(bucket, world):
        assert world == 2
        calls.append((bucket, bucket.clone()))
        return 0.5

    monkeypatch.setattr(training, 'allreduce_gradients', peer_sum)
    before, steps = _state(tr), tr.opt.steps
    for _ in range(3):
        assert tr.accumulate_inputs(empty, 3) is None
    assert tr.apply_accumulated() == 0
    assert len(calls) == 1 and calls[0][0] is tr.accum.bucket
    sent = calls[0][1]
    n = tr.opt.flat.numel()
    assert sent.numel() == n + 1
    assert not bool(sent[:n].any()) and bool(torch.isnan(sent[n:]).all())
    _same_state(_state(tr), before, 'every rank skips')
    assert tr.opt.steps == steps + 1 and tr.opt.applied_steps() == 1
    del calls[:]
    for s in (4, 5, 6):
        tr.accumulate_objects(*_cls_batch(dev, s), 3)
        assert calls == []
    assert tr.apply_accumulated() == 3
    assert len(calls) == 1 and tr.opt.applied_steps() == 2


# ------------------------------------------------------------------ 8. loops
def test_train_sequence_accumulates_in_groups(cuda_device):
    frontend, _, training = _pkg()
    dev = cuda_device
    cfg = _cfg()
    assert cfg.dataset_augmentation is True
    store = _adversarial_store(dev)
    plain, seen1 = _trainer(dev, cfg), []
    np.random.seed(77)
    training.train_sequence(store, plain, cfg, ORDER, window_size=4, batch_windows=3,
                            on_step=lambda k, pos, flags, out: seen1.append((k, list(pos), flags)))
    tr, tw, seen = _trainer(dev, cfg), _trainer(dev, cfg), []
    np.random.seed(77)
    losses, acc = training.train_sequence(
        store, tr, cfg, ORDER, window_size=4, batch_windows=3, grad_accumulation_steps=2,
        on_step=lambda k, pos, flags, out: seen.append((k, list(pos), flags, out)))
    assert [s[0] for s in seen1] == [0, 1, 2, 3, 4]
    assert [s[0] for s in seen] == [0, 0, 1, 1, 2]
    assert [s[1] for s in seen] == [s[1] for s in seen1] == [ORDER[i:i + 3]
                                                             for i in range(0, 13, 3)]
    for s, s1 in zip(seen, seen1):
        np.testing.assert_array_equal(s[2], s1[2])
    assert np.concatenate([s[2] for s in seen]).any()
    assert tr.opt.applied_steps() == 3 and tr.opt.steps == 3
    assert losses.shape == (5, 4) and acc.shape == (5, 3) and losses.is_cuda
    assert bool(torch.isfinite(losses).all())
    # a twin driven by hand through the same micro-batches
    for j, (_, pos, flags, out) in enumerate(seen):
        hand = tw.accumulate_frames(_real_fb(dev, pos, flags), 2)
        assert torch.equal(hand[0], out[0]) and torch.equal(hand[0], losses[j]), j   # unscaled
        if j in (1, 3, 4):
            assert tw.apply_accumulated() == (1 if j == 4 else 2)
    _same_state(_state(tr), _state(tw), 'train_sequence against the hand-driven twin')
    assert not torch.equal(tr.opt.flat, plain.opt.flat)      # five steps are not three


def test_train_dataset_counts_outer_iterations(cuda_device):
    from sequence_set_ref import make_set
    _, sequence, training = _pkg()
    dev = cuda_device
    cfg = _cfg()
    shared = make_set(dev)
    train = sequence.SequenceSet([shared.stores[0], shared.stores[2]])
    val = sequence.SequenceSet([shared.stores[3]])
    W = 4
    n = train.n_windows(W)
    tr = _trainer(dev, cfg)
    steps, vals = [], []
    torch.manual_seed(5)
    np.random.seed(5)
    losses, acc, validations = training.train_dataset(
        train, tr, cfg, val_set=val, val_indices=[0, 7, 30], max_iters=3, batch_windows=2,
        val_period=2, window_size=W, grad_accumulation_steps=2,
        on_step=lambda it, pos, flags, out: steps.append((it, pos.copy(), flags, out)),
        on_validation=lambda it, res: vals.append(it))
    torch.manual_seed(5)
    gen = training.shuffled_batches(n, 2)
    want = [next(gen) for _ in range(6)]
    assert [s[0] for s in steps] == [0, 0, 1, 1, 2, 2]
    for s, w in zip(steps, want):
        np.testing.assert_array_equal(s[1], w)
        assert s[2] is not None and len(s[2]) == 2           # flags per micro-batch
        assert s[3] is not None
    assert losses.shape == (6, 4) and acc.shape == (6, 3) and losses.is_cuda
    for i, s in enumerate(steps):
        assert torch.equal(losses[i], s[3][0]), f'row {i}'
    assert vals == [0, 2] and [v[0] for v in validations] == [0, 2]
    assert tr.opt.applied_steps() == 3 and tr.opt.steps == 3


def test_train_classifier_sequence_accumulates_in_groups(cuda_device):
    """The 40-scene fixture and the model_trained_N50 detector, as
    test_gpu_classifier_trainer builds them: four batches of two windows, K = 2."""
    from conftest import classifier_cfg, golden, model_cfg, model_state_dict
    from graph_neural_network_for_radar_perception_amd.classifier import Model_Training
    from graph_neural_network_for_radar_perception_amd.classifier import training as ct
    from graph_neural_network_for_radar_perception_amd.gnn_detector import \
        Model_Training as Detector_Training
    dev = cuda_device
    store = sref.fixture_store(dev)[1]
    mt = Detector_Training(model_cfg('model_trained_N50'), dev)
    mt.load_state_dict(model_state_dict('model_trained_N50'))
    detector = mt.to(dev).pred.eval().requires_grad_(False)
    detector.set_param_for_proposal_extraction(
        float(golden('proposals_model_trained_N300')['eps']), False)
    cfg = classifier_cfg('classifier_yml')

    def trainer():
        torch.manual_seed(41)
        return ct.ClassifierTrainer(Model_Training(cfg).to(dev).train(), cfg, lr=0.005,
                                    weight_decay=1e-4)

    tr, tw, seen = trainer(), trainer(), []
    np.random.seed(77)
    losses = ct.train_classifier_sequence(
        store, detector, tr, cfg, ORDER[:8], window_size=10, batch_windows=2,
        grad_accumulation_steps=2,
        on_step=lambda k, pos, flags, loss, inp: seen.append((k, list(pos), loss, inp)))
    assert [s[0] for s in seen] == [0, 0, 1, 1]
    assert [s[1] for s in seen] == [ORDER[i:i + 2] for i in range(0, 8, 2)]
    assert all(s[3] is not None and s[3].n_objects > 0 for s in seen)
    assert losses.shape == (4,) and losses.dtype == torch.float32 and losses.is_cuda
    assert bool(torch.isfinite(losses).all())
    assert torch.equal(losses, torch.cat([s[2] for s in seen]))
    assert tr.opt.applied_steps() == 2 and tr.opt.steps == 2
    # the same inputs through a twin by hand
    for j, (_, _, loss, inp) in enumerate(seen):
        begin, end = inp.ranges()
        _cls = (inp.object_features, inp.object_num_meas, begin, end, inp.object_class,
                inp.n_rows, inp.n_edges, inp.max_size)
        seen[j] = _cls
    for group in (seen[:2], seen[2:]):
        _cls_hand_iteration(tw, group, 2)
    _same_state(_state(tr), _state(tw), 'train_classifier_sequence against the hand-composed')
