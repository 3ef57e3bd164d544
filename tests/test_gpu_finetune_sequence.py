"""Object-head finetuning from a sequence in HBM on the GPU (training.py: HeadTrainEngine,
FinetuneTrainer, finetune_sequence, validate_finetune_sequence; gnn_detector.py:
invalidate_head_plans; objects.py: Detections.outputs / x).

Inputs: the reference's own finetuning step (tests/golden/finetune_trained_2frames.npz with
the model_trained_N50 checkpoint, as test_gpu_finetune.py loads them) and the 40-scene sequence
fixture (sequence_ref.fixture_store) at 8 windows of 10 scans, cfg.clustering_eps unchanged.

Tolerances.  Against the reference fixture and against the drop-in's loss.backward() the bounds
are test_gpu_finetune.py's (loss 1e-5 relative, accuracy 1e-6, each gradient 2e-4 max|ref| +
1e-7, + 1e-6 for a one-element gradient): the head-only step differs from both only in the
frozen backbone's arithmetic -- the fused inference kernels against the float32 tape.  Three
trainer steps against three drop-in + torch.optim.SGD steps are read per tensor as
max|w - w_dropin| / max|w_dropin - w_0|: a weight change is a positive combination of
gradients each held to 2e-4, so the ceiling is 3 x 2e-4 (three steps, and a factor for what
differs in later steps); STEP_BOUND is 1.5 x the worst reading over three input seeds on the
MI355X (profiles/finetune_head_step.jsonl), as BOUNDS of test_half_emulation.py is set.  Two
runs of the same launches on the same values are compared with torch.equal.  The validation
mean is within 1e-6 relative of the drop-in's eval-mode losses."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from conftest import golden
from sequence_ref import fixture_store
from test_gpu_finetune import _args, _finetune_model

pytestmark = pytest.mark.gpu

FIXTURE = 'finetune_trained_2frames'
POSITIONS = [14, 3, 9, 0, 20, 7, 7, 11]          # the caller's order, a repeat
W = 10
LR, WD, MOMENTUM = 0.01, 1e-4, 0.9
STEP_CEILING = 3 * 2e-4
# 1.5 x the worst per-tensor reading of test_three_steps_follow_the_dropin over its three
# seeds on an MI355X (profiles/finetune_head_step.jsonl: worst 1.110e-05, seed 2, the first
# stem layer's norm scale; every other tensor <= 6.6e-07)
STEP_BOUND = 1.67e-5
SEEDS = (0, 1, 2)
_CACHE = {}


def _pkg():
    from graph_neural_network_for_radar_perception_amd import frontend, objects, training
    return frontend, objects, training


def _store(dev):
    if 'store' not in _CACHE:
        _CACHE['store'] = fixture_store(dev)[1]
    return _CACHE['store']


def _model(dev, state=None, cfg_kw=None, seed=None):
    """The finetuning model, frozen as the reference freezes it: the trained checkpoint, a
    given state_dict, or (cfg_kw, seed) a seeded initialisation of another configuration."""
    from graph_neural_network_for_radar_perception_amd.config import default_config
    from graph_neural_network_for_radar_perception_amd.gnn_detector import \
        Model_Object_Classifier_Finetuning
    if state is None and cfg_kw is None:
        return _finetune_model(dev)
    cfg = default_config(**(cfg_kw or {}))
    if seed is not None:
        torch.manual_seed(seed)
    m = Model_Object_Classifier_Finetuning(cfg)
    if state is not None:
        m.load_state_dict(state)
    m = m.to(dev)
    m.pred.freeze_layers_except_object_class_predictor()
    return m, cfg


def _detect_fixture(m, dev):
    """objects.detect of the fixture's two frames and their node classes [N]."""
    objects = _pkg()[1]
    a = _args(golden(FIXTURE), dev)
    det = objects.detect(m.pred, a['node_features'], a['edge_features'], a['edge_index'],
                         a['other_features'])
    return det, torch.cat(a['node_class_labels'], 0), a


def _head_step(m, cfg, det, node_class):
    """One head-only forward and backward on the model's head engine, no update."""
    objects = _pkg()[1]
    eng = m.head_engine()
    ncl = int(det.cluster_ptr.numel()) - 1
    gt = objects.majority_class(node_class, det.cluster_ptr, det.cluster_idx, cfg.num_classes)
    loss, acc, tape = eng.forward(det.outputs.x, det.cluster_ptr, det.cluster_idx, ncl, gt,
                                  det.frame_ptr, len(det.frame_sizes))
    eng.backward(tape, torch.ones(1, dtype=torch.float32, device=eng.device))
    return eng, loss, acc


def _head_names(m):
    return [n for n, _ in m.named_parameters() if n.startswith('pred.predict_class.')]


def _grad_check(name, got, ref):
    ref = ref.astype(np.float64)
    tol = 2e-4 * float(np.max(np.abs(ref))) + (1e-6 if ref.size == 1 else 1e-7)
    err = float(np.max(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)))
    print(f'{name}: err {err:.3e} tol {tol:.3e} ({err / tol:.3f} of it)')
    return err, tol


def frame_lists(fb, gb):
    """The drop-in's per-frame list arguments from a batch on the device: each frame's rows of
    the node features, its destination-major edges (source -> destination, frame-local) with
    their features, its positions and its node classes."""
    g = gb.graph
    fp = fb.frame_ptr.cpu().tolist()
    ep = g.seg_ptr[fb.frame_ptr.to(torch.int64)].cpu().tolist()
    xy = torch.stack((fb.arrays['meas_px'], fb.arrays['meas_py']), dim=-1)
    out = dict(node_features=[], edge_features=[], other_features=[], edge_index=[],
               adj_matrix=[], node_class_labels=[])
    for f in range(fb.n_frames):
        a, b, e0, e1 = fp[f], fp[f + 1], ep[f], ep[f + 1]
        out['node_features'].append(gb.node_features[a:b])
        out['edge_features'].append(gb.edge_features[e0:e1])
        out['edge_index'].append(torch.stack((g.src[e0:e1], g.dst[e0:e1]), 0).to(torch.int64) - a)
        out['other_features'].append(xy[a:b])
        out['adj_matrix'].append(None)
        out['node_class_labels'].append(fb.labels['class_labels'][a:b])
    return out


def _batch(dev, pos, flags=None):
    frontend = _pkg()[0]
    dd, gd = frontend.dynamic_frame(_store(dev).windows(pos, W), False, with_keys=True,
                                    flip=flags)
    return frontend.frame_batch(dd, gd)


# ------------------------------------------------------------------ G1
def test_head_only_step_matches_reference(cuda_device):
    """The reference's own finetuning step (loss.backward() of its
    Model_Object_Classifier_Finetuning on two frames): loss, accuracy and every predict_class
    gradient of the head-only step, from objects.detect's node embeddings."""
    dev = cuda_device
    d = golden(FIXTURE)
    m, cfg = _model(dev)
    det, node_class, _ = _detect_fixture(m, dev)
    assert det.outputs.x is det.x and det.x.dtype == torch.float32
    assert det.x.shape[0] == node_class.shape[0]
    eng, loss, acc = _head_step(m, cfg, det, node_class)
    want = float(d['loss'])
    print('loss', float(loss), 'reference', want, 'accuracy', float(acc), float(d['accuracy']))
    assert loss.shape == (1,) and acc.shape == (1,) and loss.is_cuda
    assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want)), (float(loss), want)
    assert abs(float(acc) - float(d['accuracy'])) <= 1e-6
    names = _head_names(m)
    assert sorted('g/' + n for n in names) == sorted(k for k in d.files if k.startswith('g/'))
    params = dict(m.named_parameters())
    worst = []
    for n in names:
        err, tol = _grad_check(n, eng.grads[id(params[n])], d['g/' + n])
        worst.append((err <= tol, n, err, tol))
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]
    n_head = sum(params[n].numel() for n in names)
    assert eng.flat_bucket.numel() == n_head + 1 and eng.loss_slots.numel() == 1
    assert eng.flat_grad.numel() == n_head
    assert eng.flat_grad.data_ptr() == eng.flat_bucket.data_ptr()
    assert [id(p) for p in eng.params] == [id(params[n]) for n in names]
    assert all(p.grad is None for p in m.parameters())      # nothing went through autograd


# ------------------------------------------------------------------ G2
@pytest.mark.parametrize('case', ['yml', 'layer'])
def test_head_only_step_matches_the_dropin_backward(cuda_device, case):
    """The same step against Model_Object_Classifier_Finetuning(...).backward() on a twin of
    the same weights and the same frames: the trained yml model, and a seeded model with layer
    normalisation (the frame-wide statistics of the stem's node rows and the head's cluster
    rows)."""
    dev = cuda_device
    kw = dict() if case == 'yml' else dict(cfg_kw=dict(norm_layer='layer_normalization'),
                                           seed=11)
    m, cfg = _model(dev, **kw)
    twin, _ = _model(dev, **kw)
    for a, b in zip(m.parameters(), twin.parameters()):
        assert torch.equal(a, b)
    det, node_class, args = _detect_fixture(m, dev)
    eng, loss, acc = _head_step(m, cfg, det, node_class)
    assert eng.frame_norm == (case == 'layer')
    twin.train()
    loss_t, acc_t = twin(**args)
    loss_t.backward()
    print(case, 'loss', float(loss), 'drop-in', float(loss_t.detach()), 'clusters',
          int(det.cluster_ptr.numel()) - 1)
    want = float(loss_t.detach())
    assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want))
    assert abs(float(acc) - float(acc_t)) <= 1e-6
    bad = []
    params, tparams = dict(m.named_parameters()), dict(twin.named_parameters())
    for n in _head_names(m):
        ref = tparams[n].grad.detach().cpu().numpy()
        assert float(np.abs(ref).max()) > 0, n
        err, tol = _grad_check(f'{case} {n}', eng.grads[id(params[n])], ref)
        if err > tol:
            bad.append((n, err, tol))
    assert not bad, bad


# ------------------------------------------------------------------ G3
def _three_steps(dev, seed):
    """Three FinetuneTrainer steps and three drop-in + torch.optim.SGD steps on one batch of
    four windows drawn by ``seed``: ({tensor: reading}, trainer, w_0 state_dict)."""
    _, objects, training = _pkg()
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
    store = _store(dev)
    pos = np.random.default_rng(seed).choice(store.n_windows(W), 4, replace=False)
    fb = _batch(dev, pos)
    m, cfg = _model(dev)
    twin, _ = _model(dev)
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = training.FinetuneTrainer(m, cfg, lr=LR, weight_decay=WD, optim='sgd',
                                  momentum=MOMENTUM)
    opt = torch.optim.SGD([p for p in twin.parameters() if p.requires_grad], lr=LR,
                          momentum=MOMENTUM, weight_decay=WD)
    lists = frame_lists(fb, build_graph_batch(fb, cfg))
    twin.train()
    cache = {}
    for it in range(3):
        det = objects.detect_frames(m.pred, fb, cfg, cache=cache)
        loss, acc = tr.step_detections(det, fb.labels['class_labels'])
        opt.zero_grad()
        loss_t, acc_t = twin(**lists)
        loss_t.backward()
        opt.step()
        print(f'seed {seed} step {it}: loss {float(loss):.6f} drop-in {float(loss_t.detach()):.6f} '
              f'accuracy {float(acc):.4f} {float(acc_t):.4f} '
              f'clusters {int(det.cluster_ptr.numel()) - 1}')
        assert bool(torch.isfinite(loss).all())
    assert tr.opt.applied_steps() == 3
    new, ref = m.state_dict(), twin.state_dict()
    readings = {}
    for n in _head_names(m):
        moved = float((ref[n] - w0[n]).abs().max())
        assert moved > 0, n
        readings[n] = float((new[n] - ref[n]).abs().max()) / moved
    return readings, tr, w0


@pytest.mark.parametrize('seed', SEEDS)
def test_three_steps_follow_the_dropin(cuda_device, seed):
    """Three trainer steps against three drop-in steps with torch.optim.SGD (momentum 0.9, the
    same lr and weight decay) from one checkpoint: per predict_class tensor
    max|w - w_dropin| / max|w_dropin - w_0| <= STEP_BOUND, and every other parameter
    bit-unchanged.  $RG_FINETUNE_REPORT: a file the readings are appended to."""
    readings, tr, w0 = _three_steps(cuda_device, seed)
    worst = max(readings.values())
    for n, r in readings.items():
        print(f'seed {seed} {n}: {r:.3e} ({r / STEP_BOUND:.3f} of the bound)')
    path = os.environ.get('RG_FINETUNE_REPORT')
    if path:
        with open(path, 'a') as fh:
            fh.write(json.dumps({'test': 'three_steps_follow_the_dropin', 'seed': seed,
                                 'worst': worst, 'ceiling': STEP_CEILING, 'bound': STEP_BOUND,
                                 'tensors': readings}) + '\n')
    assert STEP_BOUND <= STEP_CEILING
    assert worst <= STEP_BOUND, (worst, STEP_BOUND)
    for k, v in tr.model.state_dict().items():
        if not k.startswith('pred.predict_class.'):
            assert torch.equal(v, w0[k]), k


def test_adamw_step_and_a_bad_label(cuda_device):
    """cfg.optim_finetuning = 'adamw': one step moves predict_class alone.  A node class
    outside [0, num_classes) then puts NaN in the loss slot: that step is skipped on the
    device (weights, both moments and the applied count stay), without a host read."""
    training = _pkg()[2]
    dev = cuda_device
    m, cfg = _model(dev)
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = training.FinetuneTrainer(m, cfg, lr=LR, weight_decay=WD, optim='adamw')
    det, node_class, _ = _detect_fixture(m, dev)
    loss, acc = tr.step_detections(det, node_class)
    assert bool(torch.isfinite(loss).all()) and tr.opt.applied_steps() == 1
    assert torch.equal(tr.engine.loss_slots, loss)
    for k, v in m.state_dict().items():
        assert torch.equal(v, w0[k]) != k.startswith('pred.predict_class.'), k
    flat, state = tr.opt.flat.clone(), [b.clone() for b in tr.opt.state_bufs]
    bad = node_class.clone()
    bad[int(det.cluster_idx[0])] = cfg.num_classes
    loss, _ = tr.step_detections(_detect_fixture(m, dev)[0], bad)
    assert bool(torch.isfinite(loss).all())          # the loss of the labels that counted
    assert bool(torch.isnan(tr.engine.loss_slots).all())
    assert torch.equal(tr.opt.flat, flat)
    for a, b in zip(tr.opt.state_bufs, state):
        assert torch.equal(a, b)
    assert tr.opt.applied_steps() == 1 and tr.opt.steps == 2
    with pytest.raises(ValueError, match='node classes'):
        tr.step_detections(det, node_class[:-1])


# ------------------------------------------------------------------ G4
def test_packed_images_follow_the_head(cuda_device):
    """Every image packed from predict_class exists before training (the inference plans by
    objects.detect, both train engines' chains by one drop-in forward and backward, the head
    engine's by its own step).  After three trainer steps the trained model's proposal forward
    equals, bit for bit, that of a fresh model built from its state_dict, and so does the
    drop-in's training forward and backward.

    Fails with FinetuneTrainer's on_update re-pack turned into a no-op
    (Model_Object_Classifier_Finetuning.invalidate_head_plans = lambda self: None): the old
    model then keeps computing its object logits from the first step's images (checked once on
    an MI355X: obj_cls differs from the fresh model's)."""
    _, objects, training = _pkg()
    dev = cuda_device
    m, cfg = _model(dev)
    det0, node_class, args = _detect_fixture(m, dev)
    before = det0.obj_cls.clone()
    m.train()
    m(**args)[0].backward()
    for p in m.parameters():
        p.grad = None
    _head_step(m, cfg, det0, node_class)
    tr = training.FinetuneTrainer(m, cfg, lr=LR, weight_decay=WD)
    assert tr.engine is m.head_engine()
    det = _detect_fixture(m, dev)[0]
    assert torch.equal(det.obj_cls, before)          # the same values from the flat buffer
    w0 = tr.opt.flat.clone()
    for _ in range(3):
        det = _detect_fixture(m, dev)[0]
        loss, _ = tr.step_detections(det, node_class)
        assert bool(torch.isfinite(loss).all())
    assert tr.opt.applied_steps() == 3 and not torch.equal(tr.opt.flat, w0)
    fresh, _ = _model(dev, state={k: v.detach().clone() for k, v in m.state_dict().items()})
    for a, b in zip(m.parameters(), fresh.parameters()):
        assert torch.equal(a, b)
    got, want = _detect_fixture(m, dev)[0], _detect_fixture(fresh, dev)[0]
    assert torch.equal(got.cluster_ptr, want.cluster_ptr)
    assert torch.equal(got.cluster_idx, want.cluster_idx)
    for k in ('node_cls', 'node_reg', 'link_cls', 'x'):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert torch.equal(got.obj_cls, want.obj_cls), 'stale inference image of the object head'
    assert not torch.equal(got.obj_cls, before)
    # the head engine and the drop-in's train engine
    eng, loss_o, _ = _head_step(m, cfg, got, node_class)
    eng_f, loss_f, _ = _head_step(fresh, cfg, want, node_class)
    assert eng_f is not eng
    assert torch.equal(loss_o, loss_f), 'stale head-engine image (forward)'
    assert torch.equal(eng.flat_grad, eng_f.flat_grad), 'stale head-engine image (backward)'
    fresh.train()
    lo, lf = m(**args)[0], fresh(**args)[0]
    lo.backward()
    lf.backward()
    assert torch.equal(lo.detach(), lf.detach()), 'stale train-engine image'
    for (n, a), b in zip(m.named_parameters(), fresh.parameters()):
        if a.requires_grad:
            assert torch.equal(a.grad, b.grad), n


# ------------------------------------------------------------------ G5
def test_finetune_sequence_two_batches(cuda_device):
    """Two batches of four windows, np.random.seed fixed: every batch steps the trainer
    exactly as the stages called by hand with the same flags do (a twin trainer, stepped
    inside on_step, ends every step with bit-equal losses, accuracies and weights)."""
    frontend, objects, training = _pkg()
    dev = cuda_device
    store = _store(dev)
    assert max(POSITIONS) < store.n_windows(W)
    m, cfg = _model(dev)
    twin, _ = _model(dev)
    assert cfg.dataset_augmentation is True
    tr = training.FinetuneTrainer(m, cfg, lr=LR, weight_decay=WD)
    tw = training.FinetuneTrainer(twin, cfg, lr=LR, weight_decay=WD)
    before = tr.opt.flat.clone()
    seen = []

    def on_step(k, pos, flags, out, det):
        seen.append((k, list(pos), flags, out, det))
        fb = _batch(dev, pos, flags)
        hand = objects.detect_frames(twin.pred, fb, cfg)
        out_h = tw.step_detections(hand, fb.labels['class_labels'])
        assert torch.equal(hand.cluster_ptr, det.cluster_ptr)
        assert torch.equal(out_h[0], out[0]) and torch.equal(out_h[1], out[1])
        assert torch.equal(tr.opt.flat, tw.opt.flat), f'step {k}'

    np.random.seed(77)
    losses, accs = training.finetune_sequence(store, tr, cfg, POSITIONS, window_size=W,
                                              batch_windows=4, on_step=on_step)
    np.random.seed(77)
    want_flags = [frontend.draw_flips(4) for _ in range(2)]
    assert [s[0] for s in seen] == [0, 1]
    assert [s[1] for s in seen] == [POSITIONS[:4], POSITIONS[4:]]
    for s, w in zip(seen, want_flags):
        np.testing.assert_array_equal(s[2], w)
    assert np.concatenate(want_flags).any() and not np.concatenate(want_flags).all()
    print('losses', losses.tolist(), 'accuracies', accs.tolist(), 'clusters',
          [int(s[4].cluster_ptr.numel()) - 1 for s in seen])
    assert losses.shape == (2,) and accs.shape == (2,) and losses.is_cuda and accs.is_cuda
    assert losses.dtype == accs.dtype == torch.float32
    assert bool(torch.isfinite(losses).all()) and bool(((accs >= 0) & (accs <= 1)).all())
    assert torch.equal(losses, torch.cat([s[3][0] for s in seen]))
    assert torch.equal(accs, torch.cat([s[3][1] for s in seen]))
    assert tr.opt.applied_steps() == 2 and tw.opt.applied_steps() == 2
    assert not torch.equal(tr.opt.flat, before)
    # the run trained on something: several proposals of several members, two classes
    for s in seen:
        sizes = np.diff(s[4].cluster_ptr.cpu().numpy())
        assert len(sizes) >= 8 and sizes.max() >= 3, sizes
    # augmentation off: nothing is drawn
    state = np.random.get_state()[1].copy()
    training.finetune_sequence(store, tr, cfg, POSITIONS[:2], window_size=W, batch_windows=2,
                               augmentation=False,
                               on_step=lambda k, pos, flags, out, det: seen.append(flags))
    assert seen[-1] is None
    np.testing.assert_array_equal(np.random.get_state()[1], state)
    assert tr.opt.applied_steps() == 3


def _no_frame_store(dev):
    """Six small scenes (test_gpu_training_feed._static_store): the windows of 2 scans at 0
    and 1 hold no / one dynamic node, so a batch of them has no frame."""
    import sequence_ref as sref
    from graph_neural_network_for_radar_perception_amd import sequence
    sizes = (30, 20, 25, 40, 45, 33)
    kinds = ('static', 'static', 'static+1', 'mixed', 'mixed', 'mixed')
    radar, odo, lists, sensors = sref.make_sequence(11, sizes, kinds)
    return sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)


def test_finetune_sequence_batch_without_a_frame(cuda_device, monkeypatch):
    """A batch whose windows give no frame: no row, no step, nothing launched on one rank (not
    even the head engine's first packing); on one of several ranks the rank joins the
    all-reduce (stubbed) with zero gradients and a NaN slot, and the update is skipped."""
    frontend, _, training = _pkg()
    dev = cuda_device
    store = _no_frame_store(dev)
    dd, gd = frontend.dynamic_frame(store.windows([0, 1], 2), with_keys=True)
    assert frontend.frame_batch(dd, gd).n_frames == 0
    m, cfg = _model(dev)
    tr = training.FinetuneTrainer(m, cfg, lr=LR, weight_decay=WD)
    before = tr.opt.flat.clone()
    seen = []
    losses, accs = training.finetune_sequence(
        store, tr, cfg, [0, 1], window_size=2, batch_windows=2, augmentation=False,
        on_step=lambda k, pos, flags, out, det: seen.append((k, out, det)))
    assert seen == [(0, None, None)]
    assert losses.shape == (0,) and accs.shape == (0,) and losses.is_cuda
    assert getattr(m, '_head_engine', None) is None
    assert torch.equal(tr.opt.flat, before)
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 0
    # world = 2
    tr.world = 2
    eng = tr.engine
    eng.flat_grad.fill_(3.0)                  # stale values the branch must clear
    calls = []

    def peer_sum(bucket, world):
        assert bucket is eng.flat_bucket and world == 2
        assert not bool(eng.flat_grad.any()) and bool(torch.isnan(eng.loss_slots).all())
        calls.append(world)
        bucket.add_(0.25)                     # the other rank's contribution
        return 0.5

    monkeypatch.setattr(training, 'allreduce_gradients', peer_sum)
    losses, _ = training.finetune_sequence(store, tr, cfg, [0, 1], window_size=2,
                                           batch_windows=2, augmentation=False)
    assert losses.shape == (0,) and calls == [2]
    assert bool((eng.flat_grad == 0.25).all()) and bool(torch.isnan(eng.loss_slots).all())
    assert torch.equal(tr.opt.flat, before)
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 1


# ------------------------------------------------------------------ G6
def test_validate_finetune_sequence(cuda_device):
    """Two batches of four windows: the mean of the drop-in's eval-mode, no_grad losses and
    accuracies over the same frames (its per-frame lists made from the same batches)."""
    _, objects, training = _pkg()
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
    dev = cuda_device
    store = _store(dev)
    m, cfg = _model(dev)
    tr = training.FinetuneTrainer(m, cfg, lr=LR, weight_decay=WD)
    fb0 = _batch(dev, POSITIONS[:4])
    tr.step_detections(objects.detect_frames(m.pred, fb0, cfg), fb0.labels['class_labels'])
    w0, s0 = tr.opt.flat.clone(), [b.clone() for b in tr.opt.state_bufs]
    assert bool(s0[0].any())                      # optimizer state that is not all zero
    n0, steps0 = tr.opt.applied_steps(), tr.opt.steps
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    state = np.random.get_state()[1].copy()
    mean, acc, n = training.validate_finetune_sequence(store, m, cfg, POSITIONS, window_size=W,
                                                       batch_windows=4)
    np.testing.assert_array_equal(np.random.get_state()[1], state)      # no flip is drawn
    want, want_acc = [], []
    m.eval()
    with torch.no_grad():
        for pos in (POSITIONS[:4], POSITIONS[4:]):
            fb = _batch(dev, pos)
            lo, ac = m(**frame_lists(fb, build_graph_batch(fb, cfg)))
            want.append(float(lo))
            want_acc.append(float(ac))
    print('validation losses', want, 'accuracies', want_acc, 'mean', mean, acc, 'counted', n)
    assert n == 2 and all(v > 0 and np.isfinite(v) for v in want)
    ref, ref_acc = float(np.mean(want)), float(np.mean(want_acc))
    assert abs(mean - ref) <= 1e-6 * abs(ref), (mean, ref)
    assert abs(acc - ref_acc) <= 1e-6 * max(abs(ref_acc), 1e-30), (acc, ref_acc)
    assert torch.equal(tr.opt.flat, w0)
    for a, b in zip(tr.opt.state_bufs, s0):
        assert torch.equal(a, b)
    assert tr.opt.applied_steps() == n0 == 1 and tr.opt.steps == steps0
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    # nothing to validate on
    none = training.validate_finetune_sequence(_no_frame_store(dev), m, cfg, [0, 1],
                                               window_size=2, batch_windows=2)
    assert np.isnan(none[0]) and np.isnan(none[1]) and none[2] == 0


# ------------------------------------------------------------------ G7
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world),
                      RANK=str(rank), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    _, _, training = _pkg()
    dev = torch.device('cuda', 0)
    m, cfg = _model(dev)
    tr = training.FinetuneTrainer(m, cfg, world=world, lr=LR, weight_decay=WD)
    tr.opt.buf.fill_(0.125)                       # momentum a skipped step must keep
    w0, b0 = tr.opt.flat.clone(), tr.opt.buf.clone()
    if rank == 0:
        det, node_class, _ = _detect_fixture(m, dev)
        out = tr.step_detections(det, node_class)
        finite = bool(torch.isfinite(out[0]).all())
    else:                                         # a batch without a proposal
        out = tr.step_detections(None, None)
        finite = out is None
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f'ft{rank}.npz'), finite=finite,
             same_w=bool(torch.equal(tr.opt.flat, w0)), same_b=bool(torch.equal(tr.opt.buf, b0)),
             applied=tr.opt.applied_steps(), steps=tr.opt.steps,
             slot_nan=bool(torch.isnan(tr.engine.loss_slots).all()), w=tr.opt.flat.cpu().numpy())
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_one_without_a_proposal(tmp_path, cuda_device):
    """Two gloo ranks on the one card: rank 0 steps on the fixture's frames, rank 1's batch has
    no proposal.  Rank 1 joins the all-reduce with NaN in its loss slot, so both ranks skip:
    head weights and momentum bit-unchanged on both, one launch counted, none applied -- and
    neither rank waits for the other (the processes join)."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_rank_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [np.load(tmp_path / f'ft{r}.npz') for r in range(world)]
    for r, d in enumerate(res):
        assert bool(d['finite']), r               # rank 0's own loss was finite
        assert bool(d['slot_nan']), r             # the summed loss every rank saw
        assert bool(d['same_w']) and bool(d['same_b']), r
        assert int(d['applied']) == 0 and int(d['steps']) == 1, r
    np.testing.assert_array_equal(res[0]['w'], res[1]['w'])
