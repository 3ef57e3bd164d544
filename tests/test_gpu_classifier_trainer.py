"""The classifier's trainer and loop on the GPU (classifier/training.py: ClassifierTrainer,
train_classifier_sequence, validate_classifier_sequence; classifier/classifier.py:
invalidate_plans; objects.py: ClassifierInputs.max_size, detect_frames).

Model and samples are tests/golden/classifier_yml.npz, as test_gpu_classifier.py builds them;
the sequence is the 40-scene fixture (sequence_ref.fixture_store) with the model_trained_N50
detector and the proposals fixture's eps, as test_gpu_sequence.py builds them.

Tolerances: the optimizer arithmetic is held to test_gpu_optim.py's bounds for the same
kernels (SGD 2e-7 max|w| + 1e-9; AdamW 1e-6 relative with the 1e-3 floor); every other
comparison is between two runs of the same launches on the same values and is torch.equal
(the fused backward and the ordered pooling backward are bit-reproducible);
the validation mean is within 1e-6 relative (only the host mean differs)."""
import numpy as np
import pytest
import torch

from conftest import classifier_cfg, classifier_samples, golden, model_cfg, model_state_dict
from sequence_ref import fixture_store

pytestmark = pytest.mark.gpu

NAME = 'classifier_yml'
ORDER = [14, 3, 9, 0, 20, 7, 7, 11, 1, 18, 5, 16, 2]        # the caller's order, a repeat
_CACHE = {}


def _pkg():
    from graph_neural_network_for_radar_perception_amd import frontend, objects
    from graph_neural_network_for_radar_perception_amd import training as det_training
    from graph_neural_network_for_radar_perception_amd.classifier import engine as ce
    from graph_neural_network_for_radar_perception_amd.classifier import training as ct
    return frontend, objects, det_training, ce, ct


def _model(dev, state=None):
    from graph_neural_network_for_radar_perception_amd.classifier import Model_Training
    m = Model_Training(classifier_cfg(NAME))
    if state is None:
        d = golden(NAME)
        state = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith('w/')}
    m.load_state_dict(state)
    return m.to(dev).train()


def _lists(dev):
    ss = classifier_samples(golden(NAME))
    return ([s['nf'].to(dev) for s in ss], [s['ei'].to(dev) for s in ss],
            [s['osz'].to(dev) for s in ss], [s['gt'].to(dev) for s in ss])


def _batch(dev, nan=False):
    """prepare_batch_objects of the fixture's samples; nan: the first row's rcs is NaN (the
    first object pools its own rows only, classifier.py:60-62, so its logits are NaN)."""
    ct = _pkg()[4]
    nf, _, osz, gt = _lists(dev)
    if nan:
        nf = [t.clone() for t in nf]
        nf[0][0, 4] = float('nan')
    return ct.prepare_batch_objects(nf, osz, gt)


def _trainer(m, optim='sgd', **kw):
    ct = _pkg()[4]
    return ct.ClassifierTrainer(m, classifier_cfg(NAME), lr=0.005, weight_decay=1e-4,
                                optim=optim, **kw)


def _detector(dev):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    name = 'model_trained_N50'
    mt = Model_Training(model_cfg(name), dev)
    mt.load_state_dict(model_state_dict(name))
    m = mt.to(dev).pred.eval().requires_grad_(False)
    m.set_param_for_proposal_extraction(float(golden('proposals_model_trained_N300')['eps']),
                                        False)
    return m


def _sequence(dev):
    if 'seq' not in _CACHE:
        _CACHE['seq'] = (fixture_store(dev)[1], _detector(dev))
    return _CACHE['seq']


# ------------------------------------------------------------------ 1. optimizer arithmetic
@pytest.mark.parametrize('optim', ['sgd', 'adamw'])
def test_step_objects_optimizer_arithmetic_matches_torch(cuda_device, optim):
    """Six step_objects calls, the third on a batch with a NaN rcs: the step's own gradients
    (engine.flat_grad) fed to torch.optim + MultiStepLR with the reference's rule (no
    opt.step(), no sched.step() on a NaN loss) give the same weights after every step."""
    dev = cuda_device
    nan_step, steps, ms = 2, 6, [1, 3]
    m = _model(dev)
    tr = _trainer(m, optim, milestones=ms)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in tr.opt.params]
    if optim == 'sgd':
        opt_t = torch.optim.SGD(ref, lr=0.005, momentum=0.9, weight_decay=1e-4)
    else:
        opt_t = torch.optim.AdamW(ref, lr=0.005, weight_decay=1e-4)
    sch_t = torch.optim.lr_scheduler.MultiStepLR(opt_t, milestones=ms, gamma=0.1)
    clean, bad = _batch(dev), _batch(dev, nan=True)
    lrs = []
    for it in range(steps):
        w0 = tr.opt.flat.clone()
        s0 = [b.clone() for b in tr.opt.state_bufs]
        loss = tr.step_objects(*(bad if it == nan_step else clean))
        assert loss.shape == (1,) and loss.dtype == torch.float32 and loss.is_cuda
        grad, slot = tr.engine.flat_grad.clone(), tr.engine.loss_slots.clone()
        assert torch.equal(slot, loss) or (torch.isnan(slot).all() and torch.isnan(loss).all())
        if it == nan_step:
            assert bool(torch.isnan(slot).all())
            assert torch.equal(tr.opt.flat, w0), 'a skipped step changed the weights'
            for a, b in zip(tr.opt.state_bufs, s0):
                assert torch.equal(a, b), 'a skipped step changed the optimizer state'
        else:
            assert bool(torch.isfinite(slot).all()) and bool(torch.isfinite(grad).all())
            o = 0
            for p in ref:
                p.grad = grad[o:o + p.numel()].view_as(p).clone()
                o += p.numel()
            lrs.append(opt_t.param_groups[0]['lr'])
            opt_t.step()
            sch_t.step()
            assert not torch.equal(tr.opt.flat, w0)
        opt_t.zero_grad(set_to_none=True)
        want = torch.cat([p.detach().reshape(-1) for p in ref])
        if optim == 'sgd':
            err = float((tr.opt.flat - want).abs().max())
            bound = 2e-7 * float(want.abs().max()) + 1e-9
        else:
            err = float(((tr.opt.flat - want).abs() / (want.abs() + 1e-3)).max())
            bound = 1e-6
        print(optim, 'step', it, 'loss', float(loss), 'weight error', err, 'bound', bound)
        assert err <= bound, (it, err, bound)
    assert tr.opt.applied_steps() == steps - 1 and tr.opt.steps == steps
    assert [tr.opt.lr_at(k) for k in range(len(lrs))] == lrs
    assert len(set(lrs)) == 3                           # both milestones were crossed


# ------------------------------------------------------------------ 2. gradients
def test_step_objects_gradients_equal_forward_objects_backward(cuda_device):
    """engine.flat_grad after one step_objects == the concatenated p.grad of
    Model_Training.forward_objects(...).backward() on a twin model: the same launches on the
    same values."""
    dev = cuda_device
    tr = _trainer(_model(dev))
    loss = tr.step_objects(*_batch(dev))
    twin = _model(dev)
    nf, _, osz, gt = _lists(dev)
    loss2 = twin.forward_objects(nf, osz, gt)
    loss2.backward()
    want = torch.cat([p.grad.reshape(-1) for p in twin.parameters()])
    assert torch.equal(loss.reshape(()), loss2.detach())
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(tr.engine.flat_grad, want)


# ------------------------------------------------------------------ 3. no stale image
@pytest.mark.parametrize('optim', ['sgd', 'adamw'])
def test_no_packed_image_is_stale_after_training_steps(cuda_device, optim):
    """Every packed image exists before training (the inference ChainPlans and ConvPlans,
    each ClsFusedPlan's forward set; the train chains' and the backward set by one taped
    forward and backward); after three steps the old model computes what a fresh model built from its
    state_dict computes, bit for bit -- on the inference paths and on a fourth training
    forward and backward.  An owner invalidate_plans misses keeps its old weights here."""
    _, _, _, ce, ct = _pkg()
    dev = cuda_device
    m = _model(dev)
    nf, ei, osz, gt = _lists(dev)
    batch = _batch(dev)
    bnf, bosz, begin, end, labels, n_nodes, n_edges, max_size = batch
    with torch.no_grad():       # before the optimizer re-homes the parameters, too
        before_pred = m.predict(nf, ei, osz).clone()
        m.forward_objects(nf, osz, gt)
        before_obj = ce.forward_objects(m.pred, bnf, bosz, begin, end, 'fp32', n_nodes,
                                        n_edges).clone()
    # one taped forward and backward too, so the train chains' images and each ClsFusedPlan's
    # backward set exist before the trainer is built (no_grad cannot make them)
    m.forward_objects(nf, osz, gt).backward()
    for p in m.parameters():
        p.grad = None
    eng0 = m.train_engine()
    tr = _trainer(m, optim)
    assert tr.engine is eng0
    with torch.no_grad():       # and after: the same values from the flat buffer
        assert torch.equal(m.predict(nf, ei, osz), before_pred)
        assert torch.equal(ce.forward_objects(m.pred, bnf, bosz, begin, end, 'fp32', n_nodes,
                                              n_edges), before_obj)
    w0 = tr.opt.flat.clone()
    for _ in range(3):          # every step after the first runs on re-packed images
        assert bool(torch.isfinite(tr.step_objects(*batch)).all())
    assert tr.opt.applied_steps() == 3 and not torch.equal(tr.opt.flat, w0)
    fresh = _model(dev, {k: v.detach().clone() for k, v in m.state_dict().items()})
    for a, b in zip(m.parameters(), fresh.parameters()):
        assert torch.equal(a, b)
    with torch.no_grad():
        got_obj = ce.forward_objects(m.pred, bnf, bosz, begin, end, 'fp32', n_nodes, n_edges)
        want_obj = ce.forward_objects(fresh.pred, bnf, bosz, begin, end, 'fp32', n_nodes,
                                      n_edges)
        got_pred, want_pred = m.predict(nf, ei, osz), fresh.predict(nf, ei, osz)
        got_loss, want_loss = m.forward_objects(nf, osz, gt), fresh.forward_objects(nf, osz, gt)
    assert torch.equal(got_obj, want_obj), 'stale fused-layer / chain image (forward_objects)'
    assert torch.equal(got_pred, want_pred), 'stale inference plan (edge-list predict)'
    assert torch.equal(got_loss, want_loss)
    assert not torch.equal(got_obj, before_obj) and not torch.equal(got_pred, before_pred)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    eng, eng_f = tr.engine, fresh.train_engine()
    assert eng is m.train_engine() and eng_f is not eng
    loss_o, tape = eng.forward_objects(*batch)
    eng.backward(tape, one)
    loss_f, tape_f = eng_f.forward_objects(*batch)
    eng_f.backward(tape_f, one)
    assert torch.equal(loss_o, loss_f), 'stale train-chain / fused image (training forward)'
    assert torch.equal(eng.flat_grad, eng_f.flat_grad), 'stale image in the backward'
    assert float(eng.flat_grad.abs().max()) > 0


# ------------------------------------------------------------------ 4. empty batch
def _empty_inputs(dev):
    objects = _pkg()[1]
    d = golden('objects_batch4')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    xy = up(np.stack((d['px'], d['py']), axis=-1))
    inp = objects.classifier_inputs(xy, up(d['rcs']), up(d['cluster_ptr']), up(d['cluster_idx']),
                                    up(d['frame_ptr']), d['noise'],
                                    min_meas=int(d['size'].max()) + 1, node_labels=up(d['labels']))
    assert inp.n_objects == 0 and inp.n_rows == 0 and inp.max_size == 0
    return inp


def test_step_inputs_skips_an_empty_batch(cuda_device):
    dev = cuda_device
    tr = _trainer(_model(dev))
    before = tr.opt.flat.clone()
    assert tr.step_inputs(_empty_inputs(dev)) is None
    assert torch.equal(tr.opt.flat, before)
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 0


def test_step_inputs_empty_batch_on_one_of_several_ranks(cuda_device, monkeypatch):
    """world > 1, this rank's batch without an object: the rank joins the all-reduce (stubbed:
    the peer's finite gradients and loss are added to the bucket) with zero gradients and a
    NaN slot, so the summed loss is NaN and the optimizer launch skips the update."""
    det_training = _pkg()[2]
    dev = cuda_device
    tr = _trainer(_model(dev))
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

    monkeypatch.setattr(det_training, 'allreduce_gradients', peer_sum)
    before = tr.opt.flat.clone()
    assert tr.step_inputs(_empty_inputs(dev)) is None
    assert calls == [2]
    assert bool((eng.flat_grad == 0.25).all()) and bool(torch.isnan(eng.loss_slots).all())
    assert eng.loss_slots.numel() == 1
    assert eng.flat_grad.data_ptr() == eng.flat_bucket.data_ptr()      # views of one bucket
    assert torch.equal(tr.opt.flat, before)
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 1


def _no_frame_store(dev):
    """Six small scenes (test_gpu_training_feed._static_store): the windows of 2 scans at 0
    and 1 hold no / one dynamic node, so a batch of them has no frame."""
    import sequence_ref as sref
    from graph_neural_network_for_radar_perception_amd import sequence
    sizes = (30, 20, 25, 40, 45, 33)
    kinds = ('static', 'static', 'static+1', 'mixed', 'mixed', 'mixed')
    radar, odo, lists, sensors = sref.make_sequence(11, sizes, kinds)
    return sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)


def test_step_inputs_none_builds_no_engine_on_one_rank(cuda_device):
    """world == 1: an empty or missing batch launches nothing -- not even the train engine's
    first packing."""
    dev = cuda_device
    m = _model(dev)
    tr = _trainer(m)
    assert tr.step_inputs(None) is None and tr.step_inputs(_empty_inputs(dev)) is None
    assert getattr(m, '_train_engine', None) is None
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 0


def test_sequence_loop_no_frame_batch_on_one_of_several_ranks(cuda_device, monkeypatch):
    """train_classifier_sequence over a batch without a frame, world = 2: the loop hands the
    batch to step_inputs, so the rank joins the all-reduce (stubbed) with zero gradients and a
    NaN slot instead of leaving its peers waiting; the update is skipped."""
    frontend, _, det_training, _, ct = _pkg()
    dev = cuda_device
    store = _no_frame_store(dev)
    detector = _sequence(dev)[1]
    cfg = classifier_cfg(NAME)
    dd, gd = frontend.dynamic_frame(store.windows([0, 1], 2), with_keys=True)
    assert frontend.frame_batch(dd, gd).n_frames == 0
    tr = _trainer(_model(dev))
    tr.world = 2
    eng = tr.engine
    eng.flat_grad.fill_(3.0)                  # stale values the branch must clear
    calls, seen = [], []

    def peer_sum(bucket, world):
        assert bucket is eng.flat_bucket and world == 2
        assert not bool(eng.flat_grad.any()) and bool(torch.isnan(eng.loss_slots).all())
        calls.append(world)
        bucket.add_(0.25)                     # the other rank's contribution
        return 0.5

    monkeypatch.setattr(det_training, 'allreduce_gradients', peer_sum)
    before = tr.opt.flat.clone()
    losses = ct.train_classifier_sequence(
        store, detector, tr, cfg, [0, 1], window_size=2, batch_windows=2, augmentation=False,
        on_step=lambda k, pos, flags, loss, inp: seen.append((k, loss, inp)))
    assert seen == [(0, None, None)]
    assert losses.shape == (0,) and losses.is_cuda
    assert calls == [2]
    assert bool((eng.flat_grad == 0.25).all()) and bool(torch.isnan(eng.loss_slots).all())
    assert torch.equal(tr.opt.flat, before)
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 1


# ------------------------------------------------------------------ 5. max_size
@pytest.mark.parametrize('name', ['objects_edge', 'objects_batch4'])
def test_classifier_inputs_max_size_rides_the_one_read(cuda_device, monkeypatch, name):
    objects = _pkg()[1]
    dev = cuda_device
    d = golden(name)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    args = (up(np.stack((d['px'], d['py']), axis=-1)), up(d['rcs']), up(d['cluster_ptr']),
            up(d['cluster_idx']), up(d['frame_ptr']), d['noise'])
    labels = up(d['labels'])
    torch.cuda.synchronize()
    reads = []
    for meth in ('cpu', 'tolist', 'item'):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, _meth=meth, **kw):
            if self.is_cuda:
                reads.append(_meth)
            return _orig(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, meth, counted)
    made = {}
    for m_ in (1, 2, 4, int(d['size'].max()), int(d['size'].max()) + 1):
        del reads[:]
        made[m_] = objects.classifier_inputs(*args, min_meas=m_, node_labels=labels)
        assert reads == ['cpu'], (m_, reads)               # the stage's one host read
    monkeypatch.undo()
    for m_, inp in made.items():
        kept = d['size'][d['size'] >= m_]
        assert isinstance(inp.max_size, int)
        assert inp.n_objects == len(kept)
        if len(kept):
            assert inp.max_size == int(inp.object_num_meas.max()) == int(kept.max())
        else:
            assert inp.max_size == 0


# ------------------------------------------------------------------ 6. the sequence loop
def test_train_classifier_sequence_three_steps(cuda_device):
    """The 40-scene fixture, W = 10, 13 positions in 3 batches of at most 5, seed 77: every
    batch steps the trainer exactly as the stages called by hand do (a twin trainer, stepped
    inside on_step, ends every step with bit-equal weights).

    Positions ORDER = [14, 3, 9, 0, 20 | 7, 7, 11, 1, 18 | 5, 16, 2] with the proposals
    fixture's eps, unchanged.  Observed on an MI355X, per batch: 234 / 246 / 154 kept objects,
    65 / 67 / 45 of them with >= 3 members, the largest 25 / 42 / 42 members, object labels
    {0, 1, 2, 3, 5, 6} in every batch (asserted below: >= 8 kept per batch, one object of
    >= 3 members and two distinct labels in the run; the counts are printed)."""
    frontend, objects, _, _, ct = _pkg()
    dev = cuda_device
    store, detector = _sequence(dev)
    cfg = classifier_cfg(NAME)
    assert cfg.dataset_augmentation is True
    assert not bool(getattr(cfg, 'reject_static_meas_by_ransac', False))
    W, B = 10, 5
    assert max(ORDER) < store.n_windows(W)
    tr, tw = _trainer(_model(dev)), _trainer(_model(dev))
    before = tr.opt.flat.clone()
    seen, counts = [], []

    def on_step(k, pos, flags, loss, inp):
        seen.append((k, list(pos), flags, loss, inp))
        # the same batch by hand, on the twin
        dd, gd = frontend.dynamic_frame(store.windows(pos, W), False, with_keys=True, flip=flags)
        fb = frontend.frame_batch(dd, gd)
        det = objects.detect_frames(detector, fb, cfg)
        hand = objects.classifier_inputs(det.xy, det.rcs, det.cluster_ptr, det.cluster_idx,
                                         det.frame_ptr, cfg.meas_noise_cov, 2,
                                         node_labels=fb.labels['class_labels'],
                                         num_classes=int(cfg.num_classes))
        loss_h = tw.step_inputs(hand)
        assert torch.equal(hand.object_features, inp.object_features)
        assert torch.equal(hand.object_class, inp.object_class)
        assert torch.equal(loss_h, loss)
        assert torch.equal(tr.opt.flat, tw.opt.flat), f'step {k}'
        sizes = inp.object_num_meas.cpu().numpy()
        counts.append((inp.n_objects, int((sizes >= 3).sum()), int(sizes.max()),
                       sorted(set(inp.object_class.cpu().tolist()))))

    np.random.seed(77)
    losses = ct.train_classifier_sequence(store, detector, tr, cfg, ORDER, window_size=W,
                                          batch_windows=B, on_step=on_step)
    np.random.seed(77)
    want_flags = [frontend.draw_flips(n) for n in (5, 5, 3)]
    print('kept objects, objects of >= 3 members, largest, labels per batch:', counts)
    assert [s[0] for s in seen] == [0, 1, 2]
    assert [s[1] for s in seen] == [ORDER[:5], ORDER[5:10], ORDER[10:]]
    for s, w in zip(seen, want_flags):
        np.testing.assert_array_equal(s[2], w)
    assert np.concatenate(want_flags).any() and not np.concatenate(want_flags).all()
    assert losses.shape == (3,) and losses.dtype == torch.float32 and losses.is_cuda
    assert bool(torch.isfinite(losses).all())
    assert torch.equal(losses, torch.cat([s[3] for s in seen]))
    assert tr.opt.applied_steps() == 3 and tw.opt.applied_steps() == 3
    assert not torch.equal(tr.opt.flat, before)
    # the run trained on something
    assert all(c[0] >= 8 for c in counts), counts
    assert sum(c[1] for c in counts) >= 1, counts
    assert len(set().union(*[c[3] for c in counts])) >= 2, counts
    # augmentation off: nothing is drawn
    state = np.random.get_state()[1].copy()
    ct.train_classifier_sequence(store, detector, tr, cfg, ORDER[:2], window_size=W,
                                 batch_windows=2, augmentation=False,
                                 on_step=lambda k, pos, flags, loss, inp: seen.append(flags))
    assert seen[-1] is None
    np.testing.assert_array_equal(np.random.get_state()[1], state)
    assert tr.opt.applied_steps() == 4


# ------------------------------------------------------------------ 7. validation
def test_validate_classifier_sequence(cuda_device, monkeypatch):
    """Three batches, the second with a NaN rcs in its first row (put there as the inputs
    leave classifier_inputs): the mean is over the other two, whose losses the test computes
    with Model_Training.forward_objects on the per-frame samples."""
    frontend, objects, _, _, ct = _pkg()
    dev = cuda_device
    store, detector = _sequence(dev)
    cfg = classifier_cfg(NAME)
    W, B = 10, 5
    m = _model(dev)
    tr = _trainer(m)
    tr.step_objects(*_batch(dev))                 # optimizer state that is not all zero
    real = objects.classifier_inputs
    made = []

    def with_nan(*a, **kw):
        inp = real(*a, **kw)
        if len(made) == 1:
            inp.object_features[0, 4] = float('nan')
        made.append(inp)
        return inp

    monkeypatch.setattr(objects, 'classifier_inputs', with_nan)
    w0, s0 = tr.opt.flat.clone(), [b.clone() for b in tr.opt.state_bufs]
    n0, steps0 = tr.opt.applied_steps(), tr.opt.steps
    state = np.random.get_state()[1].copy()
    mean, n = ct.validate_classifier_sequence(store, detector, m, cfg, ORDER, window_size=W,
                                              batch_windows=B)
    np.testing.assert_array_equal(np.random.get_state()[1], state)      # no flip is drawn
    assert len(made) == 3 and all(i.n_objects > 0 for i in made)
    want = []
    with torch.no_grad():
        for inp in made:
            ss = inp.samples()
            want.append(float(m.forward_objects([s['object_features'] for s in ss],
                                                [s['object_num_meas'] for s in ss],
                                                [s['object_class'] for s in ss])))
    print('validation batch losses', want, 'mean', mean, 'counted', n)
    assert np.isnan(want[1]) and np.isfinite(want[0]) and np.isfinite(want[2])
    assert n == 2
    ref = (want[0] + want[2]) / 2
    assert abs(mean - ref) <= 1e-6 * abs(ref), (mean, ref)
    assert torch.equal(tr.opt.flat, w0)
    for a, b in zip(tr.opt.state_bufs, s0):
        assert torch.equal(a, b)
    assert tr.opt.applied_steps() == n0 == 1 and tr.opt.steps == steps0
