"""The two-stage flow's scoring on the GPU: rg_cluster_class_from_objects in guarded buffers,
rg_eval_class_confusion, DetectionEvaluator's classifier source and shared association,
object_list with the classifier's classes, and evaluate_sequence / evaluate_classifier_sequence
end to end.

Every comparison is between integers or between float32 bit patterns: the scattered score is
compared with objects.softmax_max of the same row (one device function behind both), the count
matrices with numpy.add.at or with the existing evaluators on one-hot logits of the same
classes.  No tolerance is involved."""
import numpy as np
import pytest
import torch

import sequence_ref as sref
from conftest import classifier_cfg, golden, model_cfg, model_state_dict

pytestmark = pytest.mark.gpu

NC, FALSE = 7, 6
GUARD, SENT = 256, 0xA5
COUNTS = ('confusion_matrix', 'gt_count_matrix', 'pred_count_matrix')


def _pkg():
    from graph_neural_network_for_radar_perception_amd import _native, evaluation, objects
    return _native, evaluation, objects


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_counts(got, want, what, names=COUNTS):
    for k in names:
        assert got[k].dtype == want[k].dtype == np.uint64, (what, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f'{what}: {k}')


# ------------------------------------------------------------------ 1. the scatter kernel
class Guarded:
    """A device view of exactly n elements between two bands of GUARD sentinel bytes, the body
    sentinel-filled too (the form of test_gpu_index_builders.py)."""

    def __init__(self, dev, n, dtype):
        self.dtype = np.dtype(dtype)
        self.nbytes = int(n) * self.dtype.itemsize
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.ptr = self.raw.data_ptr() + GUARD
        assert self.ptr % 8 == 0

    def zero(self):
        self.raw[GUARD:GUARD + self.nbytes].zero_()
        return self

    def numpy(self):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype)

    def check_guards(self, what):
        raw = self.raw.cpu().numpy()
        for band, name in ((raw[:GUARD], 'front'), (raw[GUARD + self.nbytes:], 'back')):
            hit = np.nonzero(band != SENT)[0]
            assert hit.size == 0, f'{what}: {name} guard overwritten at bytes {hit[:8].tolist()}'


def _logits(rng, n, nc, ld):
    """[n, ld] float32: row 0 has its maximum twice (the first must win), row 1 holds a NaN."""
    x = rng.standard_normal((n, ld)).astype(np.float32)
    if n > 0 and nc > 1:
        a, b = sorted(rng.choice(nc, 2, replace=False))
        x[0, :nc] = np.minimum(x[0, :nc], 0.5)
        x[0, a] = x[0, b] = 1.5
    if n > 1:
        x[1, int(rng.integers(0, nc))] = np.nan
    return x


def _scatter(dev, logits, nc, oc, K, fill, with_score=True):
    """rg_cluster_class_from_objects on guarded outputs: (class [K], score [K] or None, flag)."""
    nat, _, _ = _pkg()
    x = _up(logits, dev) if logits.shape[0] else torch.zeros((1, logits.shape[1]), device=dev)
    oc_t = _up(np.concatenate([np.asarray(oc, np.int32), np.zeros(1, np.int32)]), dev)
    cls, score = Guarded(dev, K, np.int64), Guarded(dev, K, np.float32)
    bad = Guarded(dev, 1, np.int32).zero()
    rc = nat.lib().rg_cluster_class_from_objects(
        x.data_ptr(), logits.shape[1], len(oc), nc, oc_t.data_ptr(), K, fill, cls.ptr,
        score.ptr if with_score else None, bad.ptr, nat.stream_ptr(dev))
    assert rc == 0, nat.lib().rg_last_error()
    torch.cuda.synchronize()
    for g, name in ((cls, 'class'), (score, 'score'), (bad, 'flag')):
        g.check_guards(name)
    return cls.numpy(), score.numpy(), int(bad.numpy()[0])


def _expected(dev, logits, nc, oc, K, fill, skip=()):
    """softmax_max of the rows gathered through oc with torch indexing; fill / 0.0 elsewhere."""
    _, _, objects = _pkg()
    want_c = torch.full((K,), fill, dtype=torch.int64, device=dev)
    want_s = torch.zeros(K, dtype=torch.float32, device=dev)
    keep = [i for i in range(len(oc)) if i not in skip]
    if keep:
        c, s = objects.softmax_max(_up(logits, dev)[:, :nc])
        rows = torch.tensor(keep, dtype=torch.int64, device=dev)
        slots = torch.tensor([int(oc[i]) for i in keep], dtype=torch.int64, device=dev)
        want_c[slots] = c[rows]
        want_s[slots] = s[rows]
    return want_c.cpu().numpy(), want_s.cpu().numpy()


@pytest.mark.parametrize('K', [0, 1, 64, 65, 130])
def test_scatter_in_guarded_buffers(cuda_device, K):
    """One wave of clusters, one over, several workgroups' worth of neither: every slot an
    object names holds softmax_max of its row bit for bit, every other slot fill_class / 0.0,
    the flag stays clear and nothing outside the [K] outputs is written."""
    dev = cuda_device
    _, _, objects = _pkg()
    rng = np.random.default_rng(1000 + K)
    for nc in (1, 7, 32):
        for ld in (nc, nc + 3):
            for n in sorted({0, min(1, K), K}):
                what = (K, nc, ld, n)
                logits = _logits(rng, n, nc, ld)
                oc = rng.permutation(K)[:n].astype(np.int32)
                fill = nc - 1
                got_c, got_s, flag = _scatter(dev, logits, nc, oc, K, fill)
                want_c, want_s = _expected(dev, logits, nc, oc, K, fill)
                assert flag == 0, what
                np.testing.assert_array_equal(got_c, want_c, err_msg=str(what))
                np.testing.assert_array_equal(_bits(got_s), _bits(want_s), err_msg=str(what))
                if n > 1 and nc > 1:
                    assert np.isnan(got_s[oc[1]]), what              # the NaN row's score
                    row = logits[0, :nc]
                    assert got_c[oc[0]] == int(np.argmax(row)) and np.sum(row == row.max()) == 2
    # without a score output only the classes are written; the Python entry gives the same
    nc, n = 7, min(K, 40)
    logits = _logits(rng, n, nc, nc)
    oc = rng.permutation(K)[:n].astype(np.int32)
    got_c, got_s, flag = _scatter(dev, logits, nc, oc, K, FALSE, with_score=False)
    want_c, want_s = _expected(dev, logits, nc, oc, K, FALSE)
    np.testing.assert_array_equal(got_c, want_c)
    assert flag == 0 and bool((got_s.view(np.uint8) == SENT).all())
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    c, s = objects.cluster_class_from_objects(_up(logits, dev), _up(oc, dev), K, FALSE, bad)
    assert c.dtype == torch.int64 and s.dtype == torch.float32 and tuple(c.shape) == (K,)
    np.testing.assert_array_equal(c.cpu().numpy(), want_c)
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(want_s))
    assert int(bad.item()) == 0


def test_scatter_reports_an_index_out_of_range(cuda_device):
    """Entries of -1, K and far beyond set the flag and write nothing: their neighbours' slots
    (0 and K - 1 among them) and both guard bands are untouched."""
    dev = cuda_device
    rng = np.random.default_rng(77)
    K, nc = 65, 7
    oc = np.array([3, -1, 64, 65, 0, 2 ** 31 - 1, 7, -2 ** 31, 63], np.int32)
    logits = rng.standard_normal((len(oc), nc)).astype(np.float32)
    got_c, got_s, flag = _scatter(dev, logits, nc, oc, K, FALSE)
    want_c, want_s = _expected(dev, logits, nc, oc, K, FALSE, skip=(1, 3, 5, 7))
    assert flag == 1
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    assert int(np.sum(want_s != 0)) == 5


# ------------------------------------------------------------------ 2. the class confusion
def _host_confusion(gt, pred, nc):
    conf, cnt = np.zeros((nc, nc), np.uint64), np.zeros(nc, np.uint64)
    np.add.at(conf, (gt, pred), 1)
    np.add.at(cnt, gt, 1)
    return dict(confusion_matrix=conf, gt_count_matrix=cnt)


@pytest.mark.parametrize('nc', [7, 32])
def test_class_confusion(cuda_device, nc):
    dev = cuda_device
    nat, evaluation, _ = _pkg()
    rng = np.random.default_rng(nc)
    total = _host_confusion(np.zeros(0, np.int64), np.zeros(0, np.int64), nc)
    ev = evaluation.ObjectClassEvaluator(nc)
    for n in (0, 1, 1000):
        gt, pred = rng.integers(0, nc, n), rng.integers(0, nc, n)
        one = evaluation.ObjectClassEvaluator(nc).update(_up(pred, dev), _up(gt, dev))
        want = _host_confusion(gt, pred, nc)
        _same_counts(one.result(None), want, n, COUNTS[:2])
        ev.update(_up(pred, dev), _up(gt, dev))                      # additive over the calls
        total = {k: total[k] + want[k] for k in total}
    _same_counts(ev.result(None), total, 'accumulated', COUNTS[:2])
    assert int(total['gt_count_matrix'].sum()) == 1001
    # update_logits: the first maximum of every row
    logits = rng.standard_normal((300, nc)).astype(np.float32)
    logits[0, :] = 0.25
    gt = rng.integers(0, nc, 300)
    lg = evaluation.ObjectClassEvaluator(nc).update_logits(_up(logits, dev), _up(gt, dev))
    _same_counts(lg.result(None), _host_confusion(gt, np.argmax(logits, axis=1), nc), 'logits',
                 COUNTS[:2])
    # a class out of range on either side: the flag is set, that row is skipped
    gt, pred = rng.integers(0, nc, 200), rng.integers(0, nc, 200)
    gt[5], pred[9], gt[150], pred[199] = nc, -1, -3, nc + 40
    ok = np.ones(200, bool)
    ok[[5, 9, 150, 199]] = False
    conf = torch.zeros((nc, nc), dtype=torch.int64, device=dev)
    cnt = torch.zeros(nc, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    g, p = _up(gt, dev), _up(pred, dev)
    assert nat.lib().rg_eval_class_confusion(g.data_ptr(), p.data_ptr(), 200, nc, conf.data_ptr(),
                                             cnt.data_ptr(), flag.data_ptr(),
                                             nat.stream_ptr(dev)) == 0
    want = _host_confusion(gt[ok], pred[ok], nc)
    assert int(flag.item()) == 1
    np.testing.assert_array_equal(conf.cpu().numpy().astype(np.uint64), want['confusion_matrix'])
    np.testing.assert_array_equal(cnt.cpu().numpy().astype(np.uint64), want['gt_count_matrix'])
    bad = evaluation.ObjectClassEvaluator(nc).update(p, g)
    with pytest.raises(RuntimeError, match='class id'):
        bad.result()


# ------------------------------------------------------------------ 3. / 4. the class source
def _lists(labels):
    """Clusters of a labelling, ordered by their lowest member (the order of rg_cluster_lists)."""
    seen, out = {}, []
    for i, l in enumerate(labels):
        if l not in seen:
            seen[l] = len(out)
            out.append([])
        out[seen[l]].append(i)
    return out


def _seeded_batch(dev, seed, sizes=(38, 43, 40)):
    """3 frames of about 40 nodes: random tracks (a third untracked), random predicted
    clusters, positions on a quarter grid (equal centre distances happen), node logits, object
    logits and classifier classes drawn independently."""
    rng = np.random.default_rng(seed)
    base = np.concatenate(([0], np.cumsum(sizes)))
    key, ptr, idx = [], [0], []
    for n, b in zip(sizes, base):
        k = rng.integers(1, 9, n)
        key.append(np.where(rng.random(n) < 0.67, k, 0))
        for m in _lists(rng.integers(0, 12, n).tolist()):
            idx += [int(b) + i for i in m]
            ptr.append(len(idx))
    N, K = int(base[-1]), len(ptr) - 1
    return dict(
        args=(_up(rng.standard_normal((N, NC)).astype(np.float32), dev),
              _up(rng.standard_normal((K, NC)).astype(np.float32), dev),
              _up(np.asarray(ptr, np.int32), dev), _up(np.asarray(idx, np.int32), dev),
              _up(rng.integers(0, 6, N), dev), _up(np.concatenate(key).astype(np.int32), dev),
              _up(base.astype(np.int32), dev)),
        xy=_up((rng.integers(0, 24, (N, 2)) * 0.25).astype(np.float32), dev),
        cluster_class=rng.integers(0, NC, K), K=K, max_frame_nodes=max(sizes))


def _one_hot(classes, dev):
    x = np.zeros((len(classes), NC), np.float32)
    x[np.arange(len(classes)), classes] = 1.0
    return _up(x, dev)


@pytest.mark.parametrize('criterion', ['inv_iou', 'l2_norm'])
@pytest.mark.parametrize('thr', [0, 1])
def test_classifier_source_equals_object_head_on_one_hot_logits(cuda_device, criterion, thr):
    """class_source='classifier' fed cluster_class against the object-head evaluator fed
    one-hot logits of the same classes: the same three count matrices."""
    dev = cuda_device
    _, evaluation, _ = _pkg()
    a = evaluation.DetectionEvaluator(NC, 0.7, thr, association_criteria=criterion,
                                      class_source='classifier')
    b = evaluation.DetectionEvaluator(NC, 0.7, thr, by_segmentation=False,
                                      association_criteria=criterion)
    for seed in (3, 4):
        bt = _seeded_batch(dev, seed)
        kw = dict(max_frame_nodes=bt['max_frame_nodes'], xy=bt['xy'])
        a.update(*bt['args'], cluster_class=_up(bt['cluster_class'], dev), **kw)
        args = list(bt['args'])
        args[1] = _one_hot(bt['cluster_class'], dev)
        b.update(*args, **kw)
        assert torch.equal(a.last['pred_class'], b.last['pred_class'])
    ra, rb = a.result(), b.result()
    _same_counts(ra, rb, (criterion, thr))
    assert int(ra['confusion_matrix'].sum()) > 0 and int(ra['pred_count_matrix'][FALSE]) > 0


@pytest.mark.parametrize('criterion', ['inv_iou', 'l2_norm'])
def test_shared_association_equals_independent_ones(cuda_device, criterion):
    """Three class sources accumulating on the first one's picks equal three that associate
    for themselves, matrix for matrix; the picks are the first one's tensors."""
    dev = cuda_device
    _, evaluation, _ = _pkg()
    mk = lambda: [evaluation.DetectionEvaluator(NC, 0.7, 1, association_criteria=criterion,  # noqa: E731
                                                class_source=s)
                  for s in evaluation.DetectionEvaluator.CLASS_SOURCES]
    shared, alone = mk(), mk()
    for seed in (5, 6):
        bt = _seeded_batch(dev, seed)
        cc = _up(bt['cluster_class'], dev)
        first = None
        for s, i in zip(shared, alone):
            i.update(*bt['args'], max_frame_nodes=bt['max_frame_nodes'], xy=bt['xy'],
                     cluster_class=cc)
            # no positions: with an association given nothing is associated here
            s.update(*bt['args'], max_frame_nodes=bt['max_frame_nodes'],
                     xy=bt['xy'] if first is None else None, cluster_class=cc, association=first)
            if first is None:
                first = s.last
            else:
                assert s.last['assoc'] is first['assoc'] and s.last['gt'] is first['gt']
    results = [e.result() for e in shared]
    for s, i, name in zip(results, alone, evaluation.DetectionEvaluator.CLASS_SOURCES):
        _same_counts(s, i.result(), (criterion, name))
    # the three sources do differ in their classes
    assert not np.array_equal(results[0]['pred_count_matrix'], results[2]['pred_count_matrix'])
    # an association from another threshold is refused on the device path too
    other = evaluation.DetectionEvaluator(NC, 0.7, 0, association_criteria=criterion)
    with pytest.raises(ValueError, match='association='):
        other.update(*bt['args'], xy=bt['xy'], association=first)


# ------------------------------------------------------------------ models
def _detector_n300(dev):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    name = 'proposals_model_trained_N300'
    d = golden(name)
    mt = Model_Training(model_cfg(name), dev)
    mt.load_state_dict(model_state_dict(name))
    m = mt.to(dev).pred.eval().requires_grad_(False)
    m.set_param_for_proposal_extraction(float(d['eps']), False)
    frames = ([_up(d['node_features'], dev)], [_up(d['edge_features'], dev)],
              [_up(d['edge_index'].astype(np.int64), dev)], [_up(d['other_features'], dev)])
    return m, frames


def _detector_n50(dev):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    name = 'model_trained_N50'
    mt = Model_Training(model_cfg(name), dev)
    mt.load_state_dict(model_state_dict(name))
    m = mt.to(dev).pred.eval().requires_grad_(False)
    m.set_param_for_proposal_extraction(float(golden('proposals_model_trained_N300')['eps']),
                                        False)
    return m, model_cfg(name)


def _random_classifier(dev, seed=11):
    """A seeded random-init classifier: the fused conv blocks run, the accuracy is beside the
    point."""
    from graph_neural_network_for_radar_perception_amd.classifier import Model_Training
    torch.manual_seed(seed)
    m = Model_Training(classifier_cfg('classifier_yml'))
    return m.to(dev).eval().requires_grad_(False)


# ------------------------------------------------------------------ 5. the object list
def test_object_list_with_classifier_classes(cuda_device):
    dev = cuda_device
    _, _, objects = _pkg()
    det_model, frames = _detector_n300(dev)
    det = objects.detect(det_model, *frames)
    K = int(det.cluster_ptr.numel()) - 1
    size = (det.cluster_ptr[1:] - det.cluster_ptr[:-1]).cpu().numpy()
    args = (det.node_cls, det.link_cls, det.obj_cls, det.xy, det.cluster_ptr, det.cluster_idx,
            det.frame_ptr, det.meas_noise_cov)
    # (a) hand-made classes and scores: the third source wins over both flags
    rng = np.random.default_rng(21)
    cc, cs = rng.integers(0, NC, K), rng.random(K).astype(np.float32)
    keep = np.nonzero(cc != FALSE)[0]
    assert 0 < len(keep) < K
    for flag in (True, False):
        ol = objects.object_list(*args, detect_object_by_segmentation_output=flag, points=False,
                                 cluster_class=_up(cc, dev), cluster_score=_up(cs, dev))
        assert ol.n_objects == len(keep)
        np.testing.assert_array_equal(ol.obj_cluster.cpu().numpy(), keep)
        np.testing.assert_array_equal(ol.obj_class.cpu().numpy(), cc[keep])
        np.testing.assert_array_equal(_bits(ol.obj_score.cpu().numpy()), _bits(cs[keep]))
        np.testing.assert_array_equal(ol.cluster_class.cpu().numpy(), cc)
        np.testing.assert_array_equal(ol.obj_size.cpu().numpy(), size[keep])
    no_score = objects.object_list(*args, points=False, cluster_class=_up(cc, dev))
    assert no_score.obj_score is None and no_score.n_objects == len(keep)
    # (b) the classifier's: below min_meas or called FALSE is no object
    clf = _random_classifier(dev)
    for min_meas in (2, 4):
        res = objects.classify_detections(det, clf, min_meas)
        ccls, cscore = res['cluster_class'].cpu().numpy(), res['cluster_score'].cpu().numpy()
        oc = res['object_cluster'].cpu().numpy()
        np.testing.assert_array_equal(oc, np.nonzero(size >= min_meas)[0])
        sc, ss = objects.softmax_max(res['logits'])
        np.testing.assert_array_equal(ccls[oc], sc.cpu().numpy())
        np.testing.assert_array_equal(_bits(cscore[oc]), _bits(ss.cpu().numpy()))
        small = size < min_meas
        assert small.any() and (ccls[small] == FALSE).all() and (cscore[small] == 0).all()
        assert int(res['bad'].item()) == 0
        ol = objects.detections_object_list(det, classifier=clf, min_meas=min_meas, points=False)
        keep = np.nonzero((size >= min_meas) & (ccls != FALSE))[0]
        print('clusters', K, 'of size >=', min_meas, int((~small).sum()), 'objects', len(keep))
        assert ol.n_objects == len(keep) and ol.centres is det.centres
        np.testing.assert_array_equal(ol.obj_cluster.cpu().numpy(), keep)
        np.testing.assert_array_equal(ol.obj_class.cpu().numpy(), ccls[keep])
        np.testing.assert_array_equal(_bits(ol.obj_score.cpu().numpy()), _bits(cscore[keep]))
        assert not np.isin(np.nonzero(small)[0], ol.obj_cluster.cpu().numpy()).any()
    # (c) without the new arguments: today's tensors
    for flag in (True, False):
        old = objects.object_list(*args, detect_object_by_segmentation_output=flag, points=False)
        new = objects.object_list(*args, detect_object_by_segmentation_output=flag, points=False,
                                  cluster_class=None, cluster_score=None)
        assert old.n_objects == new.n_objects
        for k in ('cluster', 'frame', 'class', 'score', 'size', 'mu', 'sigma', 'ellipse'):
            a, b = getattr(old, 'obj_' + k), getattr(new, 'obj_' + k)
            assert (a is None and b is None) or torch.equal(a, b), k
        assert torch.equal(old.cluster_class, new.cluster_class)


# ------------------------------------------------------------------ 6. end to end
def test_evaluate_sequence_with_classifier_end_to_end(cuda_device):
    """evaluate_sequence(classifier=) against a loop made of the existing pieces
    (evaluate_window_batch, classifier_inputs, classify_inputs, torch argmax and index_copy, the
    object-head evaluator on one-hot logits), against today's evaluate_sequence for the vote
    and the head, and against numpy.add.at for the object-level matrices."""
    from graph_neural_network_for_radar_perception_amd import sequence
    from graph_neural_network_for_radar_perception_amd.classifier import training as ct
    dev = cuda_device
    _, evaluation, objects = _pkg()
    radar, odo, lists, sensors = sref.adversarial_sequence()
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    model, cfg = _detector_n50(dev)
    clf = _random_classifier(dev)
    noise = model.meas_noise_cov
    W, B, THR, MIN_MEAS = 4, 11, 1, 2
    n = store.n_windows(W)
    assert n == 21                                          # two batches, the second short
    DE = evaluation.DetectionEvaluator
    # arm A
    det_a, seg_a, two = evaluation.evaluate_sequence(
        store, model, cfg, window_size=W, batch_windows=B,
        detection=DE(NC, cluster_size_threshold=THR), classifier=clf,
        two_stage=evaluation.TwoStageEvaluators(NC, min_meas=MIN_MEAS,
                                                cluster_size_threshold=THR),
        meas_noise_cov=noise)
    got = two.result()
    # today's evaluate_sequence for the two existing sources
    today = {}
    for name, flag in (('segmentation', True), ('object_head', False)):
        d, s = evaluation.evaluate_sequence(
            store, model, cfg, window_size=W, batch_windows=B,
            detection=DE(NC, cluster_size_threshold=THR, by_segmentation=flag))
        today[name] = d.result()
        _same_counts(got[name]['detection'], today[name], name)
    _same_counts(det_a.result(), today['segmentation'], 'the detection evaluator beside it')
    _same_counts(seg_a.result(), s.result(), 'segmentation', COUNTS[:2])
    # arm B
    head_b = DE(NC, cluster_size_threshold=THR, by_segmentation=False)
    pairs = {k: [] for k in ('gt', 'classifier', 'segmentation', 'object_head')}
    cache: dict = {}
    for i0 in range(0, n, B):
        win = store.windows(range(i0, min(i0 + B, n)), W)
        fb, out = evaluation.evaluate_window_batch(win, model, cfg, cache=cache)
        assert out is not None
        gt_class = fb.labels['class_labels']
        # the positions and the rcs column the detector's node features were built from
        # (node feature 1 is a float32 copy of meas_rcs)
        xy = torch.stack((fb.arrays['meas_px'], fb.arrays['meas_py']), dim=-1)
        inp = objects.classifier_inputs(xy, fb.arrays['meas_rcs'], out.cluster_ptr,
                                        out.cluster_idx, fb.frame_ptr, noise, MIN_MEAS,
                                        node_labels=gt_class, num_classes=NC)
        logits = objects.classify_inputs(clf, inp)
        K = int(out.cluster_ptr.numel()) - 1
        am = torch.argmax(logits, dim=1)
        oc = inp.object_cluster.to(torch.int64)
        ccls = torch.full((K,), FALSE, dtype=torch.int64, device=dev)
        ccls.index_copy_(0, oc, am)
        one_hot = torch.zeros((K, NC), dtype=torch.float32, device=dev)
        one_hot[torch.arange(K, device=dev), ccls] = 1.0
        head_b.update(out.node_cls, one_hot, out.cluster_ptr, out.cluster_idx, gt_class,
                      fb.track_key, fb.frame_ptr, max_frame_nodes=max(fb.frame_sizes))
        vote = objects.majority_class(torch.argmax(out.node_cls, dim=1),
                                      out.cluster_ptr.to(torch.int32).contiguous(),
                                      out.cluster_idx.to(torch.int32).contiguous(), NC)
        head = torch.argmax(out.obj_cls[:K], dim=1)
        pairs['gt'].append(inp.object_class.cpu().numpy())
        pairs['classifier'].append(am.cpu().numpy())
        pairs['segmentation'].append(vote[oc].cpu().numpy())
        pairs['object_head'].append(head[oc].cpu().numpy())
    _same_counts(got['classifier']['detection'], head_b.result(), 'classifier source')
    gt = np.concatenate(pairs['gt'])
    print('kept proposals', len(gt), 'classifier classes',
          np.bincount(np.concatenate(pairs['classifier']), minlength=NC).tolist(),
          'kept predicted clusters', int(got['classifier']['detection']['pred_count_matrix'].sum()))
    assert len(gt) > 0 and int(got['classifier']['detection']['pred_count_matrix'].sum()) > 0
    for name in two.SOURCES:
        want = _host_confusion(gt, np.concatenate(pairs[name]), NC)
        _same_counts(got[name]['object_class'], want, name + ' object classes', COUNTS[:2])
    # the accuracy validate_classifier_sequence lacks: the same walk, the same matrix
    oce = ct.evaluate_classifier_sequence(store, model, clf, cfg, range(n), window_size=W,
                                          batch_windows=B, min_meas=MIN_MEAS,
                                          meas_noise_cov=noise)
    assert isinstance(oce, evaluation.ObjectClassEvaluator)
    _same_counts(oce.result(), got['classifier']['object_class'], 'evaluate_classifier_sequence',
                 COUNTS[:2])
    # three independent associations count the same
    _, _, alone = evaluation.evaluate_sequence(
        store, model, cfg, window_size=W, batch_windows=B, classifier=clf,
        two_stage=evaluation.TwoStageEvaluators(NC, min_meas=MIN_MEAS, share_association=False,
                                                cluster_size_threshold=THR),
        meas_noise_cov=noise)
    for name, r in alone.result().items():
        _same_counts(r['detection'], got[name]['detection'], name + ' (own association)')
    two.merge(alone)
    assert int(two.result()['classifier']['object_class']['gt_count_matrix'].sum()) == 2 * len(gt)


# ------------------------------------------------------------------ 7. nothing to classify
def test_batch_without_a_proposal_of_min_meas(cuda_device, monkeypatch):
    """min_meas above every proposal: the classifier is not launched, nothing raises and the
    classifier source counts no predicted cluster."""
    from graph_neural_network_for_radar_perception_amd import sequence
    from graph_neural_network_for_radar_perception_amd.classifier import engine as ce
    dev = cuda_device
    _, evaluation, _ = _pkg()
    radar, odo, lists, sensors = sref.adversarial_sequence()
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    model, cfg = _detector_n50(dev)
    clf = _random_classifier(dev)

    def never(*a, **kw):
        raise AssertionError('the classifier ran without an object')

    monkeypatch.setattr(ce, 'forward_objects', never)
    big = 10 ** 6
    two = evaluation.TwoStageEvaluators(NC, min_meas=big, cluster_size_threshold=big - 1)
    det = evaluation.DetectionEvaluator(NC)
    fb, out = evaluation.evaluate_window_batch(store.windows(range(2, 13), 4), model, cfg, det,
                                               None, classifier=clf, two_stage=two)
    assert out is not None and fb.n_nodes > 0
    res = two.result()
    for name in two.SOURCES:
        assert int(res[name]['detection']['pred_count_matrix'].sum()) == 0
        assert int(res[name]['detection']['confusion_matrix'].sum()) == 0
        assert int(res[name]['object_class']['gt_count_matrix'].sum()) == 0
    # the ground truth below the threshold is dropped with it; the evaluator beside saw clusters
    assert int(res['classifier']['detection']['gt_count_matrix'].sum()) == 0
    assert int(det.result()['pred_count_matrix'].sum()) > 0
    with pytest.raises(ValueError, match='two_stage'):
        evaluation.evaluate_window_batch(store.windows(range(2, 13), 4), model, cfg,
                                         classifier=clf)
