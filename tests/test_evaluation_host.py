"""Host side of the evaluation (evaluation.py, csrc/evaluation.hip): the notebooks' summary
arithmetic, the JSON layout, merging, and the argument checks of the new C entry points (which
need only the built library: every call fails before it dereferences anything)."""
import json

import numpy as np
import pytest

from graph_neural_network_for_radar_perception_amd import _native as nat
from graph_neural_network_for_radar_perception_amd import evaluation as ev

NC = 7
CLASS_NAMES = ['CAR', 'PEDESTRIAN', 'PEDESTRIAN_GROUP', 'TWO_WHEELER', 'LARGE_VEHICLE', 'NONE',
               'FALSE']


def _counts(seed=0):
    rng = np.random.default_rng(seed)
    conf = rng.integers(0, 50, (NC, NC)).astype(np.uint64)
    conf[3, :] = 0                       # a class without ground truth or picks
    gt = conf.sum(1) + rng.integers(0, 9, NC).astype(np.uint64)
    gt[3] = 0
    pred = conf.sum(0) + rng.integers(1, 9, NC).astype(np.uint64)
    return conf, gt, pred


def test_detection_result_arithmetic():
    conf, gt, pred = _counts()
    e = ev.DetectionEvaluator().load_counts(confusion_matrix=conf, gt_count_matrix=gt,
                                            pred_count_matrix=pred)
    res = e.result()
    for k, w in (('confusion_matrix', conf), ('gt_count_matrix', gt), ('pred_count_matrix', pred)):
        assert res[k].dtype == np.uint64 and np.array_equal(res[k], w)
    keep = [0, 1, 2, 3, 4, 6]            # class index 5 leaves rows and columns
    c = conf[np.ix_(keep, keep)].astype(np.float64)
    assert res['normalized_confusion_matrix'].shape == (6, 6)
    for i in range(6):
        s = c[i].sum()
        if s == 0:
            assert np.isnan(res['normalized_confusion_matrix'][i]).all()      # 0 / 0 in the notebook
            assert np.isnan(res['recall'][i])
        else:
            assert np.array_equal(res['normalized_confusion_matrix'][i], c[i] / s * 100)
            assert res['recall'][i] == c[i, i] / float(gt[keep[i]])
        assert res['precision'][i] == c[i, i] / float(pred[keep[i]])
    assert res['precision'].shape == res['recall'].shape == (6,)
    # nothing dropped on request
    assert e.result(invalid_class_index=None)['precision'].shape == (NC,)


def test_segmentation_result_arithmetic():
    conf, gt, _ = _counts(1)
    e = ev.SegmentationEvaluator().load_counts(confusion_matrix=conf, gt_count_matrix=gt)
    res = e.result()
    assert sorted(res) == ['confusion_matrix', 'confusion_matrix_norm', 'gt_count_matrix']
    keep = [0, 1, 2, 3, 4, 6]
    norm = res['confusion_matrix_norm']
    assert norm.dtype == np.float32 and norm.shape == (6, 6)
    for i, k in enumerate(keep):
        if gt[k] == 0:
            assert (norm[i] == 0).all()                                       # the zero gt_count row
        else:
            want = (conf[k, keep].astype(np.float64) / float(gt[k]) * 100).astype(np.float32)
            assert np.array_equal(norm[i], want)
    assert (norm[3] == 0).all()


def test_to_json_round_trip_and_merge(tmp_path):
    conf, gt, pred = _counts(2)
    a = ev.DetectionEvaluator().load_counts(confusion_matrix=conf, gt_count_matrix=gt,
                                            pred_count_matrix=pred)
    path = tmp_path / 'sequence_1.json'
    a.to_json(path, CLASS_NAMES)
    with open(path) as fh:
        data = json.load(fh)
    assert list(data) == ['class_names', 'confusion_matrix', 'gt_count_matrix', 'pred_count_matrix']
    assert data['class_names'] == CLASS_NAMES
    b = ev.DetectionEvaluator().load_counts(**{k: np.array(data[k], dtype=np.uint64)
                                               for k in list(data)[1:]})
    for k, v in a.counts().items():
        assert np.array_equal(b.counts()[k], v)
    b.merge(a)
    for k, v in a.counts().items():
        assert np.array_equal(b.counts()[k], v * np.uint64(2))
    s = ev.SegmentationEvaluator().load_counts(confusion_matrix=conf, gt_count_matrix=gt)
    spath = tmp_path / 'seg.json'
    s.to_json(spath, CLASS_NAMES)
    with open(spath) as fh:
        assert list(json.load(fh)) == ['class_names', 'confusion_matrix', 'gt_count_matrix']
    s.merge(ev.SegmentationEvaluator().load_counts(confusion_matrix=conf, gt_count_matrix=gt))
    assert np.array_equal(s.counts()['gt_count_matrix'], gt * np.uint64(2))
    with pytest.raises(ValueError):
        s.merge(a)
    with pytest.raises(ValueError):
        ev.DetectionEvaluator(num_classes=7, false_class_label=7)
    with pytest.raises(ValueError):
        ev.SegmentationEvaluator(num_classes=33)


def test_l2_norm_is_not_implemented():
    with pytest.raises(NotImplementedError):
        ev.compute_gt_and_pred_associations({}, 1.0, association_criteria='l2_norm')


def test_package_docstring_names_the_evaluators():
    import graph_neural_network_for_radar_perception_amd as pkg
    assert 'DetectionEvaluator' in pkg.__doc__ and 'SegmentationEvaluator' in pkg.__doc__
    assert not hasattr(pkg, 'DetectionEvaluator')


@pytest.fixture(scope='module')
def lib():
    from graph_neural_network_for_radar_perception_amd import build
    build.build_library()
    return nat.lib()


ERR_ARG, ERR_UNSUPPORTED = 1, 3


def test_eval_entry_points_check_arguments(lib):
    f = 4096  # any non-null address: nothing is dereferenced before the checks fail
    # negative sizes
    assert lib.rg_eval_gt_clusters(f, f, f, -1, 1, f, f, f, f, f, f, f, 1 << 20, None) == ERR_ARG
    assert b'n_nodes' in lib.rg_last_error()
    assert lib.rg_eval_gt_clusters(f, f, f, 10, 0, f, f, f, f, f, f, f, 1 << 20, None) == ERR_ARG
    assert lib.rg_argmax_rows(f, 7, -1, 7, f, None) == ERR_ARG
    assert lib.rg_argmax_rows(f, 3, 10, 7, f, None) == ERR_ARG          # ld < n_cols
    assert lib.rg_eval_cluster_of(f, f, -1, 10, f, None) == ERR_ARG
    assoc = lambda n, nf, maxn, thr, ws, nbytes: lib.rg_eval_associate(  # noqa: E731
        f, n, nf, maxn, f, f, f, f, f, f, thr, 0.7, f, f, f, f, f, f, f, f, f, f, ws, nbytes, None)
    assert assoc(-1, 1, 0, 0, f, 1 << 20) == ERR_ARG
    assert assoc(10, -1, 10, 0, f, 1 << 20) == ERR_ARG
    assert assoc(10, 1, 10, -1, f, 1 << 20) == ERR_ARG
    assert assoc(10, 0, 10, 0, f, 1 << 20) == ERR_ARG                   # nodes without a frame
    assert lib.rg_eval_accumulate(f, f, f, f, f, f, f, -1, 7, 6, f, f, f, f, None) == ERR_ARG
    assert lib.rg_eval_accumulate(f, f, f, f, f, f, f, 10, 7, 7, f, f, f, f, None) == ERR_ARG
    assert b'false_class' in lib.rg_last_error()
    assert lib.rg_eval_node_confusion(f, 7, f, -1, 7, f, f, f, None) == ERR_ARG
    assert lib.rg_eval_node_confusion(f, 4, f, 10, 7, f, f, f, None) == ERR_ARG
    # a short workspace
    need = lib.rg_eval_gt_clusters_workspace_size(1000)
    assert need >= 1000 * (8 + 8 + 4 + 4 + 4 + 4)
    assert lib.rg_eval_gt_clusters(f, f, f, 1000, 4, f, f, f, f, f, f, f, need - 8, None) == ERR_ARG
    assert b'workspace' in lib.rg_last_error()
    need = lib.rg_eval_associate_workspace_size(1000, 4)
    assert need >= 1000 * 100
    assert assoc(1000, 4, 1000, 0, f, need - 8) == ERR_ARG
    assert b'workspace' in lib.rg_last_error()
    assert assoc(1000, 4, 1000, 0, None, need) == ERR_ARG
    assert lib.rg_eval_associate_workspace_size(64 * 3000, 64) > 64 * 3000 * 100
    assert lib.rg_eval_associate_workspace_size(0, 4) == 0
    # unsupported: a frame of 2^24 nodes, num_classes outside 1..32
    assert assoc(1 << 25, 2, 1 << 24, 0, f, 1 << 20) == ERR_UNSUPPORTED
    assert b'max_frame_nodes' in lib.rg_last_error()
    assert lib.rg_eval_accumulate(f, f, f, f, f, f, f, 10, 33, 6, f, f, f, f, None) == ERR_UNSUPPORTED
    assert lib.rg_eval_accumulate(f, f, f, f, f, f, f, 10, 0, 0, f, f, f, f, None) == ERR_UNSUPPORTED
    assert lib.rg_eval_node_confusion(f, 40, f, 10, 33, f, f, f, None) == ERR_UNSUPPORTED
    assert b'num_classes' in lib.rg_last_error()
    # nothing to do
    assert lib.rg_argmax_rows(f, 7, 0, 7, f, None) == 0
    assert lib.rg_eval_node_confusion(f, 7, f, 0, 7, f, f, f, None) == 0
    assert lib.rg_eval_accumulate(f, f, f, f, f, f, f, 0, 7, 6, f, f, f, f, None) == 0
