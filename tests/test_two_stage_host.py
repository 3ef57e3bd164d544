"""Host side of the two-stage scoring: the constructor and argument checks of
TwoStageEvaluators and of DetectionEvaluator's class_source / association keywords (each fails
before anything reaches the device) and the argument checks of rg_cluster_class_from_objects
and rg_eval_class_confusion on the loaded library (each fails before it dereferences
anything)."""
import pytest
import torch

from graph_neural_network_for_radar_perception_amd import _native as nat
from graph_neural_network_for_radar_perception_amd import evaluation as ev

NC = 7
N, F, NCL = 6, 2, 3
ERR_ARG, ERR_UNSUPPORTED = 1, 3


def _batch():
    """DetectionEvaluator.update's positional arguments, on the host: the checks under test
    come before the one that wants device tensors."""
    return (torch.zeros((N, NC)), torch.zeros((NCL, NC)), torch.tensor([0, 2, 4, 6]),
            torch.arange(N), torch.zeros(N, dtype=torch.int64),
            torch.zeros(N, dtype=torch.int32), torch.tensor([0, 3, 6]))


def _last_of(other):
    """What ``other.last`` holds after an update on _batch(), as far as the check reads it."""
    return dict(gt={}, assoc={}, pred_class=None, params=other._association_params(N, F, NCL))


def test_two_stage_constructor():
    with pytest.raises(ValueError, match='cluster_size_threshold'):
        ev.TwoStageEvaluators(NC, min_meas=2, cluster_size_threshold=0)
    with pytest.raises(ValueError, match='cluster_size_threshold'):
        ev.TwoStageEvaluators(NC)                         # the defaults are that pair
    with pytest.raises(ValueError, match='cluster_size_threshold'):
        ev.TwoStageEvaluators(NC, min_meas=4, cluster_size_threshold=2)
    with pytest.raises(ValueError):
        ev.TwoStageEvaluators(NC, cluster_size_threshold=1, by_segmentation=False)
    with pytest.raises(ValueError):
        ev.TwoStageEvaluators(NC, cluster_size_threshold=1, class_source='classifier')
    with pytest.raises(ValueError):
        ev.TwoStageEvaluators(NC, cluster_size_threshold=1, association_criteria='x')
    t = ev.TwoStageEvaluators(NC, min_meas=2, cluster_size_threshold=1, eps=0.5,
                              association_criteria='l2_norm')
    assert sorted(t.detection) == sorted(t.object_class) == ['classifier', 'object_head',
                                                             'segmentation']
    for s, d in t.detection.items():
        assert d.class_source == s and d.eps == 0.5 and d.cluster_size_threshold == 1
        assert d.association_criteria == 'l2_norm'
        assert isinstance(t.object_class[s], ev.ObjectClassEvaluator)
    assert ev.TwoStageEvaluators(NC, min_meas=1).min_meas == 1       # threshold 0 suffices
    assert ev.ObjectClassEvaluator.NAMES == ('confusion_matrix', 'gt_count_matrix')
    # nothing was counted: the reports of the empty evaluators are all zero
    res = t.result()
    assert sorted(res) == sorted(t.SOURCES)
    for s in t.SOURCES:
        assert int(res[s]['detection']['pred_count_matrix'].sum()) == 0
        assert res[s]['object_class']['confusion_matrix'].shape == (NC, NC)
    with pytest.raises(ValueError):
        t.merge(ev.TwoStageEvaluators(NC, min_meas=1))


def test_class_source_names():
    assert ev.DetectionEvaluator().class_source == 'segmentation'
    assert ev.DetectionEvaluator(by_segmentation=False).class_source == 'object_head'
    assert ev.DetectionEvaluator(class_source='segmentation').by_segmentation is True
    # the name wins over the flag it replaces
    assert ev.DetectionEvaluator(by_segmentation=True,
                                 class_source='object_head').by_segmentation is False
    assert ev.DetectionEvaluator(class_source='classifier').class_source == 'classifier'
    for bad in ('vote', 'Classifier', ''):
        with pytest.raises(ValueError, match='class_source'):
            ev.DetectionEvaluator(class_source=bad)


def test_classifier_source_needs_cluster_class():
    d = ev.DetectionEvaluator(class_source='classifier')
    with pytest.raises(ValueError, match='cluster_class'):
        d.update(*_batch())
    with pytest.raises(ValueError, match='cluster_class'):
        d.update(*_batch(), cluster_class=torch.zeros(NCL - 1, dtype=torch.int64))
    # with the classes the next check is the one for device tensors
    with pytest.raises(ValueError, match='device tensors'):
        d.update(*_batch(), cluster_class=torch.zeros(NCL, dtype=torch.int64))


@pytest.mark.parametrize('other', [dict(eps=0.5), dict(cluster_size_threshold=1),
                                   dict(association_criteria='l2_norm')])
def test_association_from_other_settings_is_refused(other):
    d = ev.DetectionEvaluator(NC)
    with pytest.raises(ValueError, match='association='):
        d.update(*_batch(), association=_last_of(ev.DetectionEvaluator(NC, **other)))
    # the same settings on another batch (one more cluster)
    last = _last_of(ev.DetectionEvaluator(NC))
    last['params'] = dict(last['params'], n_clusters=NCL + 1)
    with pytest.raises(ValueError, match='association='):
        d.update(*_batch(), association=last)
    # a dict that is no evaluator's ``last``
    with pytest.raises(ValueError, match='association='):
        d.update(*_batch(), association={})
    # the same settings on the same batch pass this check
    with pytest.raises(ValueError, match='device tensors'):
        d.update(*_batch(), association=_last_of(ev.DetectionEvaluator(NC, by_segmentation=False)))


@pytest.fixture(scope='module')
def lib():
    from graph_neural_network_for_radar_perception_amd import build
    build.build_library()
    return nat.lib()


def test_cluster_class_from_objects_checks_arguments(lib):
    f = 4096  # any non-null address: nothing is dereferenced before the checks fail

    def call(ld=NC, n=10, nc=NC, ncl=12, fill=6, logits=f, oc=f, cls=f, score=f, bad=f):
        return lib.rg_cluster_class_from_objects(logits, ld, n, nc, oc, ncl, fill, cls, score,
                                                 bad, None)

    assert call(nc=0, ld=0) == ERR_UNSUPPORTED
    assert b'num_classes' in lib.rg_last_error()
    assert call(nc=33, ld=40) == ERR_UNSUPPORTED
    assert call(ld=NC - 1) == ERR_ARG
    assert b'ld=' in lib.rg_last_error()
    assert call(n=-1) == ERR_ARG
    assert b'n_objects' in lib.rg_last_error()
    assert call(ncl=-1) == ERR_ARG
    for name in ('logits', 'oc', 'cls', 'bad'):
        assert call(**{name: None}) == ERR_ARG, name
        assert b'null' in lib.rg_last_error(), name
    # no clusters: nothing to fill, nothing is launched
    assert call(ncl=0, logits=None, oc=None, cls=None, score=None, bad=None) == 0
    assert 'rg_cluster_class_from_objects' in nat.header_functions()


def test_class_confusion_checks_arguments(lib):
    f = 4096

    def call(n=10, nc=NC, gt=f, pred=f, conf=f, cnt=f, bad=f):
        return lib.rg_eval_class_confusion(gt, pred, n, nc, conf, cnt, bad, None)

    assert call(nc=0) == ERR_UNSUPPORTED
    assert call(nc=33) == ERR_UNSUPPORTED
    assert call(n=-1) == ERR_ARG
    for name in ('gt', 'pred', 'conf', 'cnt', 'bad'):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(n=0, gt=None, pred=None, conf=None, cnt=None, bad=None) == 0
    assert 'rg_eval_class_confusion' in nat.header_functions()
