"""Host checks of object-head finetuning (training.py: finetune_parameters, FinetuneTrainer,
average_counted; config.py's FINETUNING attributes, set_config_gnn.py:110-114).  No device is
needed: the fused optimizer's buffers are plain tensors and the head engine is built on first
use only."""
import numpy as np
import pytest
import torch


def _cfg():
    from graph_neural_network_for_radar_perception_amd.config import default_config
    return default_config(graph_convolution_stem_channels=[64, 64])


def _model(freeze=True):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import (
        Model_Object_Classifier_Finetuning)
    torch.manual_seed(3)
    m = Model_Object_Classifier_Finetuning(_cfg())
    if freeze:
        m.pred.freeze_layers_except_object_class_predictor()
    return m


def test_config_has_the_finetuning_section():
    from graph_neural_network_for_radar_perception_amd import config
    cfg = config.default_config()
    ft = config._DEFAULTS['FINETUNING']
    assert cfg.optim_finetuning == ft['optim'] == 'sgd'
    assert cfg.max_train_iter_finetuning == ft['max_training_iterations'] == 10000
    assert cfg.learning_rate_finetuning == ft['learning_rate'] == 0.0005
    assert cfg.weight_decay_finetuning == ft['weight_decay'] == 0.0001
    assert cfg.clustering_eps == ft['clustering_eps']
    # the detector's own optimisation section is another one
    assert cfg.learning_rate == 0.005 and cfg.max_train_iter == 200000


def test_finetune_parameters_accepts_the_reference_freeze_pattern():
    from graph_neural_network_for_radar_perception_amd.training import finetune_parameters
    m = _model()
    got = finetune_parameters(m)
    want = [p for n, p in m.named_parameters() if n.startswith('pred.predict_class.')]
    assert len(got) == len(want) > 0 and all(a is b for a, b in zip(got, want))
    # the reference's own list (set_param_for_finetuning_obj_classifier.py:39)
    ref = [p for p in m.parameters() if p.requires_grad]
    assert len(ref) == len(got) and all(a is b for a, b in zip(got, ref))
    # the bare Model_Inference is taken too
    got_pred = finetune_parameters(m.pred)
    assert len(got_pred) == len(got) and all(a is b for a, b in zip(got_pred, got))


def test_finetune_parameters_refuses_other_patterns():
    from graph_neural_network_for_radar_perception_amd.training import finetune_parameters
    with pytest.raises(ValueError, match='trainable outside'):
        finetune_parameters(_model(freeze=False))
    m = _model()
    m.pred.predict_node.stem[0].block[0].weight.requires_grad = True     # one backbone tensor
    with pytest.raises(ValueError, match='pred.predict_node'):
        finetune_parameters(m)
    m = _model()
    for p in m.parameters():
        p.requires_grad = False
    with pytest.raises(ValueError, match='frozen'):
        finetune_parameters(m)
    m = _model()
    m.pred.predict_class.pred_cls.head[1].bias.requires_grad = False     # part of the head
    with pytest.raises(ValueError, match='frozen'):
        finetune_parameters(m)


def test_average_counted_rule():
    from graph_neural_network_for_radar_perception_amd.training import average_counted
    nan = float('nan')
    mean, n = average_counted([0.5, 0.0, -1.0, nan, 1.5])
    assert n == 2 and mean == 1.0
    acc, n = average_counted([0.5, 0.0, -1.0, nan, 1.5], [0.25, 1.0, 1.0, 1.0, 0.75])
    assert n == 2 and acc == 0.5
    for none in ([], [0.0], [nan, nan], [-2.0, 0.0, nan]):
        mean, n = average_counted(none)
        assert np.isnan(mean) and n == 0
        acc, n = average_counted(none, [1.0] * len(none))
        assert np.isnan(acc) and n == 0
    # float32 device losses as they are read back
    vals = np.array([0.25, np.nan, 0.75], np.float32)
    assert average_counted(vals) == (0.5, 2)
    with pytest.raises(ValueError):
        average_counted([1.0, 2.0], [1.0])


def test_trainer_takes_the_finetuning_section_and_the_head_only(tmp_path):
    from graph_neural_network_for_radar_perception_amd.training import FinetuneTrainer
    cfg = _cfg()
    m = _model()
    want = {k: v.detach().clone() for k, v in m.state_dict().items()}
    n_head = sum(p.numel() for n, p in m.named_parameters()
                 if n.startswith('pred.predict_class.'))
    tr = FinetuneTrainer(m, cfg)
    assert type(tr.opt).__name__ == 'FusedSGD' and tr.opt.momentum == 0.9
    assert tr.opt.lr == cfg.learning_rate_finetuning != cfg.learning_rate
    assert tr.opt.weight_decay == cfg.weight_decay_finetuning
    assert tr.opt.milestones == []                       # lr_scheduler = None
    assert tr.opt.flat.numel() == n_head
    assert tr.opt.on_update == m.invalidate_head_plans
    assert getattr(m, '_head_engine', None) is None      # nothing packed yet
    assert tr.step_detections(None, None) is None and tr.opt.steps == 0
    # the parameters are views of the flat buffer; the values are unchanged
    for k, v in m.state_dict().items():
        assert torch.equal(v, want[k]), k
    adam = FinetuneTrainer(_model(), cfg, optim='adamw', lr=0.01, weight_decay=0.02)
    assert type(adam.opt).__name__ == 'FusedAdamW'
    assert adam.opt.lr == 0.01 and adam.opt.weight_decay == 0.02
    with pytest.raises(ValueError, match='rmsprop'):
        FinetuneTrainer(_model(), cfg, optim='rmsprop')
    with pytest.raises(ValueError, match='trainable outside'):
        FinetuneTrainer(_model(freeze=False), cfg)
    half = _model()
    half.pred.compute_dtype = 'bf16'
    with pytest.raises(NotImplementedError, match='float32'):
        FinetuneTrainer(half, cfg)
    # save: the reference's state_dict keys
    path = tmp_path / 'finetuned.pth'
    tr.save(path)
    sd = torch.load(path, map_location='cpu')
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert torch.equal(v, want[k]), k
