"""Milliseconds per classifier training step from a sequence in HBM: the loop a caller had to
write against classifier.training.train_classifier_sequence, and the detector forward's share.

Workload: batches of 64 sliding windows x 10 scans of a seeded synthetic sequence
(synthetic.make_sequence), stride 1, consecutive batches.  The generator spreads positions
uniformly, which leaves nothing to cluster, so every tracked return is moved next to a centre
of its track (8 tracks, fixed centres in the car frame, 0.3 m scatter): the proposals then hold
objects of several members and the classifier trains on them.  The detector is the trained
checkpoint of tests/golden (model_trained_N50) with the classifier configuration's
clustering_eps; the classifier is the yml model from a fixed seed.  No flip in either path
(evaluate_window_batch has none), so both do the same work on the same windows and the same
feature values (path (b) takes the rcs from the frame's meas_rcs, path (a) from the node
features' rcs column, a copy of it).

  path (a)  train_classifier_sequence over the batch (ClassifierTrainer: fused forward and
            backward from object sizes, one optimizer launch)
  path (b)  the loop without it: evaluation.evaluate_window_batch ->
            objects.classifier_training_batch -> the per-frame sample lists ->
            Model_Training.forward(...).backward() -> torch.optim.SGD.step()

Both paths run in one process on two models of the same seed, alternating step by step over
the same batches; each step is a host clock around work that ends in a device synchronise;
median and quartiles of --steps steps after --warmup warm-ups.  The detector's forward alone
(engine.forward_batched on the batch's graph with the proposals given, so nothing waits for
the host) is timed between HIP events on the same batches and reported as a share of path
(a)'s median.  No threshold.  Prints one JSON line.

Usage:  python scripts/bench_classifier_feed.py [--steps 30] [--warmup 5] [--windows 64]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from graph_neural_network_for_radar_perception_amd import (engine, evaluation,  # noqa: E402
                                                           frontend, objects, sequence, synthetic)
from graph_neural_network_for_radar_perception_amd import gnn_detector  # noqa: E402
from graph_neural_network_for_radar_perception_amd.classifier import Model_Training  # noqa: E402
from graph_neural_network_for_radar_perception_amd.classifier import training as ct  # noqa: E402
from graph_neural_network_for_radar_perception_amd.config import (  # noqa: E402
    default_classifier_config)

CHECKPOINT = os.path.join(REPO, 'tests', 'golden', 'model_trained_N50.npz')


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def clustered_sequence(seed: int, n_scenes: int, mean_meas: int):
    """synthetic.make_sequence with every tracked return next to its track's centre."""
    radar, odo, lists, sensors = synthetic.make_sequence(seed, n_scenes, mean_meas)
    rng = np.random.default_rng(seed + 1)
    ids = np.unique(radar['track_id'])
    ids = ids[ids != b'']
    cx = rng.uniform(8.0, 70.0, len(ids))
    cy = rng.uniform(-35.0, 35.0, len(ids))
    for t, x, y in zip(ids, cx, cy):
        sel = radar['track_id'] == t
        n = int(sel.sum())
        radar['x_cc'][sel] = (x + rng.normal(0, 0.3, n)).astype(np.float32)
        radar['y_cc'][sel] = (y + rng.normal(0, 0.3, n)).astype(np.float32)
    return radar, odo, lists, sensors


def detector_model(cfg, dev):
    d = np.load(CHECKPOINT, allow_pickle=False)
    mt = gnn_detector.Model_Training(cfg, dev)
    mt.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith('w/')})
    m = mt.to(dev).pred.eval().requires_grad_(False)
    m.set_param_for_proposal_extraction(float(cfg.clustering_eps), False)
    return m


def callers_step(win, detector, model, opt, cfg, cache):
    """Path (b)."""
    fb, out = evaluation.evaluate_window_batch(win, detector, cfg, cache=cache)
    if out is None:
        return None
    # rcs: evaluate_window_batch does not return the node features; their column 1, which path
    # (a) reads (datagen_classifier.py:256), is a float32 copy of meas_rcs (the node-feature
    # kernel of csrc/graph_features.hip writes o[1] = rcs[i]), so both paths train on the same
    # values
    det = SimpleNamespace(xy=torch.stack((fb.arrays['meas_px'], fb.arrays['meas_py']), dim=-1),
                          rcs=fb.arrays['meas_rcs'], cluster_ptr=out.cluster_ptr,
                          cluster_idx=out.cluster_idx, frame_ptr=fb.frame_ptr,
                          meas_noise_cov=cfg.meas_noise_cov)
    batch, inp = objects.classifier_training_batch(
        det, fb.labels['class_labels'], int(cfg.valid_cluster_num_meas_thr),
        num_classes=int(cfg.num_classes))
    if batch is None:
        return None
    ss = inp.samples()
    opt.zero_grad()
    loss = model([s['object_features'] for s in ss], [s['edge_idx'] for s in ss],
                 [s['object_num_meas'] for s in ss], [s['object_class'] for s in ss])
    loss.backward()
    opt.step()
    return loss.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--window-size', type=int, default=10)
    ap.add_argument('--mean-meas', type=int, default=134)
    ap.add_argument('--scenes', type=int, default=600)
    args = ap.parse_args()
    if args.steps < 30 or args.warmup < 5:
        ap.error('at least 30 steps after 5 warm-ups')
    if not torch.cuda.is_available():
        raise SystemExit('bench_classifier_feed.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W = args.windows, args.window_size
    radar, odo, lists, sensors = clustered_sequence(148, args.scenes, args.mean_meas)
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    n = store.n_windows(W)
    if n < B:
        ap.error(f'{args.scenes} scenes hold {n} windows, fewer than one batch of {B}')
    starts = [(s * B) % (n - B + 1) for s in range(args.warmup + args.steps)]
    cfg = default_classifier_config()
    detector = detector_model(cfg, dev)
    models = []
    for _ in range(2):
        torch.manual_seed(148)
        models.append(Model_Training(cfg).to(dev).train())
    trainer = ct.ClassifierTrainer(models[0], cfg, world=1)
    opt_b = torch.optim.SGD(models[1].parameters(), lr=cfg.learning_rate, momentum=0.9,
                            weight_decay=cfg.weight_decay)
    min_meas = int(cfg.valid_cluster_num_meas_thr)

    ta, tb, t_fwd, n_obj, n_rows = [], [], [], [], []
    cache_b: dict = {}
    cache_f: dict = {}
    for s, i0 in enumerate(starts):
        pos = np.arange(i0, i0 + B)
        seen = []
        da, la = timed(lambda: ct.train_classifier_sequence(
            store, detector, trainer, cfg, pos, W, B, augmentation=False, min_meas=min_meas,
            on_step=lambda k, p, f, loss, inp: seen.append(inp)), dev)
        db, lb = timed(lambda: callers_step(store.windows(pos, W), detector, models[1], opt_b,
                                            cfg, cache_b), dev)
        # the detector forward alone, the proposals given, between HIP events
        dd, gd = frontend.dynamic_frame(store.windows(pos, W), with_keys=True)
        fb = frontend.frame_batch(dd, gd)
        det = objects.detect_frames(detector, fb, cfg, cache=cache_f)
        gb = det.graph_batch
        ncl = int(det.cluster_ptr.numel()) - 1
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        torch.cuda.synchronize(dev)
        e0.record()
        with torch.no_grad():
            engine.forward_batched(detector.plans(), gb.node_features, gb.edge_features,
                                   gb.graph, det.cluster_ptr, det.cluster_idx, ncl,
                                   n_pairs_cap=gb.capacity // 2 + 1,
                                   buffers=cache_f.setdefault('buffers', {}))
        e1.record()
        torch.cuda.synchronize(dev)
        if s >= args.warmup:
            ta.append(da)
            tb.append(db)
            t_fwd.append(e0.elapsed_time(e1))
            inp = seen[0]
            n_obj.append(inp.n_objects if inp is not None else 0)
            n_rows.append(inp.n_rows if inp is not None else 0)
    assert la.numel() == 1 and bool(torch.isfinite(la).all()), 'path (a) trained on nothing'
    assert lb is not None and bool(torch.isfinite(lb)), 'path (b) trained on nothing'

    med = statistics.median
    a, b, f = med(ta), med(tb), med(t_fwd)
    q = lambda v, k=1e3: [round(x * k, 3) for x in np.percentile(v, [25, 75])]  # noqa: E731
    print(json.dumps({
        'workload': f'{B} windows x {W} scans x ~{args.mean_meas} detections, clustered tracks, '
                    'yml classifier, trained detector',
        'steps': args.steps, 'warmup': args.warmup,
        'train_classifier_sequence_step_ms': round(a * 1e3, 3),
        'train_classifier_sequence_step_ms_q25_q75': q(ta),
        'callers_loop_step_ms': round(b * 1e3, 3), 'callers_loop_step_ms_q25_q75': q(tb),
        'callers_loop_over_train_classifier_sequence': round(b / a, 2),
        'detector_forward_ms': round(f, 3), 'detector_forward_ms_q25_q75': q(t_fwd, 1.0),
        'detector_forward_share_of_step': round(f / (a * 1e3), 3),
        'objects_per_step': round(float(np.mean(n_obj)), 1),
        'objects_per_step_min_max': [int(min(n_obj)), int(max(n_obj))],
        'rows_per_step': round(float(np.mean(n_rows)), 1)}))


if __name__ == '__main__':
    main()
