"""Milliseconds per object-head finetuning step from a sequence in HBM: the loop a caller had
to write around the drop-in module against training.finetune_sequence, and the head-only step's
share.

Workload: batches of 64 sliding windows x 10 scans of a seeded synthetic sequence
(synthetic.make_sequence), stride 1, consecutive batches, every tracked return moved next to a
centre of its track as scripts/bench_classifier_feed.py moves them (the proposals then hold
objects of several members).  The model is the trained checkpoint of tests/golden
(model_trained_N50) as a Model_Object_Classifier_Finetuning, frozen except predict_class, with
cfg.clustering_eps; SGD, momentum 0.9, cfg.learning_rate_finetuning / weight_decay_finetuning.
No flip in either path, so both do the same work on the same windows.

  path (a)  finetune_sequence over the batch (FinetuneTrainer: the no-grad proposal forward,
            the head-only forward and backward from its node embeddings, one optimizer launch)
  path (b)  the loop without it: store.windows -> frontend.dynamic_frame -> frame_batch ->
            graph_features.build_graph_batch -> the per-frame lists ->
            Model_Object_Classifier_Finetuning(...) -> loss.backward() ->
            torch.optim.SGD.step()

Both paths run in one process on two models of the same checkpoint, alternating step by step
over the same batches; each step is a host clock around work that ends in a device
synchronise; median and quartiles of --steps steps after --warmup warm-ups.  The head step alone
(FinetuneTrainer.step_detections on a ready Detections: majority labels, head forward and
backward, optimizer launch, re-pack; nothing in it waits for the host) is timed between HIP
events on the same batches, on path (a)'s model, and reported as a share of path (a)'s median.
No threshold.  Prints one JSON line.

Usage:  python scripts/bench_finetune_feed.py [--steps 30] [--warmup 5] [--windows 64]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from graph_neural_network_for_radar_perception_amd import (frontend, objects,  # noqa: E402
                                                           sequence, synthetic, training)
from graph_neural_network_for_radar_perception_amd.config import default_config  # noqa: E402
from graph_neural_network_for_radar_perception_amd.gnn_detector import (  # noqa: E402
    Model_Object_Classifier_Finetuning)
from graph_neural_network_for_radar_perception_amd.graph_features import (  # noqa: E402
    build_graph_batch)

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


def finetune_model(cfg, dev):
    d = np.load(CHECKPOINT, allow_pickle=False)
    m = Model_Object_Classifier_Finetuning(cfg)
    m.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith('w/')})
    m = m.to(dev)
    m.pred.freeze_layers_except_object_class_predictor()
    return m.train()


def frame_lists(fb, gb):
    """The drop-in's per-frame list arguments from a batch on the device: each frame's rows of
    the node features, its destination-major edges (source -> destination, frame-local) with
    their features, its positions and its node classes.  Two host reads (the frames' node and
    edge ranges); every list entry is a view."""
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


def callers_step(win, model, opt, cfg, cache):
    """Path (b)."""
    dd, gd = frontend.dynamic_frame(win, with_keys=True)
    fb = frontend.frame_batch(dd, gd)
    if fb.n_frames == 0:
        return None
    gb = build_graph_batch(fb, cfg, ws_cache=cache)
    opt.zero_grad()
    loss, _ = model(**frame_lists(fb, gb))
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
        raise SystemExit('bench_finetune_feed.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W = args.windows, args.window_size
    radar, odo, lists, sensors = clustered_sequence(148, args.scenes, args.mean_meas)
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    n = store.n_windows(W)
    if n < B:
        ap.error(f'{args.scenes} scenes hold {n} windows, fewer than one batch of {B}')
    starts = [(s * B) % (n - B + 1) for s in range(args.warmup + args.steps)]
    cfg = default_config()
    models = [finetune_model(cfg, dev) for _ in range(2)]
    trainer = training.FinetuneTrainer(models[0], cfg, world=1)
    opt_b = torch.optim.SGD([p for p in models[1].parameters() if p.requires_grad],
                            lr=cfg.learning_rate_finetuning, momentum=0.9,
                            weight_decay=cfg.weight_decay_finetuning)

    ta, tb, t_head, n_cl, n_nodes = [], [], [], [], []
    cache_b: dict = {}
    cache_h: dict = {}
    la = lb = None
    for s, i0 in enumerate(starts):
        pos = np.arange(i0, i0 + B)
        seen = []
        da, la = timed(lambda: training.finetune_sequence(
            store, trainer, cfg, pos, W, B, augmentation=False,
            on_step=lambda k, p, f, out, det: seen.append(det)), dev)
        db, lb = timed(lambda: callers_step(store.windows(pos, W), models[1], opt_b, cfg,
                                            cache_b), dev)
        # the head step alone on a ready Detections, between HIP events
        dd, gd = frontend.dynamic_frame(store.windows(pos, W), with_keys=True)
        fb = frontend.frame_batch(dd, gd)
        det = objects.detect_frames(models[0].pred, fb, cfg, cache=cache_h)
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        torch.cuda.synchronize(dev)
        e0.record()
        trainer.step_detections(det, fb.labels['class_labels'])
        e1.record()
        torch.cuda.synchronize(dev)
        if s >= args.warmup:
            ta.append(da)
            tb.append(db)
            t_head.append(e0.elapsed_time(e1))
            d0 = seen[0]
            n_cl.append(int(d0.cluster_ptr.numel()) - 1 if d0 is not None else 0)
            n_nodes.append(int(d0.x.shape[0]) if d0 is not None else 0)
    assert la[0].numel() == 1 and bool(torch.isfinite(la[0]).all()), 'path (a) trained on nothing'
    assert lb is not None and bool(torch.isfinite(lb)), 'path (b) trained on nothing'

    med = statistics.median
    a, b, h = med(ta), med(tb), med(t_head)
    q = lambda v, k=1e3: [round(x * k, 3) for x in np.percentile(v, [25, 75])]  # noqa: E731
    print(json.dumps({
        'workload': f'{B} windows x {W} scans x ~{args.mean_meas} detections, clustered tracks, '
                    'trained checkpoint frozen except predict_class',
        'steps': args.steps, 'warmup': args.warmup,
        'finetune_sequence_step_ms': round(a * 1e3, 3),
        'finetune_sequence_step_ms_q25_q75': q(ta),
        'callers_loop_step_ms': round(b * 1e3, 3), 'callers_loop_step_ms_q25_q75': q(tb),
        'callers_loop_over_finetune_sequence': round(b / a, 2),
        'head_step_ms': round(h, 3), 'head_step_ms_q25_q75': q(t_head, 1.0),
        'head_step_share_of_step': round(h / (a * 1e3), 3),
        'last_loss_finetune_sequence': round(float(la[0][-1]), 5),
        'last_loss_callers_loop': round(float(lb), 5),
        'proposals_per_step': round(float(np.mean(n_cl)), 1),
        'proposals_per_step_min_max': [int(min(n_cl)), int(max(n_cl))],
        'nodes_per_step': round(float(np.mean(n_nodes)), 1)}))


if __name__ == '__main__':
    main()
