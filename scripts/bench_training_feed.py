"""Milliseconds per training step from a sequence in HBM: labels made on the host against the
training feed (training.train_sequence), and the label stage alone.

Workload: batches of 64 sliding windows x 10 scans x ~134 detections per scan on the synthetic
sequence of scripts/bench_sequence.py, stride 1, consecutive batches, the yml model, x-axis flip
augmentation on in both paths (the same flags' worth of work).

  path (a)  the host-labelled step a caller has to write without the feed: SequenceStore.windows
            -> frontend.dynamic_frame -> frame_batch -> build_graph_batch, download row_ptr,
            col, the track keys and the node labels, make the labels and the ground-truth
            clusters in numpy (tests/training_feed_ref.py), upload them, RadarGNNTrainer.step
            (which builds the graph again)
  path (b)  training.train_sequence over the same windows (one batch per call)

Both paths run in one process on two models of the same seed, alternating step by step over
the same batches; each step is a host clock around work that ends in a device synchronise;
the median of --steps steps after --warmup warm-ups is reported.  The label stage alone
(training.training_labels: rg_train_labels + rg_eval_gt_clusters) is timed with HIP events
over the same batches, and so is the front-end's ground truth (frontend.compute_ground_truth)
without and with numpy's float32 track mean (rg_train_offsets), which both paths run.  Prints
one JSON line.

--determinism instead checks what the exact step_frames == step test rests on: for L = 2 and
L = 7 conv layers, two models of the same seed each take three RadarGNNTrainer.step calls on
the same three host-labelled batches (8 windows); it prints per L whether the losses, the
accuracies and the weights after the three steps are bit-equal, and fails if not.

Usage:  python scripts/bench_training_feed.py [--steps 30] [--warmup 5] [--windows 64]
        python scripts/bench_training_feed.py --determinism
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
for p in (REPO, os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import training_feed_ref as tref  # noqa: E402
from graph_neural_network_for_radar_perception_amd import (frontend, sequence,  # noqa: E402
                                                           synthetic, training)
from graph_neural_network_for_radar_perception_amd.config import default_config  # noqa: E402
from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training  # noqa: E402
from graph_neural_network_for_radar_perception_amd.graph_features import (  # noqa: E402
    FrameBatch, build_graph_batch)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def host_labelled_step(store, trainer, cfg, pos, W, flags, dev):
    """Path (a)."""
    dd, gd = frontend.dynamic_frame(store.windows(pos, W), with_keys=True, flip=flags)
    fb = frontend.frame_batch(dd, gd)
    gb = build_graph_batch(fb, cfg, ws_cache=trainer.ws_cache)
    rp = gb.row_ptr.cpu().numpy().astype(np.int64)
    col = gb.col[:int(rp[-1])].cpu().numpy().astype(np.int64)
    ei = np.stack((np.repeat(np.arange(len(rp) - 1), np.diff(rp)), col))
    key = fb.track_key.cpu().numpy()
    cls = fb.labels['class_labels'].cpu().numpy().astype(np.int64)
    off = np.stack((fb.labels['offsetx'].cpu().numpy(), fb.labels['offsety'].cpu().numpy()), -1)
    src, dst = tref.link_pairs(ei)
    ptr, idx, clab = tref.gt_clusters(key, cls, fb.frame_ptr.cpu().numpy())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    labels = {'node_class': up(cls), 'node_offsets': up(off),
              'edge_class': up(tref.edge_labels(key, src, dst)), 'cluster_labels': up(clab),
              'class_weights': torch.tensor(cfg.class_weights_dyn, dtype=torch.float32,
                                            device=dev)}
    batch = FrameBatch(fb.arrays, fb.frame_ptr, fb.frame_sizes, up(ptr.astype(np.int32)),
                       up(idx.astype(np.int32)), len(clab))
    return trainer.step(batch, labels)


def determinism(store, W, dev):
    ok = True
    for L in (2, 7):
        cfg = default_config(graph_convolution_stem_channels=[64] * L)
        runs = []
        for _ in range(2):
            torch.manual_seed(148)
            model = Model_Training(cfg, 'cpu').to(dev).train()
            tr = training.RadarGNNTrainer(model, cfg, world=1)
            np.random.seed(148)
            outs = []
            for s in range(3):
                pos = np.arange(8 * s, 8 * s + 8)
                losses, acc, _ = host_labelled_step(store, tr, cfg, pos, W,
                                                    frontend.draw_flips(8), dev)
                outs.append((losses.clone(), acc.clone()))
            runs.append((outs, tr.opt.flat.clone()))
        (o0, w0), (o1, w1) = runs
        eq_l = all(torch.equal(a[0], b[0]) for a, b in zip(o0, o1))
        eq_a = all(torch.equal(a[1], b[1]) for a, b in zip(o0, o1))
        eq_w = torch.equal(w0, w1)
        print(f'L={L}: losses equal {eq_l}, accuracies equal {eq_a}, '
              f'weights after 3 steps equal {eq_w}')
        ok = ok and eq_l and eq_a and eq_w
    if not ok:
        raise SystemExit('two identical step sequences differ')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--window-size', type=int, default=10)
    ap.add_argument('--mean-meas', type=int, default=134)
    ap.add_argument('--scenes', type=int, default=600)
    ap.add_argument('--determinism', action='store_true')
    args = ap.parse_args()
    if args.steps < 20 or args.warmup < 5:
        ap.error('at least 20 steps after 5 warm-ups')
    if not torch.cuda.is_available():
        raise SystemExit('bench_training_feed.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W = args.windows, args.window_size
    radar, odo, lists, sensors = synthetic.make_sequence(148, args.scenes, args.mean_meas)
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    if args.determinism:
        return determinism(store, W, dev)
    n = store.n_windows(W)
    if n < B:
        ap.error(f'{args.scenes} scenes hold {n} windows, fewer than one batch of {B}')
    starts = [(s * B) % (n - B + 1) for s in range(args.warmup + args.steps)]
    cfg = default_config()
    trainers = []
    for _ in range(2):
        torch.manual_seed(148)
        model = Model_Training(cfg, 'cpu').to(dev).train()
        trainers.append(training.RadarGNNTrainer(model, cfg, world=1))
    tr_a, tr_b = trainers

    np.random.seed(148)
    ta, tb, t_lab, t_gt, t_gt_np, nodes, pairs = [], [], [], [], [], [], []
    ws: dict = {}
    for s, i0 in enumerate(starts):
        pos = np.arange(i0, i0 + B)
        flags = frontend.draw_flips(B)
        da, out_a = timed(lambda: host_labelled_step(store, tr_a, cfg, pos, W, flags, dev), dev)
        # train_sequence draws its own flags from numpy's generator
        db, out_b = timed(lambda: training.train_sequence(store, tr_b, cfg, pos, W, B), dev)
        # the label stage alone, between HIP events
        dd, gd = frontend.dynamic_frame(store.windows(pos, W), with_keys=True, flip=flags)
        fb = frontend.frame_batch(dd, gd)
        gb = build_graph_batch(fb, cfg, ws_cache=ws)
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        torch.cuda.synchronize(dev)
        e0.record()
        lab = training.training_labels(fb, gb, cfg, ws)
        e1.record()
        torch.cuda.synchronize(dev)
        # the ground truth of the whole windows, with the float64 and with numpy's track mean
        d = frontend.flip_along_x(frontend.extract_and_sync_radar_data(store.windows(pos, W)), flags)
        gt_us = []
        for numpy_mean in (False, True):
            g0, g1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            torch.cuda.synchronize(dev)
            g0.record()
            frontend.compute_ground_truth(d, numpy_mean)
            g1.record()
            torch.cuda.synchronize(dev)
            gt_us.append(g0.elapsed_time(g1) * 1e3)
        if s >= args.warmup:
            t_gt.append(gt_us[0])
            t_gt_np.append(gt_us[1])
            ta.append(da)
            tb.append(db)
            t_lab.append(e0.elapsed_time(e1) * 1e3)
            nodes.append(fb.n_nodes)
            pairs.append(int(gb.graph.n_pairs_dev.item()))
    assert torch.isfinite(out_a[0]).all() and torch.isfinite(out_b[0]).all()

    med = statistics.median
    a, b, lab_us = med(ta), med(tb), med(t_lab)
    q = lambda v, k=1e3: [round(x * k, 3) for x in np.percentile(v, [25, 75])]  # noqa: E731
    print(json.dumps({
        'workload': f'{B} windows x {W} scans x ~{args.mean_meas} detections, yml model',
        'steps': args.steps, 'warmup': args.warmup,
        'host_labelled_step_ms': round(a * 1e3, 3), 'host_labelled_step_ms_q25_q75': q(ta),
        'train_sequence_step_ms': round(b * 1e3, 3), 'train_sequence_step_ms_q25_q75': q(tb),
        'host_labelled_over_train_sequence': round(a / b, 2),
        'label_stage_us': round(lab_us, 1), 'label_stage_us_q25_q75': q(t_lab, 1.0),
        'ground_truth_us': round(med(t_gt), 1), 'ground_truth_us_q25_q75': q(t_gt, 1.0),
        'ground_truth_numpy_mean_us': round(med(t_gt_np), 1),
        'ground_truth_numpy_mean_us_q25_q75': q(t_gt_np, 1.0),
        'mean_dynamic_nodes_per_batch': round(float(np.mean(nodes)), 1),
        'mean_link_pairs_per_batch': round(float(np.mean(pairs)), 1)}))


if __name__ == '__main__':
    main()
