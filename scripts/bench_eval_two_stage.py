"""What the classifier stage adds to a batch of evaluate_sequence, and what sharing the
association between the three class sources saves.

Workload: batches of 64 sliding windows x 10 scans of a seeded synthetic sequence
(synthetic.make_sequence), consecutive batches.  The generator spreads positions uniformly,
which leaves nothing to cluster, so every tracked return is moved next to a centre of its track
(as scripts/bench_classifier_feed.py does): the proposals then hold objects of several members.
The detector is the trained checkpoint of tests/golden (model_trained_N50) with the classifier
configuration's clustering_eps; the classifier is the yml model from a fixed seed.

Per association criterion ('inv_iou', 'l2_norm'), three variants of one batch
(store.windows -> evaluation.evaluate_window_batch), alternating step by step over the same
batches in one process:

  baseline     a DetectionEvaluator and a SegmentationEvaluator, no classifier: the batch of
               evaluate_sequence as it was before the classifier stage
  shared       the same plus the classifier stage (objects.classify_detections) and
               TwoStageEvaluators whose three class sources accumulate on ONE association
  independent  the same with share_association=False: three associations

The DetectionEvaluator beside the TwoStageEvaluators has their eps and threshold, so 'shared'
takes its association from it and associates once per batch where 'independent' does four
times.  Each figure is a host clock around work that ends in a device synchronise: the median
of --steps batches after --warmup warm-ups, for each of two runs of the whole measurement; the
shader clock (rg_clock_probe) is read before and after every run.  The classifier's forward
alone (objects.classify_inputs on the batch's inputs) is timed between HIP events on the same
batches and reported in ms and as a share of what 'shared' adds to the baseline.  No threshold.
Prints one JSON line.

Usage:  python scripts/bench_eval_two_stage.py [--steps 10] [--warmup 3] [--windows 64]
"""
from __future__ import annotations

import argparse
import ctypes
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

from graph_neural_network_for_radar_perception_amd import _native as nat  # noqa: E402
from graph_neural_network_for_radar_perception_amd import (evaluation, frontend,  # noqa: E402
                                                           objects, sequence, synthetic)
from graph_neural_network_for_radar_perception_amd import gnn_detector  # noqa: E402
from graph_neural_network_for_radar_perception_amd.classifier import Model_Training  # noqa: E402
from graph_neural_network_for_radar_perception_amd.config import (  # noqa: E402
    default_classifier_config)

CHECKPOINT = os.path.join(REPO, 'tests', 'golden', 'model_trained_N50.npz')
VARIANTS = ('baseline', 'shared', 'independent')


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def clock_mhz(dev, n_mfma: int = 65536, blocks: int = 256) -> float:
    """The shader clock the chip holds now (rg_clock_probe): the median over workgroups of
    shader cycles / wall-clock ticks x the tick rate."""
    out = torch.zeros(2 * blocks, dtype=torch.int64, device=dev)
    sink = torch.empty(4 * blocks, dtype=torch.float32, device=dev)
    khz = ctypes.c_int(0)
    nat.check(nat.lib().rg_clock_probe(blocks, n_mfma, out.data_ptr(), sink.data_ptr(),
                                       ctypes.byref(khz), nat.stream_ptr(dev)), 'rg_clock_probe')
    torch.cuda.synchronize(dev)
    o = out.view(blocks, 2).cpu().double()
    return round(float((o[:, 0] / o[:, 1].clamp(min=1)).median()) * khz.value / 1e3, 1)


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


def med(ts):
    return round(statistics.median(ts) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--window-size', type=int, default=10)
    ap.add_argument('--mean-meas', type=int, default=134)
    ap.add_argument('--scenes', type=int, default=600)
    ap.add_argument('--eps-iou', type=float, default=0.7, help="eps under 'inv_iou'")
    ap.add_argument('--eps-l2', type=float, default=1.5, help="eps under 'l2_norm', metres")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval_two_stage.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W = args.windows, args.window_size
    radar, odo, lists, sensors = clustered_sequence(148, args.scenes, args.mean_meas)
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    n = store.n_windows(W)
    if n < B:
        ap.error(f'{args.scenes} scenes hold {n} windows, fewer than one batch of {B}')
    starts = [(s * B) % (n - B + 1) for s in range(args.warmup + args.steps)]
    cfg = default_classifier_config()
    nc = int(cfg.num_classes)
    min_meas = int(cfg.valid_cluster_num_meas_thr)
    thr = max(min_meas - 1, 0)
    detector = detector_model(cfg, dev)
    torch.manual_seed(148)
    clf = Model_Training(cfg).to(dev).eval().requires_grad_(False)
    noise = cfg.meas_noise_cov
    eps = {'inv_iou': args.eps_iou, 'l2_norm': args.eps_l2}

    def evaluators(criterion, variant):
        kw = dict(eps=eps[criterion], cluster_size_threshold=thr, association_criteria=criterion)
        det = evaluation.DetectionEvaluator(nc, **kw)
        seg = evaluation.SegmentationEvaluator(nc)
        two = None
        if variant != 'baseline':
            two = evaluation.TwoStageEvaluators(nc, min_meas=min_meas,
                                                share_association=variant == 'shared', **kw)
        return det, seg, two

    def batch(pos, ev, cache):
        det, seg, two = ev
        win = store.windows(pos, W)
        if two is None:
            return evaluation.evaluate_window_batch(win, detector, cfg, det, seg, cache=cache)
        return evaluation.evaluate_window_batch(win, detector, cfg, det, seg, cache=cache,
                                                classifier=clf, two_stage=two,
                                                meas_noise_cov=noise)

    def classifier_forward_ms(pos, cache):
        """objects.classify_inputs alone, between HIP events, on the batch's own inputs."""
        dd, gd = frontend.dynamic_frame(store.windows(pos, W), with_keys=True)
        fb = frontend.frame_batch(dd, gd)
        d = objects.detect_frames(detector, fb, cfg, 'fp32', cache)
        inp = objects.classifier_inputs(d.xy, d.rcs, d.cluster_ptr, d.cluster_idx, d.frame_ptr,
                                        noise, min_meas, node_labels=fb.labels['class_labels'],
                                        num_classes=nc)
        objects.classify_inputs(clf, inp)                                    # warm this shape
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        objects.classify_inputs(clf, inp)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), fb.n_nodes, int(d.cluster_ptr.numel()) - 1, inp.n_objects, \
            inp.n_rows

    runs = []
    shape = {}
    for _ in range(2):
        clk0 = clock_mhz(dev)
        rec = {}
        for criterion in ('inv_iou', 'l2_norm'):
            evs = {v: evaluators(criterion, v) for v in VARIANTS}
            caches = {v: {} for v in VARIANTS}
            ts = {v: [] for v in VARIANTS}
            for s, i0 in enumerate(starts):
                pos = np.arange(i0, i0 + B)
                for v in VARIANTS:
                    dt, _ = timed(lambda: batch(pos, evs[v], caches[v]), dev)
                    if s >= args.warmup:
                        ts[v].append(dt)
            for v in VARIANTS:
                rec[f'{criterion}_{v}_ms'] = med(ts[v])
            # the variants count the same
            res = {v: evs[v][2].result() for v in VARIANTS[1:]}
            for src in res['shared']:
                for k in ('confusion_matrix', 'gt_count_matrix', 'pred_count_matrix'):
                    assert np.array_equal(res['shared'][src]['detection'][k],
                                          res['independent'][src]['detection'][k]), (src, k)
            shape[criterion + '_classifier_source_picks'] = int(
                res['shared']['classifier']['detection']['confusion_matrix'].sum())
        fcache: dict = {}
        fwd = [classifier_forward_ms(np.arange(i0, i0 + B), fcache) for i0 in starts][args.warmup:]
        rec['classifier_forward_ms'] = round(statistics.median(f[0] for f in fwd), 3)
        for criterion in ('inv_iou', 'l2_norm'):
            added = rec[f'{criterion}_shared_ms'] - rec[f'{criterion}_baseline_ms']
            rec[f'{criterion}_shared_adds_ms'] = round(added, 3)
            rec[f'{criterion}_forward_share_of_added'] = (
                round(rec['classifier_forward_ms'] / added, 3) if added > 0 else None)
        rec['shader_clock_mhz'] = [clk0, clock_mhz(dev)]
        runs.append(rec)
        for k, i in (('nodes', 1), ('clusters', 2), ('kept_objects', 3), ('member_rows', 4)):
            shape[k + '_per_batch'] = round(statistics.mean(f[i] for f in fwd), 1)
    print(json.dumps({
        'workload': f'{B} windows x {W} scans, {args.scenes} scenes of ~{args.mean_meas} '
                    f'measurements, eps {eps}, cluster_size_threshold {thr}, '
                    f'min_meas {min_meas}',
        'steps': args.steps, 'warmup': args.warmup, **shape, 'runs': runs}))


if __name__ == '__main__':
    main()
