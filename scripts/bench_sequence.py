"""Windows per second from a sequence to the dynamic frame: the host path against the
sequence store (sequence.py), and the cut's share of an evaluate_sequence step.

Workload: batches of 64 sliding windows x 10 scans x ~134 detections per scan
(sequence_148's mean scene size, 803,760 / 6,011), stride 1, consecutive batches.

  leg (a)  per window the host slices and concatenates its 10 scans
           (SequenceStore.host_window, the slicing of read_data.extract_and_sync_radar_data)
           -> frontend.scan_window_batch -> frontend.dynamic_frame
  leg (b)  SequenceStore.windows -> frontend.dynamic_frame

Both legs run in one process, alternating step by step over the same batches; each step is
a host clock around work that ends in a device synchronise; the median of --steps steps after
--warmup warm-ups is reported.  Then, over the same batches, the whole evaluate_sequence step
(cut -> front-end -> graph build -> proposal forward -> both evaluators) and the cut alone,
for the cut's share of the step.  Prints one JSON line.

Usage:  python scripts/bench_sequence.py [--steps 30] [--warmup 5] [--windows 64]
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

from graph_neural_network_for_radar_perception_amd import (evaluation, frontend,  # noqa: E402
                                                           sequence, synthetic)
from graph_neural_network_for_radar_perception_amd.config import default_config  # noqa: E402
from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training  # noqa: E402


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--window-size', type=int, default=10)
    ap.add_argument('--mean-meas', type=int, default=134)
    ap.add_argument('--scenes', type=int, default=600)
    args = ap.parse_args()
    if args.steps < 20 or args.warmup < 5:
        ap.error('at least 20 steps after 5 warm-ups')
    if not torch.cuda.is_available():
        raise SystemExit('bench_sequence.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W = args.windows, args.window_size
    radar, odo, lists, sensors = synthetic.make_sequence(148, args.scenes, args.mean_meas)
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    n = store.n_windows(W)
    if n < B:
        ap.error(f'{args.scenes} scenes hold {n} windows, fewer than one batch of {B}')
    starts = [(s * B) % (n - B + 1) for s in range(args.warmup + args.steps)]

    def leg_a(i0):
        wins = [store.host_window(i, W) for i in range(i0, i0 + B)]
        return frontend.dynamic_frame(frontend.scan_window_batch(wins, dev))

    def leg_b(i0):
        return frontend.dynamic_frame(store.windows(range(i0, i0 + B), W))

    ta, tb = [], []
    for s, i0 in enumerate(starts):
        da, (dd_a, _) = timed(lambda: leg_a(i0), dev)
        db, (dd_b, _) = timed(lambda: leg_b(i0), dev)
        if s == 0:  # the two legs produce the same dynamic frames
            assert all(torch.equal(dd_a[k], dd_b[k]) for k in dd_a), 'legs disagree'
        if s >= args.warmup:
            ta.append(da)
            tb.append(db)

    # the cut's share of an evaluate_sequence step
    cfg = default_config()
    model = Model_Training(cfg, dev)
    trained = os.path.join(REPO, 'tests', 'golden', 'model_trained_N50.npz')
    if os.path.exists(trained):
        d = np.load(trained)
        model.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files
                               if k.startswith('w/')})
    det = model.to(dev).pred.eval().requires_grad_(False)
    det.set_param_for_proposal_extraction(1.4, False)
    ev_d = evaluation.DetectionEvaluator(int(cfg.num_classes))
    ev_s = evaluation.SegmentationEvaluator(int(cfg.num_classes))
    cache: dict = {}
    t_step, t_cut, nodes = [], [], []
    for s, i0 in enumerate(starts):
        dc, _ = timed(lambda: store.windows(range(i0, i0 + B), W), dev)

        def step():
            win = store.windows(range(i0, i0 + B), W)
            return evaluation.evaluate_window_batch(win, det, cfg, ev_d, ev_s, cache=cache)
        ds, (fb, _) = timed(step, dev)
        if s >= args.warmup:
            t_cut.append(dc)
            t_step.append(ds)
            nodes.append(fb.n_nodes)
    ev_d.result()

    med = statistics.median
    a, b, cut, step_t = med(ta), med(tb), med(t_cut), med(t_step)
    q = lambda v: [round(x * 1e3, 3) for x in np.percentile(v, [25, 75])]  # noqa: E731
    print(json.dumps({
        'workload': f'{B} windows x {W} scans x ~{args.mean_meas} detections',
        'steps': args.steps, 'warmup': args.warmup,
        'measurements_per_batch': int((store.prefix[np.arange(B) + W]
                                       - store.prefix[np.arange(B)]).sum()),
        'host_path_ms': round(a * 1e3, 3), 'host_path_ms_q25_q75': q(ta),
        'store_path_ms': round(b * 1e3, 3), 'store_path_ms_q25_q75': q(tb),
        'host_path_windows_per_s': round(B / a, 1),
        'store_path_windows_per_s': round(B / b, 1),
        'store_over_host': round(a / b, 2),
        'cut_ms': round(cut * 1e3, 3), 'evaluate_step_ms': round(step_t * 1e3, 3),
        'cut_share_of_evaluate_step': round(cut / step_t, 4),
        'evaluate_windows_per_s': round(B / step_t, 1),
        'mean_dynamic_nodes_per_batch': round(float(np.mean(nodes)), 1)}))


if __name__ == '__main__':
    main()
