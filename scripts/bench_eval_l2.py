"""DetectionEvaluator.update under 'l2_norm' and under 'inv_iou' on one batch, beside the batch's
proposal forward.

Workload: 64 frames x 3000 nodes of the metric configuration M (synthetic.make_batch, trained
weights, k = 10): the detector's proposal forward (objects.detect_frames) gives the predicted
clusters; the ground truth is the generator's clusters as tracks, its background nodes
untracked (one singleton ground-truth cluster each).

  forward      graph build + proposal forward of the batch (objects.detect_frames)
  inv_iou      DetectionEvaluator.update, association by 1 - IoU (rg_eval_associate)
  l2_norm      DetectionEvaluator.update, association by centre distance: two rg_cluster_stats
               and rg_eval_associate_l2
  worst        'l2_norm' with every node a singleton cluster on both sides: 64 frames of
               3000 x 3000 distances, the largest matrix a frame of M can have

Each figure is a host clock around work that ends in a device synchronise: the median of
--steps calls after --warmup warm-ups, for each of two runs of the whole measurement; the shader
clock (rg_clock_probe) is read before and after every run.  Prints one JSON line.

Usage:  python scripts/bench_eval_l2.py [--steps 10] [--warmup 3] [--frames 64] [--nodes 3000]
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
from graph_neural_network_for_radar_perception_amd import evaluation, objects, synthetic  # noqa: E402
from graph_neural_network_for_radar_perception_amd.config import default_config  # noqa: E402
from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training  # noqa: E402
from graph_neural_network_for_radar_perception_amd.graph_features import FrameBatch  # noqa: E402


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


def median_ms(fn, dev, steps, warmup):
    ts = [timed(fn, dev)[0] for _ in range(warmup + steps)][warmup:]
    return round(statistics.median(ts) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--nodes', type=int, default=3000)
    ap.add_argument('--eps', type=float, default=1.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval_l2.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, n = args.frames, args.nodes
    cfg = default_config()
    model = Model_Training(cfg, dev)
    trained = os.path.join(REPO, 'tests', 'golden', 'model_trained_N50.npz')
    if os.path.exists(trained):
        d = np.load(trained)
        model.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files
                               if k.startswith('w/')})
    det = model.to(dev).pred.eval().requires_grad_(False)
    det.set_param_for_proposal_extraction(1.4, False)

    frames = synthetic.make_batch(B, n)
    fb = FrameBatch.from_frames(frames, None, device=dev)
    N = fb.n_nodes
    # tracks: the generator's clusters (the first round(0.7 n / 12) ids), background untracked
    n_tracks = max(1, int(round(round(0.7 * n) / 12.0)))
    key = np.concatenate([np.where(f['cluster_id'] < n_tracks, f['cluster_id'] + 1, 0)
                          for f in frames]).astype(np.int32)
    rng = np.random.default_rng(7)
    track_key = torch.from_numpy(key).to(dev)
    gt_class = torch.from_numpy(rng.integers(0, 5, N)).to(dev)
    cache: dict = {}
    forward = lambda: objects.detect_frames(det, fb, cfg, 'fp32', cache)  # noqa: E731
    d0 = forward()
    out = d0.outputs
    xy = d0.xy
    ones = torch.arange(N + 1, dtype=torch.int32, device=dev)
    zero_key = torch.zeros(N, dtype=torch.int32, device=dev)

    def evaluator(criterion):
        return evaluation.DetectionEvaluator(int(cfg.num_classes), args.eps,
                                             association_criteria=criterion)

    def update(ev, worst=False):
        if worst:
            return ev.update(out.node_cls, out.obj_cls, ones, ones[:N], gt_class, zero_key,
                             fb.frame_ptr, max_frame_nodes=n, xy=xy)
        return ev.update(out.node_cls, out.obj_cls, out.cluster_ptr, out.cluster_idx, gt_class,
                         track_key, fb.frame_ptr, max_frame_nodes=n, xy=xy)

    runs = []
    for _ in range(2):
        clk0 = clock_mhz(dev)
        ev_i, ev_l, ev_w = evaluator('inv_iou'), evaluator('l2_norm'), evaluator('l2_norm')
        rec = {'forward_ms': median_ms(forward, dev, args.steps, args.warmup),
               'inv_iou_update_ms': median_ms(lambda: update(ev_i), dev, args.steps, args.warmup),
               'l2_norm_update_ms': median_ms(lambda: update(ev_l), dev, args.steps, args.warmup),
               'l2_norm_worst_update_ms': median_ms(lambda: update(ev_w, True), dev, args.steps,
                                                    args.warmup)}
        # the association alone, on the centres the update computed
        last = ev_l.last
        p_ptr = evaluation._full_ptr(out.cluster_ptr, N)
        p_idx = out.cluster_idx.to(torch.int32).contiguous()
        ws: dict = {}
        rec['l2_norm_associate_ms'] = median_ms(
            lambda: evaluation.associate_l2(fb.frame_ptr, last['gt']['cluster_ptr'],
                                            last['gt']['cluster_idx'], p_ptr, p_idx,
                                            last['gt_mu'], last['pred_mu'], args.eps, 0, n, ws),
            dev, args.steps, args.warmup)
        rec['shader_clock_mhz'] = [clk0, clock_mhz(dev)]
        runs.append(rec)
        for ev in (ev_i, ev_l, ev_w):
            ev.result()
    kept = ev_l.last['assoc']
    per_frame = lambda t: round(float(t.sum().item()) / B, 1)  # noqa: E731
    print(json.dumps({
        'workload': f'{B} frames x {n} nodes, metric configuration M, eps {args.eps}',
        'steps': args.steps, 'warmup': args.warmup,
        'gt_clusters_per_frame': per_frame(kept['gt_kept']),
        'pred_clusters_per_frame': per_frame(kept['pred_kept']),
        'picks_per_frame': per_frame(kept['pick_count']),
        'runs': runs}))


if __name__ == '__main__':
    main()
