"""Milliseconds per outer iteration of gradient accumulation from a sequence in HBM: the
trainer's accumulate_frames / apply_accumulated against the loop a caller had to write before
them, with four plain steps for scale.

Workload: one outer iteration = K = 4 micro-batches of 16 sliding windows x 10 scans x ~134
detections per scan on the synthetic sequence of scripts/bench_sequence.py, consecutive
batches, the yml model, no flip.  Every path runs the same feed per micro-batch
(SequenceStore.windows -> frontend.dynamic_frame -> frame_batch) inside its timed region.

  path (a)  RadarGNNTrainer.accumulate_frames x K, then apply_accumulated (one fused optimizer
            launch with the NaN skip and MultiStepLR on the device, one re-pack)
  path (b)  the loop without them: per micro-batch build_graph_batch, training_labels, the
            three host sizes, training.train_step_losses and (total_loss / K).backward() --
            autograd accumulates p.grad -- then torch.optim.SGD.step() and zero_grad
  path (c)  for scale: K plain RadarGNNTrainer.step_frames calls (K optimizer steps, K re-packs)

The three run in one process on three models of the same seed, alternating iteration by
iteration over the same batches; each iteration is a host clock around work that ends in a
device synchronise; the median of --steps iterations after --warmup warm-ups is reported, with
the shader clock the chip held right before and right after the timed region
(rg_clock_probe).  The accumulator's own cost per micro-batch -- the scaled losses written
into the slots and the engine's bucket added to the accumulator's, one elementwise pass --
is timed alone between HIP events.  Prints one JSON line.

Usage:  python scripts/bench_accumulate_feed.py [--steps 30] [--warmup 5]
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
from graph_neural_network_for_radar_perception_amd import (frontend, sequence,  # noqa: E402
                                                           synthetic, training)
from graph_neural_network_for_radar_perception_amd.config import default_config  # noqa: E402
from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training  # noqa: E402
from graph_neural_network_for_radar_perception_amd.graph_features import \
    build_graph_batch  # noqa: E402


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


def feed(store, pos, W):
    dd, gd = frontend.dynamic_frame(store.windows(pos, W), with_keys=True, numpy_mean=True)
    return frontend.frame_batch(dd, gd)


def accumulated(store, trainer, group, W):
    """Path (a)."""
    for pos in group:
        trainer.accumulate_frames(feed(store, pos, W), len(group))
    return trainer.apply_accumulated()


def autograd_loop(store, model, opt, cfg, group, W, ws):
    """Path (b)."""
    eng = model.train_engine()
    K = len(group)
    for pos in group:
        fb = feed(store, pos, W)
        gb = build_graph_batch(fb, cfg, ws_cache=ws)
        g = gb.graph
        lab = training.training_labels(fb, gb, cfg, ws)
        sizes = torch.cat((gb.n_edges_dev.reshape(1), g.n_pairs_dev.reshape(1),
                           lab['n_clusters_dev'].reshape(1))).tolist()
        g.n_edges, g.n_pairs, ncl = (int(v) for v in sizes)
        losses = training.train_step_losses(
            eng, (gb.node_features, gb.edge_features, g, lab['cluster_ptr'], lab['cluster_idx'],
                  ncl, lab))
        (training.total_loss(losses) / K).backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    return losses.detach()


def plain_steps(store, trainer, group, W):
    """Path (c)."""
    for pos in group:
        out = trainer.step_frames(feed(store, pos, W))
    return out


def bucket_add_us(trainer, dev, reps: int = 200) -> float:
    """GradAccumulator.add's own work on the trainer's buckets, per call."""
    acc, eng = trainer.accum, trainer.engine
    acc.open(4)
    losses = torch.ones(training.N_LOSS_SLOTS, dtype=torch.float32, device=dev)
    eng.flat_grad.zero_()
    for _ in range(10):
        acc.add(eng, losses)
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        acc.add(eng, losses)
    e1.record()
    torch.cuda.synchronize(dev)
    acc.n_accum, acc.count = None, 0      # nothing of this is applied
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=16)
    ap.add_argument('--accumulate', type=int, default=4)
    ap.add_argument('--window-size', type=int, default=10)
    ap.add_argument('--mean-meas', type=int, default=134)
    ap.add_argument('--scenes', type=int, default=600)
    args = ap.parse_args()
    if args.steps < 20 or args.warmup < 5:
        ap.error('at least 20 iterations after 5 warm-ups')
    if not torch.cuda.is_available():
        raise SystemExit('bench_accumulate_feed.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W, K = args.windows, args.window_size, args.accumulate
    radar, odo, lists, sensors = synthetic.make_sequence(148, args.scenes, args.mean_meas)
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    n = store.n_windows(W)
    if n < B * K:
        ap.error(f'{args.scenes} scenes hold {n} windows, fewer than one iteration of {B * K}')
    cfg = default_config()
    models = []
    for _ in range(3):
        torch.manual_seed(148)
        models.append(Model_Training(cfg, 'cpu').to(dev).train())
    tr_a = training.RadarGNNTrainer(models[0], cfg, world=1)
    opt_b = torch.optim.SGD(models[1].parameters(), lr=cfg.learning_rate, momentum=0.9,
                            weight_decay=cfg.weight_decay)
    tr_c = training.RadarGNNTrainer(models[2], cfg, world=1)
    ws: dict = {}

    ta, tb, tc = [], [], []
    mhz_before = None
    for s in range(args.warmup + args.steps):
        i0 = (s * B * K) % (n - B * K + 1)
        group = [np.arange(i0 + j * B, i0 + (j + 1) * B) for j in range(K)]
        if s == args.warmup:
            mhz_before = clock_mhz(dev)
        da, n_a = timed(lambda: accumulated(store, tr_a, group, W), dev)
        db, loss_b = timed(lambda: autograd_loop(store, models[1], opt_b, cfg, group, W, ws), dev)
        dc, out_c = timed(lambda: plain_steps(store, tr_c, group, W), dev)
        assert n_a == K and bool(torch.isfinite(loss_b).all()) and out_c is not None
        if s >= args.warmup:
            ta.append(da)
            tb.append(db)
            tc.append(dc)
    mhz_after = clock_mhz(dev)
    add_us = bucket_add_us(tr_a, dev)
    assert tr_a.opt.applied_steps() == args.warmup + args.steps

    med = statistics.median
    a, b, c = med(ta), med(tb), med(tc)
    q = lambda v: [round(x * 1e3, 3) for x in np.percentile(v, [25, 75])]  # noqa: E731
    print(json.dumps({
        'workload': f'{K} micro-batches x {B} windows x {W} scans x ~{args.mean_meas} '
                    'detections, yml model',
        'steps': args.steps, 'warmup': args.warmup,
        'accumulate_apply_ms': round(a * 1e3, 3), 'accumulate_apply_ms_q25_q75': q(ta),
        'autograd_loop_ms': round(b * 1e3, 3), 'autograd_loop_ms_q25_q75': q(tb),
        'plain_steps_ms': round(c * 1e3, 3), 'plain_steps_ms_q25_q75': q(tc),
        'autograd_loop_over_accumulate': round(b / a, 3),
        'bucket_add_us_per_micro_batch': round(add_us, 2),
        'bucket_bytes': int(tr_a.accum.bucket.numel()) * 4,
        'clock_mhz_before': mhz_before, 'clock_mhz_after': mhz_after}))


if __name__ == '__main__':
    main()
