"""A mixed training batch to the dynamic frame: windows drawn at random from several sequences,
cut on the device by the sequence set (sequence.SequenceSet) against the host path.

Workload: batches of 64 windows x 10 scans x ~134 detections per scan (sequence_148's mean
scene size), every window drawn at random from the windows of 8 synthetic sequences (the
batch a shuffling loader over create_sequences_info_list's metadata hands out).

  path (a)  SequenceSet.windows -> frontend.dynamic_frame
  path (b)  per window the host slices and concatenates its 10 scans (SequenceSet.host_window,
            the slicing of read_data.extract_and_sync_radar_data) -> frontend.scan_window_batch
            -> frontend.dynamic_frame: the only way to a mixed batch without the set, as
            written -- the un-tuned host path, not a tuned competitor

Both paths run in one process, alternating step by step over the same batches; each step is a
host clock around work that ends in a device synchronise; the median of --steps steps after
--warmup warm-ups is reported, with the shader clock the chip held right before and right after
the timed region (rg_clock_probe).  Prints one JSON line.

Usage:  python scripts/bench_dataset_feed.py [--steps 30] [--warmup 5] [--windows 64]
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
from graph_neural_network_for_radar_perception_amd import frontend, sequence, synthetic  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--window-size', type=int, default=10)
    ap.add_argument('--mean-meas', type=int, default=134)
    ap.add_argument('--sequences', type=int, default=8)
    ap.add_argument('--scenes', type=int, default=300)
    args = ap.parse_args()
    if args.steps < 20 or args.warmup < 5:
        ap.error('at least 20 steps after 5 warm-ups')
    if not torch.cuda.is_available():
        raise SystemExit('bench_dataset_feed.py needs a HIP device')
    dev = torch.device('cuda', 0)
    B, W = args.windows, args.window_size
    stores = []
    for s in range(args.sequences):      # sequences of different lengths: every table differs
        radar, odo, lists, sensors = synthetic.make_sequence(148 + s, args.scenes + 7 * s,
                                                             args.mean_meas)
        stores.append(sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev))
    sset = sequence.SequenceSet(stores)
    n = sset.n_windows(W)
    if n < B:
        ap.error(f'{args.sequences} x {args.scenes} scenes hold {n} windows, fewer than {B}')
    rng = np.random.default_rng(0)
    batches = [rng.integers(0, n, B) for _ in range(args.warmup + args.steps)]

    def path_a(g):
        return frontend.dynamic_frame(sset.windows(g, W))

    def path_b(g):
        wins = [sset.host_window(int(i), W) for i in g]
        return frontend.dynamic_frame(frontend.scan_window_batch(wins, dev))

    ta, tb, meas, members = [], [], [], []
    mhz_before = None
    for s, g in enumerate(batches):
        if s == args.warmup:
            mhz_before = clock_mhz(dev)
        da, (dd_a, _) = timed(lambda: path_a(g), dev)
        db, (dd_b, _) = timed(lambda: path_b(g), dev)
        if s == 0:  # the two paths produce the same dynamic frames
            assert all(torch.equal(dd_a[k], dd_b[k]) for k in dd_a), 'paths disagree'
        if s >= args.warmup:
            ta.append(da)
            tb.append(db)
            seq, pos = sset.locate(g, W)
            members.append(len(set(seq.tolist())))
            meas.append(sum(int(stores[a].prefix[p + W] - stores[a].prefix[p])
                            for a, p in zip(seq.tolist(), pos.tolist())))
    mhz_after = clock_mhz(dev)

    med = statistics.median
    a, b = med(ta), med(tb)
    q = lambda v: [round(x * 1e3, 3) for x in np.percentile(v, [25, 75])]  # noqa: E731
    print(json.dumps({
        'workload': f'{B} windows x {W} scans x ~{args.mean_meas} detections, drawn at random '
                    f'from {n} windows of {args.sequences} sequences',
        'steps': args.steps, 'warmup': args.warmup,
        'mean_measurements_per_batch': round(float(np.mean(meas)), 1),
        'mean_sequences_per_batch': round(float(np.mean(members)), 2),
        'set_path_ms': round(a * 1e3, 3), 'set_path_ms_q25_q75': q(ta),
        'host_path_ms': round(b * 1e3, 3), 'host_path_ms_q25_q75': q(tb),
        'set_path_windows_per_s': round(B / a, 1),
        'host_path_windows_per_s': round(B / b, 1),
        'host_over_set': round(b / a, 2),
        'clock_mhz_before': mhz_before, 'clock_mhz_after': mhz_after}))


if __name__ == '__main__':
    main()
