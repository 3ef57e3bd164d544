"""The classifier's pooling backward on the training bench's workloads: rg_range_max_backward
(float atomics) against rg_range_max_backward_ordered (an argmax launch, then one thread per
channel adding in object order), which ClassifierTrainEngine.backward calls.

Same inputs, one process, the two entries alternating; HIP events around each call, median and
quartiles of --steps calls after --warmup.  x: seeded randn [N][128]; ranges: the reference's
(object_row_ranges); d_pooled: seeded randn.  Appends one JSON line per workload to
profiles/cls_pool_backward_ab.jsonl and prints it.

Usage:  python scripts/bench_pool_backward.py [--steps 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from graph_neural_network_for_radar_perception_amd import _native as nat  # noqa: E402
from graph_neural_network_for_radar_perception_amd import synthetic  # noqa: E402
from graph_neural_network_for_radar_perception_amd.classifier import engine as ce  # noqa: E402

from bench_classifier_fused import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--workloads', default='cls,wide')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'cls_pool_backward_ab.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pool_backward.py needs a HIP device')
    dev = torch.device('cuda', 0)
    lib = nat.lib()
    st = nat.stream_ptr(dev)
    C = 128
    for wl in args.workloads.split(','):
        _, sizes, _, _ = workload(wl, synthetic.SEED0)
        N, n_obj = int(sizes.sum()), len(sizes)
        begin, end = ce.object_row_ranges(torch.from_numpy(sizes).to(dev))   # one sample
        g = torch.Generator().manual_seed(3)
        x = torch.randn(N, C, generator=g).to(dev)
        dp = torch.randn(n_obj, C, generator=g).to(dev)
        ws = torch.empty(lib.rg_range_max_backward_ordered_workspace_size(n_obj, C),
                         dtype=torch.uint8, device=dev)

        def atomic(dx):
            nat.check(lib.rg_range_max_backward(x.data_ptr(), C, C, begin.data_ptr(),
                                                end.data_ptr(), n_obj, dp.data_ptr(), C,
                                                dx.data_ptr(), C, st), 'rg_range_max_backward')

        def ordered(dx):
            nat.check(lib.rg_range_max_backward_ordered(
                x.data_ptr(), C, C, begin.data_ptr(), end.data_ptr(), n_obj, dp.data_ptr(), C,
                dx.data_ptr(), C, ws.data_ptr(), ws.numel(), st), 'rg_range_max_backward_ordered')

        times = {'atomic': [], 'ordered': []}
        outs = {}
        for s in range(args.warmup + args.steps):
            for name, fn in (('atomic', atomic), ('ordered', ordered)):
                dx = torch.zeros(N, C, device=dev)
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record(torch.cuda.current_stream(dev))
                fn(dx)
                e1.record(torch.cuda.current_stream(dev))
                torch.cuda.synchronize(dev)
                outs[name] = dx
                if s >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        q = lambda v: [round(float(t), 4) for t in np.percentile(v, [50, 25, 75])]  # noqa: E731
        line = {'workload': wl, 'objects': n_obj, 'nodes': N, 'steps': args.steps,
                'atomic_ms_median_q25_q75': q(times['atomic']),
                'ordered_ms_median_q25_q75': q(times['ordered']),
                'max_abs_difference': float((outs['atomic'] - outs['ordered']).abs().max()),
                'max_abs_dx': float(outs['ordered'].abs().max())}
        print(json.dumps(line), flush=True)
        with open(args.out, 'a') as fh:
            fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
