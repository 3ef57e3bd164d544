"""The GATv2 attention layer and the Model_Inference_v2 forward on the M batch: the fused
layer (rg_gat_v2_layer: logits [E][H] the only per-edge buffer) against the composed one
(engine.gat_composed: rg_linear_f32 + rg_segment_reduce + torch elementwise operators, which
materialises the E x H C tensors).

Workload: bench.py's M batch -- 64 frames x 3000 nodes, k-NN with k = 10 -- and the yml widths
(in = Ce = 64, H = 8, C = 64, hidden 512), fp32, seeded weights.
  layer   one GATv2Conv (both node projections, attention, aggregation) on random float32 rows
  model   the seven-layer Model_Inference_v2 forward (engine.forward_batched on the prebuilt
          graph and features), every attention block fused / every block composed

Method: HIP events around each call on the launch stream, the two paths alternating step by
step in one process, medians (and quartiles) of --steps steps after --warmup warm-ups; the
shader clock (rg_clock_probe) before and after; torch.cuda.max_memory_allocated of one step of
each path above what is allocated before it.  The composed path runs at full size (it needs
about 30 GB at the M batch).  Prints one JSON line and appends it to --out.

Usage:  python scripts/bench_attention.py [--steps 10] [--warmup 3] [--frames 64] [--nodes 3000]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from graph_neural_network_for_radar_perception_amd import _native as nat  # noqa: E402
from graph_neural_network_for_radar_perception_amd import engine, synthetic  # noqa: E402
from graph_neural_network_for_radar_perception_amd.config import default_config  # noqa: E402
from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Inference_v2  # noqa: E402
from graph_neural_network_for_radar_perception_amd.graph_features import (  # noqa: E402
    FrameBatch, build_graph_batch)


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


def event_ms(fn, dev) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream(dev)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn, dev) -> int:
    """max_memory_allocated of one call above what was allocated before it."""
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize(dev)
    return int(torch.cuda.max_memory_allocated(dev) - base)


def alternate(paths: dict, dev, steps: int, warmup: int) -> dict:
    ts = {k: [] for k in paths}
    for s in range(warmup + steps):
        for k, fn in paths.items():
            t = event_ms(fn, dev)
            if s >= warmup:
                ts[k].append(t)
    out = {}
    for k, v in ts.items():
        q = np.percentile(v, [25, 75])
        out[k] = {'median_ms': round(statistics.median(v), 3),
                  'q25_q75_ms': [round(float(q[0]), 3), round(float(q[1]), 3)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--nodes', type=int, default=3000)
    ap.add_argument('--model-steps', type=int, default=5)
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'gat_v2_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_attention.py needs a HIP device')
    dev = torch.device('cuda', 0)
    cfg = default_config()
    torch.manual_seed(1234)
    model = Model_Inference_v2(cfg).to(dev).eval().requires_grad_(False)
    frames = synthetic.make_batch(args.frames, args.nodes)
    clusters = [synthetic.cluster_lists(args.nodes) for _ in frames]
    fb = FrameBatch.from_frames(frames, clusters, device=dev)
    gb = build_graph_batch(fb, cfg)
    g = gb.graph
    N, cap = g.n_nodes, g.n_edges_cap
    E = int(gb.n_edges_dev.item())
    rec = {'frames': args.frames, 'nodes_per_frame': args.nodes, 'nodes': N, 'edges': E,
           'edge_capacity': cap, 'k': cfg.k_number_nearest_points,
           'hidden': cfg.hidden_node_channels_GAT, 'heads': cfg.num_heads_GAT,
           'steps': args.steps, 'warmup': args.warmup, 'clock_mhz_before': clock_mhz(dev)}

    # ---- one layer
    gat = model.pass_messages.conv_blk[0].GATblk
    gen = torch.Generator(device='cpu').manual_seed(7)
    x = torch.randn((N, 64), generator=gen).to(dev)
    e = torch.randn((cap, 64), generator=gen).to(dev)
    out_f = torch.empty((N, 512), dtype=torch.float32, device=dev)
    out_c = torch.empty((N, 512), dtype=torch.float32, device=dev)
    ws: dict = {}
    layer = {'fused': lambda: engine.gat_v2_conv(gat, x, e, g, out=out_f, fused=True, ws_cache=ws),
             'composed': lambda: engine.gat_v2_conv(gat, x, e, g, out=out_c, fused=False)}
    rec['layer'] = alternate(layer, dev, args.steps, args.warmup)
    for k, fn in layer.items():
        rec['layer'][k]['peak_bytes'] = peak_bytes(fn, dev)
    d = (out_f - out_c).abs()
    rec['layer']['max_abs_difference'] = float(d.max())
    rec['layer']['max_abs_output'] = float(out_c.abs().max())
    rec['layer']['composed_over_fused'] = round(
        rec['layer']['composed']['median_ms'] / rec['layer']['fused']['median_ms'], 2)
    rec['clock_mhz_after_layer'] = clock_mhz(dev)

    # ---- the seven-layer model
    if not args.skip_model:
        plans = model.plans()
        bufs: dict = {}

        def forward(fused):
            for p in plans.attn:
                p.use_fused = fused
            return engine.forward_batched(plans, gb.node_features, gb.edge_features, g,
                                          fb.cluster_ptr, fb.cluster_idx, fb.n_clusters,
                                          buffers=bufs)
        paths = {'fused': lambda: forward(True), 'composed': lambda: forward(False)}
        rec['model'] = alternate(paths, dev, args.model_steps, 2)
        rec['model']['layers'] = len(plans.attn)
        outs = {k: fn() for k, fn in paths.items()}
        for k, fn in paths.items():
            rec['model'][k]['peak_bytes'] = peak_bytes(fn, dev)
        rec['model']['max_abs_node_logit_difference'] = float(
            (outs['fused'].node_cls - outs['composed'].node_cls).abs().max())
        rec['model']['composed_over_fused'] = round(
            rec['model']['composed']['median_ms'] / rec['model']['fused']['median_ms'], 2)
        rec['clock_mhz_after_model'] = clock_mhz(dev)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
