"""Native executor of the cluster-level classifier GNN.

Same kernels as the detector (``rg_mlp_chain`` for every MLP, ``rg_segment_reduce``
for the PyG aggregation), plus the classifier's own graph build and pooling
(``classifier.hip``): the block-diagonal complete graph of ``compute_edge_index``
(``datagen_classifier.py:124-133``), the reference's pooling ranges
(``classifier.py:60-68``) and their channel max (``rg_segment_reduce_ranges``), and
the focal loss (``classifier/loss.py``).  A batch of samples is one disjoint-union
graph; the pooled objects of all samples are classified by ONE stem + head chain.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from .. import _native as nat
from ..engine import (ChainPlan, ConvPlan, DeviceGraph, LayerSpec, PackedImages, _require_device,
                      cached_plan, segment_reduce, specs_from_modules)

def _dt(dtype: str):
    return torch.bfloat16 if dtype == 'bf16' else torch.float32


def _conv_plan(blk, dtype, dev) -> ConvPlan:
    return cached_plan(blk, ('conv', dtype), lambda: ConvPlan(blk, dtype, dev))


def _chain_plan(mods, dtype, dev) -> ChainPlan:
    return cached_plan(mods[0], (tuple(id(m) for m in mods), dtype),
                       lambda: ChainPlan(specs_from_modules(mods), dtype, dev))


# --------------------------------------------------------------------------- graph build
def object_complete_graph(object_size: torch.Tensor, n_nodes: int, n_edges: int,
                          want_edge_index: bool = True):
    """Device CSR (row_ptr int32 [N+1], col int32 [E]) and, optionally, the reference
    edge_index int64 [2, E] of compute_edge_index for object sizes int64 [n_obj]."""
    _require_device(object_size, 'object_size')
    lib = nat.lib()
    dev = object_size.device
    osz = object_size.to(torch.int64).contiguous()
    n_obj = int(osz.numel())
    row_ptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(n_edges, 1), dtype=torch.int32, device=dev)
    ei = torch.empty((2, n_edges), dtype=torch.int64, device=dev) if want_edge_index else None
    ws = torch.empty(lib.rg_object_graph_workspace_size(n_obj), dtype=torch.uint8, device=dev)
    nat.check(lib.rg_object_complete_graph(osz.data_ptr(), n_obj, n_nodes, n_edges,
                                           row_ptr.data_ptr(), col.data_ptr(), nat.ptr(ei),
                                           ws.data_ptr(), ws.numel(), nat.stream_ptr(dev)),
              'rg_object_complete_graph')
    return row_ptr, col, ei


def compute_edge_index(object_num_meas_list: Sequence[int], device='cuda') -> np.ndarray:
    """Drop-in for ``datagen_classifier.compute_edge_index`` (numpy int64 [2, E] in
    np.nonzero order), built on the GPU."""
    sizes = [int(n) for n in object_num_meas_list]
    N = sum(sizes)
    E = sum(n * (n - 1) for n in sizes)
    osz = torch.tensor(sizes, dtype=torch.int64, device=device)
    _, _, ei = object_complete_graph(osz, N, E)
    return ei.cpu().numpy()


def object_graph(object_size: torch.Tensor, n_nodes: int, n_edges: int) -> DeviceGraph:
    """The batch's classifier graph straight from the object sizes (no edge list):
    the complete-graph CSR is symmetric, so it is its own destination-major view."""
    lib = nat.lib()
    dev = object_size.device
    row_ptr, col, _ = object_complete_graph(object_size, n_nodes, n_edges, want_edge_index=False)
    dst = torch.empty(max(n_edges, 1), dtype=torch.int32, device=dev)
    nat.check(lib.rg_csr_rows(row_ptr.data_ptr(), n_nodes, dst.data_ptr(), nat.stream_ptr(dev)),
              'rg_csr_rows')
    return DeviceGraph(n_nodes, n_edges, row_ptr, dst, col, None, None, None, None,
                       n_edges=n_edges)


def object_row_ranges(object_size: torch.Tensor, sample_obj_ptr=None, sample_node_base=None,
                      n_samples: int = 1):
    """The reference's pooling ranges (startidx / endidx, classifier.py:60-62) of every
    object of a batch of samples: int32 (begin, end) [n_obj]."""
    lib = nat.lib()
    dev = object_size.device
    osz = object_size.to(torch.int64).contiguous()
    n_obj = int(osz.numel())
    begin = torch.empty(max(n_obj, 1), dtype=torch.int32, device=dev)
    end = torch.empty(max(n_obj, 1), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.rg_object_graph_workspace_size(n_obj), dtype=torch.uint8, device=dev)
    nat.check(lib.rg_object_row_ranges(osz.data_ptr(), n_obj, nat.ptr(sample_obj_ptr),
                                       nat.ptr(sample_node_base), int(n_samples),
                                       begin.data_ptr(), end.data_ptr(), ws.data_ptr(), ws.numel(),
                                       nat.stream_ptr(dev)), 'rg_object_row_ranges')
    return begin[:n_obj], end[:n_obj]


# --------------------------------------------------------------------------- fused layer
def object_table(object_size: torch.Tensor, n_nodes: int, n_edges: int) -> torch.Tensor:
    """The per-batch table of rg_cls_conv_layer_x3 (rg_cls_object_table): seg_ptr, every node's
    object begin and size, and the edge launch's wave table -- O(n_nodes + n_obj) int32, built
    from object sizes int64 [n_obj] on the device; shared by the batch's layers."""
    _require_device(object_size, 'object_size')
    lib = nat.lib()
    dev = object_size.device
    osz = object_size.to(torch.int64).contiguous()
    n_obj = int(osz.numel())
    table = torch.empty(lib.rg_cls_object_table_bytes(n_nodes, n_obj) // 4, dtype=torch.int32,
                        device=dev)
    ws = torch.empty(lib.rg_cls_object_table_workspace_size(n_obj), dtype=torch.uint8, device=dev)
    nat.check(lib.rg_cls_object_table(osz.data_ptr(), n_obj, int(n_nodes), int(n_edges),
                                      table.data_ptr(), ws.data_ptr(), ws.numel(),
                                      nat.stream_ptr(dev)), 'rg_cls_object_table')
    return table


class ClsFusedPlan:
    """The image set of one conv block for rg_cls_conv_layer_x3 (fp32, the exact three-term
    bf16 scheme): [0] the per-node projection [W_0's x_i columns; its x_j columns] (+ [b_0; 0]),
    [1] msg1, [2] upd.  The specs are derived from the block's msg and upd parameters, which the
    set's validity follows (PackedImages: refresh() / invalidate()).  fused is None for a block
    the kernel is not compiled for; fused_ok records the kernel's own answer.

    Training (rg_cls_conv_aggregate_x3 / rg_cls_conv_backward_x3) adds two images that follow
    the same parameters: W_1^T in the b3 chain format -- the packer transposes float32 formats
    only, so it is a derived spec of a second set (bwd_images) -- and W_pq^T in float32 for
    dx += [dP | dQ] W_pq, the transposed column block (0, 0, C) of the projection."""

    C = 128
    FMTS = (nat.RG_PACK_FAST_IN | nat.RG_PACK_X3, nat.RG_PACK_FAST_CHAIN | nat.RG_PACK_X3,
            nat.RG_PACK_FAST_IN | nat.RG_PACK_X3)
    BWD_FMTS = (nat.RG_PACK_FAST_CHAIN | nat.RG_PACK_X3, nat.RG_PACK_FAST_CHAIN | nat.RG_PACK_X3)

    def __init__(self, blk, device):
        self.aggr = blk.aggr
        self.device = torch.device(device)
        self.msg_specs = specs_from_modules(list(blk.msg))
        self.upd_specs = specs_from_modules(list(blk.upd))
        self.has_res = blk.residual_connection is not None
        self.fused_ok = None
        self.fused = None
        self.images = None
        self.bwd_images = None
        self._ws = {}
        self._dx_fast = True
        self._pack()

    def _specs(self):
        if self.has_res or self.aggr not in nat.REDUCE:
            return None
        if len(self.msg_specs) != 2 or len(self.upd_specs) != 1:
            return None
        m0, m1 = self.msg_specs
        u = self.upd_specs[0]
        C = self.C
        # compiled for the yml block only: C = 128, hidden 128, no norm, LeakyReLU
        if not (tuple(m0.weight.shape) == (C, 2 * C) and tuple(m1.weight.shape) == (C, C)
                and tuple(u.weight.shape) == (C, 2 * C)):
            return None
        if any(sp.mu is not None or sp.act != 'leakyrelu' for sp in (m0, m1, u)):
            return None
        W = m0.weight.detach().to(torch.float32)
        b = (m0.bias.detach().to(torch.float32) if m0.bias is not None
             else torch.zeros(C, dtype=torch.float32, device=W.device))
        # cat(x_i, x_j): columns [:C] meet the destination's row (P, with b_0), [C:] the source's
        pq = LayerSpec(torch.cat((W[:, :C], W[:, C:]), 0).contiguous(),
                       torch.cat((b, torch.zeros_like(b)), 0).contiguous(), None, None, m0.act)
        return [pq, m1, u]

    def _pack(self):
        self.fused = None
        specs = self._specs()
        if specs is None:
            return
        if self.images is None:
            self.images = PackedImages(specs, self.device, self.msg_specs + self.upd_specs)
        self.images.specs = specs
        self.images.get(self.FMTS)
        if self.bwd_images is not None:
            self.bwd_images.specs = self._bwd_specs()
        self.fused = True

    def _bwd_specs(self):
        """[msg1, a bare Linear of W_1^T] of rg_cls_conv_backward_x3."""
        m1 = self.msg_specs[1]
        wt = m1.weight.detach().to(torch.float32).t().contiguous()
        return [m1, LayerSpec(wt, None, None, None, 'none')]

    def refresh(self):
        if not self.fused:
            return
        stale = self.images.refresh()
        if self.bwd_images is not None and self.bwd_images.refresh():
            stale = True
        if stale:
            self._pack()

    def invalidate(self):
        for im in (self.images, self.bwd_images):
            if im is not None:
                im.invalidate()

    def ready(self, x) -> bool:
        return bool(self.fused) and self.fused_ok is not False and x.dtype == torch.float32

    def run(self, x, table, n_obj: int, x_out) -> bool:
        """One rg_cls_conv_layer_x3 call; False when the kernel refuses the layer (the caller
        then runs the unfused chains)."""
        lib = nat.lib()
        st = nat.stream_ptr(x.device)
        n = int(x.shape[0])
        ws = self._workspace(lib.rg_cls_conv_layer_x3_workspace_size(n, n_obj), st)
        rc = lib.rg_cls_conv_layer_x3(self.images.get(self.FMTS)[0][0], nat.REDUCE[self.aggr],
                                      x.data_ptr(), x.stride(0), table.data_ptr(), n, n_obj,
                                      x_out.data_ptr(), x_out.stride(0), ws.data_ptr(), ws.numel(),
                                      st)
        if rc == nat.RG_ERR_UNSUPPORTED:
            self.fused_ok = False
            return False
        nat.check(rc, 'rg_cls_conv_layer_x3')
        self.fused_ok = True
        return True


    # ------------------------------------------------------------------ training
    def _workspace(self, need: int, st) -> torch.Tensor:
        ws = self._ws.get(st)
        if ws is None or ws.numel() < need:
            ws = self._ws[st] = torch.empty(max(int(need), 1), dtype=torch.uint8, device=self.device)
        return ws

    def aggregate(self, x, table, pq, agg, workspaces=None) -> bool:
        """The layer's projection and edge launches with their results kept
        (rg_cls_conv_aggregate_x3): pq [N, 256] = P | Q, agg [N, 128] as the update MLP reads
        it.  False when the kernel refuses the layer.  workspaces: the caller's scratch owner
        (training.Workspaces: one buffer for all blocks); None: the plan's own."""
        lib = nat.lib()
        st = nat.stream_ptr(x.device)
        n = int(x.shape[0])
        need = lib.rg_cls_conv_aggregate_x3_workspace_size(n)
        ws = workspaces.get('cls_agg', need) if workspaces is not None else self._workspace(need, st)
        rc = lib.rg_cls_conv_aggregate_x3(self.images.get(self.FMTS)[0][0], nat.REDUCE[self.aggr],
                                          x.data_ptr(), x.stride(0), table.data_ptr(), n,
                                          pq.data_ptr(), agg.data_ptr(), ws.data_ptr(), ws.numel(),
                                          st)
        if rc == nat.RG_ERR_UNSUPPORTED:
            self.fused_ok = False
            return False
        nat.check(rc, 'rg_cls_conv_aggregate_x3')
        self.fused_ok = True
        return True

    def backward_edges(self, pq, d_agg, table, n_edges: int, max_degree: int, d_pq, d_w1, d_b1,
                       workspaces=None):
        """rg_cls_conv_backward_x3: d_pq [N, 256] = dP | dQ written, d_w1 / d_b1 accumulated;
        d_agg a [N, 128] view (row stride a multiple of 4).  workspaces as aggregate()'s: the
        dm / h tapes and rg_linear_grad's partials are about 160 MiB, shared by the blocks."""
        lib = nat.lib()
        st = nat.stream_ptr(pq.device)
        n = int(pq.shape[0])
        if self.bwd_images is None:
            self.bwd_images = PackedImages(self._bwd_specs(), self.device,
                                           self.msg_specs + self.upd_specs)
        layers = self.bwd_images.get(self.BWD_FMTS)[0][0]
        need = lib.rg_cls_conv_backward_x3_workspace_size(n, int(max_degree))
        ws = workspaces.get('cls_bwd', need) if workspaces is not None else self._workspace(need, st)
        nat.check(lib.rg_cls_conv_backward_x3(
            layers, nat.REDUCE[self.aggr], pq.data_ptr(), d_agg.data_ptr(), d_agg.stride(0),
            table.data_ptr(), n, int(n_edges), int(max_degree), d_pq.data_ptr(), d_w1.data_ptr(),
            d_b1.data_ptr(), ws.data_ptr(), ws.numel(), st), 'rg_cls_conv_backward_x3')

    def dx_pq(self, d_pq, out):
        """out += d_pq W_pq ([N, 256] x [256, 128]): the float32 chain kernels on the transposed
        projection, as TrainChain's dX = dZ W."""
        lib = nat.lib()
        st = nat.stream_ptr(d_pq.device)
        rows = int(d_pq.shape[0])
        block = (0, 0, self.C)
        if self._dx_fast:
            fast = self.images.get((nat.RG_PACK_F32_FAST,), True, block)[0][0]
            rc = lib.rg_mlp_chain_f32_ex(fast, 1, rows, None, nat.IN_DENSE, d_pq.data_ptr(),
                                         d_pq.stride(0), d_pq.shape[1], None, 0, 0, None, 0, 0,
                                         None, None, out.data_ptr(), out.stride(0),
                                         out.data_ptr(), out.stride(0), st)
            if rc == 0:
                return
            if rc != nat.RG_ERR_UNSUPPORTED:
                nat.check(rc, 'rg_mlp_chain_f32_ex (dx = [dP | dQ] W_pq)')
            self._dx_fast = False
        gen = self.images.get((nat.RG_F32,), True, block)[0][0]
        nat.check(lib.rg_mlp_chain(
            nat.RG_F32, gen, 1, rows, None, nat.IN_DENSE, nat.RG_F32, d_pq.data_ptr(),
            d_pq.stride(0), d_pq.shape[1], None, 0, 0, None, 0, 0, None, None, out.data_ptr(),
            out.stride(0), nat.RG_F32, out.data_ptr(), out.stride(0), nat.RG_F32, st),
            'rg_mlp_chain (dx = [dP | dQ] W_pq)')


def fused_plan(blk, dev) -> ClsFusedPlan:
    """The block's fused-layer plan (fp32)."""
    return cached_plan(blk, ('cls_fused', 'fp32'), lambda: ClsFusedPlan(blk, dev))


# --------------------------------------------------------------------------- forward
def _mark(events, name, dev):
    """HIP event on the launch stream (bench.py per-kernel timing)."""
    if events is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(dev))
        events.append((name, ev))


def run_conv_block_nodes(blk, x: torch.Tensor, edge_index: torch.Tensor, dtype: str = 'fp32',
                         g: DeviceGraph = None, events=None) -> torch.Tensor:
    """classifier residual_graph_conv_block.forward (classifier/blocks.py:70-85):
    msg = MLP(cat(x[ei[1]], x[ei[0]])), agg = aggregate at ei[1], x' = identity +
    upd(cat(x, agg)).  Chain kernel in GATHER3 mode with no edge part (w2 = 0)."""
    _require_device(x, 'node_features')
    dev = x.device
    cp = _conv_plan(blk, dtype, dev)
    N = x.shape[0]
    if g is None:
        g = DeviceGraph.from_edge_index(edge_index, N, count_pairs=False)
    E = g.n_edges
    tdt = _dt(dtype)
    x = x.to(tdt).contiguous()
    msg = torch.empty((max(E, 1), cp.c_msg), dtype=tdt, device=dev)
    if E > 0:
        _mark(events, 'message_chain:start', dev)
        cp.msg(E, msg, x, x.shape[1], mode=nat.IN_GATHER3, idx0=g.dst, idx1=g.src)
        _mark(events, 'message_chain:end', dev)
    agg = torch.empty((N, cp.c_msg), dtype=tdt, device=dev)
    if E > 0:
        _mark(events, 'segment_reduce:start', dev)
        segment_reduce(msg, g.seg_ptr, N, cp.aggr, agg)
        _mark(events, 'segment_reduce:end', dev)
    else:
        agg.zero_()
    if cp.res is not None:
        ident = torch.empty((N, cp.c_out), dtype=tdt, device=dev)
        cp.res(N, ident, x, x.shape[1])
    else:
        ident = x
    out = torch.empty((N, cp.c_out), dtype=tdt, device=dev)
    _mark(events, 'update_chain:start', dev)
    cp.upd(N, out, x, x.shape[1], mode=nat.IN_CONCAT2, in1=agg, w1=cp.c_msg, residual=ident)
    _mark(events, 'update_chain:end', dev)
    return out


def pool_and_classify(pred, x: torch.Tensor, begin: torch.Tensor, end: torch.Tensor,
                      dtype: str = 'fp32') -> torch.Tensor:
    """object_class_prediction.forward (classifier/blocks.py:171-176) for every object
    at once: channel max over rows [begin, end) (rg_segment_reduce_ranges), then the
    stem + head chain on the pooled rows.  Returns float32 [n_obj, num_classes]."""
    lib = nat.lib()
    dev = x.device
    n_obj = int(begin.numel())
    C = x.shape[1]
    tdt = _dt(dtype)
    pooled = torch.empty((max(n_obj, 1), C), dtype=tdt, device=dev)
    if n_obj > 0:
        sdt = nat.RG_BF16 if x.dtype == torch.bfloat16 else nat.RG_F32
        N = x.shape[0]
        ws = torch.empty(lib.rg_segment_reduce_ranges_workspace_size(N, C, sdt),
                         dtype=torch.uint8, device=dev)
        nat.check(lib.rg_segment_reduce_ranges(
            x.data_ptr(), sdt, x.stride(0), N, begin.data_ptr(), end.data_ptr(), n_obj, C,
            nat.REDUCE['max'], pooled.data_ptr(),
            nat.RG_BF16 if tdt == torch.bfloat16 else nat.RG_F32, pooled.stride(0),
            ws.data_ptr(), ws.numel(), nat.stream_ptr(dev)), 'rg_segment_reduce_ranges')
    head = _chain_plan(pred.chain(), dtype, dev)
    out = torch.empty((n_obj, head.out_dim), dtype=torch.float32, device=dev)
    if n_obj > 0:
        head(n_obj, out, pooled, C)
    return out


def forward_graph(model, node_features: torch.Tensor, g: DeviceGraph, begin: torch.Tensor,
                  end: torch.Tensor, dtype: str = 'fp32', events=None) -> torch.Tensor:
    """Encoder -> L conv blocks over g -> per-object max-pool over [begin, end) ->
    stem + head: logits float32 [n_obj, num_classes] (classifier.py:50-72)."""
    dev = node_features.device
    N = g.n_nodes
    enc = _chain_plan(list(model.encode_node_feat.encoder), dtype, dev)
    x = torch.empty((N, enc.out_dim), dtype=_dt(dtype), device=dev)
    xin = node_features.to(torch.float32).contiguous()
    _mark(events, 'node_encoder:start', dev)
    enc(N, x, xin, xin.shape[1])
    _mark(events, 'node_encoder:end', dev)
    for blk in model.pass_messages.conv_blk:
        x = run_conv_block_nodes(blk, x, None, dtype, g, events)
    _mark(events, 'pool_head:start', dev)
    out = pool_and_classify(model.predict_node, x, begin, end, dtype)
    _mark(events, 'pool_head:end', dev)
    return out


def forward_objects(model, node_features: torch.Tensor, object_size: torch.Tensor,
                    begin: torch.Tensor, end: torch.Tensor, dtype: str = 'fp32', n_nodes=None,
                    n_edges=None, events=None) -> torch.Tensor:
    """forward_graph straight from the object sizes int64 [n_obj] (the batch's graph is the
    union of complete graphs over consecutive rows): every conv block the fused kernel takes
    (fp32, the yml widths, no residual projection) runs rg_cls_conv_layer_x3 over the table of
    rg_cls_object_table, built once per call -- no edge list, no message buffer.  Any other block
    runs run_conv_block_nodes over object_graph's CSR, built lazily and once.  n_nodes / n_edges:
    host integers (sum n, sum n (n - 1)); read back from object_size when not given."""
    _require_device(node_features, 'node_features')
    dev = node_features.device
    osz = object_size.to(dev).to(torch.int64).contiguous()
    n_obj = int(osz.numel())
    if n_nodes is None or n_edges is None:
        hs = osz.cpu().numpy()
        n_nodes, n_edges = int(hs.sum()), int((hs * (hs - 1)).sum())
    N = int(n_nodes)
    enc = _chain_plan(list(model.encode_node_feat.encoder), dtype, dev)
    x = torch.empty((N, enc.out_dim), dtype=_dt(dtype), device=dev)
    xin = node_features.to(torch.float32).contiguous()
    _mark(events, 'node_encoder:start', dev)
    enc(N, x, xin, xin.shape[1])
    _mark(events, 'node_encoder:end', dev)
    table = g = None
    for blk in model.pass_messages.conv_blk:
        fp = fused_plan(blk, dev) if dtype == 'fp32' and N > 0 else None
        if fp is not None and fp.ready(x):
            if table is None:
                _mark(events, 'object_table:start', dev)
                table = object_table(osz, N, int(n_edges))
                _mark(events, 'object_table:end', dev)
            out = torch.empty((N, fp.C), dtype=torch.float32, device=dev)
            _mark(events, 'cls_conv_layer:start', dev)
            ok = fp.run(x, table, n_obj, out)
            _mark(events, 'cls_conv_layer:end', dev)
            if ok:
                x = out
                continue
        if g is None:
            g = object_graph(osz, N, int(n_edges))
        x = run_conv_block_nodes(blk, x, None, dtype, g, events)
    _mark(events, 'pool_head:start', dev)
    out = pool_and_classify(model.predict_node, x, begin, end, dtype)
    _mark(events, 'pool_head:end', dev)
    return out


def forward_samples(model, node_features: List[torch.Tensor], edge_index: List[torch.Tensor],
                    object_size: List[torch.Tensor], dtype: str = 'fp32') -> torch.Tensor:
    """Model_Inference.forward (classifier.py:50-72) over a list of samples batched as
    one disjoint-union graph; logits of all objects, sample after sample."""
    dev = node_features[0].device
    for t in node_features:
        _require_device(t, 'node_features')
    sizes = [int(t.shape[0]) for t in node_features]
    bases = np.cumsum([0] + sizes)
    if len(node_features) == 1:
        nf, ei = node_features[0], edge_index[0].to(torch.int64)
        osz = object_size[0].to(dev)
        sobj = nbase = None
    else:
        nf = torch.cat(node_features, 0)
        ei = torch.cat([e.to(torch.int64) + int(b) for e, b in zip(edge_index, bases[:-1])], 1)
        osz = torch.cat([o.to(dev).to(torch.int64) for o in object_size], 0)
        nobj = np.cumsum([0] + [int(o.numel()) for o in object_size])
        sobj = torch.tensor(nobj, dtype=torch.int32).to(dev)
        nbase = torch.tensor(bases[:-1], dtype=torch.int32).to(dev)
    N = int(bases[-1])
    g = DeviceGraph.from_edge_index(ei.contiguous(), N, count_pairs=False)
    begin, end = object_row_ranges(osz, sobj, nbase, len(node_features))
    return forward_graph(model, nf, g, begin, end, dtype)


def focal_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """classifier Loss.forward (classifier/loss.py:10-14) -> float32 scalar tensor."""
    lib = nat.lib()
    dev = logits.device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    lab = labels.to(torch.int64).contiguous()
    lg = logits.to(torch.float32).contiguous()
    nat.check(lib.rg_object_focal_loss(lg.data_ptr(), lg.stride(0), lab.data_ptr(),
                                       int(lg.shape[0]), int(lg.shape[1]), out.data_ptr(),
                                       nat.stream_ptr(dev)), 'rg_object_focal_loss')
    return out[0]
