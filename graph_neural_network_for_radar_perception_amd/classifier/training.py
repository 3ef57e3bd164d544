"""Native training step of the cluster-level classifier GNN: the reference trains it
with ``loss = detector(...); loss.backward(); optimizer.step()``
(``modules/neural_net/classifier/training.py``, ``Model_Training.forward`` at
``classifier.py:75-100``).  Here the forward runs the float32 chain kernel with a tape
(every layer's pre-activation and output rows) and ``loss.backward()`` runs the native
backward:

* focal loss  -> ``rg_object_focal_loss_backward`` (d logits)
* stem + head -> ``TrainChain.backward`` (activation backward, ``rg_linear_grad``,
  dX = dZ W on the chain kernel)
* max-pool over the reference's overlapping row ranges -> ``rg_range_max_backward_ordered``
* L conv blocks (message MLP on cat(x_i, x_j), ``aggr`` add / mean / max (torch's amax
  backward: ties share the gradient, ``rg_segment_amax_backward``), update MLP on
  cat(x, agg), identity or Linear + channel_normalization residual) -> the detector's
  conv backward without the edge part (x_i: segment sums over the destination-major
  CSR, x_j: sums over each node's source incidence list)
* encoder -> weights only (its input is data).

From object sizes (``forward_objects`` / ``train_step_loss_objects``): a conv block the fused
kernel takes (fp32, the yml widths, no residual projection, ``sum`` or ``mean``) keeps
``x``, ``P | Q``, ``agg`` and the update chain's tape -- nothing sized by the edge count -- and
its backward recomputes the messages per tile (``rg_cls_conv_backward_x3``: dP | dQ, dW_1, db_1),
then runs over N rows: dW_0's column blocks (``rg_linear_grad_ld``) and
dx += [dP | dQ] W_pq.  Any other block runs the unfused block over ``object_graph``'s CSR.

Gradients land in one flat buffer (one view per parameter, then one loss slot), like the
detector's ``TrainEngine``; the autograd node hands torch a copy per parameter so any
optimizer works.

The loop (``train_model``, training.py:48-135): ``ClassifierTrainer`` is one iteration with
the fused optimizer (NaN skip and MultiStepLR on the device, one all-reduce bucket),
``train_classifier_sequence`` feeds it from a ``SequenceStore`` through the detector's
proposals (``datagen_classifier.py:195-308``) and ``validate_classifier_sequence`` is the
validation pass.  ``train_model_accumulate_grad`` (training.py:138-236) is
``grad_accumulation_steps`` of that loop: ``accumulate_objects`` / ``accumulate_inputs`` per
micro-batch and one ``apply_accumulated`` per outer iteration (``training.GradAccumulator``).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .. import _native as nat
from .. import training as dt
from ..engine import DeviceGraph, cached_plans, segment_reduce
from ..training import TrainChain, TrainEngine, Workspaces
from . import engine as ce

N_LOSS_SLOTS = 1   # the focal loss, in the gradient bucket's tail


class _ClsConv:
    def __init__(self, blk, device, ws):
        self.blk = blk
        self.aggr = blk.aggr
        if self.aggr not in ('add', 'sum', 'mean', 'max'):
            raise NotImplementedError(f'classifier training with aggregation {self.aggr!r}')
        self.msg = TrainChain(list(blk.msg), device, ws)
        self.upd = TrainChain(list(blk.upd), device, ws)
        self.res = (TrainChain([blk.residual_connection], device, ws)
                    if blk.residual_connection is not None else None)

    def chains(self):
        return [c for c in (self.msg, self.upd, self.res) if c is not None]


class ClassifierTrainEngine(TrainEngine):
    """Forward-with-tape and backward of a classifier ``Model_Training`` (fp32).  Reuses
    the detector engine's segment-sum / incidence helpers."""

    def __init__(self, model_training, device):  # noqa: super().__init__ builds detector chains
        self.model = model_training
        pred = model_training.pred
        self.device = torch.device(device)
        self.ws = Workspaces(self.device)
        self.events = None   # a list: HIP events around the fused path's launches (engine._mark)
        self.enc = TrainChain(list(pred.encode_node_feat.encoder), self.device, self.ws)
        self.convs = [_ClsConv(b, self.device, self.ws) for b in pred.pass_messages.conv_blk]
        self.head = TrainChain(pred.predict_node.chain(), self.device, self.ws)
        # flat gradient buffer: one view per parameter, then the step's loss -- the ONE bucket of
        # the data-parallel all-reduce, as TrainEngine's (a NaN loss on any rank skips the step
        # on every rank)
        self.params = [p for p in model_training.parameters()]
        n = sum(p.numel() for p in self.params)
        self.flat_bucket = torch.zeros(n + N_LOSS_SLOTS, dtype=torch.float32, device=self.device)
        self.flat_grad = self.flat_bucket[:n]
        self.loss_slots = self.flat_bucket[n:]
        self.grads = {}
        o = 0
        for p in self.params:
            self.grads[id(p)] = self.flat_grad[o:o + p.numel()].view_as(p)
            o += p.numel()
        # TrainEngine._repack_in_place's memo: the job list it uploaded and its device copy
        self._repack_key = None
        self._repack_dev = None

    def chains(self):
        out = [self.enc, self.head]
        for cv in self.convs:
            out += cv.chains()
        return out

    def invalidate(self):
        """Parameters changed behind torch's version counters: the encoder, head and conv
        chains re-pack as TrainEngine's do (in place by one launch where every held image
        allows it), and every block's ClsFusedPlan -- whose images are packed from derived
        copies of the weights, so never in place -- is made stale, both image sets."""
        super().invalidate()
        for cv in self.convs:
            for p in cached_plans(cv.blk):
                if isinstance(p, ce.ClsFusedPlan):
                    p.invalidate()

    # ------------------------------------------------------------------ forward
    def forward(self, nf: torch.Tensor, g: DeviceGraph, begin: torch.Tensor, end: torch.Tensor,
                labels: torch.Tensor):
        """Batched samples: node features f32 [N, 5], object graph g, pooling ranges,
        labels int64 [n_obj] -> (loss f32 [1], tape)."""
        N, E = g.n_nodes, g.n_edges
        n_obj = int(begin.numel())
        T = {'g': g, 'N': N, 'E': E, 'n_obj': n_obj, 'begin': begin, 'end': end}
        x = torch.empty((N, self.enc.out_dim), dtype=torch.float32, device=self.device)
        xin = nf.to(torch.float32).contiguous()
        T['enc'] = self.enc.forward(N, x, xin, xin.shape[1])
        xs = [x]
        T['conv'] = []
        for cv in self.convs:
            ct, x = self._block_forward(cv, x, g)
            T['conv'].append(ct)
            xs.append(x)
        T['xs'] = xs
        return self._pool_head_loss(T, x, labels), T

    def _block_forward(self, cv, x, g: DeviceGraph):
        """One taped unfused conv block over g: (tape, x_out)."""
        f32 = dict(dtype=torch.float32, device=self.device)
        N, E = g.n_nodes, g.n_edges
        C = x.shape[1]
        ct = {}
        msg = torch.empty((max(E, 1), cv.msg.out_dim), **f32)
        ct['msg'] = cv.msg.forward(E, msg, x, C, mode=nat.IN_GATHER3, idx0=g.dst, idx1=g.src)
        ct['msg_out'] = msg   # max aggregation's backward needs the messages
        agg = torch.empty((N, cv.msg.out_dim), **f32)
        if E > 0:
            segment_reduce(msg, g.seg_ptr, N, cv.aggr, agg)
        else:
            agg.zero_()
        if cv.res is not None:
            ident = torch.empty((N, cv.upd.out_dim), **f32)
            ct['res'] = cv.res.forward(N, ident, x, C)
        else:
            ident = x
        xn = torch.empty((N, cv.upd.out_dim), **f32)
        ct['upd'] = cv.upd.forward(N, xn, x, C, mode=nat.IN_CONCAT2, in1=agg,
                                   w1=cv.msg.out_dim, residual=ident)
        return ct, xn

    def _pool_head_loss(self, T: dict, x, labels):
        """Max-pool over the objects' row ranges, stem + head, focal loss -> loss f32 [1]."""
        lib = nat.lib()
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        N, n_obj, begin, end = T['N'], T['n_obj'], T['begin'], T['end']
        C = x.shape[1]
        pooled = torch.empty((max(n_obj, 1), C), **f32)
        ws = torch.empty(lib.rg_segment_reduce_ranges_workspace_size(N, C, nat.RG_F32),
                         dtype=torch.uint8, device=dev)
        nat.check(lib.rg_segment_reduce_ranges(
            x.data_ptr(), nat.RG_F32, x.stride(0), N, begin.data_ptr(), end.data_ptr(), n_obj, C,
            nat.REDUCE['max'], pooled.data_ptr(), nat.RG_F32, pooled.stride(0), ws.data_ptr(),
            ws.numel(), nat.stream_ptr(dev)), 'rg_segment_reduce_ranges')
        logits = torch.empty((max(n_obj, 1), self.head.out_dim), **f32)
        T['head'] = self.head.forward(n_obj, logits, pooled, C)
        lab = labels.to(torch.int64).contiguous()
        loss = ce.focal_loss(logits[:n_obj], lab).reshape(1)
        T.update(logits=logits, labels=lab, pooled=pooled)
        return loss

    def forward_objects(self, nf: torch.Tensor, object_size: torch.Tensor, begin: torch.Tensor,
                        end: torch.Tensor, labels: torch.Tensor, n_nodes=None, n_edges=None,
                        max_size=None):
        """forward() straight from the object sizes int64 [n_obj] (the batch's graph is the union
        of complete graphs over consecutive rows).  A block the fused kernel takes keeps x,
        P | Q, agg and the update chain's tape; the object table is built once per step.  Any
        other block (other widths, a residual projection, aggr = 'max', a refusal) runs the taped
        unfused block over object_graph's CSR, built lazily and once.  n_nodes / n_edges /
        max_size: host integers (sum n, sum n (n - 1), max n); whichever is not given is read
        back from object_size (a host synchronisation; max_size bounds the backward's tape rows
        per chunk, so the true maximum is read rather than n_nodes assumed)."""
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        osz = object_size.to(dev).to(torch.int64).contiguous()
        n_obj = int(begin.numel())
        if n_nodes is None or n_edges is None:
            hs = osz.cpu().numpy()
            n_nodes, n_edges = int(hs.sum()), int((hs * (hs - 1)).sum())
            max_size = int(hs.max()) if hs.size else 0
        elif max_size is None:
            max_size = int(osz.max()) if osz.numel() else 0
        N, E = int(n_nodes), int(n_edges)
        max_degree = max(int(max_size) - 1, 0)
        T = {'g': None, 'N': N, 'E': E, 'n_obj': n_obj, 'begin': begin, 'end': end,
             'table': None, 'max_degree': max_degree}
        x = torch.empty((N, self.enc.out_dim), **f32)
        xin = nf.to(torch.float32).contiguous()
        T['enc'] = self.enc.forward(N, x, xin, xin.shape[1])
        xs = [x]
        T['conv'] = []
        for cv in self.convs:
            ct = self._fused_block_forward(cv, x, T, osz) if N > 0 else None
            if ct is not None:
                x = ct['out']
            else:
                if T['g'] is None:
                    T['g'] = ce.object_graph(osz, N, E)
                ct, x = self._block_forward(cv, x, T['g'])
            T['conv'].append(ct)
            xs.append(x)
        T['xs'] = xs
        return self._pool_head_loss(T, x, labels), T

    def _fused_block_forward(self, cv, x, T: dict, osz):
        """One conv block through rg_cls_conv_aggregate_x3 and the taped update chain: its tape
        {'fused', 'x', 'pq', 'agg', 'upd', 'out'}, or None for a block the fused path does not
        take.  The object table is built into T on first use."""
        if cv.aggr == 'max':   # its backward needs the messages
            return None
        fp = ce.fused_plan(cv.blk, self.device)
        if not fp.ready(x):
            return None
        f32 = dict(dtype=torch.float32, device=self.device)
        N, C = int(x.shape[0]), fp.C
        ev = getattr(self, 'events', None)
        if T['table'] is None:
            ce._mark(ev, 'object_table:start', self.device)
            T['table'] = ce.object_table(osz, N, T['E'])
            ce._mark(ev, 'object_table:end', self.device)
        pq = torch.empty((N, 2 * C), **f32)
        agg = torch.empty((N, C), **f32)
        ce._mark(ev, 'cls_conv_aggregate:start', self.device)
        ok = fp.aggregate(x, T['table'], pq, agg, self.ws)
        ce._mark(ev, 'cls_conv_aggregate:end', self.device)
        if not ok:
            return None
        xn = torch.empty((N, C), **f32)
        ct = {'fused': fp, 'x': x, 'pq': pq, 'agg': agg, 'out': xn}
        ct['upd'] = cv.upd.forward(N, xn, x, C, mode=nat.IN_CONCAT2, in1=agg, w1=C, residual=x)
        return ct

    # ------------------------------------------------------------------ backward
    def backward(self, T: dict, g_loss: torch.Tensor, zero_grads: bool = True):
        lib = nat.lib()
        dev = self.device
        st = nat.stream_ptr(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        if zero_grads:
            self.flat_grad.zero_()
        G = self.grads
        g, N, E, n_obj = T['g'], T['N'], T['E'], T['n_obj']
        logits = T['logits']
        gl = g_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_logits = torch.empty_like(logits)
        nat.check(lib.rg_object_focal_loss_backward(
            logits.data_ptr(), logits.stride(0), T['labels'].data_ptr(), n_obj, logits.shape[1],
            gl.data_ptr(), d_logits.data_ptr(), d_logits.stride(0), st),
            'rg_object_focal_loss_backward')
        x = T['xs'][-1]
        C = x.shape[1]
        d_pooled = torch.empty((max(n_obj, 1), C), **f32)
        self.head.backward(T['head'], d_logits, G, din=d_pooled)
        dx = torch.zeros((N, C), **f32)
        # (in object order, not with atomics: the ranges overlap, and a step is bit-reproducible)
        ev = getattr(self, 'events', None)
        ce._mark(ev, 'pool_backward:start', dev)
        wsb = self.ws.get('rmax', lib.rg_range_max_backward_ordered_workspace_size(n_obj, C))
        nat.check(lib.rg_range_max_backward_ordered(
            x.data_ptr(), x.stride(0), C, T['begin'].data_ptr(), T['end'].data_ptr(), n_obj,
            d_pooled.data_ptr(), d_pooled.stride(0), dx.data_ptr(), dx.stride(0), wsb.data_ptr(),
            wsb.numel(), st), 'rg_range_max_backward_ordered')
        ce._mark(ev, 'pool_backward:end', dev)
        inc = None   # (identity ptr, source incidence) of g: built when a block ran unfused
        for li in range(len(self.convs) - 1, -1, -1):
            cv, ct = self.convs[li], T['conv'][li]
            if ct.get('fused') is not None:
                dx, _ = self._fused_block_backward(cv, ct, T, dx, G)
                continue
            if inc is None:
                inc = self._graph_incidence(g)
            dx = self._block_backward(cv, ct, g, inc, T['xs'][li].shape[1], dx, G)
        self.enc.backward(T['enc'], dx, G)

    def _graph_incidence(self, g: DeviceGraph):
        return (self._identity_ptr(g.n_edges),) + self._incidence('src', g.src, None, g.n_edges,
                                                                  g.n_nodes)

    def _block_backward(self, cv, ct, g: DeviceGraph, inc, Cin: int, dx, G):
        """Backward of a block taped by _block_forward: dx of the block input."""
        lib = nat.lib()
        st = nat.stream_ptr(self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        N, E = g.n_nodes, g.n_edges
        eptr, src_ptr, src_lst = inc
        Cm = cv.msg.out_dim
        d_updin = torch.empty((N, Cin + Cm), **f32)
        cv.upd.backward(ct['upd'], dx.clone(), G, din=d_updin)
        if cv.res is not None:
            dx_new = torch.empty((N, Cin), **f32)
            cv.res.backward(ct['res'], dx, G, din=dx_new)
        else:
            dx_new = dx
        self._add_cols(d_updin, 0, Cin, dx_new)
        if E > 0:
            d_msg = torch.empty((E, Cm), **f32)
            if cv.aggr == 'max':
                m = ct['msg_out']
                nat.check(lib.rg_segment_amax_backward(
                    m.data_ptr(), m.stride(0), Cm, g.seg_ptr.data_ptr(), N,
                    d_updin[:, Cin:].data_ptr(), d_updin.stride(0), d_msg.data_ptr(),
                    d_msg.stride(0), st), 'rg_segment_amax_backward')
            else:
                scale = self._mean_scale(g, N) if cv.aggr == 'mean' else None
                self._segsum(d_updin, Cin, Cm, eptr, g.dst, scale, d_msg, accumulate=False)
            dG = torch.empty((E, cv.msg.in_dim), **f32)
            cv.msg.backward(ct['msg'], d_msg, G, din=dG)
            self._segsum(dG, 0, Cin, g.seg_ptr, None, None, dx_new, accumulate=True)
            self._segsum(dG, Cin, Cin, src_ptr, src_lst, None, dx_new, accumulate=True)
        return dx_new

    def _fused_block_backward(self, cv, ct, T, dx, G):
        """Backward of a block taped by forward_objects' fused path: (dx of the block input,
        dP | dQ [N, 256])."""
        lib = nat.lib()
        st = nat.stream_ptr(self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        fp, x = ct['fused'], ct['x']
        N, C = int(x.shape[0]), fp.C
        m0, m1 = cv.msg.specs
        # update MLP on cat(x, agg) with the identity residual: dx += its x columns
        d_updin = torch.empty((N, 2 * C), **f32)
        cv.upd.backward(ct['upd'], dx.clone(), G, din=d_updin)
        self._add_cols(d_updin, 0, C, dx)
        # the edge phase: dP | dQ, dW_1, db_1
        d_pq = torch.empty((N, 2 * C), **f32)
        db1 = G[id(m1.bias)] if m1.bias is not None else torch.zeros(C, **f32)
        ev = getattr(self, 'events', None)
        ce._mark(ev, 'cls_conv_backward:start', self.device)
        fp.backward_edges(ct['pq'], d_updin[:, C:], T['table'], T['E'], T['max_degree'], d_pq,
                          G[id(m1.weight)], db1, self.ws)
        ce._mark(ev, 'cls_conv_backward:end', self.device)
        # P | Q = W_pq x + [b_0; 0] over N rows: dW_0's x_i and x_j column blocks, db_0, dx
        dW0 = G[id(m0.weight)]
        wsz = lib.rg_linear_grad_workspace_size(N, C, C)
        ws = self.ws.get('lgrad', wsz)
        for half in (0, 1):
            db0 = G[id(m0.bias)] if (half == 0 and m0.bias is not None) else None
            nat.check(lib.rg_linear_grad_ld(
                d_pq.data_ptr() + 4 * C * half, d_pq.stride(0), N, C, C, nat.IN_DENSE,
                x.data_ptr(), x.stride(0), C, None, 0, 0, None, 0, 0, None, None,
                dW0.data_ptr() + 4 * C * half, dW0.stride(0), nat.ptr(db0), ws.data_ptr(),
                ws.numel(), st), 'rg_linear_grad_ld (dW_0 column block)')
        fp.dx_pq(d_pq, dx)
        return dx, d_pq


class _ClsTrainStep(torch.autograd.Function):
    """The classifier loss as an autograd node over every parameter."""

    @staticmethod
    def forward(ctx, engine_, batch, *params):
        loss, tape = engine_.forward(*batch)
        ctx.engine = engine_
        ctx.tape = tape
        return loss[0]

    @staticmethod
    def backward(ctx, g_loss):
        eng = ctx.engine
        eng.backward(ctx.tape, g_loss)
        ctx.tape = None
        return (None, None) + tuple(eng.grads[id(p)].clone() for p in eng.params)


def prepare_batch(node_features: List[torch.Tensor], edge_index: List[torch.Tensor],
                  object_size: List[torch.Tensor], groundtruths: List[torch.Tensor]):
    """The list arguments of Model_Training.forward as one disjoint-union batch on the
    device: (node features, DeviceGraph, pooling begin / end, labels)."""
    dev = node_features[0].device
    sizes = [int(t.shape[0]) for t in node_features]
    bases = np.cumsum([0] + sizes)
    nf = torch.cat([t.to(torch.float32) for t in node_features], 0)
    ei = torch.cat([e.to(dev).to(torch.int64) + int(b) for e, b in zip(edge_index, bases[:-1])], 1)
    osz = torch.cat([o.to(dev).to(torch.int64) for o in object_size], 0)
    if len(node_features) == 1:
        sobj = nbase = None
    else:
        nobj = np.cumsum([0] + [int(o.numel()) for o in object_size])
        sobj = torch.tensor(nobj, dtype=torch.int32).to(dev)
        nbase = torch.tensor(bases[:-1], dtype=torch.int32).to(dev)
    N = int(bases[-1])
    g = DeviceGraph.from_edge_index(ei.contiguous(), N, count_pairs=False)
    begin, end = ce.object_row_ranges(osz, sobj, nbase, len(node_features))
    labels = torch.cat([t.to(dev).to(torch.int64) for t in groundtruths], 0)
    return nf, g, begin, end, labels


def train_step_loss(engine_: ClassifierTrainEngine, batch) -> torch.Tensor:
    """Scalar classifier loss with the native backward attached."""
    return _ClsTrainStep.apply(engine_, batch, *engine_.params)


class _ClsTrainStepObjects(_ClsTrainStep):
    """_ClsTrainStep over ClassifierTrainEngine.forward_objects."""

    @staticmethod
    def forward(ctx, engine_, batch, *params):
        nf, osz, begin, end, labels, n_nodes, n_edges, max_size = batch
        loss, tape = engine_.forward_objects(nf, osz, begin, end, labels, n_nodes, n_edges,
                                             max_size)
        ctx.engine = engine_
        ctx.tape = tape
        return loss[0]


def prepare_batch_objects(node_features: List[torch.Tensor], object_size: List[torch.Tensor],
                          groundtruths: List[torch.Tensor]):
    """The list arguments of Model_Training.forward_objects (forward's without edge_index) as
    one batch on the device: (node features, object sizes, pooling begin / end, labels, n_nodes,
    n_edges, max object size) -- the last three host integers from the sizes."""
    dev = node_features[0].device
    sizes = [int(t.shape[0]) for t in node_features]
    bases = np.cumsum([0] + sizes)
    nf = torch.cat([t.to(torch.float32) for t in node_features], 0)
    hs = np.concatenate([o.detach().cpu().numpy().astype(np.int64).reshape(-1)
                         for o in object_size])
    osz = torch.from_numpy(hs).to(dev)
    if len(node_features) == 1:
        sobj = nbase = None
    else:
        nobj = np.cumsum([0] + [int(o.numel()) for o in object_size])
        sobj = torch.tensor(nobj, dtype=torch.int32).to(dev)
        nbase = torch.tensor(bases[:-1], dtype=torch.int32).to(dev)
    begin, end = ce.object_row_ranges(osz, sobj, nbase, len(node_features))
    labels = torch.cat([t.to(dev).to(torch.int64) for t in groundtruths], 0)
    return (nf, osz, begin, end, labels, int(hs.sum()), int((hs * (hs - 1)).sum()),
            int(hs.max()) if hs.size else 0)


def train_step_loss_objects(engine_: ClassifierTrainEngine, batch) -> torch.Tensor:
    """train_step_loss from object sizes: batch = (nf, object_size, begin, end, labels, n_nodes,
    n_edges, max_size) as prepare_batch_objects returns it (an integer may be None: read back from
    object_size)."""
    return _ClsTrainStepObjects.apply(engine_, tuple(batch), *engine_.params)


# ------------------------------------------------------------------ trainer and loop
def classifier_milestones(cfg, starting_iter_num: int = 0):
    """set_param_for_training_classifier.py:52-56: decay x0.1 at 60 % and 90 % of
    max_train_iter, shifted by the iteration training resumes from."""
    return [int(0.6 * cfg.max_train_iter - starting_iter_num),
            int(0.9 * cfg.max_train_iter - starting_iter_num)]


class ClassifierTrainer:
    """One data-parallel training iteration of the classifier (classifier/training.py:66-81 for
    one rank's batch): the taped forward from object sizes + focal loss -> backward -> gradient
    all-reduce -> fused optimizer step, without a host synchronisation.

    train_model's loop rules hold as in RadarGNNTrainer: the loss rides in the gradient bucket's
    tail, so after the all-reduce every rank holds the sum and the optimizer kernel skips the
    update everywhere when it is NaN (skip_batch, training.py:40-45, 76-80); the lr follows
    MultiStepLR at 60 % / 90 % of max_train_iter over the applied steps; cfg.optim picks SGD
    (momentum 0.9) or AdamW (set_param_for_training_classifier.py:43-56).  Every step ends in
    Model_Training.invalidate_plans: the optimizer writes the weights behind torch's version
    counters."""

    def __init__(self, model_training, cfg, world: int = 1, lr: Optional[float] = None,
                 weight_decay: Optional[float] = None, optim: Optional[str] = None,
                 momentum: float = 0.9, milestones=None, starting_iter_num: int = 0):
        if model_training.pred.compute_dtype != 'fp32':
            raise NotImplementedError('classifier training runs in float32 (the reference '
                                      'precision); set compute_dtype = "fp32"')
        self.model = model_training
        self.cfg = cfg
        self.world = world
        lr = cfg.learning_rate if lr is None else lr
        wd = cfg.weight_decay if weight_decay is None else weight_decay
        optim = getattr(cfg, 'optim', 'sgd') if optim is None else optim
        if milestones is None:
            milestones = classifier_milestones(cfg, starting_iter_num)
        self.opt = model_training.fused_optimizer(optim, lr, wd, momentum=momentum,
                                                  milestones=milestones)
        dt.broadcast_parameters(self.opt.flat, world)
        model_training.invalidate_plans()
        self.one = torch.ones(1, dtype=torch.float32, device=self.opt.flat.device)
        self.accum = dt.GradAccumulator(self.opt, N_LOSS_SLOTS)

    @property
    def engine(self) -> ClassifierTrainEngine:
        """The model's cached train engine (packed on first use: a HIP device only)."""
        return self.model.train_engine(self.opt.flat.device)

    def step_objects(self, node_features, object_size, begin, end, labels, n_nodes: int,
                     n_edges: int, max_size: int) -> torch.Tensor:
        """One iteration on a batch as prepare_batch_objects / ClassifierInputs give it (the
        three host integers included, so nothing is read back).  Returns the loss f32 [1] on
        the device; NaN: the update was skipped and the step not counted."""
        eng = self.engine
        loss, tape = eng.forward_objects(node_features, object_size, begin, end, labels,
                                         int(n_nodes), int(n_edges), int(max_size))
        eng.backward(tape, self.one)
        eng.loss_slots.copy_(loss)
        scale = dt.allreduce_gradients(eng.flat_bucket, self.world)
        self.opt.step(eng.flat_grad, grad_scale=scale, losses=eng.loss_slots)
        return loss

    def step_inputs(self, inp):
        """step_objects from an objects.ClassifierInputs made with node_labels.  A batch
        without a kept object -- the reference skips a None batch (training.py:64): with
        ``world == 1`` nothing runs and None is returned.  With ``world > 1`` the rank still
        joins the all-reduce, with zero gradients and NaN in its loss slot, so every rank
        skips the step and none waits for a missing peer; None is returned.  ``inp`` None (a
        batch without a frame, objects.detect_frames) is such a batch."""
        if inp is None or inp.n_objects == 0:
            if self.world > 1:
                eng = self.engine
                eng.flat_grad.zero_()
                eng.loss_slots.fill_(float('nan'))
                scale = dt.allreduce_gradients(eng.flat_bucket, self.world)
                self.opt.step(eng.flat_grad, grad_scale=scale, losses=eng.loss_slots)
            return None
        if inp.object_class is None:
            raise ValueError('step_inputs needs ClassifierInputs made with node_labels')
        begin, end = inp.ranges()
        return self.step_objects(inp.object_features, inp.object_num_meas, begin, end,
                                 inp.object_class, inp.n_rows, inp.n_edges, inp.max_size)

    # -------- gradient accumulation (train_model_accumulate_grad, training.py:138-236)
    def accumulate_objects(self, node_features, object_size, begin, end, labels, n_nodes: int,
                           n_edges: int, max_size: int, n_accum: int) -> torch.Tensor:
        """The micro-batch twin of ``step_objects``: one of up to ``n_accum`` micro-batches of
        an outer iteration.  Forward with tape, backward of ``loss / n_accum``
        (``training.GradAccumulator.g``), and the micro-batch's complete gradient and scaled
        loss are added to the accumulator; no all-reduce, no optimizer launch, no weight and no
        packed image changes until ``apply_accumulated``.  Returns the unscaled loss f32 [1].
        ValueError for ``n_accum < 1`` or one that differs from the open accumulation's."""
        self.accum.open(n_accum)
        eng = self.engine
        loss, tape = eng.forward_objects(node_features, object_size, begin, end, labels,
                                         int(n_nodes), int(n_edges), int(max_size))
        eng.backward(tape, self.accum.g(n_accum))
        self.accum.add(eng, loss)
        return loss

    def accumulate_inputs(self, inp, n_accum: int):
        """``accumulate_objects`` from an objects.ClassifierInputs made with node_labels.  A
        batch without a kept object, or ``inp`` None (a batch without a frame), contributes
        nothing -- the divisor stays ``n_accum`` (training.py:163, ``if batch_data != None``)
        -- and None is returned; it still opens the accumulation, so the apply that follows is
        the outer iteration's."""
        self.accum.open(n_accum)
        if inp is None or inp.n_objects == 0:
            return None
        if inp.object_class is None:
            raise ValueError('accumulate_inputs needs ClassifierInputs made with node_labels')
        begin, end = inp.ranges()
        return self.accumulate_objects(inp.object_features, inp.object_num_meas, begin, end,
                                       inp.object_class, inp.n_rows, inp.n_edges, inp.max_size,
                                       n_accum)

    def apply_accumulated(self) -> int:
        """Close the outer iteration: ONE gradient all-reduce and ONE optimizer launch from the
        accumulated micro-batches -- at most one applied step and one scheduler step.  A NaN
        loss in any micro-batch (on any rank) skips the update.  Returns the number of
        micro-batches that contributed; with none, ``world == 1`` launches nothing (not even
        the train engine's first packing) and ``world > 1`` joins the all-reduce with zero
        gradients and a NaN slot so that every rank skips (``training.GradAccumulator``).
        RuntimeError without an open accumulation."""
        return self.accum.apply(self.world)

    def save(self, path):
        """save_model_weights (training.py:15-17) on rank 0: the reference's state_dict keys."""
        rank = 0
        if self.world > 1:
            import torch.distributed as dist
            rank = dist.get_rank()
        if rank == 0:
            torch.save(self.model.state_dict(), path)


def _sequence_inputs(store, detector, cfg, pos, window_size, flags, min_meas, meas_noise_cov,
                     cache):
    """One batch of sliding positions to its ClassifierInputs (datagen_classifier.py:195-282 for
    every window at once): store.windows -> dynamic_frame (flipped by flags) -> frame_batch ->
    objects.detect_frames -> objects.classifier_inputs with the majority ground-truth labels.
    None for a batch without a frame."""
    from .. import frontend, objects
    ransac = bool(getattr(cfg, 'reject_static_meas_by_ransac', False))
    win = store.windows(pos, window_size)
    # (the classifier reads the class labels only: the offsets' mean is left at the default)
    dd, gd = frontend.dynamic_frame(win, ransac, with_keys=True, flip=flags)
    fb = frontend.frame_batch(dd, gd)
    det = objects.detect_frames(detector, fb, cfg, cache=cache)
    if det is None:
        return None
    if meas_noise_cov is None:
        meas_noise_cov = getattr(cfg, 'meas_noise_cov', det.meas_noise_cov)
    return objects.classifier_inputs(det.xy, det.rcs, det.cluster_ptr, det.cluster_idx,
                                     det.frame_ptr, meas_noise_cov, min_meas,
                                     node_labels=fb.labels['class_labels'],
                                     num_classes=int(cfg.num_classes))


def _batches(indices, batch_windows):
    if int(batch_windows) < 1:
        raise ValueError(f'batch_windows={batch_windows} < 1')
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    for k, i0 in enumerate(range(0, int(idx.shape[0]), int(batch_windows))):
        yield k, idx[i0:i0 + int(batch_windows)]


def train_classifier_sequence(store, detector, trainer: ClassifierTrainer, cfg, indices,
                              window_size: int = 10, batch_windows: int = 64,
                              augmentation: Optional[bool] = None, min_meas: int = 2,
                              meas_noise_cov=None, on_step=None,
                              grad_accumulation_steps: int = 1) -> torch.Tensor:
    """Classifier training from a ``sequence.SequenceStore``: the sliding positions ``indices``,
    in the caller's order, in batches of ``batch_windows``; each batch goes ``store.windows`` ->
    ``frontend.dynamic_frame`` (with the x-axis flip when ``augmentation``, default
    cfg.dataset_augmentation; the flags from ``frontend.draw_flips``, numpy's global generator,
    drawn as ``training.train_sequence`` draws them) -> ``frontend.frame_batch`` -> graph build
    and the detector's proposal forward under no_grad (``objects.detect_frames``; ``detector``
    is a Model_Inference with set_param_for_proposal_extraction done) ->
    ``objects.classifier_inputs`` with the majority ground-truth labels, objects of at least
    ``min_meas`` members kept (valid_cluster_num_meas_thr) -> ``ClassifierTrainer.step_inputs``.
    No host work per window; per batch the host waits only where ``select_dynamic``,
    ``frame_batch``, ``propose_clusters`` and the one read of ``classifier_inputs`` do.
    ``on_step(step index, positions, flags or None, loss or None, inputs)`` is called after
    every batch (inputs None for a batch without a frame; step_inputs is called for it too, so
    a rank of several still joins the step's all-reduce).  Returns the losses f32 [steps] on
    the device: one entry per batch that had an object (a skipped NaN step keeps its entry).

    ``grad_accumulation_steps`` = K > 1 (train_model_accumulate_grad, training.py:138-236):
    consecutive groups of K batches form one outer iteration -- each batch a micro-batch through
    ``ClassifierTrainer.accumulate_inputs``, then one ``apply_accumulated``; a trailing group
    shorter than K is applied with what it has, the divisor staying K.  Flags are drawn per
    micro-batch; ``on_step`` is called after every micro-batch with the OUTER iteration first
    (for a group's last micro-batch after the apply, as with K = 1); the entries are one per
    contributing micro-batch, unscaled.  All K micro-batches always run: a NaN loss skips the
    step at the apply, where the reference breaks out of the group.  K = 1 is the path above,
    unchanged."""
    from .. import frontend
    K = dt.accumulation_steps(grad_accumulation_steps)
    augmentation = bool(cfg.dataset_augmentation if augmentation is None else augmentation)
    cache: dict = {}
    losses = []
    batches = list(_batches(indices, batch_windows))
    for k, pos in batches:
        flags = frontend.draw_flips(int(pos.shape[0])) if augmentation else None
        inp = _sequence_inputs(store, detector, cfg, pos, window_size, flags, min_meas,
                               meas_noise_cov, cache)
        # (a batch without a frame goes to the trainer too: with world > 1 the rank must join
        # the step's all-reduce, or its peers wait for it)
        if K == 1:
            loss = trainer.step_inputs(inp)
        else:
            loss = trainer.accumulate_inputs(inp, K)
            if (k + 1) % K == 0 or k + 1 == len(batches):
                trainer.apply_accumulated()
        if loss is not None:
            losses.append(loss)
        if on_step is not None:
            on_step(k // K, pos, flags, loss, inp)
    if not losses:
        return torch.empty(0, dtype=torch.float32, device=trainer.opt.flat.device)
    return torch.cat(losses)


def validate_classifier_sequence(store, detector, model_training, cfg, indices,
                                 window_size: int = 10, batch_windows: int = 64,
                                 min_meas: int = 2, meas_noise_cov=None):
    """The validation loop of train_model (training.py:102-118) over a sequence: the walk of
    train_classifier_sequence without the flip, under no_grad, through the inference
    ``forward_objects`` and the focal loss.  Returns (mean of the batch losses that are not
    NaN, their number) as LossTracker averages them -- (nan, 0) when none counted; the losses
    are read back once, at the end.  Weights, optimizer state and applied steps are untouched."""
    from .. import objects
    cache: dict = {}
    losses = []
    with torch.no_grad():
        for _, pos in _batches(indices, batch_windows):
            inp = _sequence_inputs(store, detector, cfg, pos, window_size, None, min_meas,
                                   meas_noise_cov, cache)
            if inp is None or inp.n_objects == 0:
                continue
            logits = objects.classify_inputs(model_training, inp)
            losses.append(ce.focal_loss(logits, inp.object_class).reshape(1))
    if not losses:
        return float('nan'), 0
    vals = torch.cat(losses).cpu().numpy()
    vals = vals[~np.isnan(vals)]
    if vals.size == 0:
        return float('nan'), 0
    return float(np.mean(vals, dtype=np.float64)), int(vals.size)


def evaluate_classifier_sequence(store, detector, classifier_model, cfg, indices,
                                 window_size: int = 10, batch_windows: int = 64,
                                 min_meas: int = 2, meas_noise_cov=None, evaluator=None):
    """The accuracy validate_classifier_sequence lacks: the same walk (no flip, no_grad, a
    ``SequenceStore`` or a ``SequenceSet``) with every kept proposal's predicted class -- the
    first maximum of its logits -- counted against its majority ground-truth class, lowest
    label on a tie (datagen_classifier.py:50-60), in an ``evaluation.ObjectClassEvaluator``
    (new unless given).  Nothing is read back: ``result()`` of the returned evaluator is the
    only read of the counters.  Weights, optimizer state and applied steps are untouched."""
    from .. import evaluation, objects
    if evaluator is None:
        evaluator = evaluation.ObjectClassEvaluator(int(cfg.num_classes))
    cache: dict = {}
    with torch.no_grad():
        for _, pos in _batches(indices, batch_windows):
            inp = _sequence_inputs(store, detector, cfg, pos, window_size, None, min_meas,
                                   meas_noise_cov, cache)
            if inp is None or inp.n_objects == 0:
                continue
            evaluator.update_logits(objects.classify_inputs(classifier_model, inp),
                                    inp.object_class)
    return evaluator
