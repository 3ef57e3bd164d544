"""Detection and segmentation evaluation on the GPU (csrc/evaluation.hip).

The reference's evaluation (modules/performance/detection_accuracy.py,
segmentation_accuracy.py, performance_eval_detection.ipynb, performance_eval_segmentation.ipynb)
for batches of frames:

  gt_clusters                        compute_node_idx_for_each_cluster (datagen_gnn.py:15-45)
  associate                          the size filter of detection_accuracy.py:141-164 and
                                     compute_gt_and_pred_associations (:192-273), all frames
  compute_gt_and_pred_associations   the drop-in for the reference function (one frame)
  cluster_centres, associate_l2      the same association under the 'l2_norm' criterion: the
                                     float32 distance between cluster centres (:211-213, 225)
  compute_gt_and_pred_associations_l2  the drop-in with that criterion (one frame)
  DetectionEvaluator                 performance_eval_detection.ipynb: confusion matrix,
                                     ground-truth and prediction counts, precision, recall
  SegmentationEvaluator              performance_eval_segmentation.ipynb: node-level confusion
  ObjectClassEvaluator               the same matrix over proposals: predicted class against
                                     the majority node class (datagen_classifier.py:50-60)
  TwoStageEvaluators                 detection and object-level counts for the three class
                                     sources (vote, object head, cluster-level classifier;
                                     detection_accuracy.py:95-109) on one association

The predicted node class is the argmax of the ``node_cls`` logits, lowest index on a tie.  The
reference takes the argmax of the float32 softmax (detection_accuracy.py:97-98), which is the
same class except where two logits within an ulp of each other round to equal probabilities:
there the reference returns the lower index even when its logit is the smaller one.

Counters live on the device as int64 tensors; ``update`` enqueues kernels on the current stream
and never synchronises, ``result`` reads the counters back once.
"""
from __future__ import annotations

import json
from typing import List, Optional, Sequence

import numpy as np

from . import _native as nat

INVALID_CLS_IDX = 5  # the 'NONE' class both notebooks delete before reporting


def _torch():
    import torch
    return torch


def _i32(dev, n, fill=None):
    torch = _torch()
    if fill is None:
        return torch.empty(max(int(n), 1), dtype=torch.int32, device=dev)
    return torch.full((max(int(n), 1),), fill, dtype=torch.int32, device=dev)


def _workspace(cache: Optional[dict], name: str, nbytes: int, dev):
    torch = _torch()
    cache = cache if cache is not None else {}
    t = cache.get(name)
    if t is None or t.numel() < nbytes or t.device != dev:
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        cache[name] = t
    return t


def _rows(x):
    """A float32 matrix with unit column stride (its row stride is passed as ld)."""
    torch = _torch()
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.dim() != 2:
        raise ValueError(f'expected a [rows, classes] matrix, got {tuple(x.shape)}')
    if x.shape[0] > 0 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def argmax_rows(x):
    """int64 [rows]: the index of the first maximum of every row (rg_argmax_rows)."""
    torch = _torch()
    x = _rows(x)
    n, nc = int(x.shape[0]), int(x.shape[1])
    out = torch.empty(max(n, 1), dtype=torch.int64, device=x.device)
    if n > 0:
        nat.check(nat.lib().rg_argmax_rows(x.data_ptr(), x.stride(0), n, nc, out.data_ptr(),
                                           nat.stream_ptr(x.device)), 'rg_argmax_rows')
    return out[:n]


def gt_clusters(track_key, node_class, frame_ptr, ws_cache: Optional[dict] = None) -> dict:
    """Ground-truth clusters of a batch from per-node track keys (int32, 0 = no track): per
    frame the tracked clusters in ascending key order, then one singleton per untracked node
    (compute_node_idx_for_each_cluster, datagen_gnn.py:15-45).  Device tensors, no sync:
    cluster_of [N], cluster_ptr [N+1] (entries past the last cluster repeat N), cluster_idx
    [N], frame_clusters [F], cluster_class int64 [N], n_clusters [1]."""
    torch = _torch()
    dev = track_key.device
    N, F = int(track_key.shape[0]), int(frame_ptr.shape[0]) - 1
    lib = nat.lib()
    key = track_key.to(torch.int32).contiguous()
    cls = node_class.to(torch.int64).contiguous()
    fptr = frame_ptr.to(torch.int32).contiguous()
    out = dict(cluster_of=_i32(dev, N), cluster_ptr=_i32(dev, N + 1), cluster_idx=_i32(dev, N),
               frame_clusters=_i32(dev, F),
               cluster_class=torch.empty(max(N, 1), dtype=torch.int64, device=dev),
               n_clusters=_i32(dev, 1))
    wsz = lib.rg_eval_gt_clusters_workspace_size(N)
    ws = _workspace(ws_cache, 'eval_gt_ws', wsz, dev)
    nat.check(lib.rg_eval_gt_clusters(key.data_ptr(), cls.data_ptr(), fptr.data_ptr(), N, F,
                                      out['cluster_of'].data_ptr(), out['cluster_ptr'].data_ptr(),
                                      out['cluster_idx'].data_ptr(),
                                      out['frame_clusters'].data_ptr(),
                                      out['cluster_class'].data_ptr(),
                                      out['n_clusters'].data_ptr(), ws.data_ptr(), wsz,
                                      nat.stream_ptr(dev)), 'rg_eval_gt_clusters')
    out['frame_clusters'] = out['frame_clusters'][:F]
    return out


def _full_ptr(cluster_ptr, N):
    """cluster_ptr padded to N + 1 entries, the tail repeating N (the rg_cluster_lists form)."""
    torch = _torch()
    ptr = cluster_ptr.to(torch.int32)
    if ptr.numel() > N + 1:
        raise ValueError(f'{ptr.numel() - 1} clusters for {N} nodes')
    if ptr.numel() == N + 1:
        return ptr.contiguous()
    full = torch.full((N + 1,), N, dtype=torch.int32, device=ptr.device)
    full[:ptr.numel()] = ptr
    return full


def cluster_of(cluster_ptr, cluster_idx, N):
    """int32 [N]: the cluster of every node of a CSR (-1 = in none)."""
    dev = cluster_ptr.device
    out = _i32(dev, N)
    ncl = int(cluster_ptr.numel()) - 1
    nat.check(nat.lib().rg_eval_cluster_of(cluster_ptr.data_ptr(), cluster_idx.data_ptr(), ncl, N,
                                           out.data_ptr(), nat.stream_ptr(dev)),
              'rg_eval_cluster_of')
    return out


def associate(frame_ptr, gt_of, gt_ptr, gt_idx, pred_of, pred_ptr, pred_idx, eps: float,
              cluster_size_threshold: int = 0, max_frame_nodes: Optional[int] = None,
              ws_cache: Optional[dict] = None) -> dict:
    """Size filter + greedy 1 - IoU association of every frame (rg_eval_associate).  All
    arguments are int32 device tensors over the batch's N nodes (``*_ptr`` with N + 1
    entries).  Returns device tensors: gt_kept / pred_kept [N]; pick_start / pick_count [F];
    pick_gt, pick_pred, pick_d, pick_positive, pick_gt_cluster, pick_pred_cluster [N] -- frame
    f's picks, in pick order, are the slots pick_start[f] .. + pick_count[f]."""
    torch = _torch()
    dev = gt_of.device
    N, F = int(gt_of.shape[0]), int(frame_ptr.shape[0]) - 1
    lib = nat.lib()
    out = dict(gt_kept=_i32(dev, N), pred_kept=_i32(dev, N), pick_start=_i32(dev, F),
               pick_count=_i32(dev, F), pick_gt=_i32(dev, N), pick_pred=_i32(dev, N),
               pick_d=torch.empty(max(N, 1), dtype=torch.float32, device=dev),
               pick_positive=_i32(dev, N), pick_gt_cluster=_i32(dev, N),
               pick_pred_cluster=_i32(dev, N))
    wsz = lib.rg_eval_associate_workspace_size(N, F)
    ws = _workspace(ws_cache, 'eval_assoc_ws', wsz, dev)
    maxn = N if max_frame_nodes is None else int(max_frame_nodes)
    nat.check(lib.rg_eval_associate(
        frame_ptr.data_ptr(), N, F, maxn, gt_of.data_ptr(), gt_ptr.data_ptr(), gt_idx.data_ptr(),
        pred_of.data_ptr(), pred_ptr.data_ptr(), pred_idx.data_ptr(), int(cluster_size_threshold),
        float(eps), out['gt_kept'].data_ptr(), out['pred_kept'].data_ptr(),
        out['pick_start'].data_ptr(), out['pick_count'].data_ptr(), out['pick_gt'].data_ptr(),
        out['pick_pred'].data_ptr(), out['pick_d'].data_ptr(), out['pick_positive'].data_ptr(),
        out['pick_gt_cluster'].data_ptr(), out['pick_pred_cluster'].data_ptr(), ws.data_ptr(), wsz,
        nat.stream_ptr(dev)), 'rg_eval_associate')
    for k in ('pick_start', 'pick_count'):
        out[k] = out[k][:F]
    for k in ('gt_kept', 'pred_kept', 'pick_gt', 'pick_pred', 'pick_d', 'pick_positive',
              'pick_gt_cluster', 'pick_pred_cluster'):
        out[k] = out[k][:N]
    return out


def cluster_centres(xy, cluster_ptr, cluster_idx):
    """float32 [N, 2]: the centre (sample mean of the members' positions) of every cluster of a
    CSR over N nodes, indexed by cluster id, 0 in the slots past the last cluster
    (rg_cluster_stats over the padded CSR: compute_proposals' means bit for bit).  xy float32
    [N, >= 2] on the device."""
    torch = _torch()
    xy = xy.detach()
    if xy.dim() != 2 or int(xy.shape[1]) < 2:
        raise ValueError(f'expected [N, >= 2] positions, got {tuple(xy.shape)}')
    if xy.dtype != torch.float32:
        xy = xy.to(torch.float32)
    if xy.shape[0] > 0 and xy.stride(1) != 1:
        xy = xy.contiguous()
    dev = xy.device
    N = int(xy.shape[0])
    mu = torch.zeros((max(N, 1), 2), dtype=torch.float32, device=dev)
    if N > 0:
        ptr = _full_ptr(cluster_ptr, N)
        idx = cluster_idx.to(torch.int32).contiguous()
        size = _i32(dev, N)
        sigma = torch.empty((N, 4), dtype=torch.float32, device=dev)
        bad = _i32(dev, 1, 0)
        noise = np.zeros(4, dtype=np.float32)
        nat.check(nat.lib().rg_cluster_stats(
            xy.data_ptr(), xy.stride(0), N, ptr.data_ptr(), idx.data_ptr(), N, noise.ctypes.data,
            size.data_ptr(), mu.data_ptr(), sigma.data_ptr(), None, None, bad.data_ptr(),
            nat.stream_ptr(dev)), 'rg_cluster_stats')
    return mu[:N]


def associate_l2(frame_ptr, gt_ptr, gt_idx, pred_ptr, pred_idx, gt_mu, pred_mu, eps: float,
                 cluster_size_threshold: int = 0, max_frame_nodes: Optional[int] = None,
                 ws_cache: Optional[dict] = None) -> dict:
    """Size filter + greedy association of every frame by the float32 distance between cluster
    centres, the reference's 'l2_norm' criterion (rg_eval_associate_l2).  The CSRs are int32
    device tensors over the batch's N nodes (``*_ptr`` with N + 1 entries); gt_mu / pred_mu
    float32 [N, 2] hold the centres by cluster id (``cluster_centres``).  Returns the dict
    ``associate`` returns (``frame_picks`` reads it) plus bad_value int32 [1], set when a kept
    cluster of a frame with picks to make has a centre that is not finite (such a frame has no
    picks; the reference raises).  Distances of 9,999,999 or more are outside the domain."""
    torch = _torch()
    dev = gt_ptr.device
    N, F = int(gt_ptr.shape[0]) - 1, int(frame_ptr.shape[0]) - 1
    lib = nat.lib()
    mus = []
    for name, mu in (('gt_mu', gt_mu), ('pred_mu', pred_mu)):
        if mu.dtype != torch.float32 or tuple(mu.shape) != (N, 2):
            raise ValueError(f'{name}: expected float32 [{N}, 2], got {mu.dtype} '
                             f'{tuple(mu.shape)}')
        mus.append(mu.contiguous())
    out = dict(gt_kept=_i32(dev, N), pred_kept=_i32(dev, N), pick_start=_i32(dev, F),
               pick_count=_i32(dev, F), pick_gt=_i32(dev, N), pick_pred=_i32(dev, N),
               pick_d=torch.empty(max(N, 1), dtype=torch.float32, device=dev),
               pick_positive=_i32(dev, N), pick_gt_cluster=_i32(dev, N),
               pick_pred_cluster=_i32(dev, N), bad_value=_i32(dev, 1, 0))
    wsz = lib.rg_eval_associate_l2_workspace_size(N, F)
    ws = _workspace(ws_cache, 'eval_assoc_l2_ws', wsz, dev)
    maxn = N if max_frame_nodes is None else int(max_frame_nodes)
    nat.check(lib.rg_eval_associate_l2(
        frame_ptr.data_ptr(), N, F, maxn, gt_ptr.data_ptr(), gt_idx.data_ptr(),
        pred_ptr.data_ptr(), pred_idx.data_ptr(), int(cluster_size_threshold), float(eps),
        mus[0].data_ptr(), mus[1].data_ptr(), out['gt_kept'].data_ptr(),
        out['pred_kept'].data_ptr(), out['pick_start'].data_ptr(), out['pick_count'].data_ptr(),
        out['pick_gt'].data_ptr(), out['pick_pred'].data_ptr(), out['pick_d'].data_ptr(),
        out['pick_positive'].data_ptr(), out['pick_gt_cluster'].data_ptr(),
        out['pick_pred_cluster'].data_ptr(), out['bad_value'].data_ptr(), ws.data_ptr(), wsz,
        nat.stream_ptr(dev)), 'rg_eval_associate_l2')
    for k in ('pick_start', 'pick_count'):
        out[k] = out[k][:F]
    for k in ('gt_kept', 'pred_kept', 'pick_gt', 'pick_pred', 'pick_d', 'pick_positive',
              'pick_gt_cluster', 'pick_pred_cluster'):
        out[k] = out[k][:N]
    return out


def frame_picks(assoc: dict) -> List[dict]:
    """The picks of ``associate`` / ``associate_l2`` per frame, on the host (one
    synchronisation): a list of dicts with gt, pred (int32), d (float32) and positive (bool)
    arrays in pick order."""
    h = {k: v.cpu().numpy() for k, v in assoc.items() if k.startswith('pick_')}
    out = []
    for s, c in zip(h['pick_start'], h['pick_count']):
        sl = slice(int(s), int(s) + int(c))
        out.append(dict(gt=h['pick_gt'][sl].copy(), pred=h['pick_pred'][sl].copy(),
                        d=h['pick_d'][sl].copy(), positive=h['pick_positive'][sl] != 0))
    return out


def _csr_from_sets(sets: Sequence[set], remap: dict, N: int, what: str):
    of = np.full(max(N, 1), -1, dtype=np.int32)
    ptr = np.full(N + 1, N, dtype=np.int32)
    idx = np.zeros(max(N, 1), dtype=np.int32)
    pos = 0
    for c, s in enumerate(sets):
        if len(s) == 0:
            raise ValueError(f'{what} cluster {c} is empty (the reference divides by zero)')
        mem = sorted(remap[v] for v in s)
        ptr[c] = pos
        for m in mem:
            if of[m] != -1:
                raise ValueError(f'{what} clusters {of[m]} and {c} share a measurement')
            of[m] = c
        idx[pos:pos + len(mem)] = mem
        pos += len(mem)
    ptr[len(sets):] = pos
    return of, ptr, idx, pos


def compute_gt_and_pred_associations(det_and_gt_clusters, eps, association_criteria='inv_iou',
                                     false_class_label=6, device=None):
    """Drop-in for detection_accuracy.compute_gt_and_pred_associations (:192-273): the same
    dict of lists in, the same four numpy arrays out, element for element; the association
    runs on the GPU.  This entry point is the 'inv_iou' criterion; 'l2_norm' is
    ``compute_gt_and_pred_associations_l2`` and keeps raising here."""
    torch = _torch()
    if association_criteria == 'l2_norm':
        raise NotImplementedError("association_criteria='l2_norm' is not implemented by this "
                                  "function: call compute_gt_and_pred_associations_l2")
    if association_criteria != 'inv_iou':
        raise ValueError(f'association_criteria {association_criteria!r}')
    d = det_and_gt_clusters
    n_pred, n_gt = len(d['cluster_mean_list_pred']), len(d['cluster_mean_list_gt'])
    empty = np.zeros(shape=(0, ))
    if n_pred == 0 or n_gt == 0:
        return {'obj_class_gt_associated': empty, 'obj_class_pred_associated': empty,
                'obj_class_gt': np.array(d['obj_class_gt']) if n_gt > 0 else empty,
                'obj_class_pred': np.array(d['obj_class_pred']) if n_pred > 0 else empty}
    obj_class_pred = np.array(d['obj_class_pred'])
    obj_class_gt = np.array(d['obj_class_gt'])
    gt_sets, pred_sets = d['cluster_member_list_gt'], d['cluster_member_list_pred']
    universe = sorted(set().union(*gt_sets, *pred_sets))
    remap = {v: i for i, v in enumerate(universe)}
    N = len(universe)
    dev = torch.device(device) if device is not None else torch.device('cuda',
                                                                       torch.cuda.current_device())
    g_of, g_ptr, g_idx, g_n = _csr_from_sets(gt_sets, remap, N, 'ground-truth')
    p_of, p_ptr, p_idx, p_n = _csr_from_sets(pred_sets, remap, N, 'predicted')
    # a side that does not cover every node leaves the tail of its member list unused
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    fptr = up(np.array([0, N], dtype=np.int32))
    res = associate(fptr, up(g_of), up(g_ptr), up(g_idx), up(p_of), up(p_ptr), up(p_idx),
                    float(eps), cluster_size_threshold=0)
    return _associated_arrays(frame_picks(res)[0], obj_class_gt, obj_class_pred,
                              false_class_label)


def _associated_arrays(pk, obj_class_gt, obj_class_pred, false_class_label):
    """detection_accuracy.py:237-273 from one frame's picks: the positive picks' classes, then
    the negative picks' predicted classes against ``false_class_label``."""
    pos = pk['positive']
    gi, pi = pk['gt'].astype(np.int64), pk['pred'].astype(np.int64)
    pos_gt = obj_class_gt[gi[pos]]
    pos_pred = obj_class_pred[pi[pos]]
    neg_pred = obj_class_pred[pi[~pos]]
    neg_gt = np.repeat(false_class_label, repeats=neg_pred.shape[0])
    return {'obj_class_gt_associated': np.concatenate((pos_gt, neg_gt), axis=0),
            'obj_class_pred_associated': np.concatenate((pos_pred, neg_pred), axis=0),
            'obj_class_gt': obj_class_gt, 'obj_class_pred': obj_class_pred}


def _centre_rows(means, n_rows: int, what: str) -> np.ndarray:
    out = np.zeros((n_rows, 2), dtype=np.float32)
    for i, m in enumerate(means):
        m = np.asarray(m)
        if m.dtype != np.float32:
            raise TypeError(f'cluster_mean_list_{what}[{i}] is {m.dtype}, expected the float32 '
                            'means compute_proposals returns')
        if m.shape != (2,):
            raise ValueError(f'cluster_mean_list_{what}[{i}] has shape {m.shape}, expected (2,)')
        out[i] = m
    return out


def compute_gt_and_pred_associations_l2(det_and_gt_clusters, eps, false_class_label=6,
                                        device=None):
    """detection_accuracy.compute_gt_and_pred_associations (:192-273) with
    association_criteria='l2_norm': the same dict in, the same four numpy arrays out (the
    float64 empties of conditions 2-4 included); the association runs on the GPU
    (``associate_l2``).  Only ``cluster_mean_list_*`` (float32 [2] arrays, as compute_proposals
    returns them; any other dtype is a TypeError) and ``obj_class_*`` are read, not the member
    sets.  A centre that is not finite is a ValueError (the reference fails on np.min of NaN)."""
    torch = _torch()
    d = det_and_gt_clusters
    n_pred, n_gt = len(d['cluster_mean_list_pred']), len(d['cluster_mean_list_gt'])
    empty = np.zeros(shape=(0, ))
    if n_pred == 0 or n_gt == 0:
        return {'obj_class_gt_associated': empty, 'obj_class_pred_associated': empty,
                'obj_class_gt': np.array(d['obj_class_gt']) if n_gt > 0 else empty,
                'obj_class_pred': np.array(d['obj_class_pred']) if n_pred > 0 else empty}
    obj_class_pred = np.array(d['obj_class_pred'])
    obj_class_gt = np.array(d['obj_class_gt'])
    # one frame of N = max(G, P) nodes; cluster i of either side is the node i
    N = max(n_gt, n_pred)
    g_mu = _centre_rows(d['cluster_mean_list_gt'], N, 'gt')
    p_mu = _centre_rows(d['cluster_mean_list_pred'], N, 'pred')
    dev = torch.device(device) if device is not None else torch.device('cuda',
                                                                       torch.cuda.current_device())
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    ptr = lambda n: up(np.minimum(np.arange(N + 1), n).astype(np.int32))  # noqa: E731
    idx = up(np.arange(N, dtype=np.int32))
    res = associate_l2(up(np.array([0, N], dtype=np.int32)), ptr(n_gt), idx, ptr(n_pred), idx,
                       up(g_mu), up(p_mu), float(eps), cluster_size_threshold=0)
    pk = frame_picks(res)[0]
    if int(res['bad_value'].item()):
        raise ValueError('a cluster centre is not finite')
    return _associated_arrays(pk, obj_class_gt, obj_class_pred, false_class_label)


# ------------------------------------------------------------------------- reporting
def _drop(a: np.ndarray, index: Optional[int], axes) -> np.ndarray:
    if index is None or index >= a.shape[0]:
        return a
    for ax in axes:
        a = np.delete(a, index, axis=ax)
    return a


def detection_report(confusion, gt_count, pred_count, invalid_class_index=INVALID_CLS_IDX) -> dict:
    """performance_eval_detection.ipynb, the summary cell: class ``invalid_class_index`` dropped
    from rows and columns, the row-normalised confusion matrix in percent, precision =
    diag / pred_count, recall = diag / gt_count (0 / 0 is nan, as in the notebook)."""
    conf = _drop(np.asarray(confusion, dtype=np.uint64), invalid_class_index, (0, 1))
    gt = _drop(np.asarray(gt_count, dtype=np.uint64), invalid_class_index, (0,))
    pred = _drop(np.asarray(pred_count, dtype=np.uint64), invalid_class_index, (0,))
    idx = np.arange(conf.shape[0])
    with np.errstate(divide='ignore', invalid='ignore'):
        norm = conf / np.sum(conf, axis=-1, keepdims=True) * 100
        precision = conf[idx, idx] / pred
        recall = conf[idx, idx] / gt
    return {'normalized_confusion_matrix': norm, 'precision': precision, 'recall': recall}


def segmentation_report(confusion, gt_count, invalid_class_index=INVALID_CLS_IDX) -> dict:
    """performance_eval_segmentation.ipynb, the summary cell: class ``invalid_class_index``
    dropped, each row divided by its ground-truth count, in percent, float32; a row without
    ground truth is 0."""
    conf = _drop(np.asarray(confusion, dtype=np.uint64), invalid_class_index, (0, 1))
    gt = _drop(np.asarray(gt_count, dtype=np.uint64), invalid_class_index, (0,))
    norm = np.zeros(conf.shape, dtype=np.float32)
    for i in range(gt.shape[0]):
        num_gt = gt[i]
        if num_gt > 0:
            norm[i, :] = conf[i, :] / num_gt * 100
        else:
            norm[i, :] = 0.0
    return {'confusion_matrix_norm': norm}


class _Counters:
    """int64 counters: a device tensor per name, created by the first update, plus a host part
    (merged evaluators).  ``counts`` synchronises once."""

    NAMES: tuple = ()

    def __init__(self, num_classes: int):
        if not 1 <= int(num_classes) <= 32:
            raise ValueError(f'num_classes={num_classes} outside 1..32')
        self.num_classes = int(num_classes)
        self._host = {k: np.zeros(self._shape(k), dtype=np.int64) for k in self.NAMES}
        self._dev = None
        self._bad = None
        self._ws: dict = {}

    def _shape(self, name):
        nc = self.num_classes
        return (nc, nc) if name == 'confusion_matrix' else (nc,)

    def _device_counters(self, dev):
        torch = _torch()
        if self._dev is None:
            self._dev = {k: torch.zeros(self._shape(k), dtype=torch.int64, device=dev)
                         for k in self.NAMES}
            # [0]: a class id out of range, [1]: a centre that is not finite ('l2_norm'),
            # [2]: an index out of range in the object stage that fed the evaluator
            self._bad = torch.zeros(3, dtype=torch.int32, device=dev)
        elif self._bad.device != dev:
            raise ValueError(f'evaluator lives on {self._bad.device}, update came from {dev}')
        return self._dev

    def counts(self) -> dict:
        out = {k: v.copy() for k, v in self._host.items()}
        if self._dev is not None:
            torch = _torch()
            flat = torch.cat([self._dev[k].reshape(-1) for k in self.NAMES]
                             + [self._bad.to(torch.int64)]).cpu().numpy()
            if flat[-3]:
                raise RuntimeError('a class id outside [0, num_classes) reached the evaluator')
            if flat[-2]:
                raise RuntimeError("a cluster centre that is not finite reached the 'l2_norm' "
                                   'association (the reference raises on such a frame)')
            if flat[-1]:
                raise RuntimeError('a member, label or cluster index outside its range reached '
                                   'the object stage that fed the evaluator')
            off = 0
            for k in self.NAMES:
                n = int(np.prod(self._shape(k)))
                out[k] += flat[off:off + n].reshape(self._shape(k))
                off += n
        return {k: v.astype(np.uint64) for k, v in out.items()}

    def merge(self, other):
        """Add another evaluator's counters (another rank's, another sequence's)."""
        if type(other) is not type(self) or other.num_classes != self.num_classes:
            raise ValueError('merge needs an evaluator of the same kind and num_classes')
        for k, v in other.counts().items():
            self._host[k] += v.astype(np.int64)
        return self

    def load_counts(self, **counts):
        """Add host count matrices (for instance read back from ``to_json`` files)."""
        for k in self.NAMES:
            a = np.asarray(counts[k], dtype=np.int64)
            if a.shape != self._shape(k):
                raise ValueError(f'{k}: shape {a.shape}, expected {self._shape(k)}')
            self._host[k] += a
        return self

    def to_json(self, path, class_names):
        """The reference's per-sequence file: class_names and the count matrices as lists."""
        data = {'class_names': list(class_names)}
        for k, v in self.counts().items():
            data[k] = v.tolist()
        with open(path, 'w') as fh:
            json.dump(data, fh, indent=4)
        return data


class DetectionEvaluator(_Counters):
    """performance_eval_detection.ipynb on the device: per batch the ground-truth clusters from
    the track keys, the predicted clusters' classes, the size filter, the greedy association
    (compute_gt_and_pred_associations) and the three count matrices.  association_criteria is
    the reference's: 'inv_iou' (1 - IoU of the member sets) or 'l2_norm' (the float32 distance
    between the cluster centres, which needs the node positions: ``update(..., xy=)``).

    class_source names where a predicted cluster's class comes from (detection_accuracy.py:95-109
    has the first two): 'segmentation' (the majority of its node classes), 'object_head' (the
    detector's object head) or 'classifier' (the cluster-level classifier's class, handed to
    ``update`` as ``cluster_class``).  None keeps ``by_segmentation``'s meaning."""

    CLASS_SOURCES = ('segmentation', 'object_head', 'classifier')

    NAMES = ('confusion_matrix', 'gt_count_matrix', 'pred_count_matrix')

    def __init__(self, num_classes: int = 7, eps: float = 0.7, cluster_size_threshold: int = 0,
                 by_segmentation: bool = True, false_class_label: int = 6,
                 association_criteria: str = 'inv_iou', class_source: Optional[str] = None):
        super().__init__(num_classes)
        if class_source is None:
            class_source = 'segmentation' if by_segmentation else 'object_head'
        elif class_source not in self.CLASS_SOURCES:
            raise ValueError(f'class_source {class_source!r}: one of {self.CLASS_SOURCES}')
        else:
            by_segmentation = class_source == 'segmentation'
        self.class_source = class_source
        if association_criteria not in ('inv_iou', 'l2_norm'):
            raise ValueError(f"association_criteria {association_criteria!r}: "
                             "'inv_iou' or 'l2_norm'")
        self.association_criteria = association_criteria
        if not 0 <= int(false_class_label) < self.num_classes:
            raise ValueError(f'false_class_label={false_class_label} outside [0, {num_classes})')
        if int(cluster_size_threshold) < 0:
            raise ValueError('cluster_size_threshold < 0')
        self.eps = float(eps)
        self.cluster_size_threshold = int(cluster_size_threshold)
        self.by_segmentation = bool(by_segmentation)
        self.false_class_label = int(false_class_label)

    def _association_params(self, N: int, F: int, ncl: int) -> dict:
        """What two evaluators must agree on to share one batch's association."""
        return dict(association_criteria=self.association_criteria, eps=self.eps,
                    cluster_size_threshold=self.cluster_size_threshold, n_nodes=N, n_frames=F,
                    n_clusters=ncl)

    def update(self, node_cls, obj_cls, pred_cluster_ptr, pred_cluster_idx, node_gt_class,
               track_key, frame_ptr, max_frame_nodes: Optional[int] = None, xy=None,
               cluster_class=None, association: Optional[dict] = None):
        """One batch, every tensor on the device, no host synchronisation.  node_cls f32
        [N, C] logits, obj_cls f32 [clusters, C] logits (read only when not by_segmentation),
        pred_cluster_ptr / pred_cluster_idx the predicted clusters' CSR over global node ids
        (as engine.propose_clusters returns them), node_gt_class [N], track_key int32 [N]
        (0 = no track), frame_ptr int32 [F + 1].  max_frame_nodes bounds the largest frame
        (default: N); it must stay below 2^24 under 'inv_iou'.  xy float32 [N, >= 2]: the
        node positions, required under 'l2_norm' and ignored under 'inv_iou'.  ``self.last``
        keeps the batch's device tensors (ground-truth clusters, predicted classes, picks;
        under 'l2_norm' also the centres gt_mu / pred_mu by cluster id) until the next
        update.

        cluster_class int64 [clusters] on the device: the predicted clusters' classes under
        class_source='classifier' (required there; neither node_cls' argmax nor obj_cls is
        read), ignored otherwise.

        association: the ``last`` of another DetectionEvaluator that was updated on this same
        batch with the same criterion, eps and cluster_size_threshold (anything else is a
        ValueError).  The association does not depend on the classes, so the ground-truth
        clusters and the picks are taken from there and only the class source and the counts
        are this evaluator's: several class sources cost one association per batch."""
        torch = _torch()
        N, F = int(node_cls.shape[0]), int(frame_ptr.shape[0]) - 1
        ncl = int(pred_cluster_ptr.numel()) - 1
        by_classifier = self.class_source == 'classifier'
        if by_classifier:
            if cluster_class is None:
                raise ValueError("class_source='classifier' needs the clusters' classes "
                                 '(cluster_class)')
            if int(cluster_class.numel()) < ncl:
                raise ValueError(f'cluster_class has {cluster_class.numel()} entries for {ncl} '
                                 'clusters')
        if association is not None:
            want = self._association_params(N, F, ncl)
            have = association.get('params')
            if have != want:
                raise ValueError(f'association= comes from an update with {have}, this one is '
                                 f'{want}: share an association only between evaluators updated '
                                 'on the same batch with the same criterion, eps and '
                                 'cluster_size_threshold')
        dev = node_cls.device
        if dev.type != 'cuda':
            raise ValueError('DetectionEvaluator.update needs device tensors')
        l2 = self.association_criteria == 'l2_norm'
        if l2 and xy is None and association is None:
            raise ValueError("association_criteria='l2_norm' needs the node positions (xy)")
        lib = nat.lib()
        st = nat.stream_ptr(dev)
        acc = self._device_counters(dev)
        if N == 0 or F <= 0:
            return self
        fptr = frame_ptr.to(torch.int32).contiguous()
        p_ptr = _full_ptr(pred_cluster_ptr, N)
        p_idx = pred_cluster_idx.to(torch.int32).contiguous()
        if by_classifier:
            p_cls = (cluster_class.detach().to(dev, torch.int64).reshape(-1).contiguous()
                     if ncl > 0 else torch.zeros(1, dtype=torch.int64, device=dev))
        elif self.by_segmentation:
            node_pred = argmax_rows(node_cls)
            p_cls = torch.empty(max(ncl, 1), dtype=torch.int64, device=dev)
            nat.check(lib.rg_cluster_majority_label(node_pred.data_ptr(), p_ptr.data_ptr(),
                                                    p_idx.data_ptr(), ncl, self.num_classes,
                                                    p_cls.data_ptr(), self._bad.data_ptr(), st),
                      'rg_cluster_majority_label')
        else:
            if int(obj_cls.shape[0]) < ncl:
                raise ValueError(f'obj_cls has {obj_cls.shape[0]} rows for {ncl} clusters')
            p_cls = argmax_rows(obj_cls) if ncl > 0 else torch.zeros(1, dtype=torch.int64,
                                                                     device=dev)
        gt_mu = pred_mu = None
        if association is not None:
            gt, res = association['gt'], association['assoc']
            gt_mu, pred_mu = association.get('gt_mu'), association.get('pred_mu')
            if 'bad_value' in res:
                self._bad[1:2].bitwise_or_(res['bad_value'])
        else:
            gt = gt_clusters(track_key, node_gt_class, fptr, self._ws)
            if l2:
                if int(xy.shape[0]) != N:
                    raise ValueError(f'xy has {xy.shape[0]} rows for {N} nodes')
                gt_mu = cluster_centres(xy, gt['cluster_ptr'], gt['cluster_idx'])
                pred_mu = cluster_centres(xy, p_ptr, p_idx)
                res = associate_l2(fptr, gt['cluster_ptr'], gt['cluster_idx'], p_ptr, p_idx,
                                   gt_mu, pred_mu, self.eps, self.cluster_size_threshold,
                                   max_frame_nodes, self._ws)
                # the kernel sets, never clears: one flag serves every update
                self._bad[1:2].bitwise_or_(res['bad_value'])
            else:
                p_of = cluster_of(p_ptr, p_idx, N)
                res = associate(fptr, gt['cluster_of'], gt['cluster_ptr'], gt['cluster_idx'],
                                p_of, p_ptr, p_idx, self.eps, self.cluster_size_threshold,
                                max_frame_nodes, self._ws)
        nat.check(lib.rg_eval_accumulate(
            res['pick_gt_cluster'].data_ptr(), res['pick_pred_cluster'].data_ptr(),
            res['pick_positive'].data_ptr(), res['gt_kept'].data_ptr(),
            res['pred_kept'].data_ptr(), gt['cluster_class'].data_ptr(), p_cls.data_ptr(), N,
            self.num_classes, self.false_class_label, acc['confusion_matrix'].data_ptr(),
            acc['gt_count_matrix'].data_ptr(), acc['pred_count_matrix'].data_ptr(),
            self._bad.data_ptr(), st), 'rg_eval_accumulate')
        self.last = dict(gt=gt, pred_class=p_cls[:ncl], assoc=res,
                         params=self._association_params(N, F, ncl))
        if l2:
            self.last.update(gt_mu=gt_mu, pred_mu=pred_mu)
        return self

    def update_frames(self, detector_outputs, node_gt_class, track_key, xy=None):
        """A batch straight from ``Model_Inference.forward_frames(..., cluster_node_idx=None,
        other_features)``: its 5-tuple (node_cls, node_reg, link_cls, obj_cls, per-frame lists
        of frame-local member indices), with the per-frame lists of ground-truth node classes
        and track keys and, under 'l2_norm', of node positions (xy: float32 [n, >= 2] each)."""
        torch = _torch()
        node_cls, _, _, obj_cls, lists = detector_outputs
        dev = node_cls.device
        sizes = [int(t.shape[0]) for t in node_gt_class]
        if len(lists) != len(sizes) or len(track_key) != len(sizes):
            raise ValueError('one cluster list, class tensor and key tensor per frame')
        bases = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        members, counts = [], []
        for f, frame in enumerate(lists):
            for m in frame:
                members.append(m.to(dev, torch.int64) + int(bases[f]))
                counts.append(int(m.shape[0]))
        N = int(bases[-1])
        idx = (torch.cat(members) if members else torch.zeros(0, dtype=torch.int64, device=dev))
        idx = idx.to(torch.int32)
        if idx.numel() < N:  # nodes in no cluster: pad the member list to its [N] form
            idx = torch.cat([idx, torch.zeros(N - idx.numel(), dtype=torch.int32, device=dev)])
        ptr = torch.from_numpy(np.concatenate(([0], np.cumsum(counts))).astype(np.int32)).to(dev)
        fptr = torch.from_numpy(bases.astype(np.int32)).to(dev)
        cat = lambda ts, dt: torch.cat([torch.as_tensor(t).reshape(-1).to(dev, dt)  # noqa: E731
                                        for t in ts]) if ts else torch.zeros(0, dtype=dt, device=dev)
        pos = None
        if self.association_criteria == 'l2_norm':
            if xy is None or len(xy) != len(sizes):
                raise ValueError("association_criteria='l2_norm' needs one xy array per frame")
            pos = (torch.cat([torch.as_tensor(t)[:, :2].to(dev, torch.float32) for t in xy])
                   if sizes else torch.zeros((0, 2), dtype=torch.float32, device=dev))
        return self.update(node_cls, obj_cls, ptr, idx, cat(node_gt_class, torch.int64),
                           cat(track_key, torch.int32), fptr,
                           max_frame_nodes=max(sizes) if sizes else 0, xy=pos)

    def result(self, invalid_class_index: Optional[int] = INVALID_CLS_IDX) -> dict:
        """One synchronisation: the three count matrices (numpy uint64) and the notebook's
        precision, recall and normalized_confusion_matrix (class 5 dropped)."""
        out = self.counts()
        out.update(detection_report(out['confusion_matrix'], out['gt_count_matrix'],
                                    out['pred_count_matrix'], invalid_class_index))
        return out


class SegmentationEvaluator(_Counters):
    """performance_eval_segmentation.ipynb on the device: confusion[gt class, predicted class]
    and gt_count over the nodes of every batch."""

    NAMES = ('confusion_matrix', 'gt_count_matrix')

    def __init__(self, num_classes: int = 7):
        super().__init__(num_classes)

    def update(self, node_cls, node_gt_class):
        """node_cls f32 [N, C] logits and node_gt_class [N] on the device; no host sync."""
        torch = _torch()
        x = _rows(node_cls)
        dev = x.device
        if dev.type != 'cuda':
            raise ValueError('SegmentationEvaluator.update needs device tensors')
        if int(x.shape[1]) != self.num_classes:
            raise ValueError(f'node_cls has {x.shape[1]} classes, evaluator {self.num_classes}')
        acc = self._device_counters(dev)
        gt = node_gt_class.to(dev, torch.int64).reshape(-1).contiguous()
        if gt.numel() != x.shape[0]:
            raise ValueError(f'{x.shape[0]} rows of logits, {gt.numel()} classes')
        nat.check(nat.lib().rg_eval_node_confusion(
            x.data_ptr(), x.stride(0) if x.shape[0] > 0 else self.num_classes, gt.data_ptr(),
            int(x.shape[0]), self.num_classes, acc['confusion_matrix'].data_ptr(),
            acc['gt_count_matrix'].data_ptr(), self._bad.data_ptr(), nat.stream_ptr(dev)),
            'rg_eval_node_confusion')
        return self

    def result(self, invalid_class_index: Optional[int] = INVALID_CLS_IDX) -> dict:
        out = self.counts()
        out.update(segmentation_report(out['confusion_matrix'], out['gt_count_matrix'],
                                       invalid_class_index))
        return out


class ObjectClassEvaluator(_Counters):
    """The object-level confusion matrix of the two-stage flow: confusion[gt class, predicted
    class] and gt_count over proposals, as SegmentationEvaluator keeps them over nodes.  The
    ground truth of a proposal is its majority node class, lowest label on a tie
    (datagen_classifier.py:50-60: what ``objects.classifier_inputs(node_labels=)`` returns as
    ``object_class`` and what the classifier trains on)."""

    NAMES = ('confusion_matrix', 'gt_count_matrix')

    def __init__(self, num_classes: int = 7):
        super().__init__(num_classes)

    def update(self, pred_class, gt_class):
        """pred_class and gt_class [rows] class ids on the device (rg_eval_class_confusion); no
        host sync."""
        torch = _torch()
        dev = pred_class.device
        if dev.type != 'cuda':
            raise ValueError('ObjectClassEvaluator.update needs device tensors')
        pred = pred_class.detach().to(torch.int64).reshape(-1).contiguous()
        gt = gt_class.detach().to(dev, torch.int64).reshape(-1).contiguous()
        if gt.numel() != pred.numel():
            raise ValueError(f'{pred.numel()} predicted classes, {gt.numel()} ground-truth '
                             'classes')
        acc = self._device_counters(dev)
        if pred.numel() > 0:
            nat.check(nat.lib().rg_eval_class_confusion(
                gt.data_ptr(), pred.data_ptr(), int(pred.numel()), self.num_classes,
                acc['confusion_matrix'].data_ptr(), acc['gt_count_matrix'].data_ptr(),
                self._bad.data_ptr(), nat.stream_ptr(dev)), 'rg_eval_class_confusion')
        return self

    def update_logits(self, logits, gt_class):
        """logits f32 [rows, C] (the classifier's, one row per kept object): the predicted
        class is ``argmax_rows``."""
        x = _rows(logits)
        if x.device.type != 'cuda':
            raise ValueError('ObjectClassEvaluator.update_logits needs device tensors')
        if int(x.shape[1]) != self.num_classes:
            raise ValueError(f'logits have {x.shape[1]} classes, evaluator {self.num_classes}')
        return self.update(argmax_rows(x), gt_class)

    def result(self, invalid_class_index: Optional[int] = INVALID_CLS_IDX) -> dict:
        out = self.counts()
        out.update(segmentation_report(out['confusion_matrix'], out['gt_count_matrix'],
                                       invalid_class_index))
        return out


class TwoStageEvaluators:
    """The two-stage flow scored next to the single-stage class sources, on one association.

    ``detection``: a DetectionEvaluator per class source ('segmentation', 'object_head',
    'classifier'; detection_accuracy.py:95-109 with the classifier as the third) -- per batch
    the first one associates, the other two accumulate on its picks
    (``share_association=False``: each associates for itself; the counts are the same).
    ``object_class``: an ObjectClassEvaluator per source over the proposals the classifier
    keeps (size >= min_meas), so the vote and the head are scored on the classifier's objects.

    The reference's detection evaluation keeps clusters of size > cluster_size_threshold, the
    classifier sees those of size >= min_meas: the constructor wants cluster_size_threshold >=
    min_meas - 1, so that every cluster the association keeps has a classifier class and no
    fill value ever reaches a count matrix.  detection_kwargs are DetectionEvaluator's (eps,
    cluster_size_threshold, false_class_label, association_criteria)."""

    SOURCES = DetectionEvaluator.CLASS_SOURCES

    def __init__(self, num_classes: int = 7, min_meas: int = 2, share_association: bool = True,
                 **detection_kwargs):
        for k in ('by_segmentation', 'class_source'):
            if k in detection_kwargs:
                raise ValueError(f'{k} is set per source by TwoStageEvaluators')
        if int(min_meas) < 0:
            raise ValueError(f'min_meas={min_meas} < 0')
        thr = int(detection_kwargs.get('cluster_size_threshold', 0))
        if thr < int(min_meas) - 1:
            raise ValueError(f'cluster_size_threshold={thr} < min_meas - 1 = {int(min_meas) - 1}: '
                             'the association would keep clusters the classifier never sees')
        self.num_classes = int(num_classes)
        self.min_meas = int(min_meas)
        self.share_association = bool(share_association)
        self.detection = {s: DetectionEvaluator(num_classes, class_source=s, **detection_kwargs)
                          for s in self.SOURCES}
        self.object_class = {s: ObjectClassEvaluator(num_classes) for s in self.SOURCES}

    @property
    def association_criteria(self) -> str:
        return self.detection['segmentation'].association_criteria

    def shares_with(self, other: DetectionEvaluator) -> bool:
        """Whether ``other``'s association of a batch is the one these evaluators would make."""
        d = self.detection['segmentation']
        return (self.share_association and other.association_criteria == d.association_criteria
                and other.eps == d.eps
                and other.cluster_size_threshold == d.cluster_size_threshold)

    def update(self, node_cls, obj_cls, pred_cluster_ptr, pred_cluster_idx, node_gt_class,
               track_key, frame_ptr, classified: dict, max_frame_nodes: Optional[int] = None,
               xy=None, association: Optional[dict] = None):
        """One batch: DetectionEvaluator.update's arguments and ``classified``, the dict of
        ``objects.classify_detections(..., node_labels=node_gt_class)`` on the same clusters.
        ``association``: the ``last`` of a DetectionEvaluator already updated on this batch
        with the same criterion, eps and threshold (``shares_with``), to associate not even
        once here.  No host synchronisation."""
        torch = _torch()
        N, F = int(node_cls.shape[0]), int(frame_ptr.shape[0]) - 1
        inp = classified['inputs']
        if inp.object_class is None:
            raise ValueError('classify_detections was run without node_labels: no ground truth '
                             'per object')
        if inp.min_meas != self.min_meas:
            raise ValueError(f'the classifier kept proposals of size >= {inp.min_meas}, these '
                             f'evaluators were built for min_meas={self.min_meas}')
        if N == 0 or F <= 0:
            return self
        ccls = classified['cluster_class']
        for s in self.SOURCES:
            self.detection[s].update(node_cls, obj_cls, pred_cluster_ptr, pred_cluster_idx,
                                     node_gt_class, track_key, frame_ptr,
                                     max_frame_nodes=max_frame_nodes, xy=xy, cluster_class=ccls,
                                     association=association)
            if self.share_association and association is None:
                association = self.detection[s].last
        clf = self.object_class['classifier']
        clf._device_counters(node_cls.device)
        clf._bad[2:3].bitwise_or_(classified['bad'])
        if inp.n_objects == 0:
            return self
        oc = inp.object_cluster.to(torch.int64)
        clf.update_logits(classified['logits'], inp.object_class)
        for s in ('segmentation', 'object_head'):
            pred = self.detection[s].last['pred_class'].index_select(0, oc)
            self.object_class[s].update(pred, inp.object_class)
        return self

    def merge(self, other):
        """Add another TwoStageEvaluators' counters (another rank's, another sequence's)."""
        if type(other) is not type(self) or other.num_classes != self.num_classes \
                or other.min_meas != self.min_meas:
            raise ValueError('merge needs TwoStageEvaluators of the same num_classes and '
                             'min_meas')
        for s in self.SOURCES:
            self.detection[s].merge(other.detection[s])
            self.object_class[s].merge(other.object_class[s])
        return self

    def result(self, invalid_class_index: Optional[int] = INVALID_CLS_IDX) -> dict:
        """One dict per source: {'detection': DetectionEvaluator.result(), 'object_class':
        ObjectClassEvaluator.result()}."""
        return {s: dict(detection=self.detection[s].result(invalid_class_index),
                        object_class=self.object_class[s].result(invalid_class_index))
                for s in self.SOURCES}

    def to_json(self, prefix, class_names) -> dict:
        """The reference's per-sequence files, two per source: ``<prefix>_<source>_detection
        .json`` and ``<prefix>_<source>_object_class.json``."""
        return {s: dict(
            detection=self.detection[s].to_json(f'{prefix}_{s}_detection.json', class_names),
            object_class=self.object_class[s].to_json(f'{prefix}_{s}_object_class.json',
                                                      class_names))
            for s in self.SOURCES}


# ------------------------------------------------------------------------- a whole sequence
def evaluate_window_batch(win, model, cfg, detection: Optional[DetectionEvaluator] = None,
                          segmentation: Optional[SegmentationEvaluator] = None,
                          dtype: str = 'fp32', reject_outlier_by_ransac: bool = False,
                          cache: Optional[dict] = None, classifier=None,
                          two_stage: Optional[TwoStageEvaluators] = None, meas_noise_cov=None):
    """One batch of windows (a batch ``frontend.ScanWindow``) through the front-end, the graph
    build, the detector's proposal forward and the evaluators' ``update``: what the notebooks
    do per frame (performance_eval_detection.ipynb, performance_eval_segmentation.ipynb),
    for every window of the batch at once.  ``model`` is a ``Model_Inference`` with its
    proposal parameters set; ``cache`` keeps workspaces and buffers between batches.  Returns
    the batch's FrameBatch (``frontend.frame_batch``) and the forward's outputs (None for a
    batch without a frame of more than one node).

    With ``classifier`` (the cluster-level classifier's model; ``two_stage`` is then required)
    the batch also runs ``objects.classify_detections`` with the ground-truth node classes
    (``two_stage.min_meas``; ``meas_noise_cov`` defaults to the detector's) and updates
    ``two_stage``, on ``detection``'s association where ``two_stage.shares_with(detection)``.
    The one host read that adds is ``objects.classifier_inputs``'.  Without a classifier
    nothing of this runs."""
    from . import frontend, objects
    if not getattr(model, 'extract_proposals', False):
        raise ValueError('the detector has no proposal branch: set_param_for_proposal_extraction')
    if classifier is not None and two_stage is None:
        raise ValueError('a classifier needs the evaluators it updates (two_stage)')
    cache = cache if cache is not None else {}
    dd, gd = frontend.dynamic_frame(win, reject_outlier_by_ransac, with_keys=True)
    fb = frontend.frame_batch(dd, gd)
    det = objects.detect_frames(model, fb, cfg, dtype, cache)
    if det is None:
        return fb, None
    out = det.outputs
    gt_class = fb.labels['class_labels']
    if detection is not None:
        xy = det.xy if detection.association_criteria == 'l2_norm' else None
        detection.update(out.node_cls, out.obj_cls, out.cluster_ptr, out.cluster_idx, gt_class,
                         fb.track_key, fb.frame_ptr, max_frame_nodes=max(fb.frame_sizes), xy=xy)
    if segmentation is not None:
        segmentation.update(out.node_cls, gt_class)
    if classifier is not None:
        res = objects.classify_detections(det, classifier, two_stage.min_meas, meas_noise_cov,
                                          node_labels=gt_class,
                                          num_classes=two_stage.num_classes)
        shared = None
        if detection is not None and fb.n_nodes > 0 and two_stage.shares_with(detection):
            shared = detection.last
        xy = det.xy if two_stage.association_criteria == 'l2_norm' else None
        two_stage.update(out.node_cls, out.obj_cls, out.cluster_ptr, out.cluster_idx, gt_class,
                         fb.track_key, fb.frame_ptr, res, max_frame_nodes=max(fb.frame_sizes),
                         xy=xy, association=shared)
    return fb, out


def evaluate_sequence(store, model, cfg, window_size: int = 10, batch_windows: int = 64,
                      dtype: str = 'fp32', detection: Optional[DetectionEvaluator] = None,
                      segmentation: Optional[SegmentationEvaluator] = None,
                      reject_outlier_by_ransac: bool = False, classifier=None,
                      two_stage: Optional[TwoStageEvaluators] = None, meas_noise_cov=None):
    """Every sliding window of a ``sequence.SequenceStore`` to the notebooks' count matrices:
    per batch of ``batch_windows`` consecutive sliding positions ``store.windows`` ->
    ``evaluate_window_batch``.  No host work per window; per batch the host waits only where
    ``frontend.select_dynamic`` and ``engine.propose_clusters`` already do and for the one
    ``frame_ptr`` read of ``frontend.frame_batch``.  Returns (detection, segmentation), new
    evaluators unless given; their ``result()`` is the only read of the counters.

    With ``classifier`` every batch also goes through the second stage and the return is
    (detection, segmentation, two_stage): ``two_stage`` a TwoStageEvaluators, by default of
    min_meas = 2 with ``detection``'s eps and criterion and its cluster_size_threshold raised
    to at least 1 (the least the constructor accepts for min_meas = 2).  Per batch the host
    waits once more, in ``objects.classifier_inputs``."""
    if int(batch_windows) < 1:
        raise ValueError(f'batch_windows={batch_windows} < 1')
    detection = detection if detection is not None else DetectionEvaluator(int(cfg.num_classes))
    segmentation = (segmentation if segmentation is not None
                    else SegmentationEvaluator(int(cfg.num_classes)))
    if classifier is not None and two_stage is None:
        two_stage = TwoStageEvaluators(
            detection.num_classes, min_meas=2, eps=detection.eps,
            cluster_size_threshold=max(detection.cluster_size_threshold, 1),
            false_class_label=detection.false_class_label,
            association_criteria=detection.association_criteria)
    n = store.n_windows(window_size)
    cache: dict = {}
    for i0 in range(0, n, int(batch_windows)):
        win = store.windows(range(i0, min(i0 + int(batch_windows), n)), window_size)
        if classifier is None:
            evaluate_window_batch(win, model, cfg, detection, segmentation, dtype,
                                  reject_outlier_by_ransac, cache)
        else:
            evaluate_window_batch(win, model, cfg, detection, segmentation, dtype,
                                  reject_outlier_by_ransac, cache, classifier, two_stage,
                                  meas_noise_cov)
    if classifier is None:
        return detection, segmentation
    return detection, segmentation, two_stage
