"""The object stage on the GPU (csrc/objects.hip): from the detector's clusters to the object
list and to the cluster-level classifier's inputs, for a batch of frames, with no host loop.

  cluster_stats        compute_cluster_sample_mean_and_cov / compute_proposals
                       (modules/inference/inference.py:23-47) + np.linalg.eig of the covariance
  cov_ellipse          compute_cov_ellipse (modules/inference/ellipse.py:4-37)
  classifier_inputs    extract_and_compute_features_and_labels + remove_low_quality_proposals
                       + compute_graph (data_generator/datagen_classifier.py:35-124, 166-190)
  object_list          the numbers of process_frame (modules/inference/output.py:99-171)
  compute_proposals, compute_cov_ellipse    drop-ins with the reference's signatures
  detect, classify_proposals, classifier_training_batch    the two-stage glue
  classify_detections, cluster_class_from_objects    the classifier as a class source per
                       proposal cluster (output.py:111-128 with the second stage's class)

Everything works on global node ids, ``frame_ptr`` int32 [F + 1] and clusters as the CSR that
``engine.propose_clusters`` returns.  Kernels are enqueued on the current stream.
``classifier_inputs`` reads three integers back once (kept objects, member rows, edges) to size
its tensors and the classifier graph; ``object_list`` reads the number of kept objects on first
use.  These are the stage's only synchronisations.

The mean and the covariance are bit-identical to the reference: one thread owns a cluster and
adds its members in list order in float32 without contraction, which is numpy's order.  The
eigen-decomposition follows LAPACK's 2 x 2 standardisation (``eig_sym2_np`` restates it).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import _native as nat


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------- the eigen convention
def eig_sym2_np(cov):
    """np.linalg.eig of a symmetric float32 2 x 2 matrix [[a, b], [b, d]] restated in numpy
    float32, as the kernel computes it (LAPACK sgeev -> slanv2): b == 0 gives (a, d) and the
    identity; otherwise p = (a - d) / 2, z = p + sign(p) sqrt(p^2 + b^2) (+ when p == 0, the
    root scaled as LAPACK does), values (d + z, d - b / z * b), vectors the columns (z, b) / h
    and (-b, z) / h with h = hypot(b, z).  Returns (values [2], vectors [2, 2])."""
    f = np.float32
    cov = np.asarray(cov, dtype=f)
    a, b, d = cov[0, 0], cov[0, 1], cov[1, 1]
    if b == 0:
        return np.array([a, d], f), np.eye(2, dtype=f)
    p = f(0.5) * (a - d)
    ab = np.abs(b)
    scale = max(np.abs(p), ab)
    zz = p / scale * p + ab / scale * ab
    z = p + np.copysign(np.sqrt(scale) * np.sqrt(zz), p)
    tau = np.hypot(b, z)
    cs, sn = z / tau, b / tau
    return (np.array([d + z, d - ab / z * ab], f), np.array([[cs, -sn], [sn, cs]], f))


# ---------------------------------------------------------------- helpers
def _xy(t):
    torch = _torch()
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.dim() != 2 or t.shape[1] < 2:
        raise ValueError(f'expected [N, >= 2] positions, got {tuple(t.shape)}')
    if t.shape[0] > 0 and t.stride(1) != 1:
        t = t.contiguous()
    return t


def _col(t):
    """A float32 column as (tensor, element stride)."""
    torch = _torch()
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.dim() != 1:
        raise ValueError(f'expected a column, got {tuple(t.shape)}')
    return t, (int(t.stride(0)) if t.numel() > 1 else 1)


def _noise(meas_noise_cov) -> np.ndarray:
    n = np.ascontiguousarray(np.asarray(meas_noise_cov, dtype=np.float32).reshape(2, 2))
    if n[0, 1] != n[1, 0]:
        raise ValueError('meas_noise_cov is not symmetric')
    return n


def _i32(t):
    torch = _torch()
    return t.to(torch.int32).contiguous()


def _empty(dev, shape, dtype):
    """An uninitialised tensor that always has storage (a kernel may be handed its pointer)."""
    torch = _torch()
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape)) if shape else 1
    return torch.empty(max(n, 1), dtype=dtype, device=dev)[:n].reshape(shape)


def _frame_ptr(frame_ptr, N, dev):
    torch = _torch()
    if frame_ptr is None:
        return torch.tensor([0, N], dtype=torch.int32, device=dev)
    return _i32(frame_ptr.to(dev))


# ---------------------------------------------------------------- statistics and ellipse
def cluster_stats(xy, cluster_ptr, cluster_idx, meas_noise_cov) -> dict:
    """Per cluster (rg_cluster_stats), device tensors, no synchronisation: size int32 [K], mu
    f32 [K, 2], sigma f32 [K, 2, 2], eigval f32 [K, 2], eigvec f32 [K, 2, 2] (columns), bad
    int32 [1] (set when a member index lies outside the nodes).  xy f32 [N, >= 2],
    cluster_ptr int32 [K + 1], cluster_idx int32 [<= N]."""
    torch = _torch()
    xy = _xy(xy)
    dev = xy.device
    N, K = int(xy.shape[0]), int(cluster_ptr.numel()) - 1
    if int(cluster_idx.numel()) > max(N, 1):
        raise ValueError(f'{cluster_idx.numel()} members for {N} nodes: clusters overlap')
    ptr, idx = _i32(cluster_ptr), _i32(cluster_idx)
    noise = _noise(meas_noise_cov)
    f32 = torch.float32
    out = dict(size=_empty(dev, K, torch.int32), mu=_empty(dev, (K, 2), f32),
               sigma=_empty(dev, (K, 2, 2), f32), eigval=_empty(dev, (K, 2), f32),
               eigvec=_empty(dev, (K, 2, 2), f32),
               bad=torch.zeros(1, dtype=torch.int32, device=dev))
    if K > 0:
        nat.check(nat.lib().rg_cluster_stats(
            xy.data_ptr(), xy.stride(0), N, ptr.data_ptr(), idx.data_ptr(), K, noise.ctypes.data,
            out['size'].data_ptr(), out['mu'].data_ptr(), out['sigma'].data_ptr(),
            out['eigval'].data_ptr(), out['eigvec'].data_ptr(), out['bad'].data_ptr(),
            nat.stream_ptr(dev)), 'rg_cluster_stats')
    return out


def cov_ellipse(stats: dict, chi_sq: float = 2, n_points: int = 100, points: bool = True) -> dict:
    """compute_cov_ellipse of every cluster of ``cluster_stats`` (rg_cov_ellipse): a, b, theta
    f32 [K] and, with ``points``, the boundary f32 [K, n_points, 2].  Defaults as output.py:165."""
    torch = _torch()
    if int(n_points) < 1:
        raise ValueError(f'n_points={n_points} < 1')
    mu = stats['mu']
    dev, K = mu.device, int(mu.shape[0])
    abt = _empty(dev, (K, 3), torch.float32)
    pts = _empty(dev, (K, int(n_points), 2), torch.float32) if points else None
    if K > 0:
        nat.check(nat.lib().rg_cov_ellipse(
            stats['eigval'].data_ptr(), stats['eigvec'].data_ptr(), mu.data_ptr(), K,
            float(chi_sq), int(n_points), abt.data_ptr(), nat.ptr(pts), nat.stream_ptr(dev)),
            'rg_cov_ellipse')
    return dict(a=abt[:, 0], b=abt[:, 1], theta=abt[:, 2], abt=abt, points=pts)


def softmax_max(logits):
    """(class int64 [rows], score f32 [rows]) = torch.max(softmax(logits, -1), -1): the first
    maximum, as evaluation.argmax_rows, and its float32 softmax value (rg_softmax_max)."""
    torch = _torch()
    x = logits.detach()
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.dim() != 2:
        raise ValueError(f'expected a [rows, classes] matrix, got {tuple(x.shape)}')
    n, nc = int(x.shape[0]), int(x.shape[1])
    if not 1 <= nc <= 32:
        raise ValueError(f'num_classes={nc} outside 1..32')
    if n > 0 and x.stride(1) != 1:
        x = x.contiguous()
    cls = _empty(x.device, n, torch.int64)
    score = _empty(x.device, n, torch.float32)
    if n > 0:
        nat.check(nat.lib().rg_softmax_max(x.data_ptr(), x.stride(0), n, nc, cls.data_ptr(),
                                           score.data_ptr(), nat.stream_ptr(x.device)),
                  'rg_softmax_max')
    return cls, score


def majority_class(node_class, cluster_ptr, cluster_idx, num_classes: int, bad=None):
    """int64 [K]: the most frequent member class, lowest class on a tie (compute_object_labels;
    torch.argmax(torch.bincount(...)) of output.py:116) -- rg_cluster_majority_label."""
    torch = _torch()
    dev = cluster_ptr.device
    K = int(cluster_ptr.numel()) - 1
    out = _empty(dev, K, torch.int64)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if K > 0:
        lab = node_class.to(dev, torch.int64).contiguous()
        nat.check(nat.lib().rg_cluster_majority_label(
            lab.data_ptr(), cluster_ptr.data_ptr(), cluster_idx.data_ptr(), K, int(num_classes),
            out.data_ptr(), bad.data_ptr(), nat.stream_ptr(dev)), 'rg_cluster_majority_label')
    return out


def cluster_class_from_objects(logits, object_cluster, n_clusters: int, fill_class: int,
                               bad=None):
    """(class int64 [K], score f32 [K]) of the K = n_clusters proposal clusters from the
    cluster-level classifier's logits f32 [K', classes] per kept object and object_cluster int32
    [K'] (ClassifierInputs.object_cluster): ``softmax_max`` of every row, bit for bit, at the
    slot of its source cluster; ``fill_class`` and 0.0 for a cluster that no object names
    (rg_cluster_class_from_objects).  No synchronisation: an object_cluster entry outside
    [0, K) sets ``bad`` (int32 [1] on the device, the stage's ``stats['bad']``; a private flag
    when None) and writes nothing."""
    torch = _torch()
    x = logits.detach()
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.dim() != 2:
        raise ValueError(f'expected a [objects, classes] matrix, got {tuple(x.shape)}')
    n, nc, K = int(x.shape[0]), int(x.shape[1]), int(n_clusters)
    if not 1 <= nc <= 32:
        raise ValueError(f'num_classes={nc} outside 1..32')
    if K < 0:
        raise ValueError(f'n_clusters={n_clusters} < 0')
    if int(object_cluster.numel()) != n:
        raise ValueError(f'{object_cluster.numel()} source clusters for {n} objects')
    if n > 0 and x.stride(1) != 1:
        x = x.contiguous()
    dev = x.device
    oc = _i32(object_cluster.to(dev))
    cls = _empty(dev, K, torch.int64)
    score = _empty(dev, K, torch.float32)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if K > 0:
        nat.check(nat.lib().rg_cluster_class_from_objects(
            x.data_ptr(), int(x.stride(0)) if n > 0 else nc, n, nc, oc.data_ptr(), K,
            int(fill_class), cls.data_ptr(), score.data_ptr(), bad.data_ptr(),
            nat.stream_ptr(dev)), 'rg_cluster_class_from_objects')
    return cls, score


def _select(ptr, idx, fptr, F, cls, num_classes, min_meas, drop_class):
    """rg_object_select: device tensors sized by the cluster count (no synchronisation)."""
    torch = _torch()
    dev = ptr.device
    K = int(ptr.numel()) - 1
    i32 = torch.int32
    sel = dict(cluster_row=_empty(dev, K, i32), obj_cluster=_empty(dev, K, i32),
               obj_row_ptr=_empty(dev, K + 1, i32), frame_obj_ptr=_empty(dev, F + 1, i32),
               frame_row_ptr=_empty(dev, F + 1, i32),
               counts=torch.zeros(3, dtype=torch.int64, device=dev))
    lib = nat.lib()
    wsz = lib.rg_object_select_workspace_size(K)
    ws = torch.empty(max(int(wsz), 1), dtype=torch.uint8, device=dev)
    nat.check(lib.rg_object_select(
        ptr.data_ptr(), idx.data_ptr(), K, fptr.data_ptr(), F, nat.ptr(cls), int(num_classes),
        int(min_meas), int(drop_class), sel['cluster_row'].data_ptr(),
        sel['obj_cluster'].data_ptr(), sel['obj_row_ptr'].data_ptr(),
        sel['frame_obj_ptr'].data_ptr(), sel['frame_row_ptr'].data_ptr(),
        sel['counts'].data_ptr(), ws.data_ptr(), wsz, nat.stream_ptr(dev)), 'rg_object_select')
    return sel


def _gather(sel, K, stats, ptr, idx, fptr, F, cls=None, score=None, ellipse=None):
    """rg_object_gather into tensors sized by the cluster count."""
    torch = _torch()
    dev = ptr.device
    f32 = torch.float32
    out = dict(size=_empty(dev, K, torch.int64), mu=_empty(dev, (K, 2), f32),
               sigma=_empty(dev, (K, 2, 2), f32), frame=_empty(dev, K, torch.int32),
               cls=_empty(dev, K, torch.int64) if cls is not None else None,
               score=_empty(dev, K, f32) if score is not None else None,
               ellipse=_empty(dev, (K, 3), f32) if ellipse is not None else None)
    if K > 0:
        nat.check(nat.lib().rg_object_gather(
            sel['obj_cluster'].data_ptr(), sel['counts'].data_ptr(), K, stats['size'].data_ptr(),
            nat.ptr(cls), nat.ptr(score), stats['mu'].data_ptr(), stats['sigma'].data_ptr(),
            nat.ptr(ellipse), ptr.data_ptr(), idx.data_ptr(), fptr.data_ptr(), F,
            out['size'].data_ptr(), nat.ptr(out['cls']), nat.ptr(out['score']),
            out['mu'].data_ptr(), out['sigma'].data_ptr(), nat.ptr(out['ellipse']),
            out['frame'].data_ptr(), nat.stream_ptr(dev)), 'rg_object_gather')
    return out


# ---------------------------------------------------------------- classifier inputs
class ClassifierInputs:
    """The classifier's inputs for a batch of frames, on the device.

    object_features f32 [M', 5], object_num_meas int64 [K'], object_class int64 [K'] (None
    without labels), object_mu f32 [K', 2], object_sigma f32 [K', 2, 2], object_cluster int32
    [K'] (the source cluster of every kept object), object_frame int32 [K'], frame_obj_ptr /
    frame_row_ptr int32 [F + 1] (each frame's range of objects / feature rows); n_objects,
    n_rows, n_edges, max_size (the largest kept object; 0 with none) and min_meas (the size
    threshold the objects were kept by) are host integers."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def graph(self):
        """(DeviceGraph, begin, end): the batch's complete-graph union and the reference's
        pooling ranges, built from the object sizes on the device (no edge list)."""
        from .classifier import engine as ce
        g = ce.object_graph(self.object_num_meas, self.n_rows, self.n_edges)
        begin, end = self.ranges()
        return g, begin, end

    def ranges(self):
        """(begin, end): the reference's pooling ranges alone -- with object_num_meas, n_rows
        and n_edges all that classifier.engine.forward_objects needs (no graph)."""
        from .classifier import engine as ce
        return ce.object_row_ranges(self.object_num_meas, self.frame_obj_ptr,
                                    self.frame_row_ptr, self.n_frames)

    def samples(self) -> List[dict]:
        """The reference's per-frame ``training_data`` dicts (datagen_classifier.py:272-280):
        object_features, object_class, object_num_meas, edge_idx (int64 [2, E], built by
        rg_object_complete_graph).  Frames without a kept object are omitted, as collate_fn
        omits them.  Reads the frame ranges and the sizes back (host view)."""
        from .classifier import engine as ce
        if self.n_objects == 0:
            return []
        fo = self.frame_obj_ptr.cpu().tolist()
        fr = self.frame_row_ptr.cpu().tolist()
        sizes = self.object_num_meas.cpu().numpy()
        out = []
        for f in range(self.n_frames):
            o0, o1, r0, r1 = fo[f], fo[f + 1], fr[f], fr[f + 1]
            if o1 == o0:
                continue
            osz = self.object_num_meas[o0:o1]
            n_edges = int(np.sum(sizes[o0:o1] * (sizes[o0:o1] - 1)))
            _, _, ei = ce.object_complete_graph(osz, r1 - r0, n_edges)
            out.append(dict(object_features=self.object_features[r0:r1],
                            object_class=(self.object_class[o0:o1]
                                          if self.object_class is not None else None),
                            object_num_meas=osz, edge_idx=ei, frame=f))
        return out


def classifier_inputs(xy, rcs, cluster_ptr, cluster_idx, frame_ptr=None, meas_noise_cov=None,
                      min_meas: int = 2, node_labels=None, num_classes: int = 7,
                      stats: Optional[dict] = None) -> ClassifierInputs:
    """extract_and_compute_features_and_labels + remove_low_quality_proposals + compute_graph
    for a whole batch.  xy f32 [N, >= 2], rcs f32 [N] (any stride), the clusters' CSR over
    global node ids, frame_ptr int32 [F + 1] (None: one frame), node_labels [N] (optional: the
    object class is their majority, lowest label on a tie).  A cluster is kept when its size
    >= min_meas (cfg.valid_cluster_num_meas_thr).

    ONE host read: the three integers (kept objects, member rows, edges) that size the outputs
    and the classifier graph, and the largest kept object (the training tape's bound) -- the
    only synchronisation of the stage."""
    torch = _torch()
    if int(min_meas) < 0:
        raise ValueError(f'min_meas={min_meas} < 0')
    if not 1 <= int(num_classes) <= 32:
        raise ValueError(f'num_classes={num_classes} outside 1..32')
    xy = _xy(xy)
    dev = xy.device
    N, K = int(xy.shape[0]), int(cluster_ptr.numel()) - 1
    ptr, idx = _i32(cluster_ptr), _i32(cluster_idx)
    fptr = _frame_ptr(frame_ptr, N, dev)
    F = int(fptr.numel()) - 1
    if stats is None:
        stats = cluster_stats(xy, ptr, idx, meas_noise_cov)
    cls = None
    if node_labels is not None:
        cls = majority_class(node_labels, ptr, idx, num_classes, stats['bad'])
    sel = _select(ptr, idx, fptr, F, None, num_classes, min_meas, -1)
    obj = _gather(sel, K, stats, ptr, idx, fptr, F, cls=cls)
    rcs_t, ld_rcs = _col(rcs)
    feats = _empty(dev, (int(idx.numel()), 5), torch.float32)
    if K > 0 and N > 0:
        nat.check(nat.lib().rg_object_features(
            xy.data_ptr(), xy.stride(0), rcs_t.data_ptr(), ld_rcs, N, ptr.data_ptr(),
            idx.data_ptr(), K, sel['cluster_row'].data_ptr(), stats['mu'].data_ptr(),
            stats['eigvec'].data_ptr(), feats.data_ptr(), nat.stream_ptr(dev)),
            'rg_object_features')
    # the largest kept object, over the kept entries only (obj['size'] past counts[0] is
    # uninitialised); it rides the one read
    kept = torch.arange(K, device=dev) < sel['counts'][0]
    mx = torch.where(kept, obj['size'], torch.zeros_like(obj['size'])).max().reshape(1) \
        if K > 0 else torch.zeros(1, dtype=torch.int64, device=dev)
    head = torch.cat([sel['counts'], stats['bad'].to(torch.int64), mx])
    head = head.cpu().tolist()                                               # the one read
    Kp, Mp, Ep, bad, max_size = (int(v) for v in head)
    if bad:
        raise RuntimeError('a member index or a node label outside its range reached the '
                           'object stage')
    return ClassifierInputs(
        object_features=feats[:Mp], object_num_meas=obj['size'][:Kp],
        object_class=obj['cls'][:Kp] if cls is not None else None, object_mu=obj['mu'][:Kp],
        object_sigma=obj['sigma'][:Kp], object_cluster=sel['obj_cluster'][:Kp],
        object_frame=obj['frame'][:Kp], obj_row_ptr=sel['obj_row_ptr'][:Kp + 1],
        frame_obj_ptr=sel['frame_obj_ptr'], frame_row_ptr=sel['frame_row_ptr'], n_objects=Kp,
        n_rows=Mp, n_edges=Ep, n_frames=F, max_size=max_size, stats=stats,
        min_meas=int(min_meas))


# ---------------------------------------------------------------- object list
class ObjectList:
    """process_frame's numbers for a batch (output.py:99-171), device tensors.

    Per node: node_class int64 / node_score f32 [N]; per link pair: link_class / link_score;
    per cluster: cluster_class int64 [K] (and cluster_score with the object head), the
    statistics ``stats`` and ``ellipse`` of every cluster; proposal centres when given.  Per
    remaining object (class != false class): obj_cluster, obj_frame, obj_class, obj_score,
    obj_size, obj_mu, obj_sigma, obj_ellipse (a, b, theta), obj_points.  The per-object tensors
    are sliced to the number of remaining objects, read back once on first use."""

    _PER_OBJECT = ('cluster', 'frame', 'class', 'score', 'size', 'mu', 'sigma', 'ellipse')

    def __init__(self, padded: dict, counts, frame_obj_ptr, n_frames, **kw):
        self._padded = padded
        self._counts = counts
        self._n = None
        self.frame_obj_ptr = frame_obj_ptr
        self.n_frames = n_frames
        self.__dict__.update(kw)

    @property
    def n_objects(self) -> int:
        if self._n is None:
            self._n = int(self._counts[0].item())
        return self._n

    def __getattr__(self, name):
        if name.startswith('obj_') and name[4:] in self._PER_OBJECT:
            t = self._padded[name[4:]]
            return None if t is None else t[:self.n_objects]
        raise AttributeError(name)

    @property
    def obj_points(self):
        """Boundary points f32 [objects, n_points, 2] of the remaining objects."""
        pts = self.ellipse['points']
        if pts is None:
            return None
        return pts[self.obj_cluster.to(_torch().int64)]

    def frames(self) -> List[dict]:
        """The per-frame host view: numpy arrays of the frame's remaining objects (cluster,
        obj_class, score, size, mean, cov, ellipse a / b / theta, boundary points)."""
        fo = self.frame_obj_ptr.cpu().tolist()
        h = {k: getattr(self, 'obj_' + k) for k in self._PER_OBJECT}
        h = {k: v.cpu().numpy() for k, v in h.items() if v is not None}
        pts = self.obj_points
        pts = pts.cpu().numpy() if pts is not None else None
        out = []
        for f in range(self.n_frames):
            sl = slice(fo[f], fo[f + 1])
            d = dict(cluster=h['cluster'][sl], obj_class=h['class'][sl], size=h['size'][sl],
                     mean=h['mu'][sl], cov=h['sigma'][sl], ellipse=h['ellipse'][sl])
            if 'score' in h:
                d['score'] = h['score'][sl]
            if pts is not None:
                d['boundary_points'] = pts[sl]
            out.append(d)
        return out


def object_list(node_cls, link_cls, obj_cls, xy, cluster_ptr, cluster_idx, frame_ptr=None,
                meas_noise_cov=None, detect_object_by_segmentation_output: bool = True,
                false_class: Optional[int] = None, chi_sq: float = 2, n_points: int = 100,
                points: bool = True, centres=None, cluster_class=None,
                cluster_score=None) -> ObjectList:
    """process_frame (output.py:99-171) for a batch: node / link class and score (max of the
    float32 softmax), the object class by the majority of the node classes or by the object
    head, the false-class filter (num_classes - 1), and size, mean, covariance and ellipse of
    the remaining objects.  No synchronisation here.

    ``cluster_class`` (int64 [K], on the device) is the third class source and takes precedence
    over both: the classes of the cluster-level classifier as ``cluster_class_from_objects``
    scatters them (output.py:111-128 with the second stage's class), ``cluster_score`` (f32 [K],
    optional) their scores.  A proposal the classifier never saw carries the false class there,
    so the filter drops it."""
    torch = _torch()
    xy = _xy(xy)
    dev = xy.device
    N, K = int(xy.shape[0]), int(cluster_ptr.numel()) - 1
    nc = int(node_cls.shape[1])
    false_class = nc - 1 if false_class is None else int(false_class)
    ptr, idx = _i32(cluster_ptr), _i32(cluster_idx)
    fptr = _frame_ptr(frame_ptr, N, dev)
    F = int(fptr.numel()) - 1
    node_class, node_score = softmax_max(node_cls)
    link_class = link_score = None
    if link_cls is not None:
        link_class, link_score = softmax_max(link_cls)
    stats = cluster_stats(xy, ptr, idx, meas_noise_cov)
    if cluster_class is not None:
        if int(cluster_class.numel()) < K:
            raise ValueError(f'cluster_class has {cluster_class.numel()} entries for {K} clusters')
        ccls = cluster_class.detach().to(dev, torch.int64).reshape(-1)[:K].contiguous()
        cscore = None
        if cluster_score is not None:
            if int(cluster_score.numel()) < K:
                raise ValueError(f'cluster_score has {cluster_score.numel()} entries for {K} '
                                 'clusters')
            cscore = cluster_score.detach().to(dev, torch.float32).reshape(-1)[:K].contiguous()
    elif detect_object_by_segmentation_output:
        ccls, cscore = majority_class(node_class, ptr, idx, nc, stats['bad']), None
    else:
        if int(obj_cls.shape[0]) < K:
            raise ValueError(f'obj_cls has {obj_cls.shape[0]} rows for {K} clusters')
        ccls, cscore = softmax_max(obj_cls[:K])
    ell = cov_ellipse(stats, chi_sq, n_points, points)
    sel = _select(ptr, idx, fptr, F, ccls if K > 0 else None, nc, 0, false_class if K > 0 else -1)
    obj = _gather(sel, K, stats, ptr, idx, fptr, F, cls=ccls, score=cscore, ellipse=ell['abt'])
    padded = {'cluster': sel['obj_cluster'], 'frame': obj['frame'], 'class': obj['cls'],
              'score': obj['score'], 'size': obj['size'], 'mu': obj['mu'], 'sigma': obj['sigma'],
              'ellipse': obj['ellipse']}
    return ObjectList(padded, sel['counts'], sel['frame_obj_ptr'], F, node_class=node_class,
                      node_score=node_score, link_class=link_class, link_score=link_score,
                      cluster_class=ccls, cluster_score=cscore, stats=stats, ellipse=ell,
                      centres=centres, false_class=false_class)


# ---------------------------------------------------------------- drop-ins
def _csr_from_lists(cluster_members_list, dev):
    torch = _torch()
    mem = [torch.as_tensor(m).reshape(-1).to(torch.int64) for m in cluster_members_list]
    lens = [int(m.numel()) for m in mem]
    ptr = torch.tensor(np.concatenate(([0], np.cumsum(lens))).astype(np.int32), device=dev)
    idx = (torch.cat([m.to(dev) for m in mem]) if mem else
           torch.zeros(0, dtype=torch.int64, device=dev)).to(torch.int32)
    return ptr, idx


def compute_proposals(cluster_members_list, px, py, meas_noise_cov, device=None):
    """Drop-in for inference.compute_proposals (inference.py:33-47): the same arguments (member
    lists, px, py numpy float32, the noise covariance), the same three lists back -- float32
    means [2], covariances [2, 2] and Python int sizes -- computed by rg_cluster_stats."""
    torch = _torch()
    dev = torch.device(device) if device is not None else torch.device(
        'cuda', torch.cuda.current_device())
    if len(cluster_members_list) == 0:
        return [], [], []
    xy = torch.from_numpy(np.stack((np.asarray(px, np.float32), np.asarray(py, np.float32)),
                                   axis=-1)).to(dev)
    ptr, idx = _csr_from_lists(cluster_members_list, dev)
    st = cluster_stats(xy, ptr, idx, meas_noise_cov)
    if int(st['bad'].item()):
        raise IndexError('a cluster member lies outside the measurements')
    mu, sigma, size = st['mu'].cpu().numpy(), st['sigma'].cpu().numpy(), st['size'].cpu().tolist()
    return [m.copy() for m in mu], [s.copy() for s in sigma], [int(n) for n in size]


def compute_cov_ellipse(mu, cov, chi_sq, n_points, device=None):
    """Drop-in for ellipse.compute_cov_ellipse (ellipse.py:4-37): (points [n_points, 2], mu);
    the points are float32 (the reference's are float64 built from float32 a, b, theta)."""
    torch = _torch()
    dev = torch.device(device) if device is not None else torch.device(
        'cuda', torch.cuda.current_device())
    cov32 = np.asarray(cov, np.float32).reshape(2, 2)
    xy = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    one = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    # one single-member cluster whose covariance is exactly the noise term
    st = cluster_stats(xy, one, one[:1], cov32)
    st['mu'] = torch.from_numpy(np.asarray(mu, np.float32).reshape(1, 2)).to(dev)
    ell = cov_ellipse(st, chi_sq, n_points, True)
    return ell['points'][0].cpu().numpy(), mu


# ---------------------------------------------------------------- two-stage glue
class Detections:
    """detect(): the detector's outputs with its proposal clusters (global node ids)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def detect(detector, node_features: Sequence, edge_features: Sequence, edge_index: Sequence,
           other_features: Sequence) -> Detections:
    """The detector's batched proposal forward (Model_Inference.forward_frames with
    cluster_node_idx=None) keeping what the object stage needs on the device: the four heads'
    logits, the proposal clusters' CSR, frame_ptr, the positions, the rcs column, the
    predicted cluster centres (rg_proposal_centres, computed once by the proposal branch) and
    the forward's outputs with the final node embeddings (``outputs``, ``x``: what
    training.FinetuneTrainer.step_detections trains the object head from)."""
    torch = _torch()
    from . import engine
    from .gnn_detector import _batch_frames, _set_frames
    if not getattr(detector, 'extract_proposals', False):
        raise ValueError('the detector has no proposal branch: set_param_for_proposal_extraction')
    engine._require_device(node_features[0], 'node_features')
    nf, ef, ei, _, _, _, sizes = _batch_frames(node_features, edge_features, edge_index,
                                               [[] for _ in node_features])
    dev = nf.device
    N = int(nf.shape[0])
    g = engine.DeviceGraph.from_edge_index(ei, N)
    _set_frames(g, sizes)
    E = g.n_edges
    e_dst = torch.empty((max(E, 1), ef.shape[1]), dtype=torch.float32, device=dev)
    if E > 0:
        nat.check(nat.lib().rg_gather_rows_f32(ef.data_ptr(), g.perm.data_ptr(), E, ef.shape[1],
                                               e_dst.data_ptr(), nat.stream_ptr(dev)),
                  'rg_gather_rows_f32')
    other_xy = torch.cat([o[:, :2].to(torch.float32) for o in other_features], 0).contiguous()
    fptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
    cache: dict = {}

    def clusters_fn(node_reg, link_cls):
        return engine.propose_clusters(
            node_reg, other_xy, fptr, sizes, detector.reg_mu, detector.reg_sigma,
            detector.clustering_eps, from_links=detector.compute_adj_mat_from_links, g=g,
            link_cls=link_cls[:g.n_pairs], ws_cache=cache)

    with torch.no_grad():
        out = engine.forward_batched(detector.plans(), nf, e_dst, g, None, None, 0,
                                     n_pairs_cap=g.n_pairs, clusters_fn=clusters_fn)
    cx, cy = cache['proposal_centres']
    return Detections(node_cls=out.node_cls, node_reg=out.node_reg,
                      link_cls=out.link_cls[:g.n_pairs], obj_cls=out.obj_cls,
                      cluster_ptr=out.cluster_ptr, cluster_idx=out.cluster_idx, frame_ptr=fptr,
                      frame_sizes=sizes, xy=other_xy, rcs=nf[:, 1],
                      centres=torch.stack((cx, cy), dim=-1),
                      meas_noise_cov=detector.meas_noise_cov, outputs=out, x=out.x)


def detect_frames(detector, fb, cfg, dtype: str = 'fp32', cache: Optional[dict] = None):
    """detect() for a ``frontend.frame_batch`` FrameBatch: the graph build, the detector's
    proposal forward under no_grad and the Detections of it -- the forward's outputs
    (``outputs``, engine.ForwardOutputs; link_cls padded to the pair capacity; ``x`` its final
    node embeddings, a buffer of ``cache`` the next call overwrites), the GraphBatch
    (``graph_batch``), frame_ptr, the positions, the rcs column (node_features[:, 1],
    datagen_classifier.py:256) and the predicted centres.  ``detector`` is a Model_Inference
    with its proposal parameters set; ``cache`` keeps workspaces and buffers between batches.
    None for a batch without a frame.  The host waits where propose_clusters does."""
    torch = _torch()
    from . import engine
    from .graph_features import build_graph_batch
    if not getattr(detector, 'extract_proposals', False):
        raise ValueError('the detector has no proposal branch: set_param_for_proposal_extraction')
    if fb.n_frames == 0:
        return None
    cache = cache if cache is not None else {}
    gb = build_graph_batch(fb, cfg, ws_cache=cache.setdefault('graph', {}))
    g = gb.graph
    other_xy = torch.stack((fb.arrays['meas_px'], fb.arrays['meas_py']), dim=-1)
    pcache = cache.setdefault('proposals', {})

    def clusters_fn(node_reg, link_cls):
        return engine.propose_clusters(
            node_reg, other_xy, fb.frame_ptr, fb.frame_sizes, detector.reg_mu,
            detector.reg_sigma, detector.clustering_eps,
            from_links=detector.compute_adj_mat_from_links, g=g, link_cls=link_cls,
            ws_cache=pcache)

    with torch.no_grad():
        out = engine.forward_batched(detector.plans(dtype), gb.node_features, gb.edge_features, g,
                                     None, None, 0, n_pairs_cap=gb.capacity // 2 + 1,
                                     buffers=cache.setdefault('buffers', {}),
                                     clusters_fn=clusters_fn)
    cx, cy = pcache['proposal_centres']
    return Detections(node_cls=out.node_cls, node_reg=out.node_reg, link_cls=out.link_cls,
                      obj_cls=out.obj_cls, cluster_ptr=out.cluster_ptr,
                      cluster_idx=out.cluster_idx, frame_ptr=fb.frame_ptr,
                      frame_sizes=fb.frame_sizes, xy=other_xy, rcs=gb.node_features[:, 1],
                      centres=torch.stack((cx, cy), dim=-1),
                      meas_noise_cov=detector.meas_noise_cov, outputs=out, x=out.x,
                      graph_batch=gb)


def detections_object_list(det: Detections, detect_object_by_segmentation_output: bool = True,
                           classifier=None, min_meas: Optional[int] = None,
                           **kw) -> ObjectList:
    """object_list of a detect() result.  With ``classifier`` (the cluster-level classifier's
    model) the object classes and scores are the second stage's: ``classify_detections`` with
    ``min_meas``, its cluster_class / cluster_score handed to ``object_list`` -- a proposal
    below min_meas, or one the classifier calls false, is no object."""
    if classifier is not None:
        res = classify_detections(det, classifier, min_meas,
                                  num_classes=int(det.node_cls.shape[1]))
        kw = dict(kw, cluster_class=res['cluster_class'], cluster_score=res['cluster_score'])
    return object_list(det.node_cls, det.link_cls, det.obj_cls, det.xy, det.cluster_ptr,
                       det.cluster_idx, det.frame_ptr, det.meas_noise_cov,
                       detect_object_by_segmentation_output, centres=det.centres, **kw)


def classify_inputs(classifier_model, inp: ClassifierInputs):
    """Classifier logits f32 [K', num_classes] of classifier_inputs (nothing is launched for
    zero objects)."""
    torch = _torch()
    from .classifier import engine as ce
    model = getattr(classifier_model, 'pred', classifier_model)
    if inp.n_objects == 0:
        nc = int(model.predict_node.pred_cls.head[1].out_features)
        return torch.zeros((0, nc), dtype=torch.float32, device=inp.object_features.device)
    begin, end = inp.ranges()
    with torch.no_grad():
        return ce.forward_objects(model, inp.object_features, inp.object_num_meas, begin, end,
                                  model.compute_dtype, n_nodes=inp.n_rows, n_edges=inp.n_edges)


def classify_detections(det, classifier_model, min_meas: Optional[int] = None,
                        meas_noise_cov=None, node_labels=None, num_classes: int = 7) -> dict:
    """The second stage of the two-stage flow for any ``Detections`` (``detect``,
    ``detect_frames``): classifier inputs -> classifier forward -> a class and a score per
    proposal cluster.  Returns the dict of ``classify_proposals`` (logits f32 [K', classes] per
    kept object, object_cluster, object_frame, ``inputs``, ``detections``) plus cluster_class
    int64 [K] / cluster_score f32 [K] over ALL proposal clusters (``cluster_class_from_objects``;
    a cluster below min_meas carries num_classes - 1, the false class, and score 0: it is no
    object of the two-stage flow, output.py:123-128 drops it) and ``bad`` (the stage's int32
    flag, also set by an object_cluster entry out of range).  With ``node_labels`` [N]
    ``inputs.object_class`` is every kept object's majority ground-truth class, lowest label on
    a tie (datagen_classifier.py:50-60).  min_meas defaults to 2.  The one host read is
    ``classifier_inputs``'."""
    noise = det.meas_noise_cov if meas_noise_cov is None else meas_noise_cov
    inp = classifier_inputs(det.xy, det.rcs, det.cluster_ptr, det.cluster_idx, det.frame_ptr,
                            noise, 2 if min_meas is None else min_meas, node_labels=node_labels,
                            num_classes=num_classes)
    logits = classify_inputs(classifier_model, inp)
    if int(logits.shape[1]) != int(num_classes):
        raise ValueError(f'the classifier has {logits.shape[1]} classes, num_classes='
                         f'{num_classes}')
    K = int(det.cluster_ptr.numel()) - 1
    bad = inp.stats['bad']
    ccls, cscore = cluster_class_from_objects(logits, inp.object_cluster, K,
                                              int(num_classes) - 1, bad)
    return dict(logits=logits, object_cluster=inp.object_cluster, object_frame=inp.object_frame,
                inputs=inp, detections=det, cluster_class=ccls, cluster_score=cscore, bad=bad)


def classify_proposals(detector, classifier_model, node_features, edge_features, edge_index,
                       other_features, min_meas: Optional[int] = None,
                       meas_noise_cov=None) -> dict:
    """The two-stage flow: detector forward with proposals -> classifier inputs -> classifier
    forward.  Returns logits f32 [K', classes] per kept object with object_cluster (the
    proposal cluster of every kept object), object_frame, the ClassifierInputs (``inputs``)
    and the Detections (``detections``).  min_meas defaults to 2
    (valid_cluster_num_meas_thr)."""
    det = detect(detector, node_features, edge_features, edge_index, other_features)
    noise = det.meas_noise_cov if meas_noise_cov is None else meas_noise_cov
    inp = classifier_inputs(det.xy, det.rcs, det.cluster_ptr, det.cluster_idx, det.frame_ptr,
                            noise, 2 if min_meas is None else min_meas)
    logits = classify_inputs(classifier_model, inp)
    return dict(logits=logits, object_cluster=inp.object_cluster, object_frame=inp.object_frame,
                inputs=inp, detections=det)


def classifier_training_batch(det, node_gt_class, min_meas: int = 2, meas_noise_cov=None,
                              num_classes: int = 7):
    """What datagen_classifier.__getitem__ + collate_fn hand the classifier's training, from a
    detect() result (or any object with xy, rcs, cluster_ptr, cluster_idx, frame_ptr) and the
    ground-truth node classes [N]: the batch tuple (node features, DeviceGraph, begin, end,
    labels) of classifier.training.prepare_batch, built on the device, and the
    ClassifierInputs.  Returns (batch, inputs); batch is None when no object is kept."""
    noise = getattr(det, 'meas_noise_cov', None) if meas_noise_cov is None else meas_noise_cov
    inp = classifier_inputs(det.xy, det.rcs, det.cluster_ptr, det.cluster_idx, det.frame_ptr,
                            noise, min_meas, node_labels=node_gt_class, num_classes=num_classes)
    if inp.n_objects == 0:
        return None, inp
    g, begin, end = inp.graph()
    return (inp.object_features, g, begin, end, inp.object_class), inp
