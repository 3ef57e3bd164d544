"""Golden fixtures of the detection evaluation made by the REFERENCE.

Runs only in the build container, where /root/reference exists (never on the GPU box; nothing
in tests/ imports this file).  ``modules/performance/detection_accuracy.py`` pulls in
``read_data.py``, which imports h5py (absent): an empty stand-in module is installed, as are
the third-party restatements of make_golden.py for the PyG / torchvision imports.  Every
result stored here comes from the reference's own functions on seeded synthetic frames:

  compute_node_idx_for_each_cluster (datagen_gnn.py:15-45)      ground-truth clusters
  compute_gt_and_pred_associations (detection_accuracy.py:192-273)  the four arrays; its
      local ``associations`` / ``distances`` (the picks) are read off the returning frame
      with a trace function, the function itself runs unmodified

The size filter (detection_accuracy.py:141-164: size > cluster_size_threshold), the majority
vote of the predicted node classes (:100-104) and the notebook's three count updates
(performance_eval_detection.ipynb) are applied here as the notebook applies them.

Usage:  python tests/golden/make_eval_golden.py   (writes tests/golden/eval_*.npz)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

NUM_CLASSES = 7
FALSE_CLASS = 6


def _import_reference():
    sys.modules.setdefault('h5py', types.ModuleType('h5py'))
    import make_golden
    make_golden._install_third_party_restatements()
    from modules.data_generator.datagen_gnn import compute_node_idx_for_each_cluster
    from modules.performance import detection_accuracy
    return compute_node_idx_for_each_cluster, detection_accuracy


def traced_associations(det_acc, clusters, eps):
    """The reference function's return value and its picks (associations, distances)."""
    grabbed = {}
    code = det_acc.compute_gt_and_pred_associations.__code__

    def tracer(frame, event, arg):
        if frame.f_code is not code:
            return None

        def local(frame, event, arg):
            if event == 'return':
                grabbed['associations'] = frame.f_locals.get('associations')
                grabbed['distances'] = frame.f_locals.get('distances')
            return local
        return local

    sys.settrace(tracer)
    try:
        out = det_acc.compute_gt_and_pred_associations(clusters, eps, false_class_label=FALSE_CLASS)
    finally:
        sys.settrace(None)
    assoc = grabbed.get('associations')
    if assoc is None or len(assoc) == 0:
        picks = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    else:
        assoc = np.asarray(assoc)
        dist = np.array(grabbed['distances'])
        assert dist.dtype == np.float32
        picks = (assoc[:, 0].astype(np.int32), assoc[:, 1].astype(np.int32), dist)
    return out, picks


# ---------------------------------------------------------------------- synthetic frames
def partition_lists(labels):
    """Clusters of a labelling in the order of rg_cluster_lists: ascending lowest member."""
    seen, lists = {}, []
    for i, l in enumerate(labels):
        if l not in seen:
            seen[l] = len(lists)
            lists.append([])
        lists[seen[l]].append(i)
    return lists


def random_frame(rng, n, n_tracks, untracked, n_pred, agree=0.7, sizes=None):
    """track ids (bytes, b'' = none), node classes, predicted clusters and node classes."""
    if n == 0:
        return dict(track=np.zeros(0, 'S32'), node_class=np.zeros(0, np.int64), pred=[],
                    pred_node_class=np.zeros(0, np.int64))
    names = np.array([('%032x' % int(v)).encode() for v in rng.integers(0, 2 ** 62, n_tracks)],
                     dtype='S32') if n_tracks else np.zeros(0, 'S32')
    t = rng.integers(0, max(n_tracks, 1), n)
    track = names[t] if n_tracks else np.full(n, b'', 'S32')
    track = np.where(rng.random(n) < untracked, np.bytes_(b''), track).astype('S32')
    node_class = rng.integers(0, 6, n).astype(np.int64)
    lab = np.where(rng.random(n) < agree, t % max(n_pred, 1), rng.integers(0, max(n_pred, 1), n))
    pred = partition_lists(lab.tolist())
    pnc = np.where(rng.random(n) < 0.6, node_class, rng.integers(0, NUM_CLASSES, n)).astype(np.int64)
    return dict(track=track, node_class=node_class, pred=pred, pred_node_class=pnc)


def frame_from_lists(gt_lists, pred_lists, n, rng):
    """A frame with the given ground-truth clusters (each a track) and predicted clusters."""
    track = np.full(n, b'', 'S32')
    for i, mem in enumerate(gt_lists):
        track[mem] = ('%032x' % (i + 1)).encode()
    covered = set(i for m in pred_lists for i in m)
    pred = [list(m) for m in pred_lists] + [[i] for i in range(n) if i not in covered]
    pred.sort(key=lambda m: m[0])
    node_class = rng.integers(0, 5, n).astype(np.int64)
    return dict(track=track, node_class=node_class, pred=pred,
                pred_node_class=rng.integers(0, NUM_CLASSES, n).astype(np.int64))


def crowded_frame(rng):
    """600 nodes, about 300 clusters a side, shuffled: 150 untracked nodes inside 3 predicted
    clusters, 3 tracks of 50 split into 150 predicted singletons (so about 147 rows and 147
    columns stay unused after the walk and are paired by the fill-in), and 300 random nodes."""
    n = 600
    gt = np.full(n, -1, np.int64)          # -1 = untracked
    pred = np.zeros(n, np.int64)
    pred[:150] = np.arange(150) // 50                     # labels 0..2
    gt[150:300] = (np.arange(150) // 50)                  # tracks 0..2
    pred[150:300] = 3 + np.arange(150)                    # labels 3..152
    t = rng.integers(0, 140, 300)
    gt[300:] = np.where(rng.random(300) < 0.08, -1, 3 + t)
    pred[300:] = 153 + np.where(rng.random(300) < 0.35, t % 150, rng.integers(0, 150, 300))
    perm = rng.permutation(n)
    gt, pred = gt[perm], pred[perm]
    names = np.array([('%032x' % int(v)).encode() for v in rng.integers(0, 2 ** 62, 143)], 'S32')
    track = np.where(gt < 0, np.bytes_(b''), names[np.maximum(gt, 0)]).astype('S32')
    node_class = rng.integers(0, 6, n).astype(np.int64)
    pnc = np.where(rng.random(n) < 0.6, node_class, rng.integers(0, NUM_CLASSES, n)).astype(np.int64)
    return dict(track=track, node_class=node_class, pred=partition_lists(pred.tolist()),
                pred_node_class=pnc)


def track_keys(track):
    """frontend._host_track_keys: ranks of the sorted unique ids, 0 = no track."""
    uniq, inv = np.unique(track, return_inverse=True)
    keys = inv.astype(np.int64) + 1
    if uniq.size and uniq[0] == b'':
        keys -= 1
    return keys


def evaluate_case(ref, frames, eps, threshold):
    node_idx_fn, det_acc = ref
    out = {'eps': np.float64(eps), 'cluster_size_threshold': np.int64(threshold),
           'n_frames': np.int64(len(frames))}
    fptr, keys, ncls, pptr, pidx, pncls, pcls = [0], [], [], [0], [], [], []
    gptr, gidx, gcls, gcount = [0], [], [], []
    conf = np.zeros((NUM_CLASSES, NUM_CLASSES), dtype=np.uint64)
    gt_count = np.zeros((NUM_CLASSES, ), dtype=np.uint64)
    pred_count = np.zeros((NUM_CLASSES, ), dtype=np.uint64)
    key_off = 0
    stats = []
    for f, fr in enumerate(frames):
        n = len(fr['track'])
        base = fptr[-1]
        fptr.append(base + n)
        k = track_keys(fr['track'])
        keys.append(np.where(k > 0, k + key_off, 0))
        key_off += int(k.max(initial=0))
        ncls.append(fr['node_class'])
        pncls.append(fr['pred_node_class'])
        for m in fr['pred']:
            pidx += [base + i for i in m]
            pptr.append(len(pidx))
        # the reference's ground-truth clusters
        gt_lists, gt_labels = node_idx_fn(fr['track'], fr['node_class'], 'cpu')
        gt_lists = [t.numpy() for t in gt_lists]
        gt_labels = gt_labels.numpy().tolist() if n else []
        for m in gt_lists:
            gidx += [base + int(i) for i in m]
            gptr.append(len(gidx))
        gcls += gt_labels
        gcount.append(len(gt_lists))
        # predicted cluster classes: the majority vote of detection_accuracy.py:100-104
        pnc = torch.from_numpy(fr['pred_node_class'])
        pred_labels = [int(torch.argmax(torch.bincount(pnc[torch.tensor(m)]))) for m in fr['pred']]
        pcls += pred_labels
        # size filter (detection_accuracy.py:141-164)
        kp = [i for i, m in enumerate(fr['pred']) if len(m) > threshold]
        kg = [i for i, m in enumerate(gt_lists) if len(m) > threshold]
        clusters = {
            'obj_class_pred': [pred_labels[i] for i in kp],
            'cluster_member_list_pred': [set(int(v) for v in fr['pred'][i]) for i in kp],
            'cluster_mean_list_pred': [np.zeros(2, np.float32) for _ in kp],
            'cluster_member_list_gt': [set(int(v) for v in gt_lists[i]) for i in kg],
            'obj_class_gt': [gt_labels[i] for i in kg],
            'cluster_mean_list_gt': [np.zeros(2, np.float32) for _ in kg]}
        res, (pg, pp, pd) = traced_associations(det_acc, clusters, eps)
        for key, v in res.items():
            out[f'f{f}/{key}'] = np.asarray(v)
        out[f'f{f}/pick_gt'], out[f'f{f}/pick_pred'], out[f'f{f}/pick_d'] = pg, pp, pd
        # the notebook's accumulation
        for v in res['obj_class_gt']:
            gt_count[int(v)] += 1
        for v in res['obj_class_pred']:
            pred_count[int(v)] += 1
        for a, b in zip(res['obj_class_gt_associated'], res['obj_class_pred_associated']):
            conf[int(a), int(b)] += 1
        overlap = sum(1 for a in clusters['cluster_member_list_gt']
                      for b in clusters['cluster_member_list_pred'] if a & b)
        stats.append(dict(n=n, G=len(kg), P=len(kp), overlapping=overlap, picks=len(pg),
                          fill_in=int(np.sum(pd == np.float32(1.0)))))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    out.update(frame_ptr=np.asarray(fptr, np.int32), track_key=cat(keys, np.int32),
               node_class=cat(ncls, np.int64), pred_node_class=cat(pncls, np.int64),
               pred_cluster_ptr=np.asarray(pptr, np.int32), pred_cluster_idx=np.asarray(pidx, np.int32),
               pred_class=np.asarray(pcls, np.int64),
               gt_cluster_ptr=np.asarray(gptr, np.int32), gt_cluster_idx=np.asarray(gidx, np.int32),
               gt_cluster_class=np.asarray(gcls, np.int64),
               gt_frame_clusters=np.asarray(gcount, np.int32),
               confusion_matrix=conf, gt_count_matrix=gt_count, pred_count_matrix=pred_count)
    return out, stats


def main():
    ref = _import_reference()
    cases = {}
    rng = np.random.default_rng(20240611)
    cases['eval_single_g_lt_p'] = ([random_frame(rng, 40, 5, 0.05, 14, agree=0.5)], 0.7, 0)
    cases['eval_single_g_gt_p'] = ([random_frame(rng, 40, 12, 0.3, 4)], 0.7, 0)
    fr = random_frame(rng, 36, 9, 0.0, 9, agree=0.8)
    while len(set(fr['track'].tolist())) != len(fr['pred']):
        fr = random_frame(rng, 36, 9, 0.0, 9, agree=0.8)
    cases['eval_single_g_eq_p'] = ([fr], 0.7, 0)
    cases['eval_one_node'] = ([random_frame(rng, 1, 1, 0.0, 1)], 0.7, 0)
    cases['eval_untracked'] = ([random_frame(rng, 30, 0, 1.0, 6, agree=0.0)], 0.7, 0)
    # cluster_size_threshold = 2: every ground-truth cluster dropped (condition 3), every
    # predicted cluster dropped (condition 2), and a frame where both sides keep some
    a = frame_from_lists([[i, i + 1] for i in range(0, 20, 2)],
                         [list(range(0, 7)), list(range(7, 20))], 20, rng)
    b = frame_from_lists([list(range(0, 9)), list(range(9, 18))],
                         [[i, i + 1] for i in range(0, 18, 2)], 18, rng)
    c = random_frame(rng, 60, 8, 0.2, 10)
    cases['eval_threshold2'] = ([a, b, c], 0.7, 2)
    # ties: a chain g_i = {2i, 2i+1}, p_i = {2i+1, 2i+2}: every overlap has IoU 1/3, so the
    # row-major order of equal distances decides; and a 6 x 7 pair sharing 3 nodes: IoU 3/10
    n = 26
    chain = frame_from_lists([[2 * i, 2 * i + 1] for i in range(12)],
                             [[2 * i + 1, 2 * i + 2] for i in range(12)], n, rng)
    grid = frame_from_lists([[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]],
                            [[0, 4, 8, 12], [1, 5, 9, 13], [2, 6, 10, 14], [3, 7, 11, 15]], 16, rng)
    three_tenths = frame_from_lists([[0, 1, 2, 3, 4, 5]], [[3, 4, 5, 6, 7, 8, 9]], 10, rng)
    cases['eval_ties'] = ([chain, grid, three_tenths], 0.7, 0)
    # a batch of unequal frames; the 600-node frame crosses wave and block boundaries
    batch = [random_frame(rng, 1, 1, 0.0, 1), random_frame(rng, 37, 6, 0.2, 8),
             random_frame(rng, 0, 0, 0.0, 0), random_frame(rng, 300, 40, 0.1, 60),
             crowded_frame(rng)]
    for tag, eps in (('eps07', 0.7), ('eps05', 0.5), ('eps10', 1.0)):
        cases['eval_batch5_' + tag] = (batch, eps, 0)
    for name, (frames, eps, thr) in cases.items():
        out, stats = evaluate_case(ref, frames, eps, thr)
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print(name, 'eps', eps, 'threshold', thr, os.path.getsize(path), 'bytes')
        for s in stats:
            print('   ', s)
        if name.startswith('eval_batch5'):
            big = stats[-1]
            assert big['G'] >= 250 and big['P'] >= 250 and big['overlapping'] > 256, big
            assert big['fill_in'] > 64, big


if __name__ == '__main__':
    main()
