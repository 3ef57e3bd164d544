"""Golden fixtures of the 'l2_norm' association made by the REFERENCE.

Runs only in the build container, where /root/reference exists (never on the GPU box; nothing
in tests/ imports this file).  The reference is imported as make_eval_golden.py imports it, and
that file's frame builders are reused.  Every result stored here comes from the reference's own
functions on seeded synthetic frames:

  compute_node_idx_for_each_cluster (datagen_gnn.py:15-45)      ground-truth clusters
  compute_proposals (inference.py:33-47)                        the float32 cluster means
  compute_gt_and_pred_associations(..., 'l2_norm') (detection_accuracy.py:192-273)
      the four arrays; its local ``associations`` / ``distances`` (the picks) are read off the
      returning frame with a trace function, the function itself runs unmodified

The size filter (detection_accuracy.py:141-164: size > cluster_size_threshold), the majority
vote of the predicted node classes (:100-104) and the notebook's three count updates are
applied here as make_eval_golden.py applies them.

Usage:  python tests/golden/make_assoc_l2_golden.py   (writes tests/golden/assoc_l2_*.npz)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_eval_golden as meg  # noqa: E402

NUM_CLASSES, FALSE_CLASS = meg.NUM_CLASSES, meg.FALSE_CLASS


def traced_l2(det_acc, clusters, eps):
    """The reference function's return value under 'l2_norm' and its picks."""
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
        out = det_acc.compute_gt_and_pred_associations(
            clusters, eps, association_criteria='l2_norm', false_class_label=FALSE_CLASS)
    finally:
        sys.settrace(None)
    assoc = grabbed.get('associations')
    if assoc is None or len(assoc) == 0:
        return out, (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assoc = np.asarray(assoc)
    dist = np.array(grabbed['distances'])
    assert dist.dtype == np.float32
    return out, (assoc[:, 0].astype(np.int32), assoc[:, 1].astype(np.int32), dist)


# ---------------------------------------------------------------------- positions
def scattered(rng, fr, spread=1.0):
    """Positions for a frame of make_eval_golden: every track around its own centre on the
    100 m grid, untracked nodes anywhere."""
    n = len(fr['track'])
    uniq, inv = np.unique(fr['track'], return_inverse=True)
    centres = rng.uniform(-50, 50, (max(len(uniq), 1), 2))
    xy = centres[inv] + rng.normal(0, spread, (n, 2)) if n else np.zeros((0, 2))
    free = fr['track'] == b''
    xy[free] = rng.uniform(-50, 50, (int(free.sum()), 2))
    fr['xy'] = xy.astype(np.float32)
    return fr


def with_xy(fr, xy):
    fr['xy'] = np.asarray(xy, np.float32).reshape(len(fr['track']), 2)
    return fr


def tied_rounds(gt_mean, pred_mean, pg, pp, pd):
    """Rounds of the reference's picks in which the minimum stood at more than one place."""
    if len(pg) == 0:
        return 0
    alive = np.ones((len(gt_mean), len(pred_mean)), bool)
    dist = np.linalg.norm(gt_mean[:, None] - pred_mean[None], axis=-1)
    tied = 0
    for g, p, d in zip(pg, pp, pd):
        assert dist[g, p] == d
        tied += int(np.sum(alive & (dist == d)) > 1)
        alive[g, :] = False
        alive[:, p] = False
    return tied


def evaluate_case(ref, frames, eps, threshold):
    node_idx_fn, det_acc = ref
    from modules.inference.inference import compute_proposals
    out = {'eps': np.float64(eps), 'cluster_size_threshold': np.int64(threshold),
           'n_frames': np.int64(len(frames))}
    fptr, keys, ncls, pptr, pidx, pncls, xys = [0], [], [], [0], [], [], []
    conf = np.zeros((NUM_CLASSES, NUM_CLASSES), dtype=np.uint64)
    gt_count = np.zeros((NUM_CLASSES, ), dtype=np.uint64)
    pred_count = np.zeros((NUM_CLASSES, ), dtype=np.uint64)
    noise = np.zeros((2, 2), np.float32)
    key_off = 0
    stats = []
    for f, fr in enumerate(frames):
        n = len(fr['track'])
        base = fptr[-1]
        fptr.append(base + n)
        k = meg.track_keys(fr['track'])
        keys.append(np.where(k > 0, k + key_off, 0))
        key_off += int(k.max(initial=0))
        ncls.append(fr['node_class'])
        pncls.append(fr['pred_node_class'])
        xys.append(fr['xy'])
        for m in fr['pred']:
            pidx += [base + i for i in m]
            pptr.append(len(pidx))
        gt_lists, gt_labels = node_idx_fn(fr['track'], fr['node_class'], 'cpu')
        gt_labels = gt_labels.numpy().tolist() if n else []
        pred_lists = [torch.tensor(m) for m in fr['pred']]
        pnc = torch.from_numpy(fr['pred_node_class'])
        pred_labels = [int(torch.argmax(torch.bincount(pnc[m]))) for m in pred_lists]
        px, py = fr['xy'][:, 0], fr['xy'][:, 1]
        mean_p, _, size_p = compute_proposals(pred_lists, px, py, noise)
        mean_g, _, size_g = compute_proposals(gt_lists, px, py, noise)
        assert all(m.dtype == np.float32 for m in mean_p + mean_g)
        # size filter (detection_accuracy.py:141-164)
        kp = [i for i, s in enumerate(size_p) if s > threshold]
        kg = [i for i, s in enumerate(size_g) if s > threshold]
        clusters = {
            'obj_class_pred': [pred_labels[i] for i in kp],
            'cluster_member_list_pred': [set(int(v) for v in fr['pred'][i]) for i in kp],
            'cluster_mean_list_pred': [mean_p[i] for i in kp],
            'cluster_member_list_gt': [set(int(v) for v in gt_lists[i].numpy()) for i in kg],
            'obj_class_gt': [gt_labels[i] for i in kg],
            'cluster_mean_list_gt': [mean_g[i] for i in kg]}
        res, (pg, pp, pd) = traced_l2(det_acc, clusters, eps)
        for key, v in res.items():
            out[f'f{f}/{key}'] = np.asarray(v)
        out[f'f{f}/pick_gt'], out[f'f{f}/pick_pred'], out[f'f{f}/pick_d'] = pg, pp, pd
        out[f'f{f}/pick_positive'] = pd <= eps
        out[f'f{f}/gt_mean'] = (np.stack(clusters['cluster_mean_list_gt']) if kg
                                else np.zeros((0, 2), np.float32))
        out[f'f{f}/pred_mean'] = (np.stack(clusters['cluster_mean_list_pred']) if kp
                                  else np.zeros((0, 2), np.float32))
        for v in res['obj_class_gt']:
            gt_count[int(v)] += 1
        for v in res['obj_class_pred']:
            pred_count[int(v)] += 1
        for a, b in zip(res['obj_class_gt_associated'], res['obj_class_pred_associated']):
            conf[int(a), int(b)] += 1
        disjoint_pos = sum(1 for g, p, d in zip(pg, pp, pd) if d <= eps and not (
            clusters['cluster_member_list_gt'][g] & clusters['cluster_member_list_pred'][p]))
        stats.append(dict(n=n, G=len(kg), P=len(kp), picks=len(pg),
                          positive=int(np.sum(pd <= eps)), disjoint_positive=disjoint_pos,
                          tied_rounds=tied_rounds(out[f'f{f}/gt_mean'], out[f'f{f}/pred_mean'],
                                                  pg, pp, pd)))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    out.update(frame_ptr=np.asarray(fptr, np.int32), track_key=cat(keys, np.int32),
               node_class=cat(ncls, np.int64), pred_node_class=cat(pncls, np.int64),
               xy=np.concatenate(xys).astype(np.float32).reshape(-1, 2),
               pred_cluster_ptr=np.asarray(pptr, np.int32),
               pred_cluster_idx=np.asarray(pidx, np.int32),
               confusion_matrix=conf, gt_count_matrix=gt_count, pred_count_matrix=pred_count)
    return out, stats


def main():
    ref = meg._import_reference()
    cases = {}
    rng = np.random.default_rng(20250307)
    sc = lambda fr: scattered(rng, fr)  # noqa: E731
    # five ordinary frames, one of them empty, one a single node
    batch = [sc(meg.random_frame(rng, 1, 1, 0.0, 1)), sc(meg.random_frame(rng, 37, 6, 0.2, 8)),
             sc(meg.random_frame(rng, 0, 0, 0.0, 0)), sc(meg.random_frame(rng, 300, 40, 0.1, 60)),
             sc(meg.random_frame(rng, 120, 15, 0.3, 25))]
    cases['assoc_l2_batch5'] = (batch, 1.5, 0)
    cases['assoc_l2_batch5_thr1'] = (batch, 0.5, 1)
    # ties: nodes on an integer grid with 3-4-5 offsets, clusters of two nodes (centres on the
    # half-integer grid), the two sides pairing the nodes differently
    n = 48
    pts = np.array([(0, 0), (3, 4), (4, 3), (6, 8), (8, 6), (5, 0), (0, 5), (3, -4)])
    xy = pts[rng.integers(0, len(pts), n)] + 10 * rng.integers(0, 2, (n, 2))
    pairs = meg.frame_from_lists([[2 * i, 2 * i + 1] for i in range(n // 2)],
                                 [[2 * i + 1, 2 * i + 2] for i in range(n // 2 - 1)], n, rng)
    singles = meg.frame_from_lists([[i] for i in range(0, 24, 2)], [], 24, rng)
    cases['assoc_l2_ties'] = ([with_xy(pairs, xy), with_xy(singles, xy[:24])], 5.0, 0)
    # G > P and P > G
    cases['assoc_l2_g_gt_p'] = ([sc(meg.random_frame(rng, 40, 12, 0.3, 4))], 2.0, 0)
    cases['assoc_l2_g_lt_p'] = ([sc(meg.random_frame(rng, 40, 5, 0.05, 14, agree=0.5))], 2.0, 0)
    # one cluster a side
    one = meg.frame_from_lists([list(range(6))], [list(range(6))], 6, rng)
    cases['assoc_l2_one_each'] = ([sc(one)], 1.0, 0)
    # threshold 2: every ground-truth cluster dropped, every predicted cluster dropped, and a
    # frame where both sides keep some
    a = meg.frame_from_lists([[i, i + 1] for i in range(0, 20, 2)],
                             [list(range(0, 7)), list(range(7, 20))], 20, rng)
    b = meg.frame_from_lists([list(range(0, 9)), list(range(9, 18))],
                             [[i, i + 1] for i in range(0, 18, 2)], 18, rng)
    c = meg.random_frame(rng, 60, 8, 0.2, 10)
    cases['assoc_l2_threshold2'] = ([sc(a), sc(b), sc(c)], 1.5, 2)
    # a positive pick between clusters that share no node: two parallel pairs 0.5 m apart
    apart = meg.frame_from_lists([[0, 1], [4, 5]], [[2, 3], [6, 7]], 8, rng)
    cases['assoc_l2_disjoint_positive'] = (
        [with_xy(apart, [(0, 0), (0, 1), (0.5, 0), (0.5, 1), (20, 0), (20, 2), (29, 0), (29, 2)])],
        1.0, 1)
    for name, (frames, eps, thr) in cases.items():
        out, stats = evaluate_case(ref, frames, eps, thr)
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print(name, 'eps', eps, 'threshold', thr, os.path.getsize(path), 'bytes')
        for s in stats:
            print('   ', s)
        if name == 'assoc_l2_ties':
            assert all(s['tied_rounds'] >= 4 for s in stats), stats
        if name == 'assoc_l2_disjoint_positive':
            assert stats[0]['disjoint_positive'] == 1 and stats[0]['picks'] == 2, stats
        if name == 'assoc_l2_threshold2':
            assert stats[0]['G'] == 0 and stats[1]['P'] == 0 and stats[2]['picks'] > 0, stats
        if name == 'assoc_l2_one_each':
            assert stats[0]['G'] == 1 and stats[0]['P'] == 1, stats


if __name__ == '__main__':
    main()
