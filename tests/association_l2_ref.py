"""Host reference of the 'l2_norm' association (detection_accuracy.py:211-213, 225-235) as a
dense numpy loop, for the tests of rg_eval_associate_l2: the float32 matrix of centre distances,
min(G, P) rounds, every round the row-major first minimum of what is left."""
import numpy as np


def distance_matrix(gt_mu, pred_mu):
    """float32 [G, P]: sqrt(fl(fl(dx dx) + fl(dy dy))), every step rounded to float32 --
    what np.linalg.norm(gt[:, None] - pred[None], axis=-1) evaluates."""
    g = np.asarray(gt_mu, np.float32).reshape(-1, 2)
    p = np.asarray(pred_mu, np.float32).reshape(-1, 2)
    dx = g[:, None, 0] - p[None, :, 0]
    dy = g[:, None, 1] - p[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def greedy(gt_mu, pred_mu, eps):
    """The picks in pick order: gt, pred (int32), d (float32), positive (bool)."""
    D = distance_matrix(gt_mu, pred_mu)
    G, P = D.shape
    m = min(G, P)
    gt, pred = np.zeros(m, np.int32), np.zeros(m, np.int32)
    d = np.zeros(m, np.float32)
    if m:
        assert np.isfinite(D).all()
    left = D.copy()
    for i in range(m):
        g, p = divmod(int(np.argmin(left)), P)     # the first minimum in row-major order
        gt[i], pred[i], d[i] = g, p, D[g, p]
        left[g, :] = np.inf
        left[:, p] = np.inf
    return dict(gt=gt, pred=pred, d=d, positive=d <= np.float32(eps))


def centres(xy, members):
    """float32 [len(members), 2]: the mean position of every cluster, summed in member order in
    float32 (compute_cluster_sample_mean_and_cov, inference.py:24)."""
    out = np.zeros((len(members), 2), np.float32)
    for i, m in enumerate(members):
        s = np.zeros(2, np.float32)
        for j in m:
            s = s + xy[j, :2]
        out[i] = s / np.float32(len(m))
    return out


def accumulate(conf, gt_count, pred_count, gt_cls, pred_cls, picks, false_class):
    """The notebook's three count updates for one frame's kept clusters and picks."""
    for c in gt_cls:
        gt_count[c] += 1
    for c in pred_cls:
        pred_count[c] += 1
    for g, p, pos in zip(picks['gt'], picks['pred'], picks['positive']):
        conf[gt_cls[g] if pos else false_class, pred_cls[p]] += 1
