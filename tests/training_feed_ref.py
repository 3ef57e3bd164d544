"""The training feed restated in numpy (csrc/training_feed.hip, training.training_labels), and
the fixture cases its tests share (tests/test_training_feed_host.py,
tests/test_gpu_training_feed.py).  Written from the semantics, not from the reference's text:

  flip            negate py and vy over the measurement ranges of the flagged windows
  edge_labels     pair (s, d) is 1 when both ends carry the same non-zero track key
  link_pairs      the pairs of an edge list with src < dst, in the list's order
  gt_clusters     per frame the tracked clusters in ascending key order, then one singleton per
                  untracked node in node order; a cluster's label is its lowest member's class

No test lives here."""
import numpy as np

FIXTURE = 'training_feed_148_s40'
CASES = ((10, 0), (10, 7), (10, 30), (4, 36))      # (window size, sliding position)
GRID = (0.0, 100.0, -50.0, 50.0)
LABEL_STATIC = 7


def case_key(W, pos, flip):
    return f'w{W}_p{pos}_f{int(bool(flip))}/'


def flip(py, vy, win_ptr, flags):
    """(py, vy) with the rows [win_ptr[w], win_ptr[w + 1]) of every flagged window negated;
    win_ptr None: one window over every row."""
    py, vy = np.array(py, copy=True), np.array(vy, copy=True)
    ptr = np.array([0, len(py)]) if win_ptr is None else np.asarray(win_ptr)
    for w, f in enumerate(np.asarray(flags).reshape(-1)):
        if f:
            sl = slice(int(ptr[w]), int(ptr[w + 1]))
            py[sl] = -py[sl]
            vy[sl] = -vy[sl]
    return py, vy


def link_pairs(edge_index):
    ei = np.asarray(edge_index)
    keep = ei[0] < ei[1]
    return ei[0][keep], ei[1][keep]


def edge_labels(key, src, dst):
    key = np.asarray(key)
    return ((key[src] == key[dst]) & (key[src] != 0)).astype(np.int64)


def gt_clusters(key, node_class, frame_ptr=None):
    """(cluster_ptr, cluster_idx, cluster_labels) over global node ids."""
    key, node_class = np.asarray(key), np.asarray(node_class)
    fp = np.array([0, len(key)]) if frame_ptr is None else np.asarray(frame_ptr)
    ptr, idx, lab = [0], [], []
    for a, b in zip(fp[:-1], fp[1:]):
        k = key[a:b]
        groups = [np.flatnonzero(k == t) for t in np.unique(k[k != 0])]
        groups += [np.array([i]) for i in np.flatnonzero(k == 0)]
        for g in groups:
            idx.extend((g + a).tolist())
            ptr.append(len(idx))
            lab.append(int(node_class[a + g[0]]))
    return np.array(ptr, np.int64), np.array(idx, np.int64), np.array(lab, np.int64)


def dynamic_frame(seq, store, W, pos, flipped):
    """The dynamic frame of sliding position ``pos`` from the sequence fixture's full window
    (``seq``: sequence_148_s40.npz, ``store``: its SequenceStore on any device): flip, the
    grid test [min, max) on the flipped values, the moving selection.  The offset to a
    track's mean flips with the positions (a mean of negated values is the negated mean).
    Returns px, py, vx, vy, class, offsets [n, 2] and the window's own track keys."""
    pre = f'w{W}_p{pos}/'
    full = {k: seq[pre + 'full/meas_' + k] for k in ('px', 'py', 'vx', 'vy')}
    cls = seq[pre + 'full_gt/class_labels']
    ox, oy = seq[pre + 'full_gt/offsetx'], seq[pre + 'full_gt/offsety']
    key = store.host_window(pos, W)['track_key']
    py, vy = flip(full['py'], full['vy'], None, [flipped])
    oy = -oy + np.float32(0) if flipped else oy      # a zero offset stays +0 (x - x)
    x0, x1, y0, y1 = GRID
    keep = (full['px'] >= x0) & (full['px'] < x1) & (py >= y0) & (py < y1) & (cls != LABEL_STATIC)
    return dict(px=full['px'][keep], py=py[keep], vx=full['vx'][keep], vy=vy[keep],
                node_class=cls[keep].astype(np.int64),
                node_offsets=np.stack((ox[keep], oy[keep]), -1).astype(np.float32),
                key=key[keep].astype(np.int64))
