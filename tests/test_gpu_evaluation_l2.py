"""The 'l2_norm' association on the GPU (rg_eval_associate_l2, evaluation.associate_l2 and the
evaluator's association_criteria) against the reference's own picks (tests/golden/assoc_l2_*.npz,
make_assoc_l2_golden.py) and the dense numpy greedy of association_l2_ref.py.  Indices, flags and
counts are integers and pick_d is an exactly specified float32: every comparison is exact."""
import numpy as np
import pytest
import torch

import association_l2_ref as l2ref
from conftest import golden, golden_names, model_cfg, model_state_dict

pytestmark = pytest.mark.gpu

NC, FALSE = 7, 6
FIXTURES = golden_names('assoc_l2_')
ARRAYS = ('obj_class_gt_associated', 'obj_class_pred_associated', 'obj_class_gt', 'obj_class_pred')
COUNTS = ('confusion_matrix', 'gt_count_matrix', 'pred_count_matrix')
LDS_CAP = 4096  # L2_LDS_CAP of evaluation.hip: kept clusters a side whose state is held in LDS


def _ev():
    from graph_neural_network_for_radar_perception_amd import evaluation
    return evaluation


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == 'f':  # bit for bit
        a, b = a.view(np.int32 if a.itemsize == 4 else np.int64), b.view(
            np.int32 if b.itemsize == 4 else np.int64)
    assert np.array_equal(a, b), (what, a, b)


def _same_picks(got, want, what):
    for k in ('gt', 'pred', 'd', 'positive'):
        _same(got[k], want[k], (what, k))


def _one_hot_logits(classes, dev):
    x = np.zeros((len(classes), NC), np.float32)
    x[np.arange(len(classes)), classes] = 1.0
    return torch.from_numpy(x).to(dev)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ fixtures
def _update_from_fixture(d, dev, criterion='l2_norm'):
    ev = _ev().DetectionEvaluator(NC, float(d['eps']), int(d['cluster_size_threshold']), True,
                                  FALSE, association_criteria=criterion)
    ev.update(_one_hot_logits(d['pred_node_class'], dev), None, _up(d['pred_cluster_ptr'], dev),
              _up(d['pred_cluster_idx'], dev), _up(d['node_class'], dev), _up(d['track_key'], dev),
              _up(d['frame_ptr'], dev), xy=_up(d['xy'], dev))
    return ev


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_picks_match_reference(cuda_device, name):
    """Per frame the reference's picks (indices, d bit for bit, flags), the kept clusters'
    centres, and the three count matrices of the notebook."""
    d = golden(name)
    ev = _update_from_fixture(d, cuda_device)
    picks = _ev().frame_picks(ev.last['assoc'])
    assoc = {k: v.cpu().numpy() for k, v in ev.last['assoc'].items()}
    gt_mu, pred_mu = ev.last['gt_mu'].cpu().numpy(), ev.last['pred_mu'].cpu().numpy()
    assert int(assoc['bad_value'][0]) == 0
    gcl = assoc['pick_gt_cluster'][assoc['pick_gt_cluster'] >= 0]
    assert len(gcl) == sum(len(p['gt']) for p in picks)            # -1 in every unused slot
    for f in range(int(d['n_frames'])):
        want = dict(gt=d[f'f{f}/pick_gt'], pred=d[f'f{f}/pick_pred'], d=d[f'f{f}/pick_d'],
                    positive=d[f'f{f}/pick_positive'])
        _same_picks(picks[f], want, (name, f))
        s, c = int(assoc['pick_start'][f]), int(assoc['pick_count'][f])
        # the picked clusters' centres are the reference's kept means
        _same(gt_mu[assoc['pick_gt_cluster'][s:s + c]], d[f'f{f}/gt_mean'][want['gt']], (f, 'gt mu'))
        _same(pred_mu[assoc['pick_pred_cluster'][s:s + c]], d[f'f{f}/pred_mean'][want['pred']],
              (f, 'pred mu'))
    res = ev.result()
    for k in COUNTS:
        _same(res[k], d[k], k)


@pytest.mark.parametrize('name', FIXTURES)
def test_drop_in_l2_returns_the_four_arrays(cuda_device, name):
    """compute_gt_and_pred_associations_l2 fed the kept means and classes returns the
    reference's four arrays, dtypes (the float64 empties of conditions 2-4) included; the
    member sets are not read."""
    d = golden(name)
    fn = _ev().compute_gt_and_pred_associations_l2
    for f in range(int(d['n_frames'])):
        g, p = d[f'f{f}/obj_class_gt'], d[f'f{f}/obj_class_pred']
        clusters = {'cluster_mean_list_gt': [m.copy() for m in d[f'f{f}/gt_mean']],
                    'cluster_mean_list_pred': [m.copy() for m in d[f'f{f}/pred_mean']],
                    'obj_class_gt': [int(v) for v in g], 'obj_class_pred': [int(v) for v in p]}
        got = fn(clusters, float(d['eps']), false_class_label=FALSE)
        assert sorted(got) == sorted(ARRAYS)
        for k in ARRAYS:
            _same(got[k], d[f'f{f}/{k}'], (f, k))


# ------------------------------------------------------------------ random sweep
SITES = np.array([(x, y) for x in np.arange(0, 3, 0.5) for y in np.arange(0, 2.5, 0.5)],
                 np.float32)


def _random_batch(seed, n_frames=200):
    """Frames of 0-40 nodes.  Every node sits on one of a few sites of a half-integer grid and
    both sides cluster the nodes of a site (by track, by predicted label): every centre is a
    site exactly, many clusters share one, equal distances are the rule."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n_frames):
        n = int(rng.integers(0, 41))
        site = rng.integers(0, int(rng.integers(1, len(SITES) + 1)), n)
        key = 1 + 4 * site + rng.integers(0, int(rng.integers(1, 5)), n)
        key = np.where(rng.random(n) < 0.8, key, 0)                 # 0 = untracked
        lab = 4 * site + rng.integers(0, int(rng.integers(1, 5)), n)
        frames.append(dict(key=key.astype(np.int32), pred_label=lab, xy=SITES[site],
                           node_class=rng.integers(0, 6, n), pred_node_class=rng.integers(0, NC, n)))
    return frames


def _lists(labels):
    """Clusters of a labelling, ordered by their lowest member (the order of rg_cluster_lists)."""
    seen, out = {}, []
    for i, l in enumerate(labels):
        if l not in seen:
            seen[l] = len(out)
            out.append([])
        out[seen[l]].append(i)
    return out


def _frame_clusters(fr, thr):
    """A frame's kept clusters a side: members, classes."""
    n = len(fr['key'])
    tracked = sorted(set(int(k) for k in fr['key'] if k))
    gt = [[i for i in range(n) if fr['key'][i] == k] for k in tracked]
    gt += [[i] for i in range(n) if fr['key'][i] == 0]
    pred = _lists(fr['pred_label'].tolist())
    gt = [m for m in gt if len(m) > thr]
    pred = [m for m in pred if len(m) > thr]
    gt_cls = [int(fr['node_class'][m[0]]) for m in gt]
    pred_cls = [int(np.argmax(np.bincount(fr['pred_node_class'][m], minlength=NC))) for m in pred]
    return gt, pred, gt_cls, pred_cls


def _expected(frames, eps, thr):
    conf = np.zeros((NC, NC), np.uint64)
    gtc, prc = np.zeros(NC, np.uint64), np.zeros(NC, np.uint64)
    picks = []
    for fr in frames:
        gt, pred, gt_cls, pred_cls = _frame_clusters(fr, thr)
        pk = l2ref.greedy(l2ref.centres(fr['xy'], gt), l2ref.centres(fr['xy'], pred), eps)
        l2ref.accumulate(conf, gtc, prc, gt_cls, pred_cls, pk, FALSE)
        picks.append(pk)
    return picks, (conf, gtc, prc)


def _run_frames(frames, eps, thr, dev, criterion='l2_norm'):
    ev = _ev().DetectionEvaluator(NC, eps, thr, True, FALSE, association_criteria=criterion)
    sizes = [len(fr['key']) for fr in frames]
    base = np.concatenate(([0], np.cumsum(sizes)))
    ptr, idx = [0], []
    for fr, b in zip(frames, base):
        for m in _lists(fr['pred_label'].tolist()):
            idx += [int(b) + i for i in m]
            ptr.append(len(idx))
    cat = lambda k, dt: np.concatenate([fr[k] for fr in frames]).astype(dt)  # noqa: E731
    ev.update(_one_hot_logits(cat('pred_node_class', np.int64), dev), None,
              _up(np.asarray(ptr, np.int32), dev), _up(np.asarray(idx, np.int32), dev),
              _up(cat('node_class', np.int64), dev), _up(cat('key', np.int32), dev),
              _up(base.astype(np.int32), dev), max_frame_nodes=max(sizes),
              xy=_up(cat('xy', np.float32), dev))
    return ev


_SWEEP = {}


def _sweep_expected(eps, thr):
    """The host reference of a sweep case, computed once."""
    if (eps, thr) not in _SWEEP:
        frames = _random_batch(int(min(eps, 9) * 10) + thr)
        _SWEEP[eps, thr] = (frames,) + _expected(frames, eps, thr)
    return _SWEEP[eps, thr]


@pytest.mark.parametrize('thr', [0, 1, 2])
@pytest.mark.parametrize('eps', [0.5, 1.5, 1e9])
def test_random_sweep_matches_host_reference(cuda_device, eps, thr):
    """200 frames of 0-40 clusters a side in one batch: the picks of every frame and the three
    count matrices equal the dense greedy's."""
    frames, picks, counts = _sweep_expected(eps, thr)
    ev = _run_frames(frames, eps, thr, cuda_device)
    got = _ev().frame_picks(ev.last['assoc'])
    assert len(got) == len(frames)
    ties = 0
    for f, (g, w) in enumerate(zip(got, picks)):
        _same_picks(g, w, (f,))
        ties += len(w['d']) - len(np.unique(w['d']))
    assert ties > 20                                            # equal distances are common
    res = ev.result()
    for k, w in zip(COUNTS, counts):
        _same(res[k], w, k)


def test_two_runs_are_bit_identical(cuda_device):
    frames, _, _ = _sweep_expected(1.5, 0)
    runs = []
    for _ in range(2):
        ev = _run_frames(frames, 1.5, 0, cuda_device)
        a = ev.last['assoc']
        out = {k: a[k].cpu().numpy() for k in ('gt_kept', 'pred_kept', 'pick_start', 'pick_count',
                                                'pick_gt_cluster', 'pick_pred_cluster')}
        out['picks'] = _ev().frame_picks(a)
        out['counts'] = ev.result()
        out['mu'] = (ev.last['gt_mu'].cpu().numpy(), ev.last['pred_mu'].cpu().numpy())
        runs.append(out)
    a, b = runs
    for k in ('gt_kept', 'pred_kept', 'pick_start', 'pick_count', 'pick_gt_cluster',
              'pick_pred_cluster'):
        _same(a[k], b[k], k)
    for f, (x, y) in enumerate(zip(a['picks'], b['picks'])):
        _same_picks(x, y, (f,))
    for k in COUNTS:
        _same(a['counts'][k], b['counts'][k], k)
    _same(a['mu'][0], b['mu'][0], 'gt_mu')
    _same(a['mu'][1], b['mu'][1], 'pred_mu')


# ------------------------------------------------------------------ shapes
def _singleton_batch(shapes, dev):
    """Frames of G ground-truth and P predicted clusters of one node each: frame f has
    max(G, P) nodes, cluster i of a side is the frame's node i.  Returns the CSRs and
    frame_ptr on the device and each frame's range of cluster ids a side."""
    fptr, g_idx, p_idx = [0], [], []
    for G, P in shapes:
        base = fptr[-1]
        fptr.append(base + max(G, P))
        g_idx += list(range(base, base + G))
        p_idx += list(range(base, base + P))
    N = fptr[-1]

    def csr(idx):
        ptr = np.minimum(np.arange(N + 1), len(idx)).astype(np.int32)
        full = np.zeros(max(N, 1), np.int32)
        full[:len(idx)] = idx
        return _up(ptr, dev), _up(full, dev)

    g_off = np.concatenate(([0], np.cumsum([s[0] for s in shapes])))
    p_off = np.concatenate(([0], np.cumsum([s[1] for s in shapes])))
    return csr(g_idx), csr(p_idx), _up(np.asarray(fptr, np.int32), dev), N, g_off, p_off


def _check_singletons(shapes, centres, dev, eps=2.0, max_frame_nodes=None):
    """centres: per frame (gt [G, 2], pred [P, 2]) float32."""
    (g_ptr, g_idx), (p_ptr, p_idx), fptr, N, g_off, p_off = _singleton_batch(shapes, dev)
    g_mu, p_mu = np.zeros((N, 2), np.float32), np.zeros((N, 2), np.float32)
    for f, (cg, cp) in enumerate(centres):
        g_mu[g_off[f]:g_off[f + 1]] = cg
        p_mu[p_off[f]:p_off[f + 1]] = cp
    res = _ev().associate_l2(fptr, g_ptr, g_idx, p_ptr, p_idx, _up(g_mu, dev), _up(p_mu, dev), eps,
                             max_frame_nodes=max_frame_nodes)
    got = _ev().frame_picks(res)
    h = {k: v.cpu().numpy() for k, v in res.items()}
    assert int(h['bad_value'][0]) == 0
    for f, ((G, P), (cg, cp)) in enumerate(zip(shapes, centres)):
        want = l2ref.greedy(cg, cp, eps)
        assert len(want['gt']) == min(G, P)
        _same_picks(got[f], want, (f, G, P))
        s = int(h['pick_start'][f])
        _same(h['pick_gt_cluster'][s:s + min(G, P)], (want['gt'] + g_off[f]).astype(np.int32),
              (f, 'gt cluster'))
        _same(h['pick_pred_cluster'][s:s + min(G, P)], (want['pred'] + p_off[f]).astype(np.int32),
              (f, 'pred cluster'))
    assert int((h['pick_gt_cluster'] >= 0).sum()) == sum(min(G, P) for G, P in shapes)
    assert int(h['gt_kept'].sum()) == sum(G for G, _ in shapes)
    assert int(h['pred_kept'].sum()) == sum(P for _, P in shapes)


def _grid_centres(rng, n, extent):
    """n centres on the half-integer grid of [0, extent)^2: ties, but not everywhere."""
    return (rng.integers(0, 2 * extent, (n, 2)) * 0.5).astype(np.float32)


@pytest.mark.parametrize('G,P', [(1, 1), (1, 65), (65, 1), (64, 64), (63, 65), (257, 255),
                                 (600, 300), (300, 600)])
def test_single_frame_shapes(cuda_device, G, P):
    """Around the wave (64 columns a rescan step) and the workgroup (512 rows a pass)."""
    rng = np.random.default_rng(1000 * G + P)
    _check_singletons([(G, P)], [(_grid_centres(rng, G, 12), _grid_centres(rng, P, 12))],
                      cuda_device)


@pytest.mark.parametrize('G,P', [(LDS_CAP + 1, 8), (8, LDS_CAP + 1)])
def test_frame_past_the_lds_state(cuda_device, G, P):
    """4096 kept clusters a side is what the LDS state of a frame holds; one more on either
    side and the frame's state lives in the workspace."""
    rng = np.random.default_rng(G)
    _check_singletons([(G, P)], [(_grid_centres(rng, G, 40), _grid_centres(rng, P, 40))],
                      cuda_device)


def test_frame_past_max_frame_nodes(cuda_device):
    """A frame with more clusters than max_frame_nodes promised also runs from the workspace;
    the smaller frame beside it runs from LDS."""
    rng = np.random.default_rng(77)
    shapes = [(257, 255), (20, 31)]
    cen = [(_grid_centres(rng, G, 12), _grid_centres(rng, P, 12)) for G, P in shapes]
    _check_singletons(shapes, cen, cuda_device, max_frame_nodes=64)


def test_mixed_batch(cuda_device):
    """An empty frame, frames with one side empty, one cluster, and a large frame."""
    rng = np.random.default_rng(5)
    shapes = [(0, 0), (5, 0), (300, 280), (0, 7), (1, 1), (33, 90)]
    cen = [(_grid_centres(rng, G, 10), _grid_centres(rng, P, 10)) for G, P in shapes]
    _check_singletons(shapes, cen, cuda_device)


@pytest.mark.parametrize('mirror', [False, True])
def test_every_row_wants_the_same_column(cuda_device, mirror):
    """300 rows against 300 co-located columns (and the mirror): every round takes the column
    every remaining row had cached, so every remaining row is rescanned in every round."""
    rng = np.random.default_rng(300 + mirror)
    spread = _grid_centres(rng, 300, 20)
    same = np.tile(np.array([[7.5, 3.0]], np.float32), (300, 1))
    cen = (same, spread) if mirror else (spread, same)
    _check_singletons([(300, 300)], [cen], cuda_device, eps=9.0)


# ------------------------------------------------------------------ domain
def test_nan_centre_is_reported(cuda_device):
    """A NaN position in the second of three frames: that frame has no picks, the other two
    have theirs, and result() raises."""
    frames = _sweep_expected(1.5, 0)[0]
    frames = [dict(fr) for fr in frames if len(fr['key']) >= 8][:3]
    xy = frames[1]['xy'].copy()
    xy[3, 0] = np.nan
    frames[1]['xy'] = xy
    ev = _run_frames(frames, 1.5, 0, cuda_device)
    got = _ev().frame_picks(ev.last['assoc'])
    assert int(ev.last['assoc']['bad_value'].item()) == 1
    assert len(got[1]['gt']) == 0
    for f in (0, 2):
        gt, pred, _, _ = _frame_clusters(frames[f], 0)
        want = l2ref.greedy(l2ref.centres(frames[f]['xy'], gt), l2ref.centres(frames[f]['xy'], pred),
                            1.5)
        assert len(want['gt']) > 0
        _same_picks(got[f], want, (f,))
    with pytest.raises(RuntimeError, match='not finite'):
        ev.result()
    with pytest.raises(ValueError, match='xy'):
        _ev().DetectionEvaluator(NC, 1.5, association_criteria='l2_norm').update(
            _one_hot_logits(np.zeros(4, np.int64), cuda_device), None,
            _up(np.array([0, 4], np.int32), cuda_device), _up(np.arange(4, dtype=np.int32), cuda_device),
            _up(np.zeros(4, np.int64), cuda_device), _up(np.ones(4, np.int32), cuda_device),
            _up(np.array([0, 4], np.int32), cuda_device))


# ------------------------------------------------------------------ 'inv_iou' is untouched
def test_inv_iou_is_untouched(cuda_device):
    """The keyword at its default and at 'inv_iou' (positions given and ignored) count what
    the reference counted for the eval_batch5_eps07 fixture."""
    d = golden('eval_batch5_eps07')
    dev = cuda_device
    args = (_one_hot_logits(d['pred_node_class'], dev), None, _up(d['pred_cluster_ptr'], dev),
            _up(d['pred_cluster_idx'], dev), _up(d['node_class'], dev), _up(d['track_key'], dev),
            _up(d['frame_ptr'], dev))
    xy = torch.full((len(d['track_key']), 2), float('nan'), device=dev)
    a = _ev().DetectionEvaluator(NC, float(d['eps']), 0, True, FALSE).update(*args).result()
    b = _ev().DetectionEvaluator(NC, float(d['eps']), 0, True, FALSE,
                                 association_criteria='inv_iou').update(*args, xy=xy).result()
    for k in COUNTS:
        _same(a[k], d[k], k)
        _same(b[k], d[k], k + " ('inv_iou')")


# ------------------------------------------------------------------ end to end
def test_evaluate_window_batch_under_l2_norm(cuda_device):
    """evaluate_window_batch with an 'l2_norm' evaluator on the synthetic sequence: the centres
    in evaluator.last are the host's means of the batch's positions, and the counts are those
    the host reference accumulates from evaluator.last's clusters and centres."""
    import sequence_ref as sref
    from graph_neural_network_for_radar_perception_amd import sequence
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    name = 'model_trained_N50'
    mt = Model_Training(model_cfg(name), dev)
    mt.load_state_dict(model_state_dict(name))
    model = mt.to(dev).pred.eval().requires_grad_(False)
    model.set_param_for_proposal_extraction(float(golden('proposals_model_trained_N300')['eps']),
                                            False)
    cfg = model_cfg(name)
    radar, odo, lists, sensors = sref.adversarial_sequence()
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    eps = 1.5
    ev = _ev().DetectionEvaluator(int(cfg.num_classes), eps, association_criteria='l2_norm')
    fb, out = _ev().evaluate_window_batch(store.windows(range(0, 5), 4), model, cfg, ev)
    assert out is not None and fb.n_frames > 1
    last = ev.last
    N = fb.n_nodes
    fptr = fb.frame_ptr.cpu().numpy()
    xy = np.stack((fb.arrays['meas_px'].cpu().numpy(), fb.arrays['meas_py'].cpu().numpy()), -1)
    gt = {k: v.cpu().numpy() for k, v in last['gt'].items()}
    G = int(gt['n_clusters'][0])
    p_ptr, p_idx = out.cluster_ptr.cpu().numpy(), out.cluster_idx.cpu().numpy()
    sides = []
    for ptr, idx, ncl, cls, mu in (
            (gt['cluster_ptr'], gt['cluster_idx'], G, gt['cluster_class'], last['gt_mu']),
            (p_ptr, p_idx, len(p_ptr) - 1, last['pred_class'].cpu().numpy(), last['pred_mu'])):
        ncl = int(np.sum(np.diff(ptr[:ncl + 1]) > 0))      # without the slots of a padded CSR
        members = [idx[ptr[c]:ptr[c + 1]] for c in range(ncl)]
        mu = mu.cpu().numpy()
        assert mu.shape == (N, 2)
        _same(mu[:ncl], l2ref.centres(xy.astype(np.float32), members), 'centres')
        frame = np.searchsorted(fptr, [m[0] for m in members], side='right') - 1
        sides.append((frame, np.asarray(cls[:ncl]), mu))
    conf = np.zeros((NC, NC), np.uint64)
    gtc, prc = np.zeros(NC, np.uint64), np.zeros(NC, np.uint64)
    picks = _ev().frame_picks(last['assoc'])
    for f in range(fb.n_frames):
        (gf, gcls, gmu), (pf, pcls, pmu) = sides
        gi, pi = np.nonzero(gf == f)[0], np.nonzero(pf == f)[0]
        pk = l2ref.greedy(gmu[gi], pmu[pi], eps)
        _same_picks(picks[f], pk, (f,))
        l2ref.accumulate(conf, gtc, prc, gcls[gi].tolist(), pcls[pi].tolist(), pk, FALSE)
    res = ev.result()
    for k, w in zip(COUNTS, (conf, gtc, prc)):
        _same(res[k], w, k)
    assert int(res['confusion_matrix'].sum()) > 0
