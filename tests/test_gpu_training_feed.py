"""The training feed on the GPU (csrc/training_feed.hip, frontend.flip_along_x,
training.training_labels / step_frames / train_sequence): the flip and label kernels against
their numpy restatement (tests/training_feed_ref.py), the whole path from a SequenceStore
against the reference's own RadarScenesDataset.__getitem__
(tests/golden/training_feed_148_s40.npz), step_frames against step on host-made labels, and
train_sequence.

Every label comparison is exact: the outputs are integers, copies, exact negations or, for the
offsets, numpy's own float32 mean (rg_train_offsets)."""
import numpy as np
import pytest
import torch

import sequence_ref as sref
import training_feed_ref as tref
from conftest import golden
from sequence_ref import fixture_store

pytestmark = pytest.mark.gpu

POISON = -7777
FLIP_SIZES = (0, 1, 63, 64, 65, 130)
_CACHE = {}


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _up(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _cfg(**kw):
    from graph_neural_network_for_radar_perception_amd.config import default_config
    return default_config(**kw)


def _fixture(dev):
    if 'fixture' not in _CACHE:
        _CACHE['fixture'] = fixture_store(dev)
    return _CACHE['fixture']


def _static_store(dev):
    """Six small scenes: the windows of 2 scans at 0 and 1 hold no / one dynamic node."""
    if 'static' not in _CACHE:
        from graph_neural_network_for_radar_perception_amd import sequence
        sizes = (30, 20, 25, 40, 45, 33)
        kinds = ('static', 'static', 'static+1', 'mixed', 'mixed', 'mixed')
        radar, odo, lists, sensors = sref.make_sequence(11, sizes, kinds)
        _CACHE['static'] = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    return _CACHE['static']


# ------------------------------------------------------------------ 1. the flip kernel
def _flip_dict(dev, sizes=FLIP_SIZES, with_ptr=True, seed=3):
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    py = rng.normal(0, 30, n).astype(np.float32)
    vy = rng.normal(0, 5, n).astype(np.float32)
    if n >= 8:      # values whose negation is a sign bit only
        py[:4] = [0.0, -0.0, np.inf, np.nan]
        vy[-3:] = [1e-45, -3.4e38, 0.0]
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    d = {'meas_py': _up(py, np.float32, dev), 'meas_vy': _up(vy, np.float32, dev),
         '_n_windows': len(sizes) if with_ptr else 1}
    if with_ptr:
        d['_win_ptr'] = _up(ptr, np.int32, dev)
    return d, py, vy, (ptr if with_ptr else None)


@pytest.mark.parametrize('flags', [[1, 0, 1, 1, 0, 1], [0] * 6, [1] * 6, [0, 1, 0, 0, 1, 0]])
@pytest.mark.parametrize('as_tensor', [False, True])
def test_flip_windows(cuda_device, flags, as_tensor):
    from graph_neural_network_for_radar_perception_amd import frontend
    d, py, vy, ptr = _flip_dict(cuda_device)
    f = torch.tensor(flags, dtype=torch.bool, device=cuda_device) if as_tensor else flags
    assert frontend.flip_along_x(d, f) is d
    want_py, want_vy = tref.flip(py, vy, ptr, flags)
    np.testing.assert_array_equal(_bits(_np(d['meas_py'])), _bits(want_py))
    np.testing.assert_array_equal(_bits(_np(d['meas_vy'])), _bits(want_vy))
    for w, fl in enumerate(flags):       # untouched windows: bit-identical
        if not fl:
            sl = slice(int(ptr[w]), int(ptr[w + 1]))
            np.testing.assert_array_equal(_bits(_np(d['meas_py'])[sl]), _bits(py[sl]))
            np.testing.assert_array_equal(_bits(_np(d['meas_vy'])[sl]), _bits(vy[sl]))


def test_flip_single_window_and_empty(cuda_device):
    from graph_neural_network_for_radar_perception_amd import frontend
    for flag in (1, 0):                  # win_ptr None: one window over everything
        d, py, vy, _ = _flip_dict(cuda_device, sizes=(323,), with_ptr=False)
        assert '_win_ptr' not in d
        frontend.flip_along_x(d, [flag])
        want_py, want_vy = tref.flip(py, vy, None, [flag])
        np.testing.assert_array_equal(_bits(_np(d['meas_py'])), _bits(want_py))
        np.testing.assert_array_equal(_bits(_np(d['meas_vy'])), _bits(want_vy))
    for with_ptr in (True, False):       # no measurement at all
        d, _, _, _ = _flip_dict(cuda_device, sizes=(0,), with_ptr=with_ptr)
        frontend.flip_along_x(d, [1])
        assert d['meas_py'].numel() == 0
    d, _, _, _ = _flip_dict(cuda_device)
    with pytest.raises(ValueError, match='flip flags'):
        frontend.flip_along_x(d, [1, 0])
    torch.cuda.synchronize()


def test_flip_happens_before_the_grid_test(cuda_device):
    """py exactly -50 is inside [-50, 50) and 50 is not: unflipped the first measurement is
    kept, flipped the second (select_dynamic sees the flipped values)."""
    from graph_neural_network_for_radar_perception_amd import frontend
    dev = cuda_device
    for flag, kept in ((0, 0), (1, 1)):
        d = {'meas_px': _up([10.0, 20.0], np.float32, dev),
             'meas_py': _up([-50.0, 50.0], np.float32, dev),
             'meas_vy': _up([1.5, -2.5], np.float32, dev),
             '_win_ptr': _up([0, 2], np.int32, dev), '_n_windows': 1}
        gt = {'class_labels': _up([6.0, 6.0], np.float32, dev)}
        frontend.flip_along_x(d, [flag])
        dd, gd = frontend.select_dynamic(d, gt)
        sign = -1.0 if flag else 1.0
        np.testing.assert_array_equal(_np(dd['meas_px']), [[10.0, 20.0][kept]])
        np.testing.assert_array_equal(_np(dd['meas_py']), [sign * [-50.0, 50.0][kept]])
        np.testing.assert_array_equal(_np(dd['meas_vy']), [sign * [1.5, -2.5][kept]])
        np.testing.assert_array_equal(_np(dd['frame_ptr']), [0, 1])


# ------------------------------------------------------------------ 2. the label kernel
def _run_labels(dev, cls, ox, oy, key, ps, pd, n_pairs, cap):
    """rg_train_labels on host arrays; pair slots past len(ps) hold indices far outside the
    nodes, every output is pre-filled with poison."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    N = len(cls)
    pad = np.full(max(cap - len(ps), 0), 10 ** 9)
    t_ps = _up(np.concatenate((ps, pad)), np.int32, dev)
    t_pd = _up(np.concatenate((pd, pad)), np.int32, dev)
    t_cls, t_ox, t_oy = (_up(a, np.float32, dev) for a in (cls, ox, oy))
    t_key = _up(key, np.int32, dev)
    t_n = _up([n_pairs], np.int32, dev)
    nc = torch.full((max(N, 1),), POISON, dtype=torch.int64, device=dev)
    no = torch.full((max(N, 1), 2), float(POISON), dtype=torch.float32, device=dev)
    ec = torch.full((max(cap, 1),), POISON, dtype=torch.int64, device=dev)
    nat.check(nat.lib().rg_train_labels(
        t_cls.data_ptr(), t_ox.data_ptr(), t_oy.data_ptr(), N, t_key.data_ptr(), t_ps.data_ptr(),
        t_pd.data_ptr(), t_n.data_ptr(), cap, nc.data_ptr(), no.data_ptr(), ec.data_ptr(),
        nat.stream_ptr(dev)), 'rg_train_labels')
    return _np(nc), _np(no), _np(ec)


def test_labels_two_nodes_one_pair(cuda_device):
    for keys, want in (([3, 3], 1), ([3, 4], 0), ([0, 0], 0), ([0, 3], 0), ([3, 0], 0)):
        nc, no, ec = _run_labels(cuda_device, [2.0, 6.0], [0.5, -0.25], [1.5, 0.0], keys, [0], [1],
                                 1, 1)
        np.testing.assert_array_equal(nc, [2, 6])
        np.testing.assert_array_equal(no, [[0.5, 1.5], [-0.25, 0.0]])
        np.testing.assert_array_equal(ec, [want])


def test_labels_without_pairs(cuda_device):
    """Frames whose graph has no pair at all (n_pairs 0): the whole capacity reads 0; no
    capacity: the pair outputs are not written; no node: nothing is written."""
    cls = np.array([6.0, 1.0, 6.0, 0.0, 4.0], np.float32)
    ox = np.arange(5, dtype=np.float32)
    nc, no, ec = _run_labels(cuda_device, cls, ox, -ox, [0, 2, 0, 2, 9], [], [], 0, 5)
    np.testing.assert_array_equal(nc, cls.astype(np.int64))
    np.testing.assert_array_equal(_bits(no), _bits(np.stack((ox, -ox), -1)))
    np.testing.assert_array_equal(ec, np.zeros(5, np.int64))
    nc, no, ec = _run_labels(cuda_device, cls, ox, -ox, [0, 2, 0, 2, 9], [], [], 0, 0)
    np.testing.assert_array_equal(nc, cls.astype(np.int64))
    np.testing.assert_array_equal(ec, [POISON])
    nc, no, ec = _run_labels(cuda_device, [], [], [], [], [], [], 0, 0)
    assert nc[0] == POISON and ec[0] == POISON and (no == POISON).all()


@pytest.mark.parametrize('U', [63, 64, 65, 257])
def test_labels_pair_counts_and_padding(cuda_device, U):
    """U pairs in a capacity of U + 70 poisoned slots: the labels of the restatement, 0 in the
    tail (whose pair slots hold indices far outside the nodes, never read); N != U on both
    sides (N = 40 < U, and N = 300 > U + 70 for the small U)."""
    rng = np.random.default_rng(U)
    for N in (40, 300):
        key = rng.choice([0, 0, 5, 5, 9, 12], N)
        cls = rng.integers(0, 7, N).astype(np.float32)
        ox, oy = rng.normal(0, 3, (2, N)).astype(np.float32)
        ps = rng.integers(0, N - 1, U)
        pd = np.array([rng.integers(s + 1, N) for s in ps])
        nc, no, ec = _run_labels(cuda_device, cls, ox, oy, key, ps, pd, U, U + 70)
        want = tref.edge_labels(key, ps, pd)
        assert want.any() and not want.all()
        np.testing.assert_array_equal(ec[:U], want)
        np.testing.assert_array_equal(ec[U:], np.zeros(70, np.int64))
        np.testing.assert_array_equal(nc, cls.astype(np.int64))
        np.testing.assert_array_equal(_bits(no), _bits(np.stack((ox, oy), -1)))
        # a device count past the capacity is cut to it
        _, _, ec2 = _run_labels(cuda_device, cls, ox, oy, key, ps, pd, U + 1000, U)
        np.testing.assert_array_equal(ec2, want)


def test_labels_key_patterns(cuda_device):
    key = [0, 0, 7, 7, 8, 0, 7]
    ps, pd = [0, 2, 2, 0, 4, 3, 5], [1, 3, 4, 2, 6, 6, 6]
    #          0/0 k/k k/k' 0/k k'/k k/k 0/k
    _, _, ec = _run_labels(cuda_device, np.zeros(7), np.zeros(7), np.zeros(7), key, ps, pd, 7, 9)
    np.testing.assert_array_equal(ec, [0, 1, 0, 0, 0, 1, 0, 0, 0])


def test_same_track_in_two_windows_does_not_link(cuda_device):
    """One sliding position twice in a batch: the store offsets the second window's keys by
    n_tracks, so a pair across the two frames of the same raw track reads 0."""
    from graph_neural_network_for_radar_perception_amd import frontend
    _, store = _fixture(cuda_device)
    dd, gd = frontend.dynamic_frame(store.windows([7, 7], 10), with_keys=True)
    fb = frontend.frame_batch(dd, gd)
    n0 = fb.frame_sizes[0]
    assert fb.frame_sizes == [n0, n0]
    key = _np(fb.track_key).astype(np.int64)
    tracked = np.flatnonzero(key[:n0] > 0)
    assert tracked.size > 10
    np.testing.assert_array_equal(key[tracked + n0] - key[tracked], store.n_tracks)
    same = tracked[key[tracked] == key[tracked[0]]]
    assert same.size >= 2
    ps = np.concatenate((tracked, same[:1]))          # across the frames, then inside one
    pd = np.concatenate((tracked + n0, same[1:2]))
    z = np.zeros(2 * n0, np.float32)
    _, _, ec = _run_labels(cuda_device, z, z, z, key, ps, pd, len(ps), len(ps))
    np.testing.assert_array_equal(ec, [0] * tracked.size + [1])


# ------------------------------------------------------------------ 2b. the offsets kernel
def _numpy_offsets(key, px, py):
    """generate_gt_offset's semantics: per track, numpy's mean of the float32 values in
    measurement order minus the values; 0 without a track."""
    ox, oy = np.zeros(len(px), np.float32), np.zeros(len(px), np.float32)
    for k in np.unique(key[key > 0]):
        m = key == k
        ox[m] = np.mean(px[m]) - px[m]
        oy[m] = np.mean(py[m]) - py[m]
    return ox, oy


def _run_offsets(dev, key, n_tracks, px, py):
    from graph_neural_network_for_radar_perception_amd import _native as nat
    lib = nat.lib()
    n = len(key)
    t_key, t_px, t_py = _up(key, np.int32, dev), _up(px, np.float32, dev), _up(py, np.float32, dev)
    ox = torch.full((max(n, 1),), float(POISON), dtype=torch.float32, device=dev)
    oy = torch.full((max(n, 1),), float(POISON), dtype=torch.float32, device=dev)
    ws = torch.full((lib.rg_train_offsets_workspace_size(n_tracks),), 0xA5, dtype=torch.uint8,
                    device=dev)
    nat.check(lib.rg_train_offsets(t_key.data_ptr(), n_tracks, t_px.data_ptr(), t_py.data_ptr(), n,
                                   ox.data_ptr(), oy.data_ptr(), ws.data_ptr(), ws.numel(),
                                   nat.stream_ptr(dev)), 'rg_train_offsets')
    return _np(ox)[:n], _np(oy)[:n]


# every branch of numpy's pairwise sum: below 8, the blocks of 8 with and without a tail, the
# block limit 128 and the split above it (one level: 129..256, two: 257.., three: 513..)
TRACK_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 64, 127, 128, 129, 136, 137, 255, 256, 257, 273, 600,
               1031)


def test_offsets_take_numpys_float32_mean(cuda_device):
    """Tracks of every size in TRACK_SIZES, their measurements interleaved at random with each
    other and with untracked ones (n_meas is no multiple of 64); keys 3 and 11 never occur.
    The offsets equal numpy's bit for bit, and differ somewhere from a float64 mean's (else
    the case would not tell the two apart)."""
    rng = np.random.default_rng(21)
    keys = [k for k in range(1, len(TRACK_SIZES) + 3) if k not in (3, 11)]
    key = np.concatenate([np.full(s, k) for s, k in zip(TRACK_SIZES, keys)] + [np.zeros(331)])
    key = rng.permutation(key).astype(np.int32)
    n = len(key)
    assert n % 64 and len(keys) == len(TRACK_SIZES)
    px = rng.uniform(0, 100, n).astype(np.float32)
    py = rng.uniform(-50, 50, n).astype(np.float32)
    want_x, want_y = _numpy_offsets(key, px, py)
    ox, oy = _run_offsets(cuda_device, key, max(keys), px, py)
    np.testing.assert_array_equal(_bits(ox), _bits(want_x))
    np.testing.assert_array_equal(_bits(oy), _bits(want_y))
    f64 = np.zeros(n, np.float32)
    for k in keys:
        m = key == k
        f64[m] = np.float32(px[m].astype(np.float64).mean()) - px[m]
    assert (f64 != want_x).any()
    # negated values (the flip): the negated offsets, a zero offset staying +0
    _, oy2 = _run_offsets(cuda_device, key, max(keys), px, -py)
    np.testing.assert_array_equal(_bits(oy2), _bits(-want_y + np.float32(0)))


def test_offsets_edge_cases(cuda_device):
    """No measurement; no track at all; one track over everything, first member at 0; keys
    outside [1, n_tracks] count as untracked."""
    dev = cuda_device
    ox, oy = _run_offsets(dev, np.zeros(0, np.int32), 5, np.zeros(0), np.zeros(0))
    assert ox.size == 0 and oy.size == 0
    rng = np.random.default_rng(4)
    px, py = rng.uniform(-50, 100, (2, 200)).astype(np.float32)
    for n_tracks in (0, 6):
        ox, oy = _run_offsets(dev, np.zeros(200, np.int32), n_tracks, px, py)
        assert not ox.any() and not oy.any()
    key = np.full(200, 2, np.int32)
    want = _numpy_offsets(key, px, py)
    got = _run_offsets(dev, key, 2, px, py)
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
    key[::3] = 9
    key[1::3] = -4
    want = _numpy_offsets(np.where(key == 2, 2, 0), px, py)
    got = _run_offsets(dev, key, 2, px, py)
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))


def test_front_end_without_flip_keeps_its_offsets(cuda_device):
    """dynamic_frame without ``flip`` is the path as it was (compute_ground_truth's float64
    mean); ``numpy_mean`` alone changes the offsets, and nothing but the offsets."""
    from graph_neural_network_for_radar_perception_amd import frontend
    _, store = _fixture(cuda_device)
    win = store.windows([7], 10)
    d = frontend.extract_and_sync_radar_data(win)
    dd0, gd0 = frontend.select_dynamic(d, frontend.compute_ground_truth(d))
    dd1, gd1 = frontend.dynamic_frame(win)
    dd2, gd2 = frontend.dynamic_frame(win, numpy_mean=True)
    dd3, gd3 = frontend.dynamic_frame(win, flip=[0], numpy_mean=False)
    for k in gd0:
        np.testing.assert_array_equal(_bits(_np(gd1[k])), _bits(_np(gd0[k])))
        np.testing.assert_array_equal(_bits(_np(gd3[k])), _bits(_np(gd0[k])))
    np.testing.assert_array_equal(_np(gd2['class_labels']), _np(gd0['class_labels']))
    for k in dd0:
        np.testing.assert_array_equal(_np(dd2[k]), _np(dd0[k]))
    pre = tref.case_key(10, 7, 0)
    want = golden(tref.FIXTURE)[pre + 'node_offsets']
    got = np.stack((_np(gd2['offsetx']), _np(gd2['offsety'])), -1)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert np.abs(np.stack((_np(gd0['offsetx']), _np(gd0['offsety'])), -1) - want).max() <= 2e-5


# ------------------------------------------------------------------ 3. against the reference
def _labels_of_case(dev, W, pos, flipped):
    key = (W, pos, flipped)
    if key not in _CACHE:
        from graph_neural_network_for_radar_perception_amd import frontend, training
        from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
        cfg = _cfg()
        _, store = _fixture(dev)
        dd, gd = frontend.dynamic_frame(store.windows([pos], W), with_keys=True, flip=[flipped])
        fb = frontend.frame_batch(dd, gd)
        gb = build_graph_batch(fb, cfg)
        _CACHE[key] = (fb, gb, training.training_labels(fb, gb, cfg))
    return _CACHE[key]


def _check_frame(d, pre, lab, gb, fb, a, b, u0, u1, c0, c1):
    """Frame [a, b) of a batch (pairs [u0, u1), clusters [c0, c1)) against fixture case pre."""
    src, dst = tref.link_pairs(d[pre + 'edge_index'])
    assert b - a == len(d[pre + 'px']) and u1 - u0 == len(src)
    np.testing.assert_array_equal(_np(gb.graph.pair_src[u0:u1]) - a, src)
    np.testing.assert_array_equal(_np(gb.graph.pair_dst[u0:u1]) - a, dst)
    np.testing.assert_array_equal(_np(lab['edge_class'][u0:u1]), d[pre + 'edge_class'])
    np.testing.assert_array_equal(_np(lab['node_class'][a:b]), d[pre + 'node_class'])
    np.testing.assert_array_equal(_bits(_np(lab['node_offsets'][a:b])),
                                  _bits(d[pre + 'node_offsets']))
    np.testing.assert_array_equal(_bits(_np(fb.arrays['meas_px'][a:b])), _bits(d[pre + 'px']))
    np.testing.assert_array_equal(_bits(_np(fb.arrays['meas_py'][a:b])), _bits(d[pre + 'py']))
    ptr = _np(lab['cluster_ptr'][c0:c1 + 1]).astype(np.int64)
    np.testing.assert_array_equal(ptr - ptr[0], d[pre + 'cluster_ptr'])
    np.testing.assert_array_equal(_np(lab['cluster_idx'][ptr[0]:ptr[-1]]) - a,
                                  d[pre + 'cluster_idx'])
    np.testing.assert_array_equal(_np(lab['cluster_labels'][c0:c1]), d[pre + 'cluster_labels'])


@pytest.mark.parametrize('W,pos,flipped', [(W, p, f) for W, p in tref.CASES for f in (0, 1)])
def test_labels_from_the_store_match_reference(cuda_device, W, pos, flipped):
    d = golden(tref.FIXTURE)
    pre = tref.case_key(W, pos, flipped)
    fb, gb, lab = _labels_of_case(cuda_device, W, pos, flipped)
    N, U = fb.n_nodes, int(gb.graph.n_pairs_dev.item())
    ncl = int(lab['n_clusters_dev'].item())
    assert lab['node_class'].dtype == lab['edge_class'].dtype == torch.int64
    assert lab['cluster_labels'].dtype == torch.int64
    assert lab['node_offsets'].dtype == torch.float32 and lab['node_offsets'].shape == (N, 2)
    assert lab['edge_class'].shape[0] == gb.graph.pair_src.shape[0] > U
    assert ncl == len(d[pre + 'cluster_labels'])
    _check_frame(d, pre, lab, gb, fb, 0, N, 0, U, 0, ncl)
    assert not bool(lab['edge_class'][U:].any())       # the capacity's tail reads 0
    # the offsets are the front-end's, interleaved bit for bit
    want = torch.stack((fb.labels['offsetx'], fb.labels['offsety']), -1)
    np.testing.assert_array_equal(_bits(_np(lab['node_offsets'])), _bits(_np(want)))
    np.testing.assert_array_equal(_np(lab['class_weights']),
                                  np.array(_cfg().class_weights_dyn, np.float32))
    if flipped:     # against the unflipped run: exact negations of the same selection
        fb0, _, lab0 = _labels_of_case(cuda_device, W, pos, 0)
        for k in ('meas_py', 'meas_vy'):
            np.testing.assert_array_equal(_np(fb.arrays[k]), -_np(fb0.arrays[k]))
        np.testing.assert_array_equal(_np(lab['node_offsets'][:, 1]),
                                      -_np(lab0['node_offsets'][:, 1]))
        np.testing.assert_array_equal(_bits(_np(lab['node_offsets'][:, 0])),
                                      _bits(_np(lab0['node_offsets'][:, 0])))


def test_node_offsets_from_the_store_match_reference(cuda_device):
    """node_offsets against the reference's items, exactly, for all eight cases.

    The front-end's own offsets (rg_frontend_labels) take each track's mean in float64 and
    differ from numpy's float32 mean in the last bit for about a third of the values; the
    training feed retakes them with numpy's mean (rg_train_offsets), so the comparison is
    exact, as set for every label of this feed."""
    d = golden(tref.FIXTURE)
    pairs = []
    for W, pos in tref.CASES:
        for flipped in (0, 1):
            pre = tref.case_key(W, pos, flipped)
            _, _, lab = _labels_of_case(cuda_device, W, pos, flipped)
            got, want = _np(lab['node_offsets']), d[pre + 'node_offsets']
            diff = np.abs(got.astype(np.float64) - want)
            print(f'{pre} node_offsets: {int((got != want).sum())} of {want.size} differ, '
                  f'max |diff| {diff.max():.3e}')
            pairs.append((pre, got, want))
    for pre, got, want in pairs:
        np.testing.assert_array_equal(got, want, err_msg=pre)


def _mixed_batch(dev):
    """The three W=10 fixture positions, flip off and on, and two windows of static scenes
    (no / one dynamic node, dropped by frame_batch) as ONE batch of 8 windows."""
    if 'mixed' not in _CACHE:
        from graph_neural_network_for_radar_perception_amd import frontend
        _, store = _fixture(dev)
        st = _static_store(dev)
        slots = [(0, 0), (0, 1), (7, 0), (7, 1), None, (30, 0), (30, 1), None]
        static_pos = iter((0, 1))
        host = [store.host_window(s[0], 10) if s else st.host_window(next(static_pos), 2)
                for s in slots]
        flags = [s[1] if s else 1 for s in slots]
        win = frontend.scan_window_batch(host, dev)
        dd, gd = frontend.dynamic_frame(win, with_keys=True, flip=flags)
        sizes = np.diff(_np(dd['frame_ptr']))
        assert sizes[4] == 0 and sizes[7] == 1
        _CACHE['mixed'] = (frontend.frame_batch(dd, gd), [s for s in slots if s])
    return _CACHE['mixed']


def _check_batch(d, cfg, fb, cases):
    """Every frame of the batch ``fb`` (graph build, training_labels) against the fixture
    cases ``cases`` [(pos, flipped)], W = 10."""
    from graph_neural_network_for_radar_perception_amd import training
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
    gb = build_graph_batch(fb, cfg)
    lab = training.training_labels(fb, gb, cfg, ws_cache={})
    fp = _np(fb.frame_ptr)
    U = int(gb.graph.n_pairs_dev.item())
    u = np.searchsorted(_np(gb.graph.pair_src[:U]), fp)
    ncl = int(lab['n_clusters_dev'].item())
    first = _np(lab['cluster_idx'])[_np(lab['cluster_ptr'][:ncl])]
    frame_of = np.searchsorted(fp, first, side='right') - 1
    assert (np.diff(frame_of) >= 0).all()
    c = np.searchsorted(frame_of, np.arange(fb.n_frames + 1))
    assert fb.n_frames == len(cases)
    for f, (pos, flipped) in enumerate(cases):
        _check_frame(d, tref.case_key(10, pos, flipped), lab, gb, fb, int(fp[f]), int(fp[f + 1]),
                     int(u[f]), int(u[f + 1]), int(c[f]), int(c[f + 1]))
    assert u[-1] == U and c[-1] == ncl
    assert not bool(lab['edge_class'][U:].any())


def test_batch_of_windows_matches_reference(cuda_device):
    fb, cases = _mixed_batch(cuda_device)
    assert fb.windows == [0, 1, 2, 3, 5, 6] and fb.n_frames == 6
    _check_batch(golden(tref.FIXTURE), _cfg(), fb, cases)


def test_store_batch_with_mixed_flags_matches_reference(cuda_device):
    """The layout train_sequence uses: several sliding positions cut by store.windows as ONE
    batch (keys offset per window, window boundaries at no multiple of 64, a position twice
    with both flags, flipped and unflipped windows side by side) -> flip -> ground truth with
    numpy's mean -> frame_batch -> labels; every frame equals its fixture item, offsets
    included."""
    from graph_neural_network_for_radar_perception_amd import frontend
    d = golden(tref.FIXTURE)
    _, store = _fixture(cuda_device)
    cases = [(7, 1), (0, 0), (30, 1), (7, 0), (0, 1), (30, 0)]
    win = store.windows([p for p, _ in cases], 10)
    assert any(int(v) % 64 for v in _np(win.win_ptr)[1:-1])
    dd, gd = frontend.dynamic_frame(win, with_keys=True, flip=[f for _, f in cases])
    _check_batch(d, _cfg(), frontend.frame_batch(dd, gd), cases)


# ------------------------------------------------------------------ 4. step_frames
def _trainer(dev, cfg, seed=31):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    from graph_neural_network_for_radar_perception_amd.training import RadarGNNTrainer
    torch.manual_seed(seed)
    m = Model_Training(cfg, 'cpu').to(dev).train()
    return RadarGNNTrainer(m, cfg, world=1)


def test_step_frames_equals_step_on_host_labels(cuda_device):
    """The first step of step_frames on the mixed batch == step on the same frames with the
    ground-truth clusters in the batch and the labels restated on the host and uploaded, bit
    for bit (two identical step calls are bit-equal)."""
    from graph_neural_network_for_radar_perception_amd.graph_features import (FrameBatch,
                                                                                build_graph_batch)
    dev = cuda_device
    cfg = _cfg(graph_convolution_stem_channels=[64] * 2)
    fb, _ = _mixed_batch(dev)
    tr = _trainer(dev, cfg)
    losses, acc, gb = tr.step_frames(fb)
    assert tr.opt.applied_steps() == 1
    # the path a caller writes without the feed: build, download, label in numpy, upload, step
    ei = _np(build_graph_batch(fb, cfg).edge_index())
    key = _np(fb.track_key)
    cls = _np(fb.labels['class_labels']).astype(np.int64)
    src, dst = tref.link_pairs(ei)
    ptr, idx, clab = tref.gt_clusters(key, cls, _np(fb.frame_ptr))
    host = {'node_class': cls,
            'node_offsets': np.stack((_np(fb.labels['offsetx']), _np(fb.labels['offsety'])), -1),
            'edge_class': tref.edge_labels(key, src, dst), 'cluster_labels': clab}
    up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    up['class_weights'] = torch.tensor(cfg.class_weights_dyn, dtype=torch.float32, device=dev)
    batch = FrameBatch(fb.arrays, fb.frame_ptr, fb.frame_sizes, _up(ptr, np.int32, dev),
                       _up(idx, np.int32, dev), len(clab))
    tr2 = _trainer(dev, cfg)
    losses2, acc2, _ = tr2.step(batch, up)
    assert torch.isfinite(losses).all() and float(losses.sum()) > 0
    assert torch.equal(losses, losses2) and torch.equal(acc, acc2)
    assert torch.equal(tr.opt.flat, tr2.opt.flat)
    assert gb.graph.n_pairs == len(src) and gb.graph.n_edges == ei.shape[1]


def test_step_frames_skips_an_empty_batch(cuda_device):
    from graph_neural_network_for_radar_perception_amd import frontend
    dev = cuda_device
    cfg = _cfg(graph_convolution_stem_channels=[64] * 2)
    st = _static_store(dev)
    dd, gd = frontend.dynamic_frame(st.windows([0, 0], 2), with_keys=True, flip=[0, 1])
    fb = frontend.frame_batch(dd, gd)
    assert fb.n_frames == 0
    tr = _trainer(dev, cfg)
    before = tr.opt.flat.clone()
    assert tr.step_frames(fb) is None
    assert torch.equal(tr.opt.flat, before) and tr.opt.applied_steps() == 0 and tr.opt.steps == 0


def test_step_frames_empty_batch_on_one_of_several_ranks(cuda_device, monkeypatch):
    """world > 1, this rank's batch empty: the rank joins the all-reduce (stubbed here: the
    peer's finite gradients and losses are added to the bucket) with zero gradients and NaN
    loss slots, so the summed loss is NaN and the optimizer launch skips the update: the
    weights and applied_steps stay, one launch is counted."""
    from graph_neural_network_for_radar_perception_amd import frontend, training
    dev = cuda_device
    cfg = _cfg(graph_convolution_stem_channels=[64] * 2)
    st = _static_store(dev)
    dd, gd = frontend.dynamic_frame(st.windows([0, 0], 2), with_keys=True, flip=[0, 1])
    fb = frontend.frame_batch(dd, gd)
    assert fb.n_frames == 0
    tr = _trainer(dev, cfg)
    tr.world = 2
    eng = tr.engine
    eng.flat_grad.fill_(3.0)                  # stale values the branch must clear
    calls = []

    def peer_sum(bucket, world):
        assert bucket is eng.flat_bucket and world == 2
        assert not bool(eng.flat_grad.any()) and bool(torch.isnan(eng.loss_slots).all())
        calls.append(world)
        bucket.add_(0.25)                     # the other rank's contribution
        return 0.5

    monkeypatch.setattr(training, 'allreduce_gradients', peer_sum)
    before = tr.opt.flat.clone()
    assert tr.step_frames(fb) is None
    assert calls == [2]
    assert bool((eng.flat_grad == 0.25).all()) and bool(torch.isnan(eng.loss_slots).all())
    assert torch.equal(tr.opt.flat, before)
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 1


# ------------------------------------------------------------------ 5. train_sequence
def test_train_sequence_three_steps(cuda_device):
    from graph_neural_network_for_radar_perception_amd import frontend, sequence, training
    dev = cuda_device
    cfg = _cfg(graph_convolution_stem_channels=[64] * 2)
    assert cfg.dataset_augmentation is True
    radar, odo, lists, sensors = sref.adversarial_sequence()
    store = sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev)
    tr = _trainer(dev, cfg)
    before = tr.opt.flat.clone()
    order = [14, 3, 9, 0, 20, 7, 7, 11, 1, 18, 5, 16, 2]       # the caller's order, a repeat
    seen = []
    np.random.seed(77)
    losses, acc = training.train_sequence(
        store, tr, cfg, order, window_size=4, batch_windows=5,
        on_step=lambda k, pos, flags, out: seen.append((k, list(pos), flags, out)))
    np.random.seed(77)
    want_flags = [frontend.draw_flips(n) for n in (5, 5, 3)]
    assert [s[0] for s in seen] == [0, 1, 2]
    assert [s[1] for s in seen] == [order[:5], order[5:10], order[10:]]
    for s, w in zip(seen, want_flags):
        np.testing.assert_array_equal(s[2], w)
    assert np.concatenate(want_flags).any() and not np.concatenate(want_flags).all()
    assert losses.shape == (3, 4) and acc.shape == (3, 3) and losses.is_cuda
    assert torch.isfinite(losses).all() and torch.isfinite(acc).all()
    assert torch.equal(losses[0], seen[0][3][0])
    assert tr.opt.applied_steps() == 3
    assert not torch.equal(tr.opt.flat, before)
    # the drawn flags reached the data: the first step's edge features (relative positions and
    # velocities: a flip changes their y parts; the node features are mirror-invariant) are
    # those of the same windows flipped by those flags, and not those of the opposite flags
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch

    def features(flags):
        dd, gd = frontend.dynamic_frame(store.windows(order[:5], 4), with_keys=True, flip=flags)
        gb = build_graph_batch(frontend.frame_batch(dd, gd), cfg)
        return gb.edge_features[:int(gb.n_edges_dev.item())]

    assert want_flags[0].any()
    got = seen[0][3][2]
    got = got.edge_features[:int(got.n_edges_dev.item())]
    assert got.shape[0] > 100
    assert torch.equal(got, features(want_flags[0]))
    other = features(~want_flags[0])
    assert other.shape == got.shape and not torch.equal(got, other)
    # augmentation off: nothing is drawn
    state = np.random.get_state()[1].copy()
    training.train_sequence(store, tr, cfg, order[:2], window_size=4, batch_windows=2,
                            augmentation=False,
                            on_step=lambda k, pos, flags, out: seen.append(flags))
    assert seen[-1] is None
    np.testing.assert_array_equal(np.random.get_state()[1], state)
