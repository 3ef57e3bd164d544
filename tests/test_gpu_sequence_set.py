"""sequence.SequenceSet on the GPU (csrc/sequence.hip, rg_sequence_set_windows) and the detector
loop built on it (training.validate_frames / validate_sequence / save / train_dataset).

The cut is compared bit for bit: with SequenceStore.windows for a set of one, with the host
path (host_window -> scan_window_batch) and with the numpy restatement
(tests/sequence_set_ref.py) for mixed batches; the entry point is also called directly into
guarded buffers.  Downstream comparisons are two runs of the same kernels on the same values
and are exact too.  The one tolerance is on validate_sequence's float64 means against numpy's
float64 mean of the same <= 3 positive float32 rows: the two may add them in another order, two
additions of relative error <= 2^-53 each on either side, so rtol 4e-15 is asked."""
import ctypes

import numpy as np
import pytest
import torch

import sequence_ref as sref
import sequence_set_ref as ssref
from conftest import golden, model_cfg, model_state_dict
from sequence_set_ref import DATA_KEYS, PER_SCAN, make_set, set_cut

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 256


def _mods():
    from graph_neural_network_for_radar_perception_amd import frontend, sequence, training
    return sequence, frontend, training


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(_bits(_np(got)), _bits(_np(want)), err_msg=what)


def _cfg():
    from graph_neural_network_for_radar_perception_amd.config import default_config
    return default_config(graph_convolution_stem_channels=[64] * 2)


def _trainer(dev, cfg, seed=31):
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    from graph_neural_network_for_radar_perception_amd.training import RadarGNNTrainer
    torch.manual_seed(seed)
    m = Model_Training(cfg, 'cpu').to(dev).train()
    return RadarGNNTrainer(m, cfg, world=1)


def _private_set(dev, members=(0, 2)):
    """Stores of this test's own (a test that writes into a store, or wants fewer members)."""
    sequence = _mods()[0]
    inputs = ssref.member_inputs()
    return sequence.SequenceSet([sequence.SequenceStore.from_numpy(*inputs[i], dev)
                                 for i in members])


def _check_against_restatement(sset, got, g, W):
    seq, pos = sset.locate(g, W)
    ref = set_cut(sset.stores, sset.n_tracks, list(zip(seq.tolist(), pos.tolist())), W)
    for k in PER_SCAN + ('src_row', 'meas_scan', 'track_key'):
        t = getattr(got, k)
        assert t.dtype == {'mount': torch.float64, 'odometry': torch.float64}.get(k, torch.int32)
        np.testing.assert_array_equal(_bits(_np(t).reshape(ref[k].shape)), _bits(ref[k]),
                                      err_msg=f'{k} W={W}')
    for k in DATA_KEYS:
        np.testing.assert_array_equal(_bits(_np(got.arrays[k])), _bits(ref[k]), err_msg=k)
    np.testing.assert_array_equal(_np(got.win_seq), seq)
    assert got.win_seq.dtype == torch.int32 and got.n_tracks == len(g) * sset.n_tracks
    return ref


# ------------------------------------------------------------------ 1. a set of one store
@pytest.mark.parametrize('W', [1, 4, 10, 24])
def test_one_store_set_equals_store_windows(cuda_device, W):
    from test_gpu_sequence import _index_sets
    sequence = _mods()[0]
    store = make_set(cuda_device).stores[0]
    one = sequence.SequenceSet([store])
    assert one.n_windows(W) == store.n_windows(W) and one.n_tracks == store.n_tracks
    for idx in _index_sets(store.n_windows(W)):
        got, want = one.windows(idx, W), store.windows(idx, W)
        assert (got.n_windows, got.n_scans, got.n_meas, got.n_tracks) == \
            (want.n_windows, want.n_scans, want.n_meas, want.n_tracks)
        assert set(got.arrays) == set(want.arrays)
        for k in want.arrays:
            _same(got.arrays[k], want.arrays[k], f'{k} W={W} {idx}')
        for k in PER_SCAN + ('track_key', 'meas_scan', 'src_row'):
            _same(getattr(got, k), getattr(want, k), f'{k} W={W} {idx}')
        assert not bool(got.win_seq.any())


# ------------------------------------------------------------------ 2. mixed == host path
def _mixed_indices(sset, W):
    """Global windows that straddle every member boundary (last of s, first of the next member
    that has a window), repeat a window and visit the members out of order."""
    st = sset._starts(W)
    have = [s for s in range(len(sset.stores)) if st[s + 1] > st[s]]
    g = []
    for s in have[:-1]:
        g += [int(st[s + 1]) - 1, int(st[s + 1])]
    g += [g[0], g[0]]
    g += [int(st[have[-1]]), int(st[have[0]]), int(st[have[-1] + 1]) - 1, int(st[have[1]])]
    return g


@pytest.mark.parametrize('W', [1, 4, 10])
def test_mixed_batch_equals_host_path(cuda_device, W):
    _, frontend, _ = _mods()
    sset = make_set(cuda_device)
    T = sset.n_tracks
    g = _mixed_indices(sset, W)
    seq, _ = sset.locate(g, W)
    assert len(set(seq.tolist())) == (4 if W < 4 else 3) and (np.diff(seq) < 0).any()
    got = sset.windows(g, W)
    host = [sset.host_window(x, W) for x in g]
    want = frontend.scan_window_batch(host, cuda_device)
    assert (got.n_windows, got.n_scans, got.n_meas) == (want.n_windows, want.n_scans,
                                                        want.n_meas) == \
        (len(g), len(g) * W, sum(len(h['x_cc']) for h in host))
    assert set(got.arrays) == set(want.arrays)
    for k in want.arrays:
        _same(got.arrays[k], want.arrays[k], f'{k} W={W}')
    for k in PER_SCAN:
        _same(getattr(got, k), getattr(want, k), f'{k} W={W}')
    gk, wk = _np(got.track_key).astype(np.int64), _np(want.track_key).astype(np.int64)
    assert got.track_key.dtype == torch.int32
    np.testing.assert_array_equal(gk == 0, wk == 0)
    np.testing.assert_array_equal(np.unique(gk, return_inverse=True)[1],
                                  np.unique(wk, return_inverse=True)[1])
    wp = _np(got.win_ptr)
    for b in range(len(g)):
        k = gk[wp[b]:wp[b + 1]]
        k = k[k > 0]
        assert ((k > b * T) & (k <= (b + 1) * T)).all()
    assert (gk > 0).any()
    _check_against_restatement(sset, got, g, W)
    assert not np.isnan(_np(got.arrays['x_cc'])).any()        # no row of a gap was read


# ------------------------------------------------------------------ 3. the scan's chunks
@pytest.mark.parametrize('W,B', [(1, 255), (1, 256), (1, 257), (1, 513), (4, 64)])
def test_scan_chunk_boundary(cuda_device, W, B):
    """n_windows * W at and around one pass of the scan's workgroup (256) and past two."""
    sset = make_set(cuda_device)
    n = sset.n_windows(W)
    g = [(i * 37 + 5) % n for i in range(B)]                  # every member, out of order
    assert len(set(sset.locate(g, W)[0].tolist())) >= 3
    _check_against_restatement(sset, sset.windows(g, W), g, W)


# ------------------------------------------------------------------ 4. guarded buffers
class _Guarded:
    """``count`` items of ``dtype`` between two bands of GUARD sentinel bytes, the body
    pre-filled with the sentinel too."""

    def __init__(self, dev, count, dtype):
        self.dtype, self.count = np.dtype(dtype), int(count)
        self.nbytes = self.count * self.dtype.itemsize
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.ptr = self.raw.data_ptr() + GUARD

    def body(self):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype)

    def check_guards(self, what):
        raw = self.raw.cpu().numpy()
        for band, name in ((raw[:GUARD], 'front'), (raw[GUARD + self.nbytes:], 'back')):
            hit = np.nonzero(band != SENT)[0]
            assert hit.size == 0, f'{what}: {name} guard overwritten at bytes {hit[:8].tolist()}'


_OUT_DTYPES = dict(scan_ptr=np.int32, scan_ref=np.int32, win_ptr=np.int32, mount=np.float64,
                   odometry=np.float64, meas_scan=np.int32, src_row=np.int32, x_cc=np.float32,
                   y_cc=np.float32, azimuth_sc=np.float32, vr=np.float32,
                   vr_compensated=np.float32, rcs=np.float32, timestamp=np.int64,
                   sensor_id=np.int64, label_id=np.int64, track_key=np.int32)


def _guarded_call(sset, pairs, W, capacity, rows, bad=None):
    """rg_sequence_set_windows straight through ctypes, every output of exactly its stated size
    (the per-measurement ones ``rows`` long) between guard bands.  Returns (rc, buffers)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    dev = sset.device
    B = len(pairs)
    n_ws = B * W
    counts = dict(scan_ptr=n_ws + 1, scan_ref=n_ws, win_ptr=B + 1, mount=3 * n_ws,
                  odometry=5 * n_ws)
    bufs = {k: _Guarded(dev, counts.get(k, rows), dt) for k, dt in _OUT_DTYPES.items()}
    out = nat.rg_window_batch(**{k: v.ptr for k, v in bufs.items()})
    win = torch.tensor(list(pairs) or [(0, 0)], dtype=torch.int32, device=dev).reshape(-1, 2)
    args = dict(seqs=sset._table.data_ptr(), n_seq=len(sset.stores), key_stride=sset.n_tracks,
                win=win.data_ptr(), n_windows=B, W=W, capacity=capacity)
    args.update(bad or {})      # an argument the buffers were not sized for: must be refused
    torch.cuda.synchronize()
    rc = nat.lib().rg_sequence_set_windows(
        args['seqs'], args['n_seq'], args['key_stride'], args['win'], args['n_windows'],
        args['W'], args['capacity'], ctypes.byref(out), nat.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, bufs


def _check_guarded(bufs, ref, capacity, what):
    sentinel = {k: np.frombuffer(bytes([SENT]) * np.dtype(dt).itemsize, dtype=dt)[0]
                for k, dt in _OUT_DTYPES.items()}
    for k, g in bufs.items():
        g.check_guards(f'{what}: {k}')
        body = g.body()
        if k in PER_SCAN:
            np.testing.assert_array_equal(_bits(body), _bits(ref[k].reshape(-1)),
                                          err_msg=f'{what}: {k}')
            continue
        np.testing.assert_array_equal(_bits(body[:capacity]), _bits(ref[k][:capacity]),
                                      err_msg=f'{what}: {k}')
        tail = body[capacity:]                 # rows at or beyond the capacity: never written
        assert (_bits(tail) == _bits(np.full(1, sentinel[k]))[0]).all(), f'{what}: {k} tail'


def test_entry_point_in_guarded_buffers(cuda_device):
    sset = make_set(cuda_device)
    W = 4
    st = sset._starts(W)
    pairs = [(0, 2), (3, 5), (2, 20), (0, 2), (2, 0)]
    ref = set_cut(sset.stores, sset.n_tracks, pairs, W)
    total = int(ref['scan_ptr'][-1])
    assert total > 200 and st[-1] > 0
    for cap in (total, total - 1, 0):
        rc, bufs = _guarded_call(sset, pairs, W, cap, total)
        assert rc == 0, cap
        _check_guarded(bufs, ref, cap, f'capacity={cap}')
    # exactly `capacity` rows of room: the guard behind row capacity - 1 is the next byte
    rc, bufs = _guarded_call(sset, pairs, W, total - 1, total - 1)
    assert rc == 0
    _check_guarded(bufs, ref, total - 1, 'room for capacity rows')
    # no window: scan_ptr[0] and win_ptr[0] alone are written
    rc, bufs = _guarded_call(sset, [], W, 0, 0)
    assert rc == 0
    _check_guarded(bufs, set_cut(sset.stores, sset.n_tracks, [], W), 0, 'n_windows=0')
    assert bufs['scan_ptr'].body().tolist() == [0] and bufs['win_ptr'].body().tolist() == [0]


def test_sequence_id_outside_the_table_gives_an_empty_window(cuda_device):
    """Defined behaviour: a window whose sequence id is -1 or n_seq is empty, its poses NaN,
    nothing is read for it (the id is clamped before the descriptor is), and the other windows
    of the batch are what they are without it."""
    sset = make_set(cuda_device)
    W, n_seq = 4, len(sset.stores)
    pairs = [(0, 2), (-1, 3), (3, 5), (n_seq, 0), (2, 20)]
    ref = set_cut(sset.stores, sset.n_tracks, pairs, W)
    total = int(ref['scan_ptr'][-1])
    rc, bufs = _guarded_call(sset, pairs, W, total, total)
    assert rc == 0
    _check_guarded(bufs, ref, total, 'ids outside the table')
    wp = bufs['win_ptr'].body()
    mount, odo = bufs['mount'].body().reshape(-1, 3), bufs['odometry'].body().reshape(-1, 5)
    for b in (1, 3):
        assert wp[b + 1] == wp[b]
        assert np.isnan(mount[b * W:(b + 1) * W]).all() and np.isnan(odo[b * W:(b + 1) * W]).all()
    assert not np.isnan(np.delete(mount, np.r_[W:2 * W, 3 * W:4 * W], axis=0)).any()
    # the three real windows: the same rows as in a batch of their own, keys of their slots
    alone = set_cut(sset.stores, sset.n_tracks, [pairs[0], pairs[2], pairs[4]], W)
    np.testing.assert_array_equal(bufs['src_row'].body(), alone['src_row'])
    np.testing.assert_array_equal(_bits(bufs['rcs'].body()), _bits(alone['rcs']))


def test_host_validation_on_the_device(cuda_device):
    """With a real device table: every bad argument the host can see is refused with
    RG_ERR_ARG and nothing is launched (the outputs keep their sentinel)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    sset = make_set(cuda_device)
    pairs, W, rows = [(0, 2), (2, 0)], 4, 600
    lib = nat.lib()
    bad_args = [dict(seqs=None), dict(win=None), dict(n_seq=0), dict(n_seq=-1),
                dict(key_stride=-1), dict(W=0), dict(W=-1), dict(n_windows=-1),
                dict(capacity=-1), dict(n_windows=2 ** 30, W=2),
                dict(n_windows=2 ** 20, key_stride=2 ** 11)]
    for bad in bad_args:
        rc, bufs = _guarded_call(sset, pairs, W, rows, rows, bad)
        assert rc == 1 and b'rg_sequence_set_windows' in lib.rg_last_error(), bad
        for k, g in bufs.items():
            assert (g.raw.cpu().numpy() == SENT).all(), (bad, k)
    rc, _ = _guarded_call(sset, pairs, W, rows, rows)
    assert rc == 0


# ------------------------------------------------------------------ 5. reference frames
def _frame_parts(fb, gb, lab):
    """Per frame of a labelled batch: nodes, link pairs (local indices, edge labels) and the
    ground-truth clusters (member lists in order, classes)."""
    fp = _np(fb.frame_ptr).astype(np.int64)
    U = int(gb.graph.n_pairs_dev.item())
    src, dst = _np(gb.graph.pair_src[:U]).astype(np.int64), _np(gb.graph.pair_dst[:U])
    u = np.searchsorted(src, fp)
    ncl = int(lab['n_clusters_dev'].item())
    cptr, cidx = _np(lab['cluster_ptr'][:ncl + 1]).astype(np.int64), _np(lab['cluster_idx'])
    frame_of = np.searchsorted(fp, cidx[cptr[:ncl]], side='right') - 1
    assert (np.diff(frame_of) >= 0).all()
    c = np.searchsorted(frame_of, np.arange(fb.n_frames + 1))
    parts = []
    for f in range(fb.n_frames):
        a, b = int(fp[f]), int(fp[f + 1])
        parts.append(dict(
            node_class=_np(lab['node_class'][a:b]),
            node_offsets=_bits(_np(lab['node_offsets'][a:b])),
            pair_src=src[u[f]:u[f + 1]] - a, pair_dst=dst[u[f]:u[f + 1]] - a,
            edge_class=_np(lab['edge_class'][int(u[f]):int(u[f + 1])]),
            cluster_sizes=np.diff(cptr[c[f]:c[f + 1] + 1]),
            cluster_members=cidx[cptr[c[f]]:cptr[c[f + 1]]] - a,
            cluster_labels=_np(lab['cluster_labels'][int(c[f]):int(c[f + 1])])))
    return parts


@pytest.mark.parametrize('W', [10, 4])
def test_reference_frames_inside_a_mixed_batch(cuda_device, W):
    """The fixture's cases cut between windows of the other members: their batch slots give
    the dynamic frame and the training labels that the same windows give when cut from the
    fixture store alone, bit for bit."""
    _, frontend, training = _mods()
    from graph_neural_network_for_radar_perception_amd.graph_features import build_graph_batch
    cfg = _cfg()
    sset = make_set(cuda_device)
    fstore = sset.stores[3]
    cases = [int(p) for w, p in golden(sref.FIXTURE)['cases'].tolist() if int(w) == W]
    assert cases
    st = sset._starts(W)
    others = [int(st[0]) + 3, int(st[2]) + 7, int(st[0]) + 11, int(st[2]) + 2]
    g, slots = [others[0]], []
    for i, p in enumerate(cases):
        slots.append(len(g))
        g += [int(st[3]) + p, others[(i + 1) % len(others)]]
    T = sset.n_tracks
    dd, gd = frontend.dynamic_frame(sset.windows(g, W), with_keys=True, numpy_mean=True)
    fb = frontend.frame_batch(dd, gd)
    gb = build_graph_batch(fb, cfg)
    parts = _frame_parts(fb, gb, training.training_labels(fb, gb, cfg, ws_cache={}))
    fp = _np(dd['frame_ptr']).astype(np.int64)
    for slot, p in zip(slots, cases):
        d1, g1 = frontend.dynamic_frame(fstore.windows([p], W), with_keys=True, numpy_mean=True)
        a, b = int(fp[slot]), int(fp[slot + 1])
        assert b - a == len(d1['meas_px']) > 1, (slot, p)
        for k, v in d1.items():
            if k in ('frame_ptr', 'track_key'):
                continue
            np.testing.assert_array_equal(_bits(_np(dd[k][a:b])), _bits(_np(v)), err_msg=k)
        for k, v in g1.items():
            np.testing.assert_array_equal(_bits(_np(gd[k][a:b])), _bits(_np(v)), err_msg=k)
        k1 = _np(d1['track_key']).astype(np.int64)
        np.testing.assert_array_equal(_np(dd['track_key'][a:b]),
                                      np.where(k1 > 0, k1 + slot * T, 0))
        fb1 = frontend.frame_batch(d1, g1)
        gb1 = build_graph_batch(fb1, cfg)
        one = _frame_parts(fb1, gb1, training.training_labels(fb1, gb1, cfg, ws_cache={}))[0]
        mine = parts[fb.windows.index(slot)]
        assert len(one['edge_class']) > 0 and len(one['cluster_labels']) > 0
        for k, v in one.items():
            np.testing.assert_array_equal(mine[k], v, err_msg=f'{k} slot {slot} pos {p}')


# ------------------------------------------------------------------ 6. the existing loops
TRAIN_W = 4


def _train_indices(sset):
    st = sset._starts(TRAIN_W)
    return [int(st[0]) + 14, int(st[3]) + 3, int(st[2]) + 9, int(st[0]), int(st[3]) - 1,
            int(st[3]), int(st[2]) + 9, int(st[3]) + 30, int(st[0]) + 20, int(st[2]) + 1,
            int(st[3]) + 17, int(st[0]) + 5, int(st[2]) + 16, int(st[3]) + 8, int(st[0]) + 2,
            int(st[4]) - 1]


def test_train_sequence_over_the_set_equals_host_fed_steps(cuda_device):
    """Three steps of train_sequence over the set == three step_frames fed per batch from
    host_window -> scan_window_batch with the same flags: loss and accuracy rows and the
    weights after step 3, bit for bit."""
    _, frontend, training = _mods()
    dev = cuda_device
    cfg = _cfg()
    ransac = bool(getattr(cfg, 'reject_static_meas_by_ransac', False))
    sset = make_set(dev)
    g = _train_indices(sset)
    assert len(g) == 16 and len(set(sset.locate(g, TRAIN_W)[0].tolist())) == 3
    tr = _trainer(dev, cfg)
    seen = []
    np.random.seed(77)
    losses, acc = training.train_sequence(
        sset, tr, cfg, g, window_size=TRAIN_W, batch_windows=6, augmentation=True,
        on_step=lambda k, pos, flags, out: seen.append((list(pos), flags)))
    assert [s[0] for s in seen] == [g[:6], g[6:12], g[12:]]
    tr2 = _trainer(dev, cfg)
    np.random.seed(77)
    rows = []
    for i0 in range(0, len(g), 6):
        pos = g[i0:i0 + 6]
        flags = frontend.draw_flips(len(pos))
        np.testing.assert_array_equal(flags, seen[i0 // 6][1])
        win = frontend.scan_window_batch([sset.host_window(x, TRAIN_W) for x in pos], dev)
        dd, gd = frontend.dynamic_frame(win, ransac, with_keys=True, flip=flags, numpy_mean=True)
        rows.append(tr2.step_frames(frontend.frame_batch(dd, gd))[:2])
    assert np.concatenate([s[1] for s in seen]).any()
    assert losses.shape == (3, 4) and acc.shape == (3, 3)
    assert torch.isfinite(losses).all() and float(losses.sum()) > 0
    _same(losses, torch.stack([r[0] for r in rows]), 'losses')
    _same(acc, torch.stack([r[1] for r in rows]), 'accuracies')
    assert tr.opt.applied_steps() == tr2.opt.applied_steps() == 3
    _same(tr.opt.flat, tr2.opt.flat, 'weights after step 3')


def test_evaluate_sequence_over_the_set_sums_the_stores(cuda_device):
    from graph_neural_network_for_radar_perception_amd import evaluation
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    name = 'model_trained_N50'
    cfg = model_cfg(name)
    mt = Model_Training(cfg, dev)
    mt.load_state_dict(model_state_dict(name))
    model = mt.to(dev).pred.eval().requires_grad_(False)
    model.set_param_for_proposal_extraction(float(golden('proposals_model_trained_N300')['eps']),
                                            False)
    sequence = _mods()[0]
    sset = sequence.SequenceSet(make_set(dev).stores[:3])
    W, B = 4, 8
    assert sset.n_windows(W) == 42                  # 21 + 0 + 21: a batch straddles the members
    det, seg = evaluation.evaluate_sequence(sset, model, cfg, window_size=W, batch_windows=B)
    det_s = evaluation.DetectionEvaluator(int(cfg.num_classes))
    seg_s = evaluation.SegmentationEvaluator(int(cfg.num_classes))
    for store in sset.stores:
        d1, s1 = evaluation.evaluate_sequence(store, model, cfg, window_size=W, batch_windows=B)
        det_s.merge(d1)
        seg_s.merge(s1)
    got_d, got_s, want_d, want_s = det.result(), seg.result(), det_s.result(), seg_s.result()
    for k in ('confusion_matrix', 'gt_count_matrix', 'pred_count_matrix'):
        np.testing.assert_array_equal(got_d[k], want_d[k], err_msg=k)
    for k in ('confusion_matrix', 'gt_count_matrix'):
        np.testing.assert_array_equal(got_s[k], want_s[k], err_msg=k)
    assert int(got_s['gt_count_matrix'].sum()) > 0 and int(got_d['gt_count_matrix'].sum()) > 0


# ------------------------------------------------------------------ 7. validation
def test_validate_frames_equals_step_frames_and_changes_nothing(cuda_device):
    _, frontend, _ = _mods()
    dev = cuda_device
    cfg = _cfg()
    sset = make_set(dev)
    g = _train_indices(sset)[:6]
    dd, gd = frontend.dynamic_frame(sset.windows(g, TRAIN_W), with_keys=True, numpy_mean=True)
    fb = frontend.frame_batch(dd, gd)
    tr = _trainer(dev, cfg)
    flat, buf = tr.opt.flat.clone(), tr.opt.buf.clone()
    grad = tr.engine.flat_bucket.clone()
    val = tr.validate_frames(fb)
    assert len(val) == 2 and val[0].shape == (4,) and val[1].shape == (3,)
    _same(tr.opt.flat, flat, 'weights')
    _same(tr.opt.buf, buf, 'momentum')
    _same(tr.engine.flat_bucket, grad, 'gradient bucket')
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 0
    assert all(not p.requires_grad or p.grad is None for p in tr.model.parameters())
    step = tr.step_frames(fb)
    assert torch.isfinite(val[0]).all() and float(val[0].sum()) > 0
    _same(val[0], step[0], 'losses')
    _same(val[1], step[1], 'accuracies')
    assert tr.opt.applied_steps() == 1 and not torch.equal(tr.opt.flat, flat)
    # after the update the validation follows the new weights
    again = tr.validate_frames(fb)
    assert not torch.equal(again[0], val[0])
    # a batch without a frame
    empty = frontend.frame_batch(*frontend.dynamic_frame(
        _static_windows(dev), with_keys=True, numpy_mean=True))
    assert empty.n_frames == 0 and tr.validate_frames(empty) is None


def _static_windows(dev):
    """Two windows of static scenes: no dynamic node, so no frame to train or validate on."""
    sequence = _mods()[0]
    radar, odo, lists, sensors = sref.make_sequence(11, (30, 20, 25), ('static',) * 3)
    return sequence.SequenceStore.from_numpy(radar, odo, lists, sensors, dev).windows([0, 1], 2)


def test_validate_sequence_means_and_nan_batch(cuda_device):
    _, _, training = _mods()
    dev = cuda_device
    cfg = _cfg()
    sset = _private_set(dev)                          # written to below: not the shared set
    st = sset._starts(TRAIN_W)
    g = [0, 1, 2, 9, 10, 11, int(st[1]), int(st[1]) + 1, int(st[1]) + 2]
    tr = _trainer(dev, cfg)
    flat, buf = tr.opt.flat.clone(), tr.opt.buf.clone()

    def run():
        res = training.validate_sequence(sset, tr, cfg, g, window_size=TRAIN_W, batch_windows=3)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in res)
        mean_lo, mean_ac, n, lo, ac = res
        assert lo.shape == (3, 4) and ac.shape == (3, 3) and lo.dtype == torch.float32
        assert mean_lo.shape == (4,) and mean_ac.shape == (3,) and n.dtype == torch.int64
        total = _np(training.total_loss(lo))
        np.testing.assert_array_equal(total, ((_np(lo)[:, 0] + _np(lo)[:, 1]) + _np(lo)[:, 2])
                                      + _np(lo)[:, 3])
        for c in range(4):
            want, wn = training.average_counted(total, _np(lo)[:, c])
            assert wn == int(n)
            np.testing.assert_allclose(float(mean_lo[c]), want, rtol=4e-15, atol=0)
        for c in range(3):
            want, _ = training.average_counted(total, _np(ac)[:, c])
            np.testing.assert_allclose(float(mean_ac[c]), want, rtol=4e-15, atol=0)
        return int(n), lo, ac, total

    n0, lo0, ac0, total0 = run()
    assert n0 == 3 and (total0 > 0).all()
    # rows that the second batch alone cuts: scenes 10 and 12 of member 0 (positions 9..11
    # cover scenes 9..14, the first batch scenes 0..5, the third batch another member)
    store = sset.stores[0]
    for s in (10, 12):
        a, b = int(store.scenes[s, 0]), int(store.scenes[s, 1])
        assert b - a >= 64
        store.dev['rcs'][a:b] = float('nan')
    n1, lo1, ac1, total1 = run()
    assert n1 == 2 and np.isnan(total1[1]) and not np.isnan(total1[[0, 2]]).any()
    _same(lo1[[0, 2]], lo0[[0, 2]], 'the other batches\' losses')
    _same(ac1[[0, 2]], ac0[[0, 2]], 'the other batches\' accuracies')
    _same(tr.opt.flat, flat, 'weights')
    _same(tr.opt.buf, buf, 'momentum')
    assert tr.opt.applied_steps() == 0 and tr.opt.steps == 0


# ------------------------------------------------------------------ 8. save
def test_save_after_two_steps_loads_into_a_fresh_model(cuda_device, tmp_path):
    _, frontend, _ = _mods()
    from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
    dev = cuda_device
    cfg = _cfg()
    sset = make_set(dev)
    g = _train_indices(sset)
    tr = _trainer(dev, cfg)
    before = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    for pos in (g[:4], g[4:8]):
        dd, gd = frontend.dynamic_frame(sset.windows(pos, TRAIN_W), with_keys=True,
                                        numpy_mean=True)
        assert tr.step_frames(frontend.frame_batch(dd, gd)) is not None
    assert tr.opt.applied_steps() == 2
    path = tmp_path / 'weights.pth'
    tr.save(str(path))
    loaded = torch.load(str(path), map_location='cpu')
    torch.manual_seed(1)
    fresh = Model_Training(cfg, 'cpu')
    assert set(loaded) == set(fresh.state_dict())
    result = fresh.load_state_dict(loaded, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    now = tr.model.state_dict()
    changed = 0
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, now[k].detach().cpu()), k
        changed += int(not torch.equal(v, before[k]))
    assert changed > 0


# ------------------------------------------------------------------ 9. train_dataset
def test_train_dataset_iterations_validations_and_save(cuda_device, tmp_path):
    sequence, _, training = _mods()
    dev = cuda_device
    cfg = _cfg()
    shared = make_set(dev)
    train = sequence.SequenceSet([shared.stores[0], shared.stores[2]])
    val = sequence.SequenceSet([shared.stores[3]])
    n = train.n_windows(TRAIN_W)
    assert n == 42
    tr = _trainer(dev, cfg)
    steps, vals = [], []
    path = tmp_path / 'detector.pth'
    torch.manual_seed(5)
    np.random.seed(5)
    losses, acc, validations = training.train_dataset(
        train, tr, cfg, val_set=val, val_indices=[0, 7, 30, 36, 36], max_iters=5,
        val_period=2, batch_windows=4, window_size=TRAIN_W, weights_path=str(path),
        on_step=lambda it, pos, flags, out: steps.append((it, pos.copy(), flags, out)),
        on_validation=lambda it, res: vals.append((it, res, path.exists())))
    torch.manual_seed(5)
    gen = training.shuffled_batches(n, 4)
    want = [next(gen) for _ in range(5)]
    assert [s[0] for s in steps] == [0, 1, 2, 3, 4]
    for s, w in zip(steps, want):
        np.testing.assert_array_equal(s[1], w)
        assert s[2] is not None and len(s[2]) == 4          # cfg.dataset_augmentation
    assert losses.shape == (5, 4) and acc.shape == (5, 3) and losses.is_cuda
    for i, s in enumerate(steps):
        _same(losses[i], s[3][0], f'row {i}')
    assert tr.opt.applied_steps() == 5
    assert [v[0] for v in validations] == [0, 2, 4] == [v[0] for v in vals]
    assert all(v[2] for v in vals)                           # saved before each validation
    for (it, mean_lo, mean_ac, cnt), (_, res, _) in zip(validations, vals):
        assert mean_lo is res[0] and mean_ac is res[1] and cnt is res[2]
        assert int(cnt) == 2 and res[3].shape == (2, 4)      # 5 windows (the fixture's cases
                                                             # at W = 4 ... 36) in batches of 4
        assert torch.isfinite(mean_lo).all() and mean_lo.is_cuda
    assert not torch.equal(vals[0][1][3], vals[2][1][3])     # the weights moved in between
    # the last save holds the final weights
    loaded = torch.load(str(path), map_location='cpu')
    for k, v in tr.model.state_dict().items():
        assert torch.equal(loaded[k], v.detach().cpu()), k
    # an offset: iterations 3 and 4 only, the validation on the last one
    its = []
    out = training.train_dataset(train, tr, cfg, val_set=val, val_indices=[0], max_iters=5,
                                 iter_start_offset=3, val_period=1000, batch_windows=4,
                                 window_size=TRAIN_W, on_step=lambda it, *a: its.append(it))
    assert its == [3, 4] and out[0].shape == (2, 4) and [v[0] for v in out[2]] == [4]
    assert tr.opt.applied_steps() == 7
