"""The sequence store's host side (sequence.py) without a GPU: the scene chain and the sliding
windows against the reference's own lists (tests/golden/sequence_148_s40.npz, made by
tests/golden/make_sequence_golden.py), the window arithmetic, the host windows against the
fixture's rows, the key scheme, and every error raised before a launch."""
import ctypes

import numpy as np
import pytest

import sequence_ref as sref
from conftest import golden
from sequence_ref import FIXTURE, fixture_inputs, fixture_scenes_json, fixture_store


def _seq():
    from graph_neural_network_for_radar_perception_amd import sequence
    return sequence


def test_aggregate_scenes_matches_reference():
    d = golden(FIXTURE)
    lists = _seq().aggregate_scenes(fixture_scenes_json(d))
    assert set(lists) == set(sref.LIST_KEYS)
    for k in sref.LIST_KEYS:
        want = d['lists/' + k].tolist()
        assert lists[k] == want, k
    assert len(lists['radar_id']) == int(d['n_scenes']) == 40
    assert lists['odometry_index'][0] == 361


@pytest.mark.parametrize('W', [4, 10])
def test_sliding_windows_match_reference(W):
    d = golden(FIXTURE)
    lists = _seq().aggregate_scenes(fixture_scenes_json(d))
    wins = _seq().sliding_windows(W, lists)
    assert len(wins) == int(d[f'sliding{W}/n']) == 40 - W + 1
    for k in sref.LIST_KEYS:
        want = d[f'sliding{W}/{k}'].tolist()
        assert [w[k] for w in wins] == want, k
    assert all(set(w) == set(sref.LIST_KEYS) for w in wins)


def test_sliding_windows_short_sequence():
    lists = {k: [1, 2, 3] if k != 'radar_data_indices' else [[0, 1], [1, 2], [2, 3]]
             for k in sref.LIST_KEYS}
    assert _seq().sliding_windows(4, lists) == []
    assert len(_seq().sliding_windows(3, lists)) == 1
    assert len(_seq().sliding_windows(1, lists)) == 3


def test_n_windows():
    _, store = fixture_store('cpu')
    S = store.n_scenes
    assert S == 40
    for W in (1, 4, 10, 40):
        assert store.n_windows(W) == S - W + 1
    assert store.n_windows(1) == S
    assert store.n_windows(41) == 0 and store.n_windows(1000) == 0
    with pytest.raises(ValueError):
        store.n_windows(0)


@pytest.mark.parametrize('W,i', [(10, 0), (10, 7), (10, 30), (4, 36), (1, 39), (40, 0)])
def test_host_window_concatenates_the_fixture_rows(W, i):
    d, store = fixture_store('cpu')
    win = store.host_window(i, W)
    rind = d['lists/radar_data_indices'][i:i + W]
    rows = np.concatenate([np.arange(a, b) for a, b in rind])
    for k in sref.F32_FIELDS:
        assert win[k].dtype == np.float32
        np.testing.assert_array_equal(win[k], d['radar/' + k][rows], err_msg=k)
    for k in ('timestamp', 'sensor_id', 'label_id'):
        assert win[k].dtype == np.int64
        np.testing.assert_array_equal(win[k], d['radar/' + k][rows].astype(np.int64), err_msg=k)
    np.testing.assert_array_equal(win['track_id_bytes'], d['radar/track_id'][rows])
    assert win['n_scans'] == W
    np.testing.assert_array_equal(win['scan_ptr'],
                                  np.concatenate(([0], np.cumsum(rind[:, 1] - rind[:, 0]))))
    mount_of = {int(s): m for s, m in zip(d['sensors/id'], d['sensors/mount'])}
    want_mount = np.array([mount_of[int(r)] for r in d['lists/radar_id'][i:i + W]])
    np.testing.assert_array_equal(win['mount'], want_mount)
    oi = d['lists/odometry_index'][i:i + W]
    want_odo = np.stack([d['odometry/' + k][oi] for k in ('x_seq', 'y_seq', 'yaw_seq', 'vx',
                                                           'yaw_rate')], axis=-1)
    assert win['mount'].dtype == np.float64 and win['odometry'].dtype == np.float64
    np.testing.assert_array_equal(win['odometry'], want_odo)


def test_host_window_equals_numpy_cut():
    """host_window against the cut's numpy restatement on the adversarial sequence (empty
    scenes, scrambled ranges with gaps)."""
    radar, odo, lists, sensors = sref.adversarial_sequence()
    store = _seq().SequenceStore.from_numpy(radar, odo, lists, sensors, 'cpu')
    assert store.n_scenes == 24
    fields = {k: radar[k] for k in radar.dtype.names}
    for W in (1, 4, 10, 24):
        for i in (0, store.n_windows(W) - 1):
            win = store.host_window(i, W)
            ref = sref.cut(store.scenes, store.mount_table, store.odometry_table, fields,
                           store.track_key, store.n_tracks, [i], W)
            for k in sref.F32_FIELDS + ('timestamp', 'sensor_id', 'label_id'):
                np.testing.assert_array_equal(win[k], ref[k], err_msg=k)
            np.testing.assert_array_equal(win['scan_ptr'], ref['scan_ptr'])
            np.testing.assert_array_equal(win['mount'], ref['mount'])
            np.testing.assert_array_equal(win['odometry'], ref['odometry'])
            np.testing.assert_array_equal(win['track_key'], ref['track_key'])
            assert not np.isnan(win['x_cc']).any() and (win['label_id'] != 255).all()


def test_track_keys_rank_as_each_windows_own_unique():
    from graph_neural_network_for_radar_perception_amd import frontend
    d = golden(FIXTURE)
    radar, odo, sensors = fixture_inputs(d)
    real = (radar, odo, _seq().aggregate_scenes(fixture_scenes_json(d)), sensors)
    for radar, odo, lists, sensors in (real, sref.adversarial_sequence()):
        store = _seq().SequenceStore.from_numpy(radar, odo, lists, sensors, 'cpu')
        ids = np.asarray(radar['track_id'])
        np.testing.assert_array_equal(store.track_key == 0, ids == b'')
        assert store.n_tracks == len(set(ids.tolist()) - {b''})
        assert store.track_key.max() == store.n_tracks
        for W in (1, 4, 10):
            for i in range(0, store.n_windows(W), 3):
                win = store.host_window(i, W)
                own = frontend._host_track_keys(win)          # the window's own np.unique
                seq_keys = win['track_key']
                np.testing.assert_array_equal(seq_keys == 0, own == 0)
                # the same ranking: the dense ranks of the sequence keys are the own keys
                dense = np.unique(seq_keys, return_inverse=True)[1].reshape(-1)
                if not (seq_keys == 0).any():
                    dense = dense + 1
                np.testing.assert_array_equal(dense, own)


def test_index_and_value_errors():
    _, store = fixture_store('cpu')
    for bad in ([-1], [31], [0, 5, 31], [10 ** 12]):
        with pytest.raises(IndexError):
            store.windows(bad, 10)
    with pytest.raises(IndexError):
        store.windows([0], 41)          # no sliding position at all
    with pytest.raises(IndexError):
        store.host_window(37, 4)
    with pytest.raises(ValueError):
        store.windows([0], 0)
    with pytest.raises(ValueError):
        store.windows([], 10)
    # B * T must stay below 2^31
    store.n_tracks = 2 ** 30
    with pytest.raises(ValueError, match='int32'):
        store.windows([0, 1], 10)


def test_from_numpy_rejects_inconsistent_inputs():
    d = golden(FIXTURE)
    radar, odo, sensors = fixture_inputs(d)
    lists = _seq().aggregate_scenes(fixture_scenes_json(d))
    make = _seq().SequenceStore.from_numpy
    short = dict(radar, vr=radar['vr'][:-1])
    with pytest.raises(ValueError):
        make(short, odo, lists, sensors, 'cpu')
    with pytest.raises(KeyError):
        make({k: v for k, v in radar.items() if k != 'rcs'}, odo, lists, sensors, 'cpu')
    with pytest.raises(ValueError, match='odometry_index'):
        make(radar, odo[:100], lists, sensors, 'cpu')
    with pytest.raises(KeyError, match='radar_'):
        make(radar, odo, lists, {k: v for k, v in sensors.items() if k != 'radar_3'}, 'cpu')
    far = dict(lists, radar_data_indices=lists['radar_data_indices'][:-1] + [[0, 10 ** 7]])
    with pytest.raises(ValueError, match='radar_data_indices'):
        make(radar, odo, far, sensors, 'cpu')


def test_native_argument_validation_launches_nothing():
    """rg_sequence_windows refuses null tables, W < 1 and negative sizes with RG_ERR_ARG before
    anything is launched (no device is needed to get here)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd import build
    build.build_library()
    lib = nat.lib()
    f = 4096  # any non-null address: nothing is dereferenced before the checks fail

    def seq(**kw):
        s = nat.rg_sequence(**{k: f for k, t in nat.rg_sequence._fields_ if t is ctypes.c_void_p})
        s.n_scenes, s.n_sensors, s.n_odometry, s.n_meas, s.n_tracks = 24, 4, 27, 1000, 8
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def out(**kw):
        o = nat.rg_window_batch(**{k: f for k, _ in nat.rg_window_batch._fields_})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(s, o, first=f, B=2, W=4, cap=100):
        return lib.rg_sequence_windows(ctypes.byref(s) if s is not None else None, first, B, W,
                                       cap, ctypes.byref(o) if o is not None else None, None)

    cases = [
        (call(None, out()), b'null'), (call(seq(), None), b'null'),
        (call(seq(), out(), first=None), b'null'),
        (call(seq(scenes=None), out()), b'table'), (call(seq(mount=None), out()), b'table'),
        (call(seq(odometry=None), out()), b'table'),
        (call(seq(vr=None), out()), b'measurement'),
        (call(seq(track_key=None), out()), b'measurement'),
        (call(seq(), out(scan_ptr=None)), b'per-scan'),
        (call(seq(), out(odometry=None)), b'per-scan'),
        (call(seq(), out(timestamp=None)), b'per-measurement'),
        (call(seq(), out(), W=0), b'W=0'), (call(seq(), out(), W=-3), b'W=-3'),
        (call(seq(), out(), B=-1), b'n_windows=-1'), (call(seq(), out(), cap=-5), b'capacity=-5'),
        (call(seq(n_meas=-1), out()), b'negative'), (call(seq(n_scenes=-2), out()), b'negative'),
        (call(seq(n_tracks=-1), out()), b'negative'),
        (call(seq(n_tracks=2 ** 30), out(), B=4), b'int32'),
        (call(seq(), out(), B=2 ** 30, W=4), b'windows of'),
        (call(seq(scenes=f + 4), out()), b'aligned'),
    ]
    for i, (rc, _) in enumerate(cases):
        assert rc == 1, i
    # the message of the last failing call is kept
    assert call(seq(), out(), W=0) == 1 and b'W=0' in lib.rg_last_error()
    assert call(seq(scenes=None), out()) == 1 and b'table' in lib.rg_last_error()
    with pytest.raises(RuntimeError, match='rg_sequence_windows'):
        nat.check(call(seq(), out(), W=0), 'rg_sequence_windows')


@pytest.mark.timeout(1200)
def test_sequence_host_code_under_asan_ubsan():
    """rg_sequence_windows' host code -- the argument checks, the int32 products at and past
    their limits -- under AddressSanitizer + UndefinedBehaviorSanitizer (host side only), driven
    by the stand-alone tests/sequence_sanitize_main.cpp; any sanitizer report or failed check
    fails the run.  CPU only: no path it takes reaches a kernel launch."""
    import os
    import subprocess
    from graph_neural_network_for_radar_perception_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = build.build_sanitized_driver(os.path.join(here, 'sequence_sanitize_main.cpp'))
    env = dict(os.environ, ASAN_OPTIONS='abort_on_error=1:detect_leaks=0',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', HIP_VISIBLE_DEVICES='')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert 'AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
