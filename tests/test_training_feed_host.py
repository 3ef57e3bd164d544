"""The training feed without a GPU: the numpy restatement (tests/training_feed_ref.py) against
the reference's own RadarScenesDataset.__getitem__ (tests/golden/training_feed_148_s40.npz,
made by tests/golden/make_training_feed_golden.py), the exported entry points, the flip draws
and every error the native entry points raise before a launch."""
import numpy as np
import pytest

import training_feed_ref as tref
from conftest import golden
from sequence_ref import fixture_store

CASES = [(W, pos, f) for W, pos in tref.CASES for f in (0, 1)]


def test_fixture_holds_the_cases():
    d = golden(tref.FIXTURE)
    assert d['cases'].tolist() == [list(c) for c in tref.CASES]
    for W, pos, f in CASES:
        pre = tref.case_key(W, pos, f)
        seed, draw = int(d[pre + 'seed']), float(d[pre + 'draw'])
        if f:      # the seed that forced the flip reproduces the stored draw
            np.random.seed(seed)
            assert np.random.rand() == draw and draw >= 0.5
        else:      # dataset_augmentation False: nothing was drawn
            assert seed == -1 and np.isnan(draw)


@pytest.mark.parametrize('W,pos,flipped', CASES)
def test_restatement_equals_reference(W, pos, flipped):
    """(a) flip + selection, node labels, edge labels and clusters restated in numpy equal the
    reference's item bit for bit; the case exercises every label kind."""
    d = golden(tref.FIXTURE)
    seq, store = fixture_store('cpu')
    pre = tref.case_key(W, pos, flipped)
    got = tref.dynamic_frame(seq, store, W, pos, flipped)
    for k in ('px', 'py', 'vx', 'vy'):
        assert got[k].dtype == np.float32
        np.testing.assert_array_equal(got[k].view(np.int32), d[pre + k].view(np.int32), err_msg=k)
    np.testing.assert_array_equal(got['node_class'], d[pre + 'node_class'])
    np.testing.assert_array_equal(got['node_offsets'].view(np.int32),
                                  d[pre + 'node_offsets'].view(np.int32))
    if flipped:   # against the unflipped item: exact negations, the same selection
        off = tref.case_key(W, pos, 0)
        for k in ('py', 'vy'):
            np.testing.assert_array_equal(d[pre + k], -d[off + k])
        np.testing.assert_array_equal(d[pre + 'node_offsets'][:, 1], -d[off + 'node_offsets'][:, 1])
        for k in ('px', 'vx', 'node_class', 'edge_class', 'cluster_ptr', 'cluster_idx'):
            np.testing.assert_array_equal(d[pre + k], d[off + k])
    key = got['key']
    src, dst = tref.link_pairs(d[pre + 'edge_index'])
    np.testing.assert_array_equal(tref.edge_labels(key, src, dst), d[pre + 'edge_class'])
    ptr, idx, lab = tref.gt_clusters(key, got['node_class'])
    np.testing.assert_array_equal(ptr, d[pre + 'cluster_ptr'])
    np.testing.assert_array_equal(idx, d[pre + 'cluster_idx'])
    np.testing.assert_array_equal(lab, d[pre + 'cluster_labels'])
    # what the case must exercise
    assert len(key) >= 2
    ec = d[pre + 'edge_class']
    assert (ec == 1).any() and (ec == 0).any()
    sizes = np.diff(ptr)
    tracked = key[idx[ptr[:-1]]] != 0
    assert (sizes[tracked] >= 2).any() and (~tracked).any() and (sizes[~tracked] == 1).all()


def test_restated_flip_and_labels_edge_cases():
    py = np.arange(6, dtype=np.float32)
    vy = -np.arange(6, dtype=np.float32)
    fpy, fvy = tref.flip(py, vy, [0, 2, 2, 6], [1, 1, 0])
    np.testing.assert_array_equal(fpy, [-0.0, -1, 2, 3, 4, 5])
    assert np.signbit(fpy[0]) and not np.signbit(fvy[0])     # the sign bit flips, even of zero
    np.testing.assert_array_equal(fvy, [0, 1, -2, -3, -4, -5])
    key = np.array([0, 0, 5, 5, 9, 0])
    np.testing.assert_array_equal(
        tref.edge_labels(key, np.array([0, 2, 2, 0]), np.array([1, 3, 4, 2])), [0, 1, 0, 0])
    ptr, idx, lab = tref.gt_clusters(key, np.array([6, 6, 1, 1, 3, 6]), [0, 3, 6])
    np.testing.assert_array_equal(ptr, [0, 1, 2, 3, 4, 5, 6])
    np.testing.assert_array_equal(idx, [2, 0, 1, 3, 4, 5])
    np.testing.assert_array_equal(lab, [1, 6, 6, 1, 3, 6])


def test_entry_points_exported_and_bound():
    """(b) the library exports the feed's entry points and _native binds them."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd import build
    build.build_library()
    lib = nat.lib()
    for name in ('rg_frontend_flip', 'rg_train_labels', 'rg_train_offsets',
                 'rg_train_offsets_workspace_size'):
        assert name in nat.header_functions(), name
        assert name in nat._SIGNATURES, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize('n', [0, 1, 7, 64])
def test_draw_flips_is_the_reference_stream(n):
    """(c) draw_flips(n) = n successive np.random.rand() >= 0.5, generator state included."""
    from graph_neural_network_for_radar_perception_amd import frontend
    np.random.seed(1234 + n)
    want = np.array([np.random.rand() >= 0.5 for _ in range(n)], dtype=bool)
    state = np.random.get_state()
    np.random.seed(1234 + n)
    got = frontend.draw_flips(n)
    after = np.random.get_state()
    assert got.dtype == np.bool_ and got.shape == (n,)
    np.testing.assert_array_equal(got, want)
    assert after[0] == state[0] and after[2:] == state[2:]
    np.testing.assert_array_equal(after[1], state[1])
    if n == 64:
        assert got.any() and not got.all()


def test_native_argument_validation_launches_nothing():
    """Both entry points refuse bad arguments with RG_ERR_ARG and a message before anything is
    launched; empty inputs are valid (no device is needed to get here)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd import build
    build.build_library()
    lib = nat.lib()
    f = 4096  # any non-null address: nothing is dereferenced before the checks fail

    def flip(py=f, vy=f, wp=f, nw=4, fl=f, n=100):
        return lib.rg_frontend_flip(py, vy, wp, nw, fl, n, None)

    def labels(cls=f, ox=f, oy=f, N=100, key=f, ps=f, pd=f, npairs=f, cap=1000, nc=f, no=f, ec=f):
        return lib.rg_train_labels(cls, ox, oy, N, key, ps, pd, npairs, cap, nc, no, ec, None)

    need = lib.rg_train_offsets_workspace_size(50)
    assert need >= 51 * 16

    def offsets(key=f, nt=50, px=f, py=f, n=100, ox=f, oy=f, ws=f, nbytes=need):
        return lib.rg_train_offsets(key, nt, px, py, n, ox, oy, ws, nbytes, None)

    cases = [
        (lambda: offsets(nt=-1), b'n_tracks=-1'), (lambda: offsets(n=-1), b'n_meas=-1'),
        (lambda: offsets(nt=2 ** 31 - 1, nbytes=2 ** 40), b'too large'),
        (lambda: offsets(key=None), b'null'), (lambda: offsets(px=None), b'null'),
        (lambda: offsets(py=None), b'null'), (lambda: offsets(ox=None), b'null'),
        (lambda: offsets(oy=None), b'null'), (lambda: offsets(ws=None), b'workspace'),
        (lambda: offsets(nbytes=need - 1), b'workspace'), (lambda: offsets(ws=f + 4), b'aligned'),
        (lambda: flip(n=-1), b'n_meas=-1'), (lambda: flip(nw=-1), b'n_windows=-1'),
        (lambda: flip(wp=None, nw=2), b'win_ptr'), (lambda: flip(py=None), b'null'),
        (lambda: flip(vy=None), b'null'), (lambda: flip(fl=None), b'null'),
        (lambda: labels(N=-1), b'n_nodes=-1'), (lambda: labels(cap=-1), b'pair_capacity=-1'),
        (lambda: labels(N=2 ** 30), b'int32'), (lambda: labels(cap=2 ** 31), b'int32'),
        (lambda: labels(cls=None), b'null node'), (lambda: labels(ox=None), b'null node'),
        (lambda: labels(oy=None), b'null node'), (lambda: labels(nc=None), b'null node'),
        (lambda: labels(no=None), b'null node'), (lambda: labels(ps=None), b'null pair'),
        (lambda: labels(pd=None), b'null pair'), (lambda: labels(npairs=None), b'null pair'),
        (lambda: labels(ec=None), b'null pair'), (lambda: labels(key=None), b'track_key'),
        (lambda: labels(no=f + 4), b'aligned'),
    ]
    for i, (call, needle) in enumerate(cases):
        assert call() == 1, i
        assert needle in lib.rg_last_error(), (i, lib.rg_last_error())
    assert flip(py=None, vy=None, wp=None, nw=1, fl=None, n=0) == 0
    assert flip(nw=0) == 0
    assert offsets(key=None, px=None, py=None, n=0, ox=None, oy=None, ws=None, nbytes=0) == 0
    assert labels(cls=None, ox=None, oy=None, N=0, key=None, ps=None, pd=None, npairs=None, cap=0,
                  nc=None, no=None, ec=None) == 0
    with pytest.raises(RuntimeError, match='rg_train_labels'):
        nat.check(labels(N=-1), 'rg_train_labels')


@pytest.mark.timeout(1200)
def test_training_feed_host_code_under_asan_ubsan():
    """(d) the host code of rg_frontend_flip and rg_train_labels -- every argument check, the
    int32 limits at and past them -- under AddressSanitizer + UndefinedBehaviorSanitizer (host
    side only), driven by the stand-alone tests/training_feed_sanitize_main.cpp; any sanitizer
    report or failed check fails the run.  CPU only: no path it takes reaches a launch."""
    import os
    import subprocess
    from graph_neural_network_for_radar_perception_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = build.build_sanitized_driver(os.path.join(here, 'training_feed_sanitize_main.cpp'))
    env = dict(os.environ, ASAN_OPTIONS='abort_on_error=1:detect_leaks=0',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', HIP_VISIBLE_DEVICES='')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert 'AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
