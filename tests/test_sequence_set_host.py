"""sequence.SequenceSet on the host (global window order, locate, host_window, the entry
point's argument checks), sequence.dataset_indices against the reference's three lines and
training.shuffled_batches against the DataLoader it restates.  The stores lie on the cpu
device: nothing here cuts a window on a GPU."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from sequence_set_ref import make_set

WS = (1, 3, 4, 10, 24, 25)


def _set():
    return make_set('cpu')


@pytest.mark.parametrize('W', WS)
def test_n_windows_and_locate(W):
    sset = _set()
    scenes = [s.n_scenes for s in sset.stores]
    assert scenes[:3] == [24, 3, 24] and scenes[3] >= 25
    counts = [max(n - W + 1, 0) for n in scenes]
    assert sset.n_windows(W) == sum(counts)
    assert [s.n_windows(W) for s in sset.stores] == counts
    if W >= 4:
        assert counts[1] == 0                         # the member that contributes none
    if W == 25:
        assert counts[0] == 0 and counts[2] == 0 and counts[3] > 0
    # the whole list: members in order, sliding positions ascending
    want_seq = np.concatenate([np.full(c, i, np.int64) for i, c in enumerate(counts)])
    want_pos = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    seq, pos = sset.locate(np.arange(sum(counts)), W)
    assert seq.dtype == np.int64 and pos.dtype == np.int64
    np.testing.assert_array_equal(seq, want_seq)
    np.testing.assert_array_equal(pos, want_pos)
    # the first and last window of every member that has one, out of order and repeated
    start = np.concatenate(([0], np.cumsum(counts)))
    for i, c in enumerate(counts):
        if c == 0:
            assert i not in seq
            continue
        g = [int(start[i + 1]) - 1, int(start[i]), int(start[i + 1]) - 1]
        seq_i, pos_i = sset.locate(g, W)
        np.testing.assert_array_equal(seq_i, [i, i, i])
        np.testing.assert_array_equal(pos_i, [c - 1, 0, c - 1])
    for bad in (-1, sum(counts)):
        with pytest.raises(IndexError, match='outside'):
            sset.locate([0, bad], W)
        with pytest.raises(IndexError):
            sset.host_window(bad, W)
    empty = sset.locate([], W)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)


def test_empty_result_when_no_member_is_long_enough():
    from graph_neural_network_for_radar_perception_amd import sequence
    sset = _set()
    short = sequence.SequenceSet(sset.stores[:3])
    assert short.n_windows(24) == 2 and short.n_windows(25) == 0
    with pytest.raises(IndexError):
        short.locate([0], 25)
    with pytest.raises(ValueError, match='window_size'):
        short.n_windows(0)
    with pytest.raises(ValueError, match='no window'):
        short.windows([], 4)


def test_constructor_checks():
    from graph_neural_network_for_radar_perception_amd import sequence
    with pytest.raises(ValueError, match='at least one'):
        sequence.SequenceSet([])
    sset = _set()
    assert sset.n_tracks == max(s.n_tracks for s in sset.stores) >= 1
    assert len({s.n_tracks for s in sset.stores}) > 1          # the stride is not every member's
    moved = copy.copy(sset.stores[1])
    moved.device = torch.device('meta')
    with pytest.raises(ValueError, match='lies on'):
        sequence.SequenceSet([sset.stores[0], moved])
    # the descriptor table: one rg_sequence per member, in order, as the stores hold them
    from graph_neural_network_for_radar_perception_amd import _native as nat
    raw = sset._table.numpy().tobytes()
    assert len(raw) == len(sset.stores) * ctypes.sizeof(nat.rg_sequence)
    for i, s in enumerate(sset.stores):
        one = bytes(s._seq)
        assert raw[i * len(one):(i + 1) * len(one)] == one


@pytest.mark.parametrize('W', [1, 3, 10])
def test_host_window_is_the_located_stores(W):
    sset = _set()
    n = sset.n_windows(W)
    seq, pos = sset.locate(np.arange(n), W)
    edges = np.nonzero(np.diff(seq))[0]
    for g in sorted({0, n - 1, *edges.tolist(), *(edges + 1).tolist()}):
        got = sset.host_window(g, W)
        want = sset.stores[int(seq[g])].host_window(int(pos[g]), W)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f'{k} g={g}')


@pytest.mark.parametrize('n,num,shuffle', [(97, 0, False), (97, 10, False), (97, 10, True),
                                           (97, 0, True), (40, 40, True), (41, 40, False),
                                           (5, 2, True)])
def test_dataset_indices_restates_the_reference_lines(n, num, shuffle):
    from graph_neural_network_for_radar_perception_amd import sequence
    np.random.seed(1234)
    got = sequence.dataset_indices(n, num, shuffle)
    state = np.random.get_state()[1].copy()
    # set_param_for_training_gnn.py:81-88 on a metadata list that holds its own indices
    np.random.seed(1234)
    metadata = list(range(n))
    if num > 0:
        sample_di = int(len(metadata) / num)
        metadata = metadata[0::sample_di]
    if shuffle:
        random_idx = np.arange(len(metadata))
        np.random.shuffle(random_idx)
        metadata = [metadata[idx] for idx in random_idx]
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, metadata)
    np.testing.assert_array_equal(np.random.get_state()[1], state)   # the same draws, no more
    if shuffle and len(metadata) > 4:
        assert list(got) != sorted(got)


def test_shuffled_batches_is_the_infinite_shuffling_loader():
    from torch.utils.data import DataLoader
    from graph_neural_network_for_radar_perception_amd import training
    torch.manual_seed(3)
    gen = training.shuffled_batches(10, 4)
    got = [next(gen) for _ in range(8)]                   # two and a half epochs + one batch
    torch.manual_seed(3)
    loader = DataLoader(list(range(10)), batch_size=4, shuffle=True)
    want = []
    while len(want) < 8:                                  # infinite_loader (common.py:35-38)
        for batch in loader:
            want.append(batch.numpy())
    assert [len(b) for b in got] == [4, 4, 2, 4, 4, 2, 4, 4]
    for g, w in zip(got, want):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w)
    for e in range(2):                                    # every epoch is a permutation
        assert sorted(np.concatenate(got[3 * e:3 * e + 3]).tolist()) == list(range(10))
    assert not np.array_equal(np.concatenate(got[:3]), np.concatenate(got[3:6]))
    with pytest.raises(ValueError):
        next(training.shuffled_batches(0, 4))


def test_average_counted_on_tensors_follows_the_host_rule():
    from graph_neural_network_for_radar_perception_amd.training import average_counted, total_loss
    nan = float('nan')
    lo = torch.tensor([0.5, 0.0, -1.0, nan, 1.5])
    va = torch.tensor([[0.25, 1.0], [1.0, 2.0], [1.0, nan], [nan, 1.0], [0.75, 3.0]])
    mean, n = average_counted(lo, va)
    assert mean.dtype == torch.float64 and n.dtype == torch.int64 and int(n) == 2
    for c in range(2):
        want, wn = average_counted(lo.numpy(), va[:, c].numpy())
        assert wn == 2 and float(mean[c]) == want
    mean, n = average_counted(lo)
    assert float(mean) == 1.0 and int(n) == 2
    mean, n = average_counted(torch.tensor([0.0, nan]), torch.ones(2, 3))
    assert int(n) == 0 and bool(torch.isnan(mean).all()) and mean.shape == (3,)
    mean, n = average_counted(torch.empty(0), torch.empty(0, 4))
    assert int(n) == 0 and mean.shape == (4,) and bool(torch.isnan(mean).all())
    rows = torch.tensor([[0.1, 0.2, 0.3, 0.4], [1e8, 1.0, -1e8, 1.0]])
    want = [np.float32(0) + r[0] + r[1] + r[2] + r[3] for r in rows.numpy()]   # sum(values())
    np.testing.assert_array_equal(total_loss(rows).numpy(), np.array(want, np.float32))


def test_set_entry_argument_validation_launches_nothing():
    """rg_sequence_set_windows refuses every bad argument the host can see with RG_ERR_ARG and
    a message before anything is launched (no device is needed to get here)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from graph_neural_network_for_radar_perception_amd import build
    build.build_library()
    lib = nat.lib()
    f = 4096  # any non-null address: nothing is dereferenced before the checks fail

    def out(**kw):
        o = nat.rg_window_batch(**{k: f for k, _ in nat.rg_window_batch._fields_})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, seqs=f, n_seq=4, stride=8, win=f, B=2, W=4, cap=100):
        return lib.rg_sequence_set_windows(seqs, n_seq, stride, win, B, W, cap,
                                           ctypes.byref(o) if o is not None else None, None)

    cases = [
        (lambda: call(out(), seqs=None), b'null'), (lambda: call(out(), win=None), b'null'),
        (lambda: call(None), b'null'),
        (lambda: call(out(), n_seq=0), b'n_seq=0'), (lambda: call(out(), n_seq=-2), b'n_seq=-2'),
        (lambda: call(out(), stride=-1), b'key_stride=-1'),
        (lambda: call(out(), W=0), b'W=0'), (lambda: call(out(), W=-3), b'W=-3'),
        (lambda: call(out(), B=-1), b'n_windows=-1'),
        (lambda: call(out(), cap=-5), b'capacity=-5'),
        (lambda: call(out(), B=2 ** 30, W=2), b'windows of'),
        (lambda: call(out(), B=2 ** 31 - 1, W=2 ** 31 - 1), b'windows of'),
        (lambda: call(out(), B=4, stride=2 ** 29), b'int32'),
        (lambda: call(out(), B=2 ** 30, W=1, stride=2 ** 31 - 1), b'int32'),
        (lambda: call(out(scan_ptr=None)), b'per-scan'),
        (lambda: call(out(odometry=None)), b'per-scan'),
        (lambda: call(out(timestamp=None)), b'per-measurement'),
        (lambda: call(out(src_row=None)), b'per-measurement'),
        (lambda: call(out(), seqs=f + 4), b'aligned'),
    ]
    for i, (fn, needle) in enumerate(cases):
        assert fn() == 1, i
        msg = lib.rg_last_error()
        assert b'rg_sequence_set_windows' in msg and needle in msg, (i, msg)
    with pytest.raises(RuntimeError, match='rg_sequence_set_windows'):
        nat.check(call(out(), W=0), 'rg_sequence_set_windows')


@pytest.mark.timeout(1200)
def test_sequence_set_host_code_under_asan_ubsan():
    """rg_sequence_set_windows' host code -- the argument checks, the int32 products at and
    past their limits -- under AddressSanitizer + UndefinedBehaviorSanitizer (host side only),
    driven by the stand-alone tests/sequence_set_sanitize_main.cpp; any sanitizer report or
    failed check fails the run.  CPU only: no path it takes reaches a kernel launch."""
    import os
    import subprocess
    from graph_neural_network_for_radar_perception_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = build.build_sanitized_driver(os.path.join(here, 'sequence_set_sanitize_main.cpp'))
    env = dict(os.environ, ASAN_OPTIONS='abort_on_error=1:detect_leaks=0',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', HIP_VISIBLE_DEVICES='')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert 'AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
