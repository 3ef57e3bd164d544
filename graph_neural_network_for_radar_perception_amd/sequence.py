"""A RadarScenes sequence in HBM, and sliding windows cut from it on the device.

The reference walks a sequence with ``get_sequence_data`` (read_data.py:416-439) and then,
for every sliding position, slices ``radar_data_all_scenes`` scene by scene on the host
(``extract_frame`` -> ``extract_and_sync_radar_data``, :227-303, 442-486).  Here the sequence
is uploaded once (``SequenceStore``) and any batch of sliding windows is cut from it by one
native call (``rg_sequence_windows``, csrc/sequence.hip) into the batch ``ScanWindow`` that
``frontend.extract_and_sync_radar_data`` consumes:

  aggregate_scenes   aggregate_dataset (read_data.py:164-200) on a parsed scenes.json
  sliding_windows    create_dataset_sliding_window (read_data.py:203-224)
  SequenceStore      the arrays of get_sequence_data on the device; ``windows`` is
                     extract_frame's slicing for a batch of sliding positions
  SequenceSet        several stores as the one window list of create_sequences_info_list
                     (read_data.py:330-396); ``windows`` cuts a batch from any mix of them
                     (``rg_sequence_set_windows``)
  dataset_indices    the stride and shuffle of set_param_for_training_gnn.py:81-88 on indices

Nothing here reads a file: the caller parses scenes.json / sensors.json and reads the .h5
arrays.

Track keys.  ``ScanWindow`` holds integer track keys (0 = the empty track id b'').  A window
built on the host ranks its own ids with ``np.unique``; the store ranks the ids of the WHOLE
sequence once (b'' -> 0, the others 1..T in sorted order) and the cut gives batch slot b the
keys ``k + b * T``.  Both steps are strictly increasing maps of the byte-string order, so
within a window the store's keys order, and group, the measurements exactly as the window's
own ranks do -- and that is all the consumers read (``rg_frontend_labels`` sums per key,
``rg_eval_gt_clusters`` lists a frame's tracks in ascending key order).  The same track seen
by two windows of a batch gets two keys, as ``frontend.scan_window_batch``'s offsets make it.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence

import numpy as np

from . import _native as nat

LIST_KEYS = ('current_timestamps', 'radar_id', 'odometry_timestamp', 'odometry_index',
             'radar_data_indices')
F32_FIELDS = ('x_cc', 'y_cc', 'azimuth_sc', 'vr', 'vr_compensated', 'rcs')
ODOMETRY_FIELDS = ('x_seq', 'y_seq', 'yaw_seq', 'vx', 'yaw_rate')
INT32_MAX = 2 ** 31 - 1


def aggregate_scenes(scenes_data: dict) -> Dict[str, list]:
    """aggregate_dataset (read_data.py:164-200) on an already parsed scenes.json: the scenes
    in chain order (first_timestamp, then every next_timestamp) as five lists keyed like a
    window of ``sliding_windows``."""
    scenes = scenes_data['scenes']
    out = {k: [] for k in LIST_KEYS}
    ts = scenes_data['first_timestamp']
    while ts is not None:
        scene = scenes[str(ts)]
        out['current_timestamps'].append(ts)
        out['radar_id'].append(scene['sensor_id'])
        out['odometry_timestamp'].append(scene['odometry_timestamp'])
        out['odometry_index'].append(scene['odometry_index'])
        out['radar_data_indices'].append(scene['radar_indices'])
        ts = scene['next_timestamp']
    return out


def sliding_windows(window_size: int, lists: Dict[str, list]) -> List[dict]:
    """create_dataset_sliding_window (read_data.py:203-224): one dict per sliding position
    with the same keys and the same slices; S - W + 1 entries, none when S < W."""
    n = len(lists['current_timestamps'])
    return [{k: lists[k][i:i + window_size] for k in LIST_KEYS}
            for i in range(n - window_size + 1)]


def _field(data, name):
    try:
        return np.asarray(data[name])
    except (KeyError, ValueError, IndexError) as exc:
        raise KeyError(f'radar_data has no field {name!r}') from exc


def _upload_small(a: np.ndarray, dev):
    """A small host array to the device without a host synchronisation (page-locked staging,
    asynchronous copy on the current stream)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dev.type == 'cuda':
        return t.pin_memory().to(dev, non_blocking=True)
    return t.to(dev)


class SequenceStore:
    """One sequence on the device: the measurement fields, the scene table (int32
    [S, 4]: begin, end, mount row, odometry row), the mount table (f64 [n_sensors, 3]) and
    the odometry table (f64 [n_odo, 5]); the host keeps the scene table, the prefix sums of
    the scene sizes and the arrays it was built from (``host_window``)."""

    def __init__(self, host: dict, scenes: np.ndarray, mount: np.ndarray, odometry: np.ndarray,
                 track_key: np.ndarray, n_tracks: int, lists: Dict[str, list], device):
        import torch
        self.device = torch.device(device)
        self.host = host
        self.scenes = scenes
        self.mount_table = mount
        self.odometry_table = odometry
        self.track_key = track_key
        self.n_tracks = int(n_tracks)
        self.lists = lists
        self.n_scenes = int(scenes.shape[0])
        self.n_meas = int(track_key.shape[0])
        sizes = np.maximum(scenes[:, 1].astype(np.int64) - scenes[:, 0], 0)
        self.prefix = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        dev = self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.dev = {k: up(host[k]) for k in F32_FIELDS + ('timestamp', 'sensor_id', 'label_id')}
        self.dev['track_key'] = up(track_key)
        self.dev['scenes'] = up(scenes)
        self.dev['mount'] = up(mount)
        self.dev['odometry'] = up(odometry)
        d = self.dev
        self._seq = nat.rg_sequence(
            scenes=d['scenes'].data_ptr(), mount=d['mount'].data_ptr(),
            odometry=d['odometry'].data_ptr(), timestamp=d['timestamp'].data_ptr(),
            sensor_id=d['sensor_id'].data_ptr(), label_id=d['label_id'].data_ptr(),
            track_key=d['track_key'].data_ptr(), n_scenes=self.n_scenes,
            n_sensors=int(mount.shape[0]), n_odometry=int(odometry.shape[0]),
            n_meas=self.n_meas, n_tracks=self.n_tracks,
            **{k: d[k].data_ptr() for k in F32_FIELDS})

    @staticmethod
    def from_numpy(radar_data, odometry, lists: Dict[str, list], sensors: dict,
                   device) -> 'SequenceStore':
        """radar_data: the structured array f["radar_data"][:] (or a dict of equally long
        arrays) with timestamp, sensor_id, azimuth_sc, rcs, vr, vr_compensated, x_cc, y_cc,
        track_id (byte strings), label_id; odometry: the structured array f["odometry"][:];
        lists: ``aggregate_scenes``' result; sensors: the parsed sensors.json (keys
        'radar_<id>').  Everything is uploaded once; the track ids become integer keys once
        (np.unique over the sequence's byte strings)."""
        host = {k: np.ascontiguousarray(_field(radar_data, k), dtype=np.float32)
                for k in F32_FIELDS}
        host['timestamp'] = np.ascontiguousarray(_field(radar_data, 'timestamp'), dtype=np.int64)
        host['sensor_id'] = np.ascontiguousarray(_field(radar_data, 'sensor_id'), dtype=np.uint8)
        host['label_id'] = np.ascontiguousarray(_field(radar_data, 'label_id'), dtype=np.uint8)
        host['track_id'] = _field(radar_data, 'track_id')
        n_meas = int(host['timestamp'].shape[0])
        for k, v in host.items():
            if v.ndim != 1 or v.shape[0] != n_meas:
                raise ValueError(f'radar_data[{k!r}]: shape {v.shape}, expected ({n_meas},)')
        if n_meas > INT32_MAX:
            raise ValueError(f'{n_meas} measurements do not fit int32 row indices')
        for k in LIST_KEYS:
            if len(lists[k]) != len(lists['radar_id']):
                raise ValueError(f'lists[{k!r}] has {len(lists[k])} entries, radar_id '
                                 f'{len(lists["radar_id"])}')
        n_scenes = len(lists['radar_id'])
        # mount table: one row per sensor, ascending id
        ids = sorted(int(v['id']) if 'id' in v else int(name.split('_')[1])
                     for name, v in sensors.items())
        row_of = {i: r for r, i in enumerate(ids)}
        mount = np.array([[sensors[f'radar_{i}'][c] for c in ('x', 'y', 'yaw')] for i in ids],
                         dtype=np.float64).reshape(len(ids), 3)
        odo = np.stack([np.asarray(odometry[c], dtype=np.float64) for c in ODOMETRY_FIELDS],
                       axis=-1).reshape(-1, 5)
        scenes = np.zeros((n_scenes, 4), dtype=np.int32)
        if n_scenes:
            rng = np.asarray(lists['radar_data_indices'], dtype=np.int64).reshape(n_scenes, 2)
            if (rng < 0).any() or (rng > n_meas).any():
                raise ValueError(f'radar_data_indices outside [0, {n_meas}]')
            oi = np.asarray(lists['odometry_index'], dtype=np.int64)
            if (oi < 0).any() or (oi >= odo.shape[0]).any():
                raise ValueError(f'odometry_index outside [0, {odo.shape[0]})')
            missing = sorted({int(r) for r in lists['radar_id']} - set(row_of))
            if missing:
                raise KeyError(f'sensors has no radar_{missing[0]}')
            scenes[:, :2] = rng
            scenes[:, 2] = [row_of[int(r)] for r in lists['radar_id']]
            scenes[:, 3] = oi
        uniq, inv = np.unique(host['track_id'], return_inverse=True)
        keys = inv.astype(np.int64).reshape(-1) + 1
        if uniq.size and uniq[0] == b'':
            keys -= 1                                # b'' sorts first: key 0 = no track
        n_tracks = int(keys.max(initial=0))
        return SequenceStore(host, scenes, mount, odo, keys.astype(np.int32), n_tracks,
                             {k: list(lists[k]) for k in LIST_KEYS}, device)

    def n_windows(self, window_size: int) -> int:
        """The number of sliding positions (create_dataset_sliding_window): S - W + 1."""
        if int(window_size) < 1:
            raise ValueError(f'window_size={window_size} < 1')
        return max(self.n_scenes - int(window_size) + 1, 0)

    def _check(self, indices, window_size: int) -> np.ndarray:
        nw = self.n_windows(window_size)
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        bad = idx[(idx < 0) | (idx >= nw)]
        if bad.size:
            raise IndexError(f'window {int(bad[0])} outside [0, {nw}) for window_size='
                             f'{window_size}')
        return idx

    def host_window(self, i: int, window_size: int = 10) -> dict:
        """Sliding position i as host arrays in ``synthetic.make_scan_window``'s layout (the
        input of ``frontend.ScanWindow.from_numpy``): the slicing and concatenation of
        extract_and_sync_radar_data (read_data.py:250-291) for one window."""
        i = int(self._check([i], window_size)[0])
        W = int(window_size)
        sc = self.scenes[i:i + W]
        sl = [slice(int(a), int(max(a, b))) for a, b in sc[:, :2]]
        h = self.host
        out = {k: np.concatenate([h[k][s] for s in sl]) for k in F32_FIELDS + ('timestamp',)}
        for k in ('sensor_id', 'label_id'):
            out[k] = np.concatenate([h[k][s] for s in sl]).astype(np.int64)
        out['track_id_bytes'] = np.concatenate([h['track_id'][s] for s in sl])
        out['track_key'] = np.concatenate([self.track_key[s] for s in sl]).astype(np.int64)
        ptr = np.concatenate(([0], np.cumsum([s.stop - s.start for s in sl]))).astype(np.int64)
        out.update(n_scans=W, scan_ptr=ptr, mount=self.mount_table[sc[:, 2]].copy(),
                   odometry=self.odometry_table[sc[:, 3]].copy())
        return out

    def windows(self, indices: Sequence[int], window_size: int = 10):
        """The sliding positions ``indices`` (host integers; repeats and overlaps allowed) as
        ONE batch ``frontend.ScanWindow``, as ``frontend.scan_window_batch`` builds it from
        the host windows: one small asynchronous upload of the positions and one native call
        (two launches), no host synchronisation.  The window also carries ``meas_scan`` (the
        window-scan of every measurement) and ``src_row`` (its row in the sequence)."""
        import torch
        from .frontend import ScanWindow
        idx = self._check(indices, window_size)
        W, B = int(window_size), int(idx.shape[0])
        if B == 0:
            raise ValueError('no window requested')
        if B * max(self.n_tracks, 1) > INT32_MAX or B * W > INT32_MAX:
            raise ValueError(f'{B} windows x {self.n_tracks} tracks (x {W} scans) leave int32')
        total = int((self.prefix[idx + W] - self.prefix[idx]).sum())
        if total > INT32_MAX:
            raise ValueError(f'{total} measurements in one batch do not fit int32 offsets')
        dev = self.device
        first = _upload_small(idx.astype(np.int32), dev)
        n_ws = B * W
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        arrays = {k: torch.empty(total, **f32) for k in F32_FIELDS}
        for k in ('timestamp', 'sensor_id', 'label_id'):
            arrays[k] = torch.empty(total, **i64)
        scan_ptr, scan_ref = torch.empty(n_ws + 1, **i32), torch.empty(n_ws, **i32)
        win_ptr = torch.empty(B + 1, **i32)
        mount = torch.empty((n_ws, 3), dtype=torch.float64, device=dev)
        odo = torch.empty((n_ws, 5), dtype=torch.float64, device=dev)
        key, meas_scan, src_row = (torch.empty(total, **i32) for _ in range(3))
        out = nat.rg_window_batch(
            scan_ptr=scan_ptr.data_ptr(), scan_ref=scan_ref.data_ptr(),
            win_ptr=win_ptr.data_ptr(), mount=mount.data_ptr(), odometry=odo.data_ptr(),
            meas_scan=meas_scan.data_ptr(), src_row=src_row.data_ptr(),
            track_key=key.data_ptr(), **{k: v.data_ptr() for k, v in arrays.items()})
        nat.check(nat.lib().rg_sequence_windows(ctypes.byref(self._seq), first.data_ptr(), B, W,
                                                total, ctypes.byref(out), nat.stream_ptr(dev)),
                  'rg_sequence_windows')
        w = ScanWindow(arrays, scan_ptr, mount, odo, key, B * self.n_tracks, scan_ref, win_ptr)
        w.meas_scan, w.src_row = meas_scan, src_row
        return w


class SequenceSet:
    """Several sequences on one device as ONE list of sliding windows, in the order of
    ``create_sequences_info_list`` (read_data.py:330-396): the stores in the given order and,
    within a store, the sliding positions in ascending order; a store with fewer than W scenes
    contributes no window.  ``windows`` cuts a batch from any mix of the stores in one native
    call (``rg_sequence_set_windows``), so the set goes wherever a ``SequenceStore`` goes
    (``n_windows`` and ``windows`` are all the sequence loops read).

    Track keys: batch slot b gets the keys ``k + b * T_max`` with ``T_max`` the largest
    ``n_tracks`` of the stores (at least 1), so its non-zero keys lie in
    ``(b * T_max, (b + 1) * T_max]`` and within a window they order and group the measurements
    as the window's own store's keys do (the module docstring's argument, unchanged).

    Sharding a batch across ranks stays with the caller, who passes each rank its indices."""

    def __init__(self, stores: Sequence[SequenceStore]):
        import torch
        self.stores = list(stores)
        if not self.stores:
            raise ValueError('a SequenceSet needs at least one SequenceStore')
        self.device = self.stores[0].device
        for i, s in enumerate(self.stores):
            if s.device != self.device:
                raise ValueError(f'store {i} lies on {s.device}, store 0 on {self.device}')
        self.n_tracks = max(max(s.n_tracks for s in self.stores), 1)      # T_max
        table = (nat.rg_sequence * len(self.stores))(*(s._seq for s in self.stores))
        raw = np.frombuffer(bytes(table), dtype=np.uint8).copy()
        self._table = torch.from_numpy(raw).to(self.device)    # the descriptors, uploaded once

    def _starts(self, window_size: int) -> np.ndarray:
        """Global index of every store's first window, and the total: int64 [n_stores + 1]."""
        counts = [s.n_windows(window_size) for s in self.stores]
        return np.concatenate(([0], np.cumsum(counts))).astype(np.int64)

    def n_windows(self, window_size: int) -> int:
        return int(self._starts(window_size)[-1])

    def locate(self, indices, window_size: int):
        """Global windows to (store index int64 [B], sliding position int64 [B]), host."""
        starts = self._starts(window_size)
        nw = int(starts[-1])
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        bad = idx[(idx < 0) | (idx >= nw)]
        if bad.size:
            raise IndexError(f'window {int(bad[0])} outside [0, {nw}) for window_size='
                             f'{window_size}')
        seq = np.searchsorted(starts, idx, side='right').astype(np.int64) - 1
        return seq, idx - starts[seq]

    def host_window(self, g: int, window_size: int = 10) -> dict:
        """Global window g as host arrays: the located store's ``host_window``."""
        seq, pos = self.locate([g], window_size)
        return self.stores[int(seq[0])].host_window(int(pos[0]), window_size)

    def windows(self, indices: Sequence[int], window_size: int = 10):
        """The global windows ``indices`` (host integers; any mix of the stores, repeats
        allowed) as ONE batch ``frontend.ScanWindow``, as ``SequenceStore.windows`` gives it:
        one small asynchronous upload (store, position per window) and one native call, no
        host synchronisation.  The window carries ``meas_scan``, ``src_row`` (the row inside
        the window's own store) and ``win_seq`` (int32 [B]: the window's store)."""
        import torch
        from .frontend import ScanWindow
        seq, pos = self.locate(indices, window_size)
        W, B, T = int(window_size), int(seq.shape[0]), self.n_tracks
        if B == 0:
            raise ValueError('no window requested')
        if B * T > INT32_MAX or B * W > INT32_MAX:
            raise ValueError(f'{B} windows x {T} tracks (x {W} scans) leave int32')
        total = 0
        for s in np.unique(seq):
            p, prefix = pos[seq == s], self.stores[int(s)].prefix
            total += int((prefix[p + W] - prefix[p]).sum())
        if total > INT32_MAX:
            raise ValueError(f'{total} measurements in one batch do not fit int32 offsets')
        dev = self.device
        win = _upload_small(np.stack((seq, pos), axis=1).astype(np.int32), dev)
        n_ws = B * W
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        arrays = {k: torch.empty(total, **f32) for k in F32_FIELDS}
        for k in ('timestamp', 'sensor_id', 'label_id'):
            arrays[k] = torch.empty(total, **i64)
        scan_ptr, scan_ref = torch.empty(n_ws + 1, **i32), torch.empty(n_ws, **i32)
        win_ptr = torch.empty(B + 1, **i32)
        mount = torch.empty((n_ws, 3), dtype=torch.float64, device=dev)
        odo = torch.empty((n_ws, 5), dtype=torch.float64, device=dev)
        key, meas_scan, src_row = (torch.empty(total, **i32) for _ in range(3))
        out = nat.rg_window_batch(
            scan_ptr=scan_ptr.data_ptr(), scan_ref=scan_ref.data_ptr(),
            win_ptr=win_ptr.data_ptr(), mount=mount.data_ptr(), odometry=odo.data_ptr(),
            meas_scan=meas_scan.data_ptr(), src_row=src_row.data_ptr(),
            track_key=key.data_ptr(), **{k: v.data_ptr() for k, v in arrays.items()})
        nat.check(nat.lib().rg_sequence_set_windows(
            self._table.data_ptr(), len(self.stores), T, win.data_ptr(), B, W, total,
            ctypes.byref(out), nat.stream_ptr(dev)), 'rg_sequence_set_windows')
        w = ScanWindow(arrays, scan_ptr, mount, odo, key, B * T, scan_ref, win_ptr)
        w.meas_scan, w.src_row, w.win_seq = meas_scan, src_row, win[:, 0]
        return w


def dataset_indices(n: int, num_samples: int = 0, shuffle: bool = False) -> np.ndarray:
    """set_param_for_training_gnn.py:81-88 (and :102-109) on the indices of a metadata list
    of n windows: with ``num_samples > 0`` every ``int(n / num_samples)``-th window from the
    first, then with ``shuffle`` the ``np.random.shuffle`` permutation of an ``arange`` drawn
    from numpy's global generator.  int64, host."""
    idx = np.arange(int(n), dtype=np.int64)
    if num_samples > 0:
        idx = idx[0::int(int(n) / num_samples)]
    if shuffle:
        order = np.arange(len(idx))
        np.random.shuffle(order)
        idx = idx[order]
    return idx
