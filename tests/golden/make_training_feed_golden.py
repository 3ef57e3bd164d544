"""Golden fixture of the training feed (csrc/training_feed.hip, training.training_labels) made
by the REFERENCE.

Runs only where the reference checkout exists (never on the GPU box; nothing in tests/ imports
this file).  It loads the arrays of tests/golden/sequence_148_s40.npz (made by
make_sequence_golden.py: the first 40 scenes of sequence_148's real chain and sensors.json,
synthetic measurements with the real files' dtypes), points
``read_data.extract_radar_mount_data`` and ``read_data.extract_sensor_data_all_scenes`` at
them (the .h5 files and h5py are absent) and runs the reference's own
``RadarScenesDataset.__getitem__`` (datagen_gnn.py:82-141) with the grid, k and eps of
configuration_radarscenes_gnn.yml, at the sliding positions CASES, each with the x-axis flip
off (dataset_augmentation False: no draw) and on (dataset_augmentation True, numpy seeded so
that the item's ``np.random.rand()`` is >= 0.5; the seed and the drawn value are stored).

Stored per case ``w<W>_p<pos>_f<flip>/``: the dynamic px, py, vx, vy (other_features_dyn),
node_class, node_offsets, edge_index, edge_class, the clusters as cluster_ptr / cluster_idx,
cluster_labels, seed, draw.

Usage:  python tests/golden/make_training_feed_golden.py
        (writes tests/golden/training_feed_148_s40.npz)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.modules.setdefault('h5py', types.ModuleType('h5py'))

from modules.compute_features.grid_features import grid_properties  # noqa: E402
from modules.data_generator.datagen_gnn import RadarScenesDataset  # noqa: E402
from modules.data_utils import read_data  # noqa: E402

SOURCE = 'sequence_148_s40.npz'
CASES = ((10, 0), (10, 7), (10, 30), (4, 36))   # (window size, sliding position)
LIST_KEYS = ('current_timestamps', 'radar_id', 'odometry_timestamp', 'odometry_index',
             'radar_data_indices')
RADAR_DTYPE = np.dtype([('timestamp', '<i8'), ('sensor_id', 'u1'), ('azimuth_sc', '<f4'),
                        ('rcs', '<f4'), ('vr', '<f4'), ('vr_compensated', '<f4'),
                        ('x_cc', '<f4'), ('y_cc', '<f4'), ('track_id', 'S32'),
                        ('label_id', 'u1')])
ODOMETRY_DTYPE = np.dtype([('x_seq', '<f8'), ('y_seq', '<f8'), ('yaw_seq', '<f8'),
                           ('vx', '<f8'), ('yaw_rate', '<f8')])


class Config:   # configuration_radarscenes_gnn.yml:11-15, 26
    dataset_path = 'RadarScenesData/data'
    reject_static_meas_by_ransac = False
    ball_query_eps_square = 25
    k_number_nearest_points = 10
    include_region_confidence = True

    def __init__(self, augmentation):
        self.dataset_augmentation = augmentation


def load_source():
    d = np.load(os.path.join(HERE, SOURCE), allow_pickle=False)
    radar = np.zeros(len(d['radar/timestamp']), RADAR_DTYPE)
    for k in RADAR_DTYPE.names:
        radar[k] = d['radar/' + k]
    odo = np.zeros(len(d['odometry/vx']), ODOMETRY_DTYPE)
    for k in ODOMETRY_DTYPE.names:
        odo[k] = d['odometry/' + k]
    sensors = {'radar_%d' % int(i): dict(id=int(i), x=float(m[0]), y=float(m[1]), yaw=float(m[2]))
               for i, m in zip(d['sensors/id'], d['sensors/mount'])}
    lists = [d['lists/' + k].tolist() for k in LIST_KEYS]
    return radar, odo, sensors, lists


def seed_for(flip):
    """The first seed whose first np.random.rand() falls on the wanted side of 0.5."""
    seed = 0
    while True:
        np.random.seed(seed)
        draw = float(np.random.rand())
        if (draw >= 0.5) == flip:
            return seed, draw
        seed += 1


def main():
    radar, odo, sensors, lists = load_source()
    read_data.extract_radar_mount_data = lambda root, path: sensors
    read_data.extract_sensor_data_all_scenes = lambda name, root, path: (radar, odo)
    grid = grid_properties(0, 100, -50, 50, 0.5, 2, 0.5, 2, 0.5, 0.5)  # yml:34-44
    out = {'cases': np.array(CASES, np.int64)}
    for W, pos in CASES:
        wins = read_data.create_dataset_sliding_window(W, *lists)
        meta = [{'sequence_name': 'sequence_148', 'data': w} for w in wins]
        for flip in (False, True):
            ds = RadarScenesDataset(meta, '', grid, Config(flip), 'cpu')
            seed, draw = (-1, np.nan)
            if flip:
                seed, draw = seed_for(True)
                np.random.seed(seed)
            feats, labels = ds[pos]
            assert feats is not None, (W, pos, flip)
            other = feats['other_features_dyn'].numpy()
            pre = f'w{W}_p{pos}_f{int(flip)}/'
            for c, k in enumerate(('px', 'py', 'vx', 'vy')):
                out[pre + k] = other[:, c].copy()
            out[pre + 'node_class'] = labels['node_class'].numpy().astype(np.int64)
            out[pre + 'node_offsets'] = labels['node_offsets'].numpy().astype(np.float32)
            out[pre + 'edge_index'] = feats['edge_index_dyn'].numpy().astype(np.int64)
            out[pre + 'edge_class'] = labels['edge_class'].numpy().astype(np.int64)
            members = [c.numpy().astype(np.int64) for c in labels['cluster_node_idx']]
            out[pre + 'cluster_ptr'] = np.concatenate(
                ([0], np.cumsum([len(m) for m in members]))).astype(np.int64)
            out[pre + 'cluster_idx'] = np.concatenate(members).astype(np.int64)
            out[pre + 'cluster_labels'] = labels['cluster_labels'].numpy().astype(np.int64)
            out[pre + 'seed'] = np.int64(seed)
            out[pre + 'draw'] = np.float64(draw)
            sizes = np.diff(out[pre + 'cluster_ptr'])
            print(pre, 'nodes', other.shape[0], 'edges', out[pre + 'edge_index'].shape[1],
                  'pairs', len(out[pre + 'edge_class']), 'positive',
                  int(out[pre + 'edge_class'].sum()), 'clusters', len(sizes), 'of >= 2',
                  int((sizes >= 2).sum()), 'seed', seed, 'draw', draw)
    path = os.path.join(HERE, 'training_feed_148_s40.npz')
    np.savez_compressed(path, **out)
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
