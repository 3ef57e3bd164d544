// Sequence store: sliding windows cut from a RadarScenes sequence that lies in HBM once
// (sequence.py, SequenceStore).  Replaces, per batch of windows, the host work of
//   read_data.create_dataset_sliding_window (read_data.py:203-224): the W scenes of a
//   sliding position, and
//   the slicing of extract_and_sync_radar_data (:250-291): radar_data_all_scenes[a:b],
//   odometry_data_all_scenes[index], radar_mount_data['radar_<id>'] per scene,
// with two launches: a one-workgroup scan of the window-scans' scene sizes, then a gather
// with one wave per window-scan (a scene's rows are contiguous in the sequence, so the 64
// lanes of a wave read and write consecutive rows of every field: coalesced both ways).
// ~52 B per measurement; at 64 windows x 10 scans x ~134 rows the launches, not HBM, set
// the time.
#include "rg_common.h"

#include <math.h>

namespace rg {

constexpr int SEQ_SCAN_THREADS = 256;
constexpr int SEQ_WAVES = 4;  // window-scans per workgroup of the gather

struct SceneRange {
  int begin, count, sensor, odo;  // sensor / odo < 0: outside its table
};

// scene s of the chain, its rows cut to [0, n_meas); a scene outside the table is empty
__device__ __forceinline__ SceneRange scene_range(const rg_sequence& q, long s) {
  SceneRange r = {0, 0, -1, -1};
  if (s < 0 || s >= q.n_scenes) return r;
  const int4 row = ((const int4*)q.scenes)[s];
  r.sensor = (row.z >= 0 && row.z < q.n_sensors) ? row.z : -1;
  r.odo = (row.w >= 0 && row.w < q.n_odometry) ? row.w : -1;
  if (r.sensor < 0 || r.odo < 0) return r;
  const int a = min(max(row.x, 0), q.n_meas), b = min(max(row.y, a), q.n_meas);
  r.begin = a;
  r.count = b - a;
  return r;
}

// One workgroup: exclusive scan of the n_ws = n_windows * W scene sizes, 256 at a time with
// a running carry, and everything that exists once per window-scan.
__global__ __launch_bounds__(SEQ_SCAN_THREADS) void sequence_scan_kernel(
    rg_sequence q, const int* __restrict__ win_first, int n_windows, int W, rg_window_batch o) {
  __shared__ int wsum[SEQ_SCAN_THREADS / 64];
  const int n_ws = n_windows * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int carry = 0;
  for (int base = 0; base < n_ws; base += SEQ_SCAN_THREADS) {
    const int j = base + threadIdx.x;
    const bool live = j < n_ws;
    const int b = live ? j / W : 0, w = j - b * W;
    SceneRange r = {0, 0, -1, -1};
    if (live) r = scene_range(q, (long)win_first[b] + w);
    int incl = r.count;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = carry, tot = 0;
    for (int k = 0; k < SEQ_SCAN_THREADS / 64; ++k) {
      if (k < wave) off += wsum[k];
      tot += wsum[k];
    }
    if (live) {
      const int excl = off + incl - r.count;
      o.scan_ptr[j] = excl;
      o.scan_ref[j] = b * W + W - 1;
      if (w == 0) o.win_ptr[b] = excl;
      const bool ok = r.sensor >= 0 && r.odo >= 0;
      for (int c = 0; c < 3; ++c) o.mount[3 * (long)j + c] = ok ? q.mount[3 * r.sensor + c] : nan;
      for (int c = 0; c < 5; ++c)
        o.odometry[5 * (long)j + c] = ok ? q.odometry[5 * (long)r.odo + c] : nan;
    }
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o.scan_ptr[n_ws] = carry;
    o.win_ptr[n_windows] = carry;
  }
}

// One wave per window-scan j: its rows [scan_ptr[j], scan_ptr[j + 1]) from the scene's rows.
__global__ __launch_bounds__(64 * SEQ_WAVES) void sequence_gather_kernel(
    rg_sequence q, const int* __restrict__ win_first, int n_windows, int W, long capacity,
    rg_window_batch o) {
  const int j = blockIdx.x * SEQ_WAVES + (threadIdx.x >> 6);
  if (j >= n_windows * W) return;
  const int lane = threadIdx.x & 63;
  const int b = j / W, w = j - b * W;
  const SceneRange r = scene_range(q, (long)win_first[b] + w);
  const int m0 = o.scan_ptr[j];
  // the scan's own size bounds the source rows, the capacity the output rows
  const long lim = min((long)m0 + r.count, capacity);
  if (m0 < 0) return;
  const int key_off = b * q.n_tracks;
  for (int i = lane; i < r.count; i += 64) {
    const long m = (long)m0 + i;
    if (m >= lim) break;
    const int s = r.begin + i;
    o.meas_scan[m] = j;
    o.src_row[m] = s;
    o.x_cc[m] = q.x_cc[s];
    o.y_cc[m] = q.y_cc[s];
    o.azimuth_sc[m] = q.azimuth_sc[s];
    o.vr[m] = q.vr[s];
    o.vr_compensated[m] = q.vr_compensated[s];
    o.rcs[m] = q.rcs[s];
    o.timestamp[m] = q.timestamp[s];
    o.sensor_id[m] = (int64_t)q.sensor_id[s];
    o.label_id[m] = (int64_t)q.label_id[s];
    const int k = q.track_key[s];
    o.track_key[m] = k == 0 ? 0 : k + key_off;
  }
}

}  // namespace rg

using namespace rg;

extern "C" int rg_sequence_windows(const rg_sequence* seq, const int* win_first, int n_windows,
                                   int W, long capacity, const rg_window_batch* out,
                                   void* stream) {
  RG_REQUIRE(seq && out && win_first, RG_ERR_ARG, "rg_sequence_windows: null argument");
  RG_REQUIRE(W >= 1 && n_windows >= 0 && capacity >= 0, RG_ERR_ARG,
             "rg_sequence_windows: W=%d n_windows=%d capacity=%ld", W, n_windows, capacity);
  RG_REQUIRE(seq->n_scenes >= 0 && seq->n_sensors >= 0 && seq->n_odometry >= 0 &&
                 seq->n_meas >= 0 && seq->n_tracks >= 0,
             RG_ERR_ARG, "rg_sequence_windows: negative size in the sequence (%d scenes, %d "
             "sensors, %d odometry rows, %d measurements, %d tracks)", seq->n_scenes,
             seq->n_sensors, seq->n_odometry, seq->n_meas, seq->n_tracks);
  RG_REQUIRE((long)n_windows * W < 0x7fffffffL, RG_ERR_ARG,
             "rg_sequence_windows: %d windows of %d scans", n_windows, W);
  RG_REQUIRE((long)n_windows * seq->n_tracks < 0x7fffffffL, RG_ERR_ARG,
             "rg_sequence_windows: %d windows x %d tracks leave int32", n_windows,
             seq->n_tracks);
  RG_REQUIRE(seq->scenes && seq->mount && seq->odometry, RG_ERR_ARG,
             "rg_sequence_windows: null table");
  RG_REQUIRE(seq->n_meas == 0 ||
                 (seq->x_cc && seq->y_cc && seq->azimuth_sc && seq->vr && seq->vr_compensated &&
                  seq->rcs && seq->timestamp && seq->sensor_id && seq->label_id &&
                  seq->track_key),
             RG_ERR_ARG, "rg_sequence_windows: null measurement field");
  RG_REQUIRE(out->scan_ptr && out->scan_ref && out->win_ptr && out->mount && out->odometry,
             RG_ERR_ARG, "rg_sequence_windows: null per-scan output");
  RG_REQUIRE(capacity == 0 ||
                 (out->meas_scan && out->src_row && out->x_cc && out->y_cc && out->azimuth_sc &&
                  out->vr && out->vr_compensated && out->rcs && out->timestamp &&
                  out->sensor_id && out->label_id && out->track_key),
             RG_ERR_ARG, "rg_sequence_windows: null per-measurement output");
  RG_REQUIRE(((uintptr_t)seq->scenes & 15) == 0, RG_ERR_ARG,
             "rg_sequence_windows: the scene table must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  sequence_scan_kernel<<<1, SEQ_SCAN_THREADS, 0, st>>>(*seq, win_first, n_windows, W, *out);
  RG_LAUNCH_CHECK();
  const int n_ws = n_windows * W;
  if (n_ws > 0 && capacity > 0 && seq->n_meas > 0) {
    sequence_gather_kernel<<<ceil_div(n_ws, SEQ_WAVES), 64 * SEQ_WAVES, 0, st>>>(
        *seq, win_first, n_windows, W, capacity, *out);
    RG_LAUNCH_CHECK();
  }
  return RG_OK;
}
