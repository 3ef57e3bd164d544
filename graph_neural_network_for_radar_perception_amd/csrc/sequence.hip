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
//
// rg_sequence_set_windows (sequence.py, SequenceSet) cuts a batch whose windows come from
// several sequences -- the batch a shuffling loader over create_sequences_info_list's
// metadata (read_data.py:330-396) hands out -- with the same two kernels: they are templates
// over where window b's sequence descriptor comes from, the kernel arguments (OneSequence) or
// a device table indexed by the window's sequence id (SequenceTable).
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

// Where the windows of a batch come from.  at(b, q, scene): the descriptor of the sequence
// window b is cut from and the window's first scene (false: no such sequence, every
// window-scan of b is empty); key_offset(b): what the non-zero track keys of window b are
// shifted by.  q is a copy, so that the one sequence of the arguments stays in the kernel's
// argument registers; of a table's descriptor only the fields that are used are loaded.
struct OneSequence {  // rg_sequence_windows: every window from the sequence in the arguments
  rg_sequence q;
  const int* first;
  __device__ __forceinline__ bool at(int b, rg_sequence& out, long& scene) const {
    scene = first[b];
    out = q;
    return true;
  }
  __device__ __forceinline__ int key_offset(int b) const { return b * q.n_tracks; }
};

struct SequenceTable {  // rg_sequence_set_windows: window b from seqs[win[2b]], a device table
  const rg_sequence* seqs;
  const int* win;
  int n_seq, key_stride;
  __device__ __forceinline__ bool at(int b, rg_sequence& out, long& scene) const {
    const int id = win[2 * (long)b];
    scene = win[2 * (long)b + 1];
    if (id < 0 || id >= n_seq) return false;  // clamped before any read
    out = seqs[id];
    return true;
  }
  __device__ __forceinline__ int key_offset(int b) const { return b * key_stride; }
};

// One workgroup: exclusive scan of the n_ws = n_windows * W scene sizes, 256 at a time with
// a running carry, and everything that exists once per window-scan.
template <class Source>
__global__ __launch_bounds__(SEQ_SCAN_THREADS) void sequence_scan_kernel(
    Source src, int n_windows, int W, rg_window_batch o) {
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
    rg_sequence q = {};
    long scene = 0;
    if (live && src.at(b, q, scene)) r = scene_range(q, scene + w);
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
      const bool ok = r.sensor >= 0 && r.odo >= 0;  // only with a descriptor in q
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
// j is formed through readfirstlane, so the window's entry and its sequence's descriptor are
// read with scalar loads, once per wave and before the first store.
template <class Source>
__global__ __launch_bounds__(64 * SEQ_WAVES) void sequence_gather_kernel(
    Source src, int n_windows, int W, long capacity, rg_window_batch o) {
  const int j = blockIdx.x * SEQ_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= n_windows * W) return;
  const int lane = threadIdx.x & 63;
  const int b = j / W, w = j - b * W;
  rg_sequence q;
  long scene;
  if (!src.at(b, q, scene)) return;
  const SceneRange r = scene_range(q, scene + w);
  const int m0 = o.scan_ptr[j];
  // the scan's own size bounds the source rows, the capacity the output rows
  const long lim = min((long)m0 + r.count, capacity);
  if (m0 < 0) return;
  const int key_off = src.key_offset(b);
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

// the two launches both entry points make
template <class Source>
static int launch_windows(const Source& src, int n_windows, int W, long capacity, bool rows,
                          const rg_window_batch& out, hipStream_t st) {
  sequence_scan_kernel<Source><<<1, SEQ_SCAN_THREADS, 0, st>>>(src, n_windows, W, out);
  RG_LAUNCH_CHECK();
  const int n_ws = n_windows * W;
  if (n_ws > 0 && capacity > 0 && rows) {
    sequence_gather_kernel<Source><<<ceil_div(n_ws, SEQ_WAVES), 64 * SEQ_WAVES, 0, st>>>(
        src, n_windows, W, capacity, out);
    RG_LAUNCH_CHECK();
  }
  return RG_OK;
}

// what both entry points require of the outputs
static int check_outputs(const char* who, const rg_window_batch* out, long capacity) {
  RG_REQUIRE(out->scan_ptr && out->scan_ref && out->win_ptr && out->mount && out->odometry,
             RG_ERR_ARG, "%s: null per-scan output", who);
  RG_REQUIRE(capacity == 0 ||
                 (out->meas_scan && out->src_row && out->x_cc && out->y_cc && out->azimuth_sc &&
                  out->vr && out->vr_compensated && out->rcs && out->timestamp &&
                  out->sensor_id && out->label_id && out->track_key),
             RG_ERR_ARG, "%s: null per-measurement output", who);
  return RG_OK;
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
  if (int rc = check_outputs("rg_sequence_windows", out, capacity)) return rc;
  RG_REQUIRE(((uintptr_t)seq->scenes & 15) == 0, RG_ERR_ARG,
             "rg_sequence_windows: the scene table must be 16-byte aligned");
  const OneSequence src = {*seq, win_first};
  return launch_windows(src, n_windows, W, capacity, seq->n_meas > 0, *out, (hipStream_t)stream);
}

extern "C" int rg_sequence_set_windows(const rg_sequence* seqs, int n_seq, int key_stride,
                                       const int* win, int n_windows, int W, long capacity,
                                       const rg_window_batch* out, void* stream) {
  RG_REQUIRE(seqs && out && win, RG_ERR_ARG, "rg_sequence_set_windows: null argument");
  RG_REQUIRE(n_seq >= 1 && key_stride >= 0, RG_ERR_ARG,
             "rg_sequence_set_windows: n_seq=%d key_stride=%d", n_seq, key_stride);
  RG_REQUIRE(W >= 1 && n_windows >= 0 && capacity >= 0, RG_ERR_ARG,
             "rg_sequence_set_windows: W=%d n_windows=%d capacity=%ld", W, n_windows, capacity);
  RG_REQUIRE((long)n_windows * W < 0x7fffffffL, RG_ERR_ARG,
             "rg_sequence_set_windows: %d windows of %d scans", n_windows, W);
  RG_REQUIRE((long)n_windows * key_stride < 0x7fffffffL, RG_ERR_ARG,
             "rg_sequence_set_windows: %d windows x key stride %d leave int32", n_windows,
             key_stride);
  if (int rc = check_outputs("rg_sequence_set_windows", out, capacity)) return rc;
  RG_REQUIRE(((uintptr_t)seqs & 7) == 0, RG_ERR_ARG,
             "rg_sequence_set_windows: the descriptor table must be 8-byte aligned");
  // the descriptors lie on the device: their sizes and tables are clamped where they are read
  const SequenceTable src = {seqs, win, n_seq, key_stride};
  return launch_windows(src, n_windows, W, capacity, true, *out, (hipStream_t)stream);
}
