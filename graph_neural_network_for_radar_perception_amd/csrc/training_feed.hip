// Training feed: what RadarScenesDataset.__getitem__ (datagen_gnn.py:82-141) adds to the
// front-end's dynamic frame before a training step, for a batch of windows on the device:
//   rg_frontend_flip   the x-axis flip augmentation of get_data_for_datagen
//                      (read_data.py:522-524): meas_py, meas_vy negated for the flagged windows
//   rg_train_labels    the label tensors of datagen_gnn.py:126-134: node_class, node_offsets
//                      and the edge labels of compute_edge_labels.py:7-20 in link-pair order
//   rg_train_offsets   the offsets to the track mean of generate_gt_offset
//                      (compute_node_labels.py:50-67) with np.mean's own float32 sum (below)
// The first two are element-wise: one grid-stride pass, every lane one coalesced load and one store per
// array, no LDS, no atomics.  At a batch of 64 windows (~86 k measurements in, ~19 k nodes and
// ~114 k pairs out: ~3 MB moved) the launch, not HBM, sets the time; the cluster side of the
// labels is rg_eval_gt_clusters (evaluation.hip).
#include "rg_common.h"

namespace rg {

constexpr int FEED_THREADS = 256;
constexpr int FEED_MAX_BLOCKS = 2048;  // 8 workgroups per CU; larger inputs stride

// the window of measurement m: the last w in [0, n_windows) with win_ptr[w] <= m (an empty
// window shares its start with the next one and is never the last such w); -1 outside
// [win_ptr[0], win_ptr[n_windows])
__device__ __forceinline__ int window_of(const int* __restrict__ win_ptr, int n_windows, int m) {
  if (m < win_ptr[0] || m >= win_ptr[n_windows]) return -1;
  int lo = 0, hi = n_windows;  // win_ptr[lo] <= m < win_ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (win_ptr[mid] <= m) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(FEED_THREADS) void frontend_flip_kernel(
    float* __restrict__ py, float* __restrict__ vy, const int* __restrict__ win_ptr,
    int n_windows, const uint8_t* __restrict__ flip, int n_meas) {
  const int stride = gridDim.x * FEED_THREADS;
  for (long m = blockIdx.x * FEED_THREADS + threadIdx.x; m < n_meas; m += stride) {
    const int w = win_ptr ? window_of(win_ptr, n_windows, (int)m) : 0;
    if (w < 0 || !flip[w]) continue;
    py[m] = -py[m];
    vy[m] = -vy[m];
  }
}

__global__ __launch_bounds__(FEED_THREADS) void train_labels_kernel(
    const float* __restrict__ class_labels, const float* __restrict__ offset_x,
    const float* __restrict__ offset_y, int n_nodes, const int* __restrict__ track_key,
    const int* __restrict__ pair_src, const int* __restrict__ pair_dst,
    const int* __restrict__ n_pairs_dev, int pair_capacity, int64_t* __restrict__ node_class,
    float2* __restrict__ node_offsets, int64_t* __restrict__ edge_class) {
  const int stride = gridDim.x * FEED_THREADS;
  const int n_pairs = pair_capacity > 0 ? min(max(*n_pairs_dev, 0), pair_capacity) : 0;
  const int n = max(n_nodes, pair_capacity);
  for (long i = blockIdx.x * FEED_THREADS + threadIdx.x; i < n; i += stride) {  // long: i + stride may pass int32
    if (i < n_nodes) {
      node_class[i] = (int64_t)class_labels[i];
      node_offsets[i] = make_float2(offset_x[i], offset_y[i]);
    }
    if (i < pair_capacity) {
      int64_t label = 0;
      if (i < n_pairs) {
        const int s = pair_src[i], d = pair_dst[i];
        // an endpoint outside the nodes reads no key: label 0
        if ((unsigned)s < (unsigned)n_nodes && (unsigned)d < (unsigned)n_nodes) {
          const int ks = track_key[s];
          label = (ks == track_key[d] && ks != 0) ? 1 : 0;
        }
      }
      edge_class[i] = label;
    }
  }
}

// ---------------------------------------------------------------------------
// rg_train_offsets: the offsets to the track mean with the mean numpy takes.
// generate_gt_offset (compute_node_labels.py:60-66) calls np.mean on the float32 positions
// of a track in measurement order: a float32 pairwise sum (below 8 values one running sum;
// up to 128 values eight interleaved running sums, combined as a tree, then the last n % 8
// values one by one; above 128 values the two halves, the first a multiple of 8, summed the
// same way and added) divided by the count.  rg_frontend_labels averages in
// float64, which differs from this in the last bit for about a third of the values; a
// training label is compared with the reference's exactly, so the feed takes the same sum.
// That order is how numpy's float add reduction is written (pairwise_sum in its
// loops_utils.h.src, PW_BLOCKSIZE 128), not something numpy documents or promises: it has
// been the same from numpy 1.9 on, and tests/golden/training_feed_148_s40.npz was made with
// numpy 2.2.6.  Should a later numpy sum otherwise, the fixture made with it and
// test_offsets_take_numpys_float32_mean (against the installed np.mean) show it at once.
// ---------------------------------------------------------------------------
constexpr int PW_BLOCK = 128;   // numpy's PW_BLOCKSIZE
constexpr int PW_DEPTH = 26;    // halvings from 2^31 values down to <= 128

__global__ __launch_bounds__(FEED_THREADS) void track_extent_kernel(
    const int* __restrict__ track_key, int n_tracks, int n_meas, int* __restrict__ first,
    int* __restrict__ count) {
  const int stride = gridDim.x * FEED_THREADS;
  for (long m = blockIdx.x * FEED_THREADS + threadIdx.x; m < n_meas; m += stride) {
    const int k = track_key[m];
    if (k <= 0 || k > n_tracks) continue;
    atomicMin(first + k, (int)m);
    atomicAdd(count + k, 1);
  }
}

// the members of one track in measurement order, handed out one by one to a whole wave (every
// lane sees the same values): 64 keys per coalesced load, a ballot of the matches, the matching
// lanes' positions broadcast in lane order
struct TrackWalker {
  const int* key;
  const float* px;
  const float* py;
  int k, n_meas, base, lane;
  unsigned long long mask;
  float x, y;
  __device__ __forceinline__ float2 next() {
    while (mask == 0ull) {
      if (base >= n_meas) return make_float2(0.f, 0.f);  // never, for a count from the same keys
      const int m = base + lane;
      const bool hit = m < n_meas && key[m] == k;
      x = hit ? px[m] : 0.f;
      y = hit ? py[m] : 0.f;
      mask = __ballot(hit);
      base += 64;
    }
    const int b = __ffsll((long long)mask) - 1;
    mask &= mask - 1ull;
    return make_float2(__shfl(x, b), __shfl(y, b));
  }
};

__device__ __forceinline__ float2 add2f(float2 a, float2 b) {
  return make_float2(a.x + b.x, a.y + b.y);
}

// numpy's sum of the next n <= PW_BLOCK members
__device__ float2 pairwise_block(TrackWalker& w, int n) {
  if (n < 8) {
    float2 res = make_float2(0.f, 0.f);
    for (int i = 0; i < n; ++i) res = add2f(res, w.next());
    return res;
  }
  float2 r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = w.next();
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = add2f(r[j], w.next());
  }
  float2 res = add2f(add2f(add2f(r[0], r[1]), add2f(r[2], r[3])),
                     add2f(add2f(r[4], r[5]), add2f(r[6], r[7])));
  for (; i < n; ++i) res = add2f(res, w.next());
  return res;
}

// one wave per track key: mean[k] = numpy's float32 mean of the track's px and py
__global__ __launch_bounds__(FEED_THREADS) void track_mean_kernel(
    const int* __restrict__ track_key, const float* __restrict__ px,
    const float* __restrict__ py, int n_tracks, int n_meas, const int* __restrict__ first,
    const int* __restrict__ count, float2* __restrict__ mean) {
  __shared__ int s_size[FEED_THREADS / 64][PW_DEPTH], s_state[FEED_THREADS / 64][PW_DEPTH];
  __shared__ float2 s_part[FEED_THREADS / 64][PW_DEPTH];
  const int k = 1 + blockIdx.x * (FEED_THREADS / 64) + (threadIdx.x >> 6);
  if (k > n_tracks) return;
  const int n = count[k];
  if (n <= 0) return;
  const int lane = threadIdx.x & 63;
  const int f = min(max(first[k], 0), n_meas);
  TrackWalker w{track_key, px, py, k, n_meas, f & ~63, lane, 0ull, 0.f, 0.f};
  float2 sum;
  if (n <= PW_BLOCK) {
    sum = pairwise_block(w, n);
  } else {
    // the recursion of the pairwise sum in member order: a node's size, the sum of its first
    // half once that is done, and what is left to do (0 enter, 1 second half, 2 combine).
    // The stack is indexed at run time, so it lives in LDS, a slice per wave (as registers
    // it would be scratch memory for every wave, for the few tracks above 128 members);
    // every lane writes and reads the same values at the same addresses: no barrier
    int* size = s_size[threadIdx.x >> 6];
    int* state = s_state[threadIdx.x >> 6];
    float2* part = s_part[threadIdx.x >> 6];
    int sp = 0;
    size[0] = n;
    state[0] = 0;
    sum = make_float2(0.f, 0.f);
    while (sp >= 0) {
      const int s = size[sp];
      if (s <= PW_BLOCK) {
        sum = pairwise_block(w, s);
        --sp;
        continue;
      }
      int half = s / 2;
      half -= half % 8;
      if (state[sp] == 0) {
        state[sp] = 1;
        size[sp + 1] = half;
        state[sp + 1] = 0;
        ++sp;
      } else if (state[sp] == 1) {
        part[sp] = sum;
        state[sp] = 2;
        size[sp + 1] = s - half;
        state[sp + 1] = 0;
        ++sp;
      } else {
        sum = add2f(part[sp], sum);
        --sp;
      }
    }
  }
  // numpy divides the float32 sum by the count in float64 and rounds once to float32
  if (lane == 0)
    mean[k] = make_float2((float)((double)sum.x / (double)n), (float)((double)sum.y / (double)n));
}

__global__ __launch_bounds__(FEED_THREADS) void track_offsets_kernel(
    const int* __restrict__ track_key, const float* __restrict__ px,
    const float* __restrict__ py, int n_tracks, int n_meas, const float2* __restrict__ mean,
    float* __restrict__ offx, float* __restrict__ offy) {
  const int stride = gridDim.x * FEED_THREADS;
  for (long m = blockIdx.x * FEED_THREADS + threadIdx.x; m < n_meas; m += stride) {
    const int k = track_key[m];
    float2 o = make_float2(0.f, 0.f);  // untracked measurements keep 0
    if (k > 0 && k <= n_tracks) {
      const float2 mu = mean[k];
      o = make_float2(mu.x - px[m], mu.y - py[m]);
    }
    offx[m] = o.x;
    offy[m] = o.y;
  }
}

}  // namespace rg

using namespace rg;

static size_t offsets_part(int n_tracks, size_t elem) {
  return (((size_t)n_tracks + 1) * elem + 255) / 256 * 256;
}

extern "C" size_t rg_train_offsets_workspace_size(int n_tracks) {
  if (n_tracks < 0) return 0;
  return 2 * offsets_part(n_tracks, sizeof(int)) + offsets_part(n_tracks, sizeof(float2));
}

extern "C" int rg_train_offsets(const int* track_key, int n_tracks, const float* px,
                                const float* py, int n_meas, float* offset_x, float* offset_y,
                                void* workspace, size_t workspace_bytes, void* stream) {
  RG_REQUIRE(n_tracks >= 0 && n_meas >= 0, RG_ERR_ARG, "rg_train_offsets: n_tracks=%d n_meas=%d",
             n_tracks, n_meas);
  RG_REQUIRE(n_tracks < 0x7fffffff && n_meas <= 0x7f7f7f7f, RG_ERR_ARG,
             "rg_train_offsets: n_tracks=%d or n_meas=%d too large", n_tracks, n_meas);
  if (n_meas == 0) return RG_OK;
  RG_REQUIRE(track_key && px && py && offset_x && offset_y, RG_ERR_ARG,
             "rg_train_offsets: null argument");
  RG_REQUIRE(workspace && workspace_bytes >= rg_train_offsets_workspace_size(n_tracks), RG_ERR_ARG,
             "rg_train_offsets: workspace of %zu bytes, %zu needed", workspace_bytes,
             rg_train_offsets_workspace_size(n_tracks));
  RG_REQUIRE(((uintptr_t)workspace & 7) == 0, RG_ERR_ARG,
             "rg_train_offsets: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t ints = offsets_part(n_tracks, sizeof(int));
  int* first = (int*)workspace;
  int* count = (int*)((char*)workspace + ints);
  float2* mean = (float2*)((char*)workspace + 2 * ints);
  RG_CHECK_HIP(hipMemsetAsync(first, 0x7f, ints, st));  // 0x7f7f7f7f: past every index
  RG_CHECK_HIP(hipMemsetAsync(count, 0, ints, st));
  const int blocks = min(ceil_div(n_meas, FEED_THREADS), FEED_MAX_BLOCKS);
  track_extent_kernel<<<blocks, FEED_THREADS, 0, st>>>(track_key, n_tracks, n_meas, first, count);
  RG_LAUNCH_CHECK();
  if (n_tracks > 0) {
    track_mean_kernel<<<ceil_div(n_tracks, FEED_THREADS / 64), FEED_THREADS, 0, st>>>(
        track_key, px, py, n_tracks, n_meas, first, count, mean);
    RG_LAUNCH_CHECK();
  }
  track_offsets_kernel<<<blocks, FEED_THREADS, 0, st>>>(track_key, px, py, n_tracks, n_meas, mean,
                                                        offset_x, offset_y);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_frontend_flip(float* py, float* vy, const int* win_ptr, int n_windows,
                                const uint8_t* flip, int n_meas, void* stream) {
  RG_REQUIRE(n_meas >= 0 && n_windows >= 0, RG_ERR_ARG,
             "rg_frontend_flip: n_meas=%d n_windows=%d", n_meas, n_windows);
  RG_REQUIRE(win_ptr || n_windows <= 1, RG_ERR_ARG,
             "rg_frontend_flip: %d windows need win_ptr (NULL is one window)", n_windows);
  if (n_meas == 0 || n_windows == 0) return RG_OK;
  RG_REQUIRE(py && vy && flip, RG_ERR_ARG, "rg_frontend_flip: null argument");
  const int blocks = min(ceil_div(n_meas, FEED_THREADS), FEED_MAX_BLOCKS);
  frontend_flip_kernel<<<blocks, FEED_THREADS, 0, (hipStream_t)stream>>>(py, vy, win_ptr,
                                                                         n_windows, flip, n_meas);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_train_labels(const float* class_labels, const float* offset_x,
                               const float* offset_y, int n_nodes, const int* track_key,
                               const int* pair_src, const int* pair_dst, const int* n_pairs,
                               long pair_capacity, int64_t* node_class, float* node_offsets,
                               int64_t* edge_class, void* stream) {
  RG_REQUIRE(n_nodes >= 0 && pair_capacity >= 0, RG_ERR_ARG,
             "rg_train_labels: n_nodes=%d pair_capacity=%ld", n_nodes, pair_capacity);
  RG_REQUIRE((long)n_nodes * 2 <= 0x7fffffffL && pair_capacity <= 0x7fffffffL, RG_ERR_ARG,
             "rg_train_labels: %d nodes x 2 offsets or %ld pairs leave int32", n_nodes,
             pair_capacity);
  RG_REQUIRE(n_nodes == 0 || (class_labels && offset_x && offset_y && node_class && node_offsets),
             RG_ERR_ARG, "rg_train_labels: null node argument");
  RG_REQUIRE(pair_capacity == 0 || (pair_src && pair_dst && n_pairs && edge_class), RG_ERR_ARG,
             "rg_train_labels: null pair argument");
  RG_REQUIRE(pair_capacity == 0 || n_nodes == 0 || track_key, RG_ERR_ARG,
             "rg_train_labels: null track_key");
  RG_REQUIRE(((uintptr_t)node_offsets & 7) == 0, RG_ERR_ARG,
             "rg_train_labels: node_offsets must be 8-byte aligned");
  const long n = n_nodes > pair_capacity ? (long)n_nodes : pair_capacity;
  if (n == 0) return RG_OK;
  const int blocks = min(ceil_div(n, FEED_THREADS), FEED_MAX_BLOCKS);
  train_labels_kernel<<<blocks, FEED_THREADS, 0, (hipStream_t)stream>>>(
      class_labels, offset_x, offset_y, n_nodes, track_key, pair_src, pair_dst, n_pairs,
      (int)pair_capacity, node_class, (float2*)node_offsets, edge_class);
  RG_LAUNCH_CHECK();
  return RG_OK;
}
