// Detection and segmentation evaluation (modules/performance/detection_accuracy.py,
// segmentation_accuracy.py and the two performance_eval_*.ipynb notebooks) for a batch of
// frames, on the device, with no host synchronisation:
//   rg_eval_gt_clusters   : compute_node_idx_for_each_cluster (datagen_gnn.py:15-45) from
//                           per-node track keys: per frame the tracked clusters in ascending
//                           key order, then one singleton per untracked node in node order;
//   rg_argmax_rows        : predicted class = first maximum of a row of logits;
//   rg_eval_cluster_of    : node -> cluster id of a cluster CSR;
//   rg_eval_associate     : compute_gt_and_pred_associations (detection_accuracy.py:192-273)
//                           with the 'inv_iou' criterion.  The dense G x P matrix of 1 - IoU
//                           is 1.0 wherever two clusters share no node, and every node lies
//                           in at most one cluster a side, so a frame has at most N other
//                           entries: they are counted by a sort of the nodes' (gt, pred)
//                           pairs, sorted by (frame, d, gt, pred) and walked greedily by one
//                           wave per frame; the remaining picks pair the unused rows and
//                           columns in ascending order at d = 1.0f;
//   rg_eval_associate_l2  : the same function with the 'l2_norm' criterion: the dense matrix
//                           of centre distances, recomputed from the centres by one workgroup
//                           per frame and never stored (see l2_assoc_kernel);
//   rg_eval_accumulate    : the notebook's confusion / gt_count / pred_count updates;
//   rg_eval_node_confusion: the segmentation notebook's node-level confusion matrix;
//   rg_eval_class_confusion: the same matrix over rows whose prediction is a class id already
//                           (the object-level confusion of the two-stage flow).
// The accumulators are int64: integer adds make them independent of the arrival order.  Each
// block sums in LDS first and then issues one global atomic per non-zero bin.
#include "rg_common.h"
#include "scan.h"

#include <hipcub/hipcub.hpp>

// d = float32(1.0 - double(inter) / double(union)): one f64 division, one f64 subtraction,
// one rounding to f32 -- never contracted or reassociated
#pragma clang fp contract(off)

namespace rg {
namespace eval {

typedef unsigned long long u64;

static constexpr int MAXC = 32;  // classes (the detector has 7)
static constexpr int WAVE = 64;

// the frame of a node: the f in [0, nf) with fp[f] <= node < fp[f + 1] (empty frames skipped)
__device__ __forceinline__ int frame_of(const int* __restrict__ fp, int nf, int node) {
  int lo = 0, hi = nf;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (fp[mid + 1] > node) hi = mid;
    else lo = mid + 1;
  }
  return lo < nf ? lo : nf - 1;
}

__host__ __device__ inline int bits_for(long v) {  // bits needed to hold values 0..v
  int b = 1;
  while (b < 62 && (1L << b) <= v) ++b;
  return b;
}

// ------------------------------------------------------------------ ground-truth clusters

// sort key of a node: (frame, untracked, track key | node index)
__global__ void gt_keys_kernel(const int* __restrict__ track_key, const int* __restrict__ fp,
                               int nf, int n, u64* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 f = (u64)frame_of(fp, nf, i);
  const int k = track_key[i];
  keys[i] = (f << 33) | (k == 0 ? ((u64)1 << 32) | (u64)(unsigned)i : (u64)(unsigned)k);
  vals[i] = i;
}

__global__ void key_heads_kernel(const u64* __restrict__ keys, int n, u64 sentinel,
                                 int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 k = keys[i];
  flag[i] = (k != sentinel && (i == 0 || k != keys[i - 1])) ? 1 : 0;
}

// rank: exclusive scan of the head flags over the sorted nodes (rank[n] = clusters)
__global__ void gt_emit_kernel(const int* __restrict__ flag, const int* __restrict__ rank,
                               const int* __restrict__ sorted_node,
                               const int64_t* __restrict__ node_class, const int* __restrict__ fp,
                               int nf, int n, int* __restrict__ cluster_of,
                               int* __restrict__ cluster_ptr, int* __restrict__ cluster_idx,
                               int* __restrict__ frame_clusters,
                               int64_t* __restrict__ cluster_class) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nf) frame_clusters[i] = rank[fp[i + 1]] - rank[fp[i]];
  if (i > n) return;
  const int total = rank[n];
  if (i >= total) cluster_ptr[i] = n;  // entries past the last cluster repeat N
  if (i == n) return;
  const int node = sorted_node[i];
  const int c = rank[i] + flag[i] - 1;
  cluster_of[node] = c;
  cluster_idx[i] = node;
  if (flag[i]) {
    cluster_ptr[c] = i;
    cluster_class[c] = node_class[node];  // the stable sort keeps members ascending
  }
}

// ------------------------------------------------------------------ small helpers

__global__ void argmax_rows_kernel(const float* __restrict__ x, int ld, long n, int nc,
                                   int64_t* __restrict__ out) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float* row = x + (size_t)r * ld;
  float m = row[0];
  int am = 0;
  for (int k = 1; k < nc; ++k)
    if (row[k] > m) {
      m = row[k];
      am = k;
    }
  out[r] = am;
}

// position j of the member list belongs to the last cluster c with ptr[c] <= j
__global__ void cluster_of_kernel(const int* __restrict__ ptr, const int* __restrict__ idx,
                                  int ncl, int n, int* __restrict__ of) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || j >= ptr[ncl]) return;
  int lo = 0, hi = ncl;  // first c with ptr[c + 1] > j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid + 1] > j) hi = mid;
    else lo = mid + 1;
  }
  const int node = idx[j];
  if (lo < ncl && node >= 0 && node < n) of[node] = lo;
}

// ------------------------------------------------------------------ association

// per cluster: kept (size > threshold) and its frame (-1 for an empty slot of the CSR)
__global__ void cluster_info_kernel(const int* __restrict__ ptr, const int* __restrict__ idx,
                                    const int* __restrict__ fp, int nf, int n, int thr,
                                    int* __restrict__ kept, int* __restrict__ cframe) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int a = ptr[c], sz = ptr[c + 1] - a;
  kept[c] = sz > thr ? 1 : 0;
  cframe[c] = sz > 0 ? frame_of(fp, nf, idx[a]) : -1;
}

// krank: exclusive scan of kept.  Per frame the range of kept ranks [fbase, fend), and the
// kept clusters' ids in order (klist).  Clusters are ordered by frame, empty slots last.
__global__ void cluster_frames_kernel(const int* __restrict__ kept, const int* __restrict__ cframe,
                                      const int* __restrict__ krank, int n,
                                      int* __restrict__ fbase, int* __restrict__ fend,
                                      int* __restrict__ klist) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int f = cframe[c];
  if (f < 0) return;
  if (c == 0 || cframe[c - 1] != f) fbase[f] = krank[c];
  if (c == n - 1 || cframe[c + 1] != f) fend[f] = krank[c + 1];
  if (kept[c]) klist[krank[c]] = c;
}

// a node's (gt cluster, pred cluster) pair when both are kept; the sentinel sorts last
__global__ void node_pairs_kernel(const int* __restrict__ gt_of, const int* __restrict__ pred_of,
                                  const int* __restrict__ kept_g, const int* __restrict__ kept_p,
                                  int n, u64 sentinel, u64* __restrict__ keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = gt_of[i], p = pred_of[i];
  const bool ok = g >= 0 && g < n && p >= 0 && p < n && kept_g[g] && kept_p[p];
  keys[i] = ok ? ((u64)g << 32) | (u64)p : sentinel;
}

// start of every run of equal pairs (entry_pos[e]) and the end of the last one
__global__ void entry_pos_kernel(const u64* __restrict__ keys, const int* __restrict__ flag,
                                 const int* __restrict__ rank, int n, u64 sentinel,
                                 int* __restrict__ entry_pos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (keys[i] == sentinel) return;
  if (flag[i]) entry_pos[rank[i]] = i;
  if (i == n - 1 || keys[i + 1] == sentinel) entry_pos[rank[i + 1]] = i + 1;
}

// one entry per overlapping pair: inter = run length, d = float32(1 - inter / union)
__global__ void entries_kernel(const u64* __restrict__ keys, const int* __restrict__ entry_pos,
                               const int* __restrict__ rank, const int* __restrict__ gptr,
                               const int* __restrict__ pptr, const int* __restrict__ cframe_g,
                               int n, int nf, int* __restrict__ ent_g, int* __restrict__ ent_p,
                               float* __restrict__ ent_d, u64* __restrict__ keys2,
                               int* __restrict__ vals2) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  vals2[e] = e;
  if (e >= rank[n]) {
    keys2[e] = (u64)nf << 32;
    return;
  }
  const int a = entry_pos[e];
  const u64 key = keys[a];
  const int g = (int)(key >> 32), p = (int)(key & 0xffffffffu);
  const int inter = entry_pos[e + 1] - a;
  const int uni = (gptr[g + 1] - gptr[g]) + (pptr[p + 1] - pptr[p]) - inter;
  const float d = (float)(1.0 - (double)inter / (double)uni);
  ent_g[e] = g;
  ent_p[e] = p;
  ent_d[e] = d;
  // d >= 0: the bit pattern of a non-negative float orders as the float does
  keys2[e] = ((u64)cframe_g[g] << 32) | (u64)__float_as_uint(d);
}

// the range of sorted entries of every frame
__global__ void entry_ranges_kernel(const u64* __restrict__ keys2, int n, int nf,
                                    int* __restrict__ est, int* __restrict__ eend) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int f = (int)(keys2[s] >> 32);
  if (f >= nf) return;
  if (s == 0 || (int)(keys2[s - 1] >> 32) != f) est[f] = s;
  if (s == n - 1 || (int)(keys2[s + 1] >> 32) != f) eend[f] = s + 1;
}

// flags one wave writes and reads again: device-scope accesses
__device__ __forceinline__ int ld_dev(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_dev(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Picks {
  int* start;      // [F] first slot of the frame's picks
  int* count;      // [F]
  int* gt;         // [N] frame-local kept index
  int* pred;       // [N]
  float* d;        // [N]
  int* pos;        // [N] d <= eps
  int* gt_cluster;    // [N] cluster id in the CSR, -1 = unused slot
  int* pred_cluster;  // [N]
};

// One wave per frame walks the frame's entries in sorted order, 64 at a time: an entry whose
// row or column is used drops out; the rest are resolved in lane order in registers (the
// first live lane is a pick and kills the later lanes of its row and column).  Then the
// fill-in: the i-th unused row with the i-th unused column at d = 1.
__global__ __launch_bounds__(WAVE) void walk_kernel(
    const int* __restrict__ est, const int* __restrict__ eend, const int* __restrict__ order,
    const int* __restrict__ ent_g, const int* __restrict__ ent_p, const float* __restrict__ ent_d,
    const int* __restrict__ krank_g, const int* __restrict__ krank_p,
    const int* __restrict__ fbase_g, const int* __restrict__ fend_g,
    const int* __restrict__ fbase_p, const int* __restrict__ fend_p,
    const int* __restrict__ klist_g, const int* __restrict__ klist_p, int* used_g, int* used_p,
    int* unr, int* unc, float eps, Picks pk) {
  const int f = blockIdx.x;
  const int lane = threadIdx.x;
  const u64 lt = ((u64)1 << lane) - 1;
  const int bg = fbase_g[f], bp = fbase_p[f];
  const int G = fend_g[f] - bg, P = fend_p[f] - bp;
  const int m = G < P ? G : P;
  if (lane == 0) pk.start[f] = bg;
  if (m <= 0) {
    if (lane == 0) pk.count[f] = 0;
    return;
  }
  int np = 0;
  const int s1 = eend[f];
  for (int s0 = est[f]; s0 < s1 && np < m; s0 += WAVE) {
    const int s = s0 + lane;
    int g = -1, p = -1;
    float d = 0.f;
    bool live = false;
    if (s < s1) {
      const int e = order[s];
      g = ent_g[e];
      p = ent_p[e];
      d = ent_d[e];
      live = !ld_dev(used_g + g) && !ld_dev(used_p + p);
    }
    u64 todo = __ballot(live);
    u64 taken = 0;
    while (todo) {
      const int k = __ffsll(todo) - 1;
      taken |= (u64)1 << k;
      const int gk = __shfl(g, k), pkk = __shfl(p, k);
      if (g == gk || p == pkk) live = false;
      todo = __ballot(live) & ~(((u64)2 << k) - 1);
    }
    if ((taken >> lane) & 1) {
      const int slot = bg + np + __popcll(taken & lt);
      pk.gt[slot] = krank_g[g] - bg;
      pk.pred[slot] = krank_p[p] - bp;
      pk.d[slot] = d;
      pk.pos[slot] = d <= eps ? 1 : 0;
      pk.gt_cluster[slot] = g;
      pk.pred_cluster[slot] = p;
      st_dev(used_g + g, 1);
      st_dev(used_p + p, 1);
    }
    np += __popcll(taken);
    __threadfence();  // the next 64 entries read the flags just written
  }
  const int rest = m - np;
  if (rest > 0) {
    int cnt = 0;
    for (int j0 = 0; j0 < G && cnt < rest; j0 += WAVE) {
      const int j = j0 + lane;
      const bool un = j < G && !ld_dev(used_g + klist_g[bg + j]);
      const u64 mask = __ballot(un);
      if (un) st_dev(unr + bg + cnt + __popcll(mask & lt), j);
      cnt += __popcll(mask);
    }
    cnt = 0;
    for (int j0 = 0; j0 < P && cnt < rest; j0 += WAVE) {
      const int j = j0 + lane;
      const bool un = j < P && !ld_dev(used_p + klist_p[bp + j]);
      const u64 mask = __ballot(un);
      if (un) st_dev(unc + bp + cnt + __popcll(mask & lt), j);
      cnt += __popcll(mask);
    }
    __threadfence();
    const int pos1 = 1.0f <= eps ? 1 : 0;
    for (int i = lane; i < rest; i += WAVE) {
      const int gl = ld_dev(unr + bg + i), pl = ld_dev(unc + bp + i);
      const int slot = bg + np + i;
      pk.gt[slot] = gl;
      pk.pred[slot] = pl;
      pk.d[slot] = 1.0f;
      pk.pos[slot] = pos1;
      pk.gt_cluster[slot] = klist_g[bg + gl];
      pk.pred_cluster[slot] = klist_p[bp + pl];
    }
  }
  if (lane == 0) pk.count[f] = m;
}

// ------------------------------------------------------------------ l2_norm association

// The 'l2_norm' criterion: dist[g][p] = float32 Euclidean distance between the centres of the
// frame's kept clusters, a dense G x P matrix that is never stored.  One workgroup per frame;
// every row caches the minimum of its unused columns (d, column; lowest column on ties), a
// round takes the workgroup-wide minimum of (d, row) over the unused rows, and only the rows
// whose cached column was just taken are rescanned (one wave per row, 64 columns a step).
// G P distances up front, P per rescanned row: O(min(G, P) G P) when every row keeps wanting
// the same column (co-located centres).  Every loop is bounded by G, P and min(G, P).
static constexpr int L2_THREADS = 512;
static constexpr int L2_WAVES = L2_THREADS / WAVE;
// kept clusters a side of a frame whose state is held in LDS; a larger frame keeps the same
// state in the workspace
static constexpr int L2_LDS_CAP = 4096;
static constexpr int L2_SLOT_BYTES = 2 * 8 + 3 * 4 + 2;  // per cluster of the larger side

struct L2State {
  float2* cen_g;         // [G] centres of the kept ground-truth clusters (rows)
  float2* cen_p;         // [P] centres of the kept predicted clusters (columns)
  float* best_d;         // [G] minimum of the row over the unused columns
  int* best_c;           // [G] its column
  int* inv;              // [G] rows to rescan
  unsigned char* rused;  // [G]
  unsigned char* cused;  // [P]
};

__device__ __forceinline__ u64 wave_min_u64(u64 k) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(k, o);
    k = t < k ? t : k;
  }
  return k;
}

__device__ __forceinline__ bool finite_f32(float v) {
  return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}

// the picks of one frame (G, P >= 1); wkey [L2_WAVES] and n_inv are LDS
__device__ __forceinline__ void l2_frame(const L2State s, int f, int G, int P, int bg, int bp,
                                         const int* __restrict__ klist_g,
                                         const int* __restrict__ klist_p,
                                         const float* __restrict__ gt_mu,
                                         const float* __restrict__ pred_mu, float eps, Picks pk,
                                         int* bad_value, u64* wkey, int* n_inv) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int m = G < P ? G : P;
  int bad = 0;
  for (int r = tid; r < G; r += L2_THREADS) {
    const int c = klist_g[bg + r];
    const float2 v = make_float2(gt_mu[2 * (size_t)c], gt_mu[2 * (size_t)c + 1]);
    bad |= !(finite_f32(v.x) && finite_f32(v.y));
    s.cen_g[r] = v;
    s.rused[r] = 0;
    s.inv[r] = r;
  }
  for (int c = tid; c < P; c += L2_THREADS) {
    const int k = klist_p[bp + c];
    const float2 v = make_float2(pred_mu[2 * (size_t)k], pred_mu[2 * (size_t)k + 1]);
    bad |= !(finite_f32(v.x) && finite_f32(v.y));
    s.cen_p[c] = v;
    s.cused[c] = 0;
  }
  if (tid == 0) *n_inv = G;
  if (__syncthreads_or(bad)) {  // the reference raises (np.min of NaN): no picks, flag set
    if (tid == 0) {
      pk.count[f] = 0;
      atomicExch(bad_value, 1);
    }
    return;
  }
  for (int round = 0; round < m; ++round) {
    // 1. rescan: a wave per row over the unused columns.  sq orders as d does except where
    // two sq round to one d, so the square root is taken only where sq improves
    const int ninv = *n_inv;
    for (int i = wave; i < ninv; i += L2_WAVES) {
      const int r = s.inv[i];
      const float2 g = s.cen_g[r];
      float bs = 0.f, bd = 0.f;
      int bc = -1;
      for (int c = lane; c < P; c += WAVE) {
        if (s.cused[c]) continue;
        const float2 q = s.cen_p[c];
        const float dx = g.x - q.x, dy = g.y - q.y;
        const float sq = dx * dx + dy * dy;
        if (bc < 0 || sq < bs) {
          const float d = sqrt_rn(sq);
          if (bc < 0 || d < bd) {
            bd = d;
            bc = c;
          }
          bs = sq;
        }
      }
      // round < min(G, P): a column is unused, so some lane has one
      u64 key = bc >= 0 ? ((u64)__float_as_uint(bd) << 32) | (u64)(unsigned)bc : ~(u64)0;
      key = wave_min_u64(key);
      if (lane == 0) {
        s.best_d[r] = __uint_as_float((unsigned)(key >> 32));
        s.best_c[r] = (int)(unsigned)(key & 0xffffffffu);
      }
    }
    __syncthreads();
    // 2. the minimum (d, row) of the unused rows; d >= 0 orders as its bits
    u64 key = ~(u64)0;
    for (int r = tid; r < G; r += L2_THREADS)
      if (!s.rused[r]) {
        const u64 k = ((u64)__float_as_uint(s.best_d[r]) << 32) | (u64)(unsigned)r;
        key = k < key ? k : key;
      }
    key = wave_min_u64(key);
    if (lane == 0) wkey[wave] = key;
    if (tid == 0) *n_inv = 0;
    __syncthreads();
    key = wkey[0];
#pragma unroll
    for (int w = 1; w < L2_WAVES; ++w) key = wkey[w] < key ? wkey[w] : key;
    const int r1 = (int)(unsigned)(key & 0xffffffffu);
    const int c1 = s.best_c[r1];
    // 3. the pick, and the rows that wanted its column
    if (tid == 0) {
      const float d = __uint_as_float((unsigned)(key >> 32));
      const int slot = bg + round;
      pk.gt[slot] = r1;
      pk.pred[slot] = c1;
      pk.d[slot] = d;
      pk.pos[slot] = d <= eps ? 1 : 0;
      pk.gt_cluster[slot] = klist_g[bg + r1];
      pk.pred_cluster[slot] = klist_p[bp + c1];
      s.rused[r1] = 1;
      s.cused[c1] = 1;
    }
    for (int r = tid; r < G; r += L2_THREADS)
      if (r != r1 && !s.rused[r] && s.best_c[r] == c1) s.inv[atomicAdd(n_inv, 1)] = r;
    __syncthreads();
  }
  if (tid == 0) pk.count[f] = m;
}

__global__ __launch_bounds__(L2_THREADS) void l2_assoc_kernel(
    const int* __restrict__ fbase_g, const int* __restrict__ fend_g,
    const int* __restrict__ fbase_p, const int* __restrict__ fend_p,
    const int* __restrict__ klist_g, const int* __restrict__ klist_p,
    const float* __restrict__ gt_mu, const float* __restrict__ pred_mu, int lds_cap, L2State gws,
    float eps, Picks pk, int* bad_value) {
  extern __shared__ __attribute__((aligned(16))) char l2_lds[];
  __shared__ u64 wkey[L2_WAVES];
  __shared__ int n_inv;
  const int f = blockIdx.x;
  const int bg = fbase_g[f], bp = fbase_p[f];
  const int G = fend_g[f] - bg, P = fend_p[f] - bp;
  if (threadIdx.x == 0) pk.start[f] = bg;
  if (G <= 0 || P <= 0) {
    if (threadIdx.x == 0) pk.count[f] = 0;
    return;
  }
  if (G <= lds_cap && P <= lds_cap) {
    L2State s;
    s.cen_g = (float2*)l2_lds;
    s.cen_p = s.cen_g + lds_cap;
    s.best_d = (float*)(s.cen_p + lds_cap);
    s.best_c = (int*)(s.best_d + lds_cap);
    s.inv = s.best_c + lds_cap;
    s.rused = (unsigned char*)(s.inv + lds_cap);
    s.cused = s.rused + lds_cap;
    l2_frame(s, f, G, P, bg, bp, klist_g, klist_p, gt_mu, pred_mu, eps, pk, bad_value, wkey,
             &n_inv);
  } else {
    L2State s;
    s.cen_g = gws.cen_g + bg;
    s.cen_p = gws.cen_p + bp;
    s.best_d = gws.best_d + bg;
    s.best_c = gws.best_c + bg;
    s.inv = gws.inv + bg;
    s.rused = gws.rused + bg;
    s.cused = gws.cused + bp;
    l2_frame(s, f, G, P, bg, bp, klist_g, klist_p, gt_mu, pred_mu, eps, pk, bad_value, wkey,
             &n_inv);
  }
}

// ------------------------------------------------------------------ accumulation

// LDS bins of one block -> one global atomic per non-zero bin
__device__ __forceinline__ void flush_bins(const int* bins, int nbins, int64_t* const* dst,
                                           const int* first, int ndst) {
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
    const int v = bins[b];
    if (!v) continue;
    int t = 0;
    while (t + 1 < ndst && b >= first[t + 1]) ++t;
    atomicAdd((u64*)(dst[t] + (b - first[t])), (u64)v);
  }
}

__global__ __launch_bounds__(256) void accumulate_kernel(
    const int* __restrict__ pick_g, const int* __restrict__ pick_p, const int* __restrict__ pick_pos,
    const int* __restrict__ kept_g, const int* __restrict__ kept_p,
    const int64_t* __restrict__ class_g, const int64_t* __restrict__ class_p, int n, int nc,
    int false_class, int64_t* confusion, int64_t* gt_count, int64_t* pred_count,
    int* __restrict__ bad) {
  __shared__ int bins[MAXC * MAXC + 2 * MAXC];
  const int nbins = nc * nc + 2 * nc;
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) bins[b] = 0;
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int64_t cg = kept_g[i] ? class_g[i] : -1, cp = kept_p[i] ? class_p[i] : -1;
    if (kept_g[i]) {
      if (cg < 0 || cg >= nc) atomicExch(bad, 1);
      else atomicAdd(bins + nc * nc + (int)cg, 1);
    }
    if (kept_p[i]) {
      if (cp < 0 || cp >= nc) atomicExch(bad, 1);
      else atomicAdd(bins + nc * nc + nc + (int)cp, 1);
    }
    const int g = pick_g[i];
    if (g >= 0) {
      const int64_t a = pick_pos[i] ? class_g[g] : (int64_t)false_class;
      const int64_t b = class_p[pick_p[i]];
      if (a < 0 || a >= nc || b < 0 || b >= nc) atomicExch(bad, 1);
      else atomicAdd(bins + (int)a * nc + (int)b, 1);
    }
  }
  __syncthreads();
  int64_t* dst[3] = {confusion, gt_count, pred_count};
  const int first[3] = {0, nc * nc, nc * nc + nc};
  flush_bins(bins, nbins, dst, first, 3);
}

__global__ __launch_bounds__(256) void node_confusion_kernel(
    const float* __restrict__ logits, int ld, const int64_t* __restrict__ gt, long n, int nc,
    int64_t* confusion, int64_t* gt_count, int* __restrict__ bad) {
  __shared__ int bins[MAXC * MAXC + MAXC];
  const int nbins = nc * nc + nc;
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) bins[b] = 0;
  __syncthreads();
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (long)gridDim.x * blockDim.x) {
    const float* row = logits + (size_t)r * ld;
    float mx = row[0];
    int am = 0;
    for (int k = 1; k < nc; ++k)
      if (row[k] > mx) {
        mx = row[k];
        am = k;
      }
    const int64_t c = gt[r];
    if (c < 0 || c >= nc) {
      atomicExch(bad, 1);
      continue;
    }
    atomicAdd(bins + (int)c * nc + am, 1);
    atomicAdd(bins + nc * nc + (int)c, 1);
  }
  __syncthreads();
  int64_t* dst[2] = {confusion, gt_count};
  const int first[2] = {0, nc * nc};
  flush_bins(bins, nbins, dst, first, 2);
}

// the same counts for predictions that are class ids already
__global__ __launch_bounds__(256) void class_confusion_kernel(
    const int64_t* __restrict__ gt, const int64_t* __restrict__ pred, long n, int nc,
    int64_t* confusion, int64_t* gt_count, int* __restrict__ bad) {
  __shared__ int bins[MAXC * MAXC + MAXC];
  const int nbins = nc * nc + nc;
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) bins[b] = 0;
  __syncthreads();
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (long)gridDim.x * blockDim.x) {
    const int64_t c = gt[r], p = pred[r];
    if (c < 0 || c >= nc || p < 0 || p >= nc) {
      atomicExch(bad, 1);
      continue;
    }
    atomicAdd(bins + (int)c * nc + (int)p, 1);
    atomicAdd(bins + nc * nc + (int)c, 1);
  }
  __syncthreads();
  int64_t* dst[2] = {confusion, gt_count};
  const int first[2] = {0, nc * nc};
  flush_bins(bins, nbins, dst, first, 2);
}

// ------------------------------------------------------------------ workspaces

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

static size_t sort_pairs_bytes(int n) {
  size_t bytes = 0;
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(
      nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (const int*)nullptr, (int*)nullptr, n, 0,
      64);
  return e == hipSuccess ? bytes : (size_t)n * 32 + (1 << 20);
}

static size_t sort_keys_bytes(int n) {
  size_t bytes = 0;
  const hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, (const u64*)nullptr,
                                                         (u64*)nullptr, n, 0, 64);
  return e == hipSuccess ? bytes : (size_t)n * 32 + (1 << 20);
}

struct Taker {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    char* p = base ? base + off : nullptr;
    off += align_up(count * sizeof(T));
    return (T*)p;
  }
};

struct GtWs {
  u64 *keys, *keys_s;
  int *vals, *vals_s, *flag, *rank;
  void *scan_ws, *sort_ws;
  size_t sort_bytes;
};

static size_t gt_ws_layout(int n, GtWs* w, char* base) {
  Taker t{base};
  GtWs x;
  x.keys = t.take<u64>(n);
  x.keys_s = t.take<u64>(n);
  x.vals = t.take<int>(n);
  x.vals_s = t.take<int>(n);
  x.flag = t.take<int>(n);
  x.rank = t.take<int>((size_t)n + 1);
  x.scan_ws = t.take<char>(scan_workspace_bytes((long)n + 1));
  x.sort_bytes = sort_pairs_bytes(n);
  x.sort_ws = t.take<char>(x.sort_bytes);
  if (w) *w = x;
  return t.off;
}

struct AssocWs {
  int *cframe_g, *cframe_p, *krank_g, *krank_p, *klist_g, *klist_p;
  int* fr;    // [6 F]: fbase_g, fend_g, fbase_p, fend_p, est, eend (zeroed)
  int* used;  // [2 N]: used_g, used_p (zeroed)
  u64 *keys1, *keys1_s, *keys2, *keys2_s;
  int *flag, *rank, *entry_pos, *ent_g, *ent_p, *vals2, *vals2_s, *unr, *unc;
  float* ent_d;
  void *scan_ws, *sort_ws;
  size_t sort_bytes;
};

static size_t assoc_ws_layout(int n, int nf, AssocWs* w, char* base) {
  Taker t{base};
  AssocWs x;
  x.cframe_g = t.take<int>(n);
  x.cframe_p = t.take<int>(n);
  x.krank_g = t.take<int>((size_t)n + 1);
  x.krank_p = t.take<int>((size_t)n + 1);
  x.klist_g = t.take<int>(n);
  x.klist_p = t.take<int>(n);
  x.fr = t.take<int>((size_t)6 * nf);
  x.used = t.take<int>((size_t)2 * n);
  x.keys1 = t.take<u64>(n);
  x.keys1_s = t.take<u64>(n);
  x.keys2 = t.take<u64>(n);
  x.keys2_s = t.take<u64>(n);
  x.flag = t.take<int>(n);
  x.rank = t.take<int>((size_t)n + 1);
  x.entry_pos = t.take<int>((size_t)n + 1);
  x.ent_g = t.take<int>(n);
  x.ent_p = t.take<int>(n);
  x.vals2 = t.take<int>(n);
  x.vals2_s = t.take<int>(n);
  x.unr = t.take<int>(n);
  x.unc = t.take<int>(n);
  x.ent_d = t.take<float>(n);
  x.scan_ws = t.take<char>(scan_workspace_bytes((long)n + 1));
  const size_t a = sort_pairs_bytes(n), b = sort_keys_bytes(n);
  x.sort_bytes = a > b ? a : b;
  x.sort_ws = t.take<char>(x.sort_bytes);
  if (w) *w = x;
  return t.off;
}

struct L2Ws {
  int *cframe_g, *cframe_p, *krank_g, *krank_p, *klist_g, *klist_p;
  int* fr;     // [4 F]: fbase_g, fend_g, fbase_p, fend_p (zeroed)
  L2State st;  // [N] each: the state of the frames past L2_LDS_CAP
  void* scan_ws;
};

static size_t l2_ws_layout(int n, int nf, L2Ws* w, char* base) {
  Taker t{base};
  L2Ws x;
  x.cframe_g = t.take<int>(n);
  x.cframe_p = t.take<int>(n);
  x.krank_g = t.take<int>((size_t)n + 1);
  x.krank_p = t.take<int>((size_t)n + 1);
  x.klist_g = t.take<int>(n);
  x.klist_p = t.take<int>(n);
  x.fr = t.take<int>((size_t)4 * nf);
  x.st.cen_g = t.take<float2>(n);
  x.st.cen_p = t.take<float2>(n);
  x.st.best_d = t.take<float>(n);
  x.st.best_c = t.take<int>(n);
  x.st.inv = t.take<int>(n);
  x.st.rused = t.take<unsigned char>(n);
  x.st.cused = t.take<unsigned char>(n);
  x.scan_ws = t.take<char>(scan_workspace_bytes((long)n + 1));
  if (w) *w = x;
  return t.off;
}

}  // namespace eval
}  // namespace rg

using namespace rg;
using namespace rg::eval;

static constexpr int EVAL_MAX_NODES = 1 << 30;  // int32 CSR offsets and sort sizes

extern "C" size_t rg_eval_gt_clusters_workspace_size(int n_nodes) {
  if (n_nodes <= 0 || n_nodes > EVAL_MAX_NODES) return 0;
  return gt_ws_layout(n_nodes, nullptr, nullptr);
}

extern "C" int rg_eval_gt_clusters(const int* track_key, const int64_t* node_class,
                                   const int* frame_ptr, int n_nodes, int n_frames,
                                   int* cluster_of, int* cluster_ptr, int* cluster_idx,
                                   int* frame_clusters, int64_t* cluster_class, int* n_clusters,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  RG_REQUIRE(n_nodes >= 0 && n_frames >= 0, RG_ERR_ARG, "rg_eval_gt_clusters: n_nodes=%d n_frames=%d",
             n_nodes, n_frames);
  RG_REQUIRE(n_nodes <= EVAL_MAX_NODES, RG_ERR_UNSUPPORTED, "rg_eval_gt_clusters: n_nodes=%d > %d",
             n_nodes, EVAL_MAX_NODES);
  RG_REQUIRE(n_nodes == 0 || n_frames >= 1, RG_ERR_ARG, "rg_eval_gt_clusters: nodes without a frame");
  if (n_nodes == 0) {
    RG_CHECK_HIP(hipMemsetAsync(n_clusters, 0, sizeof(int), st));
    RG_CHECK_HIP(hipMemsetAsync(cluster_ptr, 0, sizeof(int), st));
    if (n_frames > 0)
      RG_CHECK_HIP(hipMemsetAsync(frame_clusters, 0, (size_t)n_frames * sizeof(int), st));
    return RG_OK;
  }
  GtWs ws;
  const size_t need = gt_ws_layout(n_nodes, &ws, (char*)workspace);
  RG_REQUIRE(workspace && workspace_bytes >= need, RG_ERR_ARG,
             "rg_eval_gt_clusters: workspace %zu < %zu", workspace_bytes, need);
  const int nb = ceil_div(n_nodes, 256);
  gt_keys_kernel<<<nb, 256, 0, st>>>(track_key, frame_ptr, n_frames, n_nodes, ws.keys, ws.vals);
  RG_LAUNCH_CHECK();
  size_t sb = ws.sort_bytes;
  int end_bit = 33 + bits_for(n_frames);
  if (end_bit > 64) end_bit = 64;
  RG_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws.sort_ws, sb, ws.keys, ws.keys_s, ws.vals,
                                                  ws.vals_s, n_nodes, 0, end_bit, st));
  key_heads_kernel<<<nb, 256, 0, st>>>(ws.keys_s, n_nodes, ~(u64)0, ws.flag);
  RG_LAUNCH_CHECK();
  const int rc = exclusive_scan(ws.flag, n_nodes, ws.rank, n_clusters, ws.scan_ws, st);
  if (rc) return rc;
  const int work = (n_nodes + 1 > n_frames ? n_nodes + 1 : n_frames);
  gt_emit_kernel<<<ceil_div(work, 256), 256, 0, st>>>(ws.flag, ws.rank, ws.vals_s, node_class,
                                                      frame_ptr, n_frames, n_nodes, cluster_of,
                                                      cluster_ptr, cluster_idx, frame_clusters,
                                                      cluster_class);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_argmax_rows(const float* x, int ld, long n_rows, int n_cols, int64_t* out,
                              void* stream) {
  RG_REQUIRE(n_rows >= 0 && n_cols >= 1 && ld >= n_cols, RG_ERR_ARG,
             "rg_argmax_rows: n_rows=%ld n_cols=%d ld=%d", n_rows, n_cols, ld);
  if (n_rows == 0) return RG_OK;
  argmax_rows_kernel<<<ceil_div(n_rows, 256), 256, 0, (hipStream_t)stream>>>(x, ld, n_rows, n_cols,
                                                                           out);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_eval_cluster_of(const int* cluster_ptr, const int* cluster_idx, int n_clusters,
                                  int n_nodes, int* cluster_of, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  RG_REQUIRE(n_nodes >= 0 && n_clusters >= 0, RG_ERR_ARG,
             "rg_eval_cluster_of: n_nodes=%d n_clusters=%d", n_nodes, n_clusters);
  if (n_nodes == 0) return RG_OK;
  RG_CHECK_HIP(hipMemsetAsync(cluster_of, 0xff, (size_t)n_nodes * sizeof(int), st));
  if (n_clusters == 0) return RG_OK;
  cluster_of_kernel<<<ceil_div(n_nodes, 256), 256, 0, st>>>(cluster_ptr, cluster_idx, n_clusters,
                                                            n_nodes, cluster_of);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" size_t rg_eval_associate_workspace_size(int n_nodes, int n_frames) {
  if (n_nodes <= 0 || n_frames <= 0 || n_nodes > EVAL_MAX_NODES) return 0;
  return assoc_ws_layout(n_nodes, n_frames, nullptr, nullptr);
}

extern "C" int rg_eval_associate(const int* frame_ptr, int n_nodes, int n_frames,
                                 int max_frame_nodes, const int* gt_of, const int* gt_ptr,
                                 const int* gt_idx, const int* pred_of, const int* pred_ptr,
                                 const int* pred_idx, int size_threshold, float eps,
                                 int* gt_kept, int* pred_kept, int* pick_start, int* pick_count,
                                 int* pick_gt, int* pick_pred, float* pick_d, int* pick_positive,
                                 int* pick_gt_cluster, int* pick_pred_cluster, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  RG_REQUIRE(n_nodes >= 0 && n_frames >= 0 && max_frame_nodes >= 0 && size_threshold >= 0,
             RG_ERR_ARG, "rg_eval_associate: n_nodes=%d n_frames=%d max_frame_nodes=%d threshold=%d",
             n_nodes, n_frames, max_frame_nodes, size_threshold);
  // beyond 2^24 nodes a frame, 1 - 1 / union rounds to 1.0f and an overlapping pair would
  // tie with the pairs that share nothing
  RG_REQUIRE(max_frame_nodes < (1 << 24) && n_nodes <= EVAL_MAX_NODES, RG_ERR_UNSUPPORTED,
             "rg_eval_associate: max_frame_nodes=%d (limit 2^24 - 1), n_nodes=%d", max_frame_nodes,
             n_nodes);
  RG_REQUIRE(n_nodes == 0 || n_frames >= 1, RG_ERR_ARG, "rg_eval_associate: nodes without a frame");
  if (n_frames == 0) return RG_OK;
  if (n_nodes == 0) {
    RG_CHECK_HIP(hipMemsetAsync(pick_start, 0, (size_t)n_frames * sizeof(int), st));
    RG_CHECK_HIP(hipMemsetAsync(pick_count, 0, (size_t)n_frames * sizeof(int), st));
    return RG_OK;
  }
  AssocWs ws;
  const size_t need = assoc_ws_layout(n_nodes, n_frames, &ws, (char*)workspace);
  RG_REQUIRE(workspace && workspace_bytes >= need, RG_ERR_ARG,
             "rg_eval_associate: workspace %zu < %zu", workspace_bytes, need);
  const int n = n_nodes, nf = n_frames, nb = ceil_div(n, 256);
  int *fbase_g = ws.fr, *fend_g = ws.fr + nf, *fbase_p = ws.fr + 2 * (size_t)nf,
      *fend_p = ws.fr + 3 * (size_t)nf, *est = ws.fr + 4 * (size_t)nf,
      *eend = ws.fr + 5 * (size_t)nf;
  int *used_g = ws.used, *used_p = ws.used + n;
  RG_CHECK_HIP(hipMemsetAsync(ws.fr, 0, (size_t)6 * nf * sizeof(int), st));
  RG_CHECK_HIP(hipMemsetAsync(ws.used, 0, (size_t)2 * n * sizeof(int), st));
  RG_CHECK_HIP(hipMemsetAsync(pick_gt_cluster, 0xff, (size_t)n * sizeof(int), st));
  RG_CHECK_HIP(hipMemsetAsync(pick_pred_cluster, 0xff, (size_t)n * sizeof(int), st));

  cluster_info_kernel<<<nb, 256, 0, st>>>(gt_ptr, gt_idx, frame_ptr, nf, n, size_threshold,
                                          gt_kept, ws.cframe_g);
  cluster_info_kernel<<<nb, 256, 0, st>>>(pred_ptr, pred_idx, frame_ptr, nf, n, size_threshold,
                                          pred_kept, ws.cframe_p);
  RG_LAUNCH_CHECK();
  int rc = exclusive_scan(gt_kept, n, ws.krank_g, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  rc = exclusive_scan(pred_kept, n, ws.krank_p, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  cluster_frames_kernel<<<nb, 256, 0, st>>>(gt_kept, ws.cframe_g, ws.krank_g, n, fbase_g, fend_g,
                                            ws.klist_g);
  cluster_frames_kernel<<<nb, 256, 0, st>>>(pred_kept, ws.cframe_p, ws.krank_p, n, fbase_p,
                                            fend_p, ws.klist_p);
  RG_LAUNCH_CHECK();

  // 1. inter of every overlapping (gt, pred) pair: the run lengths of the sorted node pairs
  const u64 sent1 = (u64)n << 32;
  node_pairs_kernel<<<nb, 256, 0, st>>>(gt_of, pred_of, gt_kept, pred_kept, n, sent1, ws.keys1);
  RG_LAUNCH_CHECK();
  size_t sb = ws.sort_bytes;
  RG_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(ws.sort_ws, sb, ws.keys1, ws.keys1_s, n, 0,
                                                 32 + bits_for(n), st));
  key_heads_kernel<<<nb, 256, 0, st>>>(ws.keys1_s, n, sent1, ws.flag);
  RG_LAUNCH_CHECK();
  rc = exclusive_scan(ws.flag, n, ws.rank, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  entry_pos_kernel<<<nb, 256, 0, st>>>(ws.keys1_s, ws.flag, ws.rank, n, sent1, ws.entry_pos);
  RG_LAUNCH_CHECK();
  // 2. d per entry; 3. entries by (frame, d, gt, pred): they are in (frame, gt, pred) order
  // already, and the radix sort by (frame, d) is stable
  entries_kernel<<<nb, 256, 0, st>>>(ws.keys1_s, ws.entry_pos, ws.rank, gt_ptr, pred_ptr,
                                     ws.cframe_g, n, nf, ws.ent_g, ws.ent_p, ws.ent_d, ws.keys2,
                                     ws.vals2);
  RG_LAUNCH_CHECK();
  sb = ws.sort_bytes;
  RG_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws.sort_ws, sb, ws.keys2, ws.keys2_s, ws.vals2,
                                                  ws.vals2_s, n, 0, 32 + bits_for(nf), st));
  entry_ranges_kernel<<<nb, 256, 0, st>>>(ws.keys2_s, n, nf, est, eend);
  RG_LAUNCH_CHECK();
  // 4.-6. the greedy walk and the fill-in, one wave per frame
  Picks pk{pick_start, pick_count, pick_gt, pick_pred, pick_d, pick_positive, pick_gt_cluster,
           pick_pred_cluster};
  walk_kernel<<<nf, WAVE, 0, st>>>(est, eend, ws.vals2_s, ws.ent_g, ws.ent_p, ws.ent_d, ws.krank_g,
                                   ws.krank_p, fbase_g, fend_g, fbase_p, fend_p, ws.klist_g,
                                   ws.klist_p, used_g, used_p, ws.unr, ws.unc, eps, pk);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" size_t rg_eval_associate_l2_workspace_size(int n_nodes, int n_frames) {
  if (n_nodes <= 0 || n_frames <= 0 || n_nodes > EVAL_MAX_NODES) return 0;
  return l2_ws_layout(n_nodes, n_frames, nullptr, nullptr);
}

extern "C" int rg_eval_associate_l2(const int* frame_ptr, int n_nodes, int n_frames,
                                    int max_frame_nodes, const int* gt_ptr, const int* gt_idx,
                                    const int* pred_ptr, const int* pred_idx, int size_threshold,
                                    float eps, const float* gt_mu, const float* pred_mu,
                                    int* gt_kept, int* pred_kept, int* pick_start,
                                    int* pick_count, int* pick_gt, int* pick_pred, float* pick_d,
                                    int* pick_positive, int* pick_gt_cluster,
                                    int* pick_pred_cluster, int* bad_value, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  RG_REQUIRE(n_nodes >= 0 && n_frames >= 0 && max_frame_nodes >= 0 && size_threshold >= 0,
             RG_ERR_ARG,
             "rg_eval_associate_l2: n_nodes=%d n_frames=%d max_frame_nodes=%d threshold=%d",
             n_nodes, n_frames, max_frame_nodes, size_threshold);
  RG_REQUIRE(n_nodes <= EVAL_MAX_NODES, RG_ERR_UNSUPPORTED, "rg_eval_associate_l2: n_nodes=%d > %d",
             n_nodes, EVAL_MAX_NODES);
  RG_REQUIRE(n_nodes == 0 || n_frames >= 1, RG_ERR_ARG,
             "rg_eval_associate_l2: nodes without a frame");
  if (n_frames == 0) return RG_OK;
  RG_REQUIRE(pick_start && pick_count, RG_ERR_ARG, "rg_eval_associate_l2: null pick_start / pick_count");
  if (n_nodes == 0) {
    RG_CHECK_HIP(hipMemsetAsync(pick_start, 0, (size_t)n_frames * sizeof(int), st));
    RG_CHECK_HIP(hipMemsetAsync(pick_count, 0, (size_t)n_frames * sizeof(int), st));
    return RG_OK;
  }
  RG_REQUIRE(frame_ptr && gt_ptr && gt_idx && pred_ptr && pred_idx && gt_mu && pred_mu && gt_kept &&
                 pred_kept && pick_gt && pick_pred && pick_d && pick_positive && pick_gt_cluster &&
                 pick_pred_cluster && bad_value,
             RG_ERR_ARG, "rg_eval_associate_l2: null pointer with n_nodes=%d", n_nodes);
  L2Ws ws;
  const size_t need = l2_ws_layout(n_nodes, n_frames, &ws, (char*)workspace);
  RG_REQUIRE(workspace && workspace_bytes >= need, RG_ERR_ARG,
             "rg_eval_associate_l2: workspace %zu < %zu", workspace_bytes, need);
  const int n = n_nodes, nf = n_frames, nb = ceil_div(n, 256);
  int *fbase_g = ws.fr, *fend_g = ws.fr + nf, *fbase_p = ws.fr + 2 * (size_t)nf,
      *fend_p = ws.fr + 3 * (size_t)nf;
  RG_CHECK_HIP(hipMemsetAsync(ws.fr, 0, (size_t)4 * nf * sizeof(int), st));
  RG_CHECK_HIP(hipMemsetAsync(pick_gt_cluster, 0xff, (size_t)n * sizeof(int), st));
  RG_CHECK_HIP(hipMemsetAsync(pick_pred_cluster, 0xff, (size_t)n * sizeof(int), st));

  // the size filter and each frame's kept clusters, as rg_eval_associate
  cluster_info_kernel<<<nb, 256, 0, st>>>(gt_ptr, gt_idx, frame_ptr, nf, n, size_threshold,
                                          gt_kept, ws.cframe_g);
  cluster_info_kernel<<<nb, 256, 0, st>>>(pred_ptr, pred_idx, frame_ptr, nf, n, size_threshold,
                                          pred_kept, ws.cframe_p);
  RG_LAUNCH_CHECK();
  int rc = exclusive_scan(gt_kept, n, ws.krank_g, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  rc = exclusive_scan(pred_kept, n, ws.krank_p, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  cluster_frames_kernel<<<nb, 256, 0, st>>>(gt_kept, ws.cframe_g, ws.krank_g, n, fbase_g, fend_g,
                                            ws.klist_g);
  cluster_frames_kernel<<<nb, 256, 0, st>>>(pred_kept, ws.cframe_p, ws.krank_p, n, fbase_p,
                                            fend_p, ws.klist_p);
  RG_LAUNCH_CHECK();

  // a frame has at most max_frame_nodes clusters a side; one past the LDS state (or past a
  // max_frame_nodes that was too small) runs from the workspace
  int cap = max_frame_nodes < L2_LDS_CAP ? max_frame_nodes : L2_LDS_CAP;
  if (cap < 1) cap = 1;
  const int lds_bytes = (cap * L2_SLOT_BYTES + 15) & ~15;
  RG_ENSURE_LDS(l2_assoc_kernel, ((L2_LDS_CAP * L2_SLOT_BYTES + 15) & ~15));
  Picks pk{pick_start, pick_count, pick_gt, pick_pred, pick_d, pick_positive, pick_gt_cluster,
           pick_pred_cluster};
  l2_assoc_kernel<<<nf, L2_THREADS, lds_bytes, st>>>(fbase_g, fend_g, fbase_p, fend_p, ws.klist_g,
                                                     ws.klist_p, gt_mu, pred_mu, cap, ws.st, eps,
                                                     pk, bad_value);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_eval_accumulate(const int* pick_gt_cluster, const int* pick_pred_cluster,
                                  const int* pick_positive, const int* gt_kept,
                                  const int* pred_kept, const int64_t* gt_class,
                                  const int64_t* pred_class, int n_nodes, int num_classes,
                                  int false_class, int64_t* confusion, int64_t* gt_count,
                                  int64_t* pred_count, int* bad_class, void* stream) {
  RG_REQUIRE(n_nodes >= 0, RG_ERR_ARG, "rg_eval_accumulate: n_nodes=%d", n_nodes);
  RG_REQUIRE(num_classes >= 1 && num_classes <= MAXC, RG_ERR_UNSUPPORTED,
             "rg_eval_accumulate: num_classes=%d outside 1..%d", num_classes, MAXC);
  RG_REQUIRE(false_class >= 0 && false_class < num_classes, RG_ERR_ARG,
             "rg_eval_accumulate: false_class=%d outside [0, %d)", false_class, num_classes);
  if (n_nodes == 0) return RG_OK;
  int nb = ceil_div(n_nodes, 256);
  if (nb > 1024) nb = 1024;
  accumulate_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(
      pick_gt_cluster, pick_pred_cluster, pick_positive, gt_kept, pred_kept, gt_class, pred_class,
      n_nodes, num_classes, false_class, confusion, gt_count, pred_count, bad_class);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_eval_node_confusion(const float* node_logits, int ld, const int64_t* node_class,
                                      long n_nodes, int num_classes, int64_t* confusion,
                                      int64_t* gt_count, int* bad_class, void* stream) {
  RG_REQUIRE(n_nodes >= 0, RG_ERR_ARG, "rg_eval_node_confusion: n_nodes=%ld", n_nodes);
  RG_REQUIRE(num_classes >= 1 && num_classes <= MAXC, RG_ERR_UNSUPPORTED,
             "rg_eval_node_confusion: num_classes=%d outside 1..%d", num_classes, MAXC);
  RG_REQUIRE(ld >= num_classes, RG_ERR_ARG, "rg_eval_node_confusion: ld=%d < %d", ld, num_classes);
  if (n_nodes == 0) return RG_OK;
  int nb = ceil_div(n_nodes, 256);
  if (nb > 1024) nb = 1024;
  node_confusion_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(node_logits, ld, node_class, n_nodes,
                                                             num_classes, confusion, gt_count,
                                                             bad_class);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_eval_class_confusion(const int64_t* gt_class, const int64_t* pred_class, long n,
                                       int num_classes, int64_t* confusion, int64_t* gt_count,
                                       int* bad_class, void* stream) {
  RG_REQUIRE(n >= 0, RG_ERR_ARG, "rg_eval_class_confusion: n=%ld", n);
  RG_REQUIRE(num_classes >= 1 && num_classes <= MAXC, RG_ERR_UNSUPPORTED,
             "rg_eval_class_confusion: num_classes=%d outside 1..%d", num_classes, MAXC);
  if (n == 0) return RG_OK;
  RG_REQUIRE(gt_class && pred_class && confusion && gt_count && bad_class, RG_ERR_ARG,
             "rg_eval_class_confusion: null pointer with n=%ld", n);
  int nb = ceil_div(n, 256);
  if (nb > 1024) nb = 1024;
  class_confusion_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(gt_class, pred_class, n, num_classes,
                                                              confusion, gt_count, bad_class);
  RG_LAUNCH_CHECK();
  return RG_OK;
}
