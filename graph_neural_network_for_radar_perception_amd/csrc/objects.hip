// The object stage between the detector and the cluster-level classifier, for a batch of
// frames on the device (global node ids, clusters as the CSR of rg_cluster_lists):
//   rg_cluster_stats   : compute_cluster_sample_mean_and_cov / compute_proposals
//                        (modules/inference/inference.py:23-47): size, mean, covariance of
//                        every cluster, and the eigen-decomposition np.linalg.eig returns for
//                        the symmetric 2 x 2 covariance (LAPACK sgeev -> slanv2: order and sign);
//   rg_cov_ellipse     : compute_cov_ellipse (modules/inference/ellipse.py:4-37);
//   rg_softmax_max     : torch.max(F.softmax(logits)) of process_frame (output.py:104-121);
//   rg_cluster_class_from_objects : the same per kept object of the cluster-level classifier,
//                        scattered to the object's source cluster (the third class source);
//   rg_object_select   : the size filter (remove_low_quality_proposals,
//                        datagen_classifier.py:166-190) and the class filter (output.py:123-128)
//                        with the compaction of the kept objects and of their member rows;
//   rg_object_gather   : per-object rows of the kept objects;
//   rg_object_features : extract_and_compute_features_and_labels
//                        (datagen_classifier.py:62-100): the eigenbasis-aligned member features.
// One thread owns one cluster's sums: they run over the members in list order, in float32,
// with contraction off, which is numpy's evaluation order -- mean and covariance are
// bit-identical to the reference.  Nothing here synchronises with the host.
#include "rg_common.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace rg {
namespace objects {

typedef unsigned long long u64;

static constexpr int MAXC = 32;  // classes (the detector has 7)
static constexpr int OBJ_MAX_NODES = 1 << 30;

// np.linalg.eig of [[a, b], [b, d]] in float32: slanv2's standardisation of the 2 x 2 block
// (the rotation (cs, sn) is the pair of eigenvectors, stored as columns)
struct Eig2 {
  float l1, l2, v00, v01, v10, v11;
};

__device__ __forceinline__ Eig2 eig_sym2(float a, float b, float d) {
  Eig2 e;
  if (b == 0.f) {
    e.l1 = a;
    e.l2 = d;
    e.v00 = 1.f;
    e.v01 = 0.f;
    e.v10 = 0.f;
    e.v11 = 1.f;
    return e;
  }
  const float p = 0.5f * (a - d);
  const float ab = fabsf(b);
  const float scale = fmaxf(fabsf(p), ab);
  const float zz = p / scale * p + ab / scale * ab;
  const float z = p + copysignf(sqrtf(scale) * sqrtf(zz), p);
  e.l1 = d + z;
  e.l2 = d - ab / z * ab;
  const float tau = hypotf(b, z);
  const float cs = z / tau, sn = b / tau;
  e.v00 = cs;
  e.v01 = -sn;
  e.v10 = sn;
  e.v11 = cs;
  return e;
}

__global__ void stats_kernel(const float* __restrict__ xy, int ld, int n_nodes,
                             const int* __restrict__ ptr, const int* __restrict__ idx, int ncl,
                             float n00, float n01, float n10, float n11, int* __restrict__ size,
                             float* __restrict__ mu, float* __restrict__ sigma,
                             float* __restrict__ eigval, float* __restrict__ eigvec,
                             int* __restrict__ bad) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncl) return;
  const int a = ptr[c], b = ptr[c + 1];
  const int n = b > a ? b - a : 0;
  float sx = 0.f, sy = 0.f;
  bool ok = a >= 0 && b <= n_nodes;
  if (ok)
    for (int p = a; p < b; ++p) {
      const int node = idx[p];
      if (node < 0 || node >= n_nodes) {
        ok = false;
        break;
      }
      sx += xy[(size_t)node * ld];
      sy += xy[(size_t)node * ld + 1];
    }
  if (!ok && bad) atomicExch(bad, 1);
  float mx = 0.f, my = 0.f;
  float s00 = n00, s01 = n01, s10 = n10, s11 = n11;
  if (ok && n > 0) {
    mx = div_rn(sx, (float)n);
    my = div_rn(sy, (float)n);
  }
  if (ok && n > 1) {
    float qxx = 0.f, qxy = 0.f, qyy = 0.f;
    for (int p = a; p < b; ++p) {
      const int node = idx[p];
      const float ex = mx - xy[(size_t)node * ld], ey = my - xy[(size_t)node * ld + 1];
      qxx += ex * ex;
      qxy += ex * ey;
      qyy += ey * ey;
    }
    const float m1 = (float)(n - 1);
    const float cxy = div_rn(qxy, m1);
    s00 = div_rn(qxx, m1) + n00;
    s01 = cxy + n01;
    s10 = cxy + n10;
    s11 = div_rn(qyy, m1) + n11;
  }
  size[c] = n;
  mu[2 * (size_t)c] = mx;
  mu[2 * (size_t)c + 1] = my;
  float* s = sigma + 4 * (size_t)c;
  s[0] = s00;
  s[1] = s01;
  s[2] = s10;
  s[3] = s11;
  const Eig2 e = eig_sym2(s00, s01, s11);
  if (eigval) {
    eigval[2 * (size_t)c] = e.l1;
    eigval[2 * (size_t)c + 1] = e.l2;
  }
  if (eigvec) {
    float* v = eigvec + 4 * (size_t)c;
    v[0] = e.v00;
    v[1] = e.v01;
    v[2] = e.v10;
    v[3] = e.v11;
  }
}

// compute_cov_ellipse as written: the angle reads ROW `largest` of v
__global__ void ellipse_kernel(const float* __restrict__ eigval, const float* __restrict__ eigvec,
                               int ncl, float chi, float* __restrict__ abt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncl) return;
  const float l0 = eigval[2 * (size_t)c], l1 = eigval[2 * (size_t)c + 1];
  const int big = l0 >= l1 ? 0 : 1;  // np.where(d == np.max(d))[0][0]
  const float a = chi * sqrtf(big == 0 ? l0 : l1);
  const float b = chi * sqrtf(big == 0 ? l1 : l0);
  const float* v = eigvec + 4 * (size_t)c + 2 * big;
  const float theta = v[0] == 0.f ? 1.57079632679489661923f : atan2f(v[1], v[0]);
  abt[3 * (size_t)c] = a;
  abt[3 * (size_t)c + 1] = b;
  abt[3 * (size_t)c + 2] = theta;
}

// points = [a cos th, b sin th] @ R^T + mu, R = [[cos t, sin t], [-sin t, cos t]],
// th = np.linspace(0, 2 pi, n_points) in float64
__global__ void ellipse_points_kernel(const float* __restrict__ abt, const float* __restrict__ mu,
                                      long total, int n_points, float* __restrict__ pts) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const long c = t / n_points;
  const int k = (int)(t - c * n_points);
  const double two_pi = 6.283185307179586476925;
  double th = 0.0;
  if (n_points > 1) th = k == n_points - 1 ? two_pi : (double)k * (two_pi / (double)(n_points - 1));
  const double px = (double)abt[3 * c] * cos(th), py = (double)abt[3 * c + 1] * sin(th);
  const float theta = abt[3 * c + 2];
  const double ct = (double)cosf(theta), st = (double)sinf(theta);
  pts[2 * t] = (float)(px * ct + py * st + (double)mu[2 * c]);
  pts[2 * t + 1] = (float)(-px * st + py * ct + (double)mu[2 * c + 1]);
}

// the first maximum of a row of logits and its float32 softmax value: the one definition
// behind rg_softmax_max and rg_cluster_class_from_objects
__device__ __forceinline__ void softmax_max_row(const float* __restrict__ row, int nc, int& am,
                                                float& score) {
  float m = row[0];
  am = 0;
  for (int k = 1; k < nc; ++k)
    if (row[k] > m) {
      m = row[k];
      am = k;
    }
  float s = 0.f;
  for (int k = 0; k < nc; ++k) s += expf(row[k] - m);
  score = 1.f / s;
}

__global__ void softmax_max_kernel(const float* __restrict__ x, int ld, long n, int nc,
                                   int64_t* __restrict__ cls, float* __restrict__ score) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int am;
  float s;
  softmax_max_row(x + (size_t)r * ld, nc, am, s);
  if (cls) cls[r] = am;
  if (score) score[r] = s;
}

// ------------------------------------------------------------------ classifier classes
// every cluster starts as one that no object names ...
__global__ void class_fill_kernel(int ncl, int64_t fill, int64_t* __restrict__ cls,
                                  float* __restrict__ score) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncl) return;
  cls[c] = fill;
  if (score) score[c] = 0.f;
}

// ... and, after it in stream order, object o writes the slot of its source cluster (the
// entries of obj_cluster are distinct: one writer per slot)
__global__ void class_scatter_kernel(const float* __restrict__ x, int ld, long n, int nc,
                                     const int* __restrict__ obj_cluster, int ncl,
                                     int64_t* __restrict__ cls, float* __restrict__ score,
                                     int* __restrict__ bad) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  const int c = obj_cluster[o];
  if (c < 0 || c >= ncl) {
    atomicExch(bad, 1);
    return;
  }
  int am;
  float s;
  softmax_max_row(x + (size_t)o * ld, nc, am, s);
  cls[c] = am;
  if (score) score[c] = s;
}

// ------------------------------------------------------------------ selection

// kept flag, member rows and n (n - 1) edges of every cluster; the edge total is an integer
// sum (wave first, then one atomic per wave), so the arrival order does not matter
__global__ __launch_bounds__(256) void select_flags_kernel(
    const int* __restrict__ ptr, int ncl, const int64_t* __restrict__ cls, int min_meas,
    int drop_class, int* __restrict__ kept, int* __restrict__ rows, int64_t* __restrict__ counts) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  u64 e = 0;
  if (c < ncl) {
    const int sz = ptr[c + 1] - ptr[c];
    bool k = sz >= min_meas && sz > 0;
    if (k && cls && drop_class >= 0 && cls[c] == (int64_t)drop_class) k = false;
    kept[c] = k ? 1 : 0;
    rows[c] = k ? sz : 0;
    if (k) e = (u64)sz * (u64)(sz - 1);
  }
  for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off);
  if ((threadIdx.x & 63) == 0 && e) atomicAdd((u64*)(counts + 2), e);
}

// the first node of cluster c (clusters come frame by frame); past the member list: INT_MAX
__device__ __forceinline__ int first_node(const int* ptr, const int* idx, int ncl, int c) {
  const int a = ptr[c];
  return a < ptr[ncl] ? idx[a] : 0x7fffffff;
}

// krank / rbase: exclusive scans of kept / rows.  Per kept cluster its object slot; per frame
// the first object and the first member row (the number of clusters whose first node lies
// before the frame is a binary search: the predicate is monotone)
__global__ void select_emit_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, int ncl,
                                   const int* __restrict__ kept, const int* __restrict__ krank,
                                   const int* __restrict__ rbase, const int* __restrict__ fp, int nf,
                                   int* __restrict__ cluster_row, int* __restrict__ obj_cluster,
                                   int* __restrict__ obj_row_ptr, int* __restrict__ frame_obj_ptr,
                                   int* __restrict__ frame_row_ptr, int64_t* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    counts[0] = krank[ncl];
    counts[1] = rbase[ncl];
    obj_row_ptr[krank[ncl]] = rbase[ncl];
  }
  if (i < ncl) {
    const int k = kept[i];
    cluster_row[i] = k ? rbase[i] : -1;
    if (k) {
      obj_cluster[krank[i]] = i;
      obj_row_ptr[krank[i]] = rbase[i];
    }
  }
  if (i <= nf && frame_obj_ptr) {
    const int node = fp[i];
    int lo = 0, hi = ncl;  // first cluster whose first node >= node
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (first_node(ptr, idx, ncl, mid) >= node) hi = mid;
      else lo = mid + 1;
    }
    frame_obj_ptr[i] = krank[lo];
    frame_row_ptr[i] = rbase[lo];
  }
}

struct GatherArgs {
  const int* obj_cluster;
  const int64_t* counts;
  const int* size;
  const int64_t* cls;
  const float* score;
  const float* mu;
  const float* sigma;
  const float* ellipse;
  const int* cluster_ptr;
  const int* cluster_idx;
  const int* frame_ptr;
  int n_frames;
  int64_t* o_size;
  int64_t* o_cls;
  float* o_score;
  float* o_mu;
  float* o_sigma;
  float* o_ellipse;
  int* o_frame;
};

__global__ void gather_kernel(GatherArgs g, int ncl) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= ncl || (int64_t)o >= g.counts[0]) return;
  const int c = g.obj_cluster[o];
  if (c < 0 || c >= ncl) return;
  if (g.o_size) g.o_size[o] = g.size[c];
  if (g.o_cls) g.o_cls[o] = g.cls[c];
  if (g.o_score) g.o_score[o] = g.score[c];
  if (g.o_mu) {
    g.o_mu[2 * (size_t)o] = g.mu[2 * (size_t)c];
    g.o_mu[2 * (size_t)o + 1] = g.mu[2 * (size_t)c + 1];
  }
  if (g.o_sigma)
    for (int k = 0; k < 4; ++k) g.o_sigma[4 * (size_t)o + k] = g.sigma[4 * (size_t)c + k];
  if (g.o_ellipse)
    for (int k = 0; k < 3; ++k) g.o_ellipse[3 * (size_t)o + k] = g.ellipse[3 * (size_t)c + k];
  if (g.o_frame) {
    const int node = g.cluster_idx[g.cluster_ptr[c]];
    int lo = 0, hi = g.n_frames;  // first f with frame_ptr[f + 1] > node
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (g.frame_ptr[mid + 1] > node) hi = mid;
      else lo = mid + 1;
    }
    g.o_frame[o] = lo < g.n_frames ? lo : g.n_frames - 1;
  }
}

// one thread per position of the member list: (x, y) = (p - mu) @ V, r, th, rcs
__global__ void features_kernel(const float* __restrict__ xy, int ld, const float* __restrict__ rcs,
                                int ld_rcs, int n_nodes, const int* __restrict__ ptr,
                                const int* __restrict__ idx, int ncl,
                                const int* __restrict__ cluster_row, const float* __restrict__ mu,
                                const float* __restrict__ eigvec, float* __restrict__ feat) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_nodes || j >= ptr[ncl]) return;
  int lo = 0, hi = ncl;  // first c with ptr[c + 1] > j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid + 1] > j) hi = mid;
    else lo = mid + 1;
  }
  if (lo >= ncl) return;
  const int base = cluster_row[lo];
  const int node = idx[j];
  if (base < 0 || node < 0 || node >= n_nodes) return;
  const float dx = xy[(size_t)node * ld] - mu[2 * (size_t)lo];
  const float dy = xy[(size_t)node * ld + 1] - mu[2 * (size_t)lo + 1];
  const float* v = eigvec + 4 * (size_t)lo;
  const float fx = dx * v[0] + dy * v[2];
  const float fy = dx * v[1] + dy * v[3];
  float* out = feat + 5 * ((size_t)base + (size_t)(j - ptr[lo]));
  out[0] = fx;
  out[1] = fy;
  out[2] = sqrtf(fx * fx + fy * fy);
  out[3] = atan2f(fy, fx);
  out[4] = rcs[(size_t)node * ld_rcs];
}

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct SelectWs {
  int *kept, *rows, *krank, *rbase;
  void* scan_ws;
};

static size_t select_ws_layout(int ncl, SelectWs* w, char* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  SelectWs x;
  x.kept = (int*)take((size_t)ncl * sizeof(int));
  x.rows = (int*)take((size_t)ncl * sizeof(int));
  x.krank = (int*)take(((size_t)ncl + 1) * sizeof(int));
  x.rbase = (int*)take(((size_t)ncl + 1) * sizeof(int));
  x.scan_ws = take(scan_workspace_bytes((long)ncl + 1));
  if (w) *w = x;
  return off;
}

}  // namespace objects
}  // namespace rg

using namespace rg;
using namespace rg::objects;

extern "C" int rg_cluster_stats(const float* xy, int ld_xy, int n_nodes, const int* cluster_ptr,
                                const int* cluster_idx, int n_clusters, const float* noise_cov,
                                int* size, float* mu, float* sigma, float* eigval, float* eigvec,
                                int* bad_index, void* stream) {
  RG_REQUIRE(n_nodes >= 0 && n_clusters >= 0 && n_nodes <= OBJ_MAX_NODES, RG_ERR_ARG,
             "rg_cluster_stats: n_nodes=%d n_clusters=%d", n_nodes, n_clusters);
  RG_REQUIRE(n_clusters <= n_nodes, RG_ERR_ARG, "rg_cluster_stats: %d clusters for %d nodes",
             n_clusters, n_nodes);
  RG_REQUIRE(noise_cov, RG_ERR_ARG, "rg_cluster_stats: noise_cov is null");
  RG_REQUIRE(noise_cov[1] == noise_cov[2], RG_ERR_ARG,
             "rg_cluster_stats: noise_cov is not symmetric (%g, %g)", (double)noise_cov[1],
             (double)noise_cov[2]);
  if (n_clusters == 0) return RG_OK;
  RG_REQUIRE(xy && cluster_ptr && cluster_idx && size && mu && sigma, RG_ERR_ARG,
             "rg_cluster_stats: null pointer with n_clusters=%d", n_clusters);
  RG_REQUIRE(ld_xy >= 2, RG_ERR_ARG, "rg_cluster_stats: ld_xy=%d < 2", ld_xy);
  stats_kernel<<<ceil_div(n_clusters, 64), 64, 0, (hipStream_t)stream>>>(
      xy, ld_xy, n_nodes, cluster_ptr, cluster_idx, n_clusters, noise_cov[0], noise_cov[1],
      noise_cov[2], noise_cov[3], size, mu, sigma, eigval, eigvec, bad_index);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_cov_ellipse(const float* eigval, const float* eigvec, const float* mu,
                              int n_clusters, float chi_sq, int n_points, float* abt,
                              float* points, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  RG_REQUIRE(n_clusters >= 0, RG_ERR_ARG, "rg_cov_ellipse: n_clusters=%d", n_clusters);
  RG_REQUIRE(n_points >= 1, RG_ERR_ARG, "rg_cov_ellipse: n_points=%d < 1", n_points);
  if (n_clusters == 0) return RG_OK;
  RG_REQUIRE(eigval && eigvec && abt && (!points || mu), RG_ERR_ARG,
             "rg_cov_ellipse: null pointer with n_clusters=%d", n_clusters);
  ellipse_kernel<<<ceil_div(n_clusters, 256), 256, 0, st>>>(eigval, eigvec, n_clusters, chi_sq,
                                                            abt);
  RG_LAUNCH_CHECK();
  if (points) {
    const long total = (long)n_clusters * n_points;
    ellipse_points_kernel<<<ceil_div(total, 256), 256, 0, st>>>(abt, mu, total, n_points, points);
    RG_LAUNCH_CHECK();
  }
  return RG_OK;
}

extern "C" int rg_softmax_max(const float* x, int ld, long n_rows, int num_classes, int64_t* cls,
                              float* score, void* stream) {
  RG_REQUIRE(n_rows >= 0, RG_ERR_ARG, "rg_softmax_max: n_rows=%ld", n_rows);
  RG_REQUIRE(num_classes >= 1 && num_classes <= MAXC, RG_ERR_UNSUPPORTED,
             "rg_softmax_max: num_classes=%d outside 1..%d", num_classes, MAXC);
  RG_REQUIRE(ld >= num_classes, RG_ERR_ARG, "rg_softmax_max: ld=%d < %d", ld, num_classes);
  if (n_rows == 0) return RG_OK;
  RG_REQUIRE(x && (cls || score), RG_ERR_ARG, "rg_softmax_max: null pointer with n_rows=%ld",
             n_rows);
  softmax_max_kernel<<<ceil_div(n_rows, 256), 256, 0, (hipStream_t)stream>>>(x, ld, n_rows,
                                                                           num_classes, cls, score);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_cluster_class_from_objects(const float* logits, int ld, long n_objects,
                                             int num_classes, const int* obj_cluster,
                                             int n_clusters, int64_t fill_class,
                                             int64_t* cluster_class, float* cluster_score,
                                             int* bad_index, void* stream) {
  RG_REQUIRE(n_objects >= 0 && n_clusters >= 0, RG_ERR_ARG,
             "rg_cluster_class_from_objects: n_objects=%ld n_clusters=%d", n_objects, n_clusters);
  RG_REQUIRE(num_classes >= 1 && num_classes <= MAXC, RG_ERR_UNSUPPORTED,
             "rg_cluster_class_from_objects: num_classes=%d outside 1..%d", num_classes, MAXC);
  RG_REQUIRE(ld >= num_classes, RG_ERR_ARG, "rg_cluster_class_from_objects: ld=%d < %d", ld,
             num_classes);
  if (n_clusters == 0) return RG_OK;
  RG_REQUIRE(cluster_class, RG_ERR_ARG,
             "rg_cluster_class_from_objects: cluster_class is null with n_clusters=%d", n_clusters);
  RG_REQUIRE(n_objects == 0 || (logits && obj_cluster && bad_index), RG_ERR_ARG,
             "rg_cluster_class_from_objects: null pointer with n_objects=%ld", n_objects);
  class_fill_kernel<<<ceil_div(n_clusters, 256), 256, 0, (hipStream_t)stream>>>(
      n_clusters, fill_class, cluster_class, cluster_score);
  RG_LAUNCH_CHECK();
  if (n_objects == 0) return RG_OK;
  class_scatter_kernel<<<ceil_div(n_objects, 256), 256, 0, (hipStream_t)stream>>>(
      logits, ld, n_objects, num_classes, obj_cluster, n_clusters, cluster_class, cluster_score,
      bad_index);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" size_t rg_object_select_workspace_size(int n_clusters) {
  if (n_clusters <= 0 || n_clusters > OBJ_MAX_NODES) return 0;
  return select_ws_layout(n_clusters, nullptr, nullptr);
}

extern "C" int rg_object_select(const int* cluster_ptr, const int* cluster_idx, int n_clusters,
                                const int* frame_ptr, int n_frames, const int64_t* cluster_class,
                                int num_classes, int min_meas, int drop_class, int* cluster_row,
                                int* obj_cluster, int* obj_row_ptr, int* frame_obj_ptr,
                                int* frame_row_ptr, int64_t* counts, void* workspace,
                                size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  RG_REQUIRE(n_clusters >= 0 && n_frames >= 0 && n_clusters <= OBJ_MAX_NODES, RG_ERR_ARG,
             "rg_object_select: n_clusters=%d n_frames=%d", n_clusters, n_frames);
  RG_REQUIRE(min_meas >= 0, RG_ERR_ARG, "rg_object_select: min_meas=%d < 0", min_meas);
  RG_REQUIRE(num_classes >= 1 && num_classes <= MAXC, RG_ERR_UNSUPPORTED,
             "rg_object_select: num_classes=%d outside 1..%d", num_classes, MAXC);
  RG_REQUIRE(drop_class >= -1 && drop_class < num_classes, RG_ERR_ARG,
             "rg_object_select: drop_class=%d outside [-1, %d)", drop_class, num_classes);
  RG_REQUIRE(counts && obj_row_ptr, RG_ERR_ARG, "rg_object_select: counts / obj_row_ptr is null");
  RG_REQUIRE(!frame_obj_ptr == !frame_row_ptr && (!frame_obj_ptr || frame_ptr), RG_ERR_ARG,
             "rg_object_select: frame_obj_ptr, frame_row_ptr and frame_ptr go together");
  if (n_clusters == 0) {
    RG_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
    RG_CHECK_HIP(hipMemsetAsync(obj_row_ptr, 0, sizeof(int), st));
    if (frame_obj_ptr) {
      RG_CHECK_HIP(hipMemsetAsync(frame_obj_ptr, 0, ((size_t)n_frames + 1) * sizeof(int), st));
      RG_CHECK_HIP(hipMemsetAsync(frame_row_ptr, 0, ((size_t)n_frames + 1) * sizeof(int), st));
    }
    return RG_OK;
  }
  RG_REQUIRE(cluster_ptr && cluster_idx && cluster_row && obj_cluster, RG_ERR_ARG,
             "rg_object_select: null pointer with n_clusters=%d", n_clusters);
  RG_REQUIRE(drop_class < 0 || cluster_class, RG_ERR_ARG,
             "rg_object_select: drop_class=%d without cluster_class", drop_class);
  SelectWs ws;
  const size_t need = select_ws_layout(n_clusters, &ws, (char*)workspace);
  RG_REQUIRE(workspace && workspace_bytes >= need, RG_ERR_ARG,
             "rg_object_select: workspace %zu < %zu", workspace_bytes, need);
  RG_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
  select_flags_kernel<<<ceil_div(n_clusters, 256), 256, 0, st>>>(
      cluster_ptr, n_clusters, cluster_class, min_meas, drop_class, ws.kept, ws.rows, counts);
  RG_LAUNCH_CHECK();
  int rc = exclusive_scan(ws.kept, n_clusters, ws.krank, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  rc = exclusive_scan(ws.rows, n_clusters, ws.rbase, nullptr, ws.scan_ws, st);
  if (rc) return rc;
  const int work = n_clusters > n_frames + 1 ? n_clusters : n_frames + 1;
  select_emit_kernel<<<ceil_div(work, 256), 256, 0, st>>>(
      cluster_ptr, cluster_idx, n_clusters, ws.kept, ws.krank, ws.rbase, frame_ptr, n_frames,
      cluster_row, obj_cluster, obj_row_ptr, frame_obj_ptr, frame_row_ptr, counts);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_object_gather(const int* obj_cluster, const int64_t* counts, int n_clusters,
                                const int* size, const int64_t* cluster_class, const float* score,
                                const float* mu, const float* sigma, const float* ellipse,
                                const int* cluster_ptr, const int* cluster_idx,
                                const int* frame_ptr, int n_frames, int64_t* obj_size,
                                int64_t* obj_class, float* obj_score, float* obj_mu,
                                float* obj_sigma, float* obj_ellipse, int* obj_frame,
                                void* stream) {
  RG_REQUIRE(n_clusters >= 0 && n_frames >= 0, RG_ERR_ARG,
             "rg_object_gather: n_clusters=%d n_frames=%d", n_clusters, n_frames);
  if (n_clusters == 0) return RG_OK;
  RG_REQUIRE(obj_cluster && counts, RG_ERR_ARG, "rg_object_gather: null pointer with n_clusters=%d",
             n_clusters);
  RG_REQUIRE((!obj_size || size) && (!obj_class || cluster_class) && (!obj_score || score) &&
                 (!obj_mu || mu) && (!obj_sigma || sigma) && (!obj_ellipse || ellipse),
             RG_ERR_ARG, "rg_object_gather: an output without its source");
  RG_REQUIRE(!obj_frame || (cluster_ptr && cluster_idx && frame_ptr && n_frames >= 1), RG_ERR_ARG,
             "rg_object_gather: obj_frame needs the cluster CSR and frame_ptr");
  GatherArgs g{obj_cluster, counts,      size,        cluster_class, score,     mu,
               sigma,       ellipse,     cluster_ptr, cluster_idx,   frame_ptr, n_frames,
               obj_size,    obj_class,   obj_score,   obj_mu,        obj_sigma, obj_ellipse,
               obj_frame};
  gather_kernel<<<ceil_div(n_clusters, 256), 256, 0, (hipStream_t)stream>>>(g, n_clusters);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" int rg_object_features(const float* xy, int ld_xy, const float* rcs, int ld_rcs,
                                  int n_nodes, const int* cluster_ptr, const int* cluster_idx,
                                  int n_clusters, const int* cluster_row, const float* mu,
                                  const float* eigvec, float* features, void* stream) {
  RG_REQUIRE(n_nodes >= 0 && n_clusters >= 0 && n_nodes <= OBJ_MAX_NODES, RG_ERR_ARG,
             "rg_object_features: n_nodes=%d n_clusters=%d", n_nodes, n_clusters);
  if (n_nodes == 0 || n_clusters == 0) return RG_OK;
  RG_REQUIRE(xy && rcs && cluster_ptr && cluster_idx && cluster_row && mu && eigvec && features,
             RG_ERR_ARG, "rg_object_features: null pointer with n_clusters=%d", n_clusters);
  RG_REQUIRE(ld_xy >= 2 && ld_rcs >= 1, RG_ERR_ARG, "rg_object_features: ld_xy=%d ld_rcs=%d",
             ld_xy, ld_rcs);
  features_kernel<<<ceil_div(n_nodes, 256), 256, 0, (hipStream_t)stream>>>(
      xy, ld_xy, rcs, ld_rcs, n_nodes, cluster_ptr, cluster_idx, n_clusters, cluster_row, mu,
      eigvec, features);
  RG_LAUNCH_CHECK();
  return RG_OK;
}
