// Float32 residual_graph_conv_block of the cluster-level classifier (classifier/blocks.py:28-85)
// over the block-diagonal complete graph of compute_edge_index, straight from the object sizes:
// no edge array, no message buffer.  Three launches per layer (rg_cls_conv_layer_x3):
//  * projection (cls_proj_kernel): the classifier's msg0 has neither normalisation nor edge
//    features, so msg0(cat(x_i, x_j)) = leaky(P[i] + Q[j]) with P = W_i x + b0 and Q = W_j x
//    formed once per node -- P | Q [N][256] f32;
//  * edge launch (cls_edge_kernel): object o owns rows [b_o, b_o + n_o); the sources of
//    destination i are those rows without i, ascending -- the order scatter_add_ sums in.  The
//    virtual edge sequence (destination-major, position q in [seg_ptr[i], seg_ptr[i + 1]) of
//    destination i) is cut into one piece of whole destinations per wave with equal edge counts
//    (the wave table), and a wave walks its piece in 32-edge tiles that may span destinations.
//    A tile row finds its destination in a 64-entry window of seg_ptr held across the wave's
//    lanes (six lane exchanges) and its source in closed form from the per-node object begin /
//    size: k = q - seg_ptr[i], j = b + k + (k >= i - b).  Per tile
//        h = leaky(P[i] + Q[j])        in accumulator registers: the B operand of msg1
//        m = leaky(W_1 h + b_1)        W_1's planes staged in LDS
//    then the message tile is transposed through a wave-private LDS tile (lane = two features)
//    and reduced IN EDGE ORDER into a running value that starts anew at each change of
//    destination (wave-uniform); a finished destination's row goes to the [N][128] aggregate
//    scratch.  Every destination lies whole in one wave and every message row depends on its own
//    edge only, so an object's bits depend neither on the other objects of the batch nor on
//    where the table cuts it.  No atomics.
//  * node launch (cls_node_kernel): x_out = x + leaky(W_u cat(x, agg) + b_u); `mean` divides by
//    n_o - 1 here, and a node of a one-member object reads an aggregate of zeros (PyG's fill).
// The projection (128 -> 256) and update (256 -> 128) images are 192 KiB each and are streamed
// from L2 through a buffer resource; msg1's 96 KiB sit in LDS.
// Every kernel is a template of the term scheme of x3_common.h; only B3 is instantiated: the
// classifier's activations are not normalised and leave the h2 domain (|a| < 2^15) on large
// objects.
#include <type_traits>

#ifndef RG_X3_SPLIT
#define RG_X3_SPLIT 4  // builtin conversions in the splits, as conv_x3.hip
#endif
#include "cls_conv_common.h"
#include "scan.h"
#include "x3_common.h"

namespace rg {
namespace clsx3 {

using namespace ::rg::x3;

static constexpr int NFT = 256;   // node and projection launches: 4 waves, one per SIMD

enum { RED_SUM = RG_REDUCE_SUM, RED_MEAN = RG_REDUCE_MEAN, RED_MAX = RG_REDUCE_MAX };

template <typename P>
struct Lay {
  static constexpr int W1 = P::image_bytes(HID, C);
  static constexpr int LDS = al16(W1) + NW * T_BYTES;
  static_assert(LDS <= DYN_LDS_MAX, "cls_conv_x3 LDS");
};

// ------------------------------------------------------------------ the object table
// (layout: cls_conv_common.h)
__global__ void sizes_kernel(const int64_t* __restrict__ object_size, int n_obj,
                             int* __restrict__ sz, int* __restrict__ pairs) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_obj) return;
  const int n = (int)object_size[c];
  sz[c] = n;
  pairs[c] = n * (n - 1);
}

// one thread per node: its object by binary search over the node offsets
__global__ void nodes_kernel(const int* __restrict__ node_off, const int* __restrict__ edge_off,
                             int n_obj, int n_nodes, int* __restrict__ seg, int* __restrict__ beg,
                             int* __restrict__ siz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int tot_e = n_obj > 0 ? edge_off[n_obj] : 0;
  if (i == 0) seg[n_nodes] = tot_e;
  if (i >= n_nodes) return;
  if (n_obj <= 0 || i >= node_off[n_obj]) {  // past the last object: a node of its own
    seg[i] = tot_e;
    beg[i] = i;
    siz[i] = 1;
    return;
  }
  int lo = 0, hi = n_obj - 1;  // last c with node_off[c] <= i (empty objects skipped)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (node_off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  const int off = node_off[lo], n = node_off[lo + 1] - off;
  seg[i] = edge_off[lo] + (i - off) * (n - 1);
  beg[i] = off;
  siz[i] = n;
}

// piece w = the destinations [wtab[w], wtab[w + 1]), wtab[w] the first node whose segment start
// reaches E w / W: equal edge counts, every destination whole in one piece
__global__ void waves_kernel(const int* __restrict__ seg, int n, int W, int* __restrict__ wtab) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w > W) return;
  const long E = seg[n];
  const long target = E * w / W;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  wtab[w] = w == W ? n : lo;
}

// ------------------------------------------------------------------ projection
// P | Q = W_pq x + [b0; 0]: W_pq packed FAST_IN (K = 128, N = 256), streamed from L2; one
// 32-row tile per wave and step
// (no __restrict__ on the pointers of this kernel and of cls_node_kernel: with it the image's
// fragment loads are invariant of the persistent tile loop, and the compiler hoists all 192 KiB
// of them out of it -- 2.4 KB of scratch per lane)
template <typename P>
__global__ __launch_bounds__(NFT) void cls_proj_kernel(const float* x, int ldx,
                                                       int n_nodes, const char* wpq,
                                                       float* pq) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const WBuf W = wbuf(wpq, P::image_bytes(C, PQW), plane_bytes(C, PQW), lane);
  const float* bias = (const float*)(wpq + P::NP * plane_bytes(C, PQW));
  const int ntiles = (n_nodes + 31) / 32;
  for (int t = blockIdx.x * (NFT / 64) + wave; t < ntiles; t += gridDim.x * (NFT / 64)) {
    const int row = t * 32 + r;
    const bool valid = row < n_nodes;
    const float* px = x + (size_t)(valid ? row : n_nodes - 1) * ldx + 8 * h;
    // the row's B operands, split once for both halves of the outputs
    typename P::terms b[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
      b[s] = P::split(*(const f32x4*)(px + 16 * s), *(const f32x4*)(px + 16 * s + 4));
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x16 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = ld_bias_frag(bias, 4 * half + m, h);
      layer_x3<8, 4, 8>(acc, W, 4 * half, [&](int s) { return b[s]; });
      if (valid) {
        float* po = pq + (size_t)row * PQW + 128 * half + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(f32x4*)(po + 32 * m + 8 * g) =
                (f32x4){acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
      }
    }
  }
}

// ------------------------------------------------------------------ edge launch
struct EArgs {
  const float* pq;   // [N][256]
  const int* seg;    // [N + 1]
  const int* beg;    // [N]
  const int* siz;    // [N]
  const int* wtab;   // [gridDim.x * NW + 1]
  float* agg;        // [N + 1][128]: row N takes the flush before a piece's first destination
  const char* w1;    // msg1, FAST_CHAIN
  int n_nodes;
};

template <typename P, int RED>
__global__ __launch_bounds__(FT) void cls_edge_kernel(EArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  stage_lds<FT>(lds, a.w1, Lay<P>::W1);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  float* T = (float*)(lds + al16(Lay<P>::W1) + wave * T_BYTES);  // [TR][TS] message rows
  const WLds w1{lds + lane * 16, plane_bytes(HID, C)};
  const float* bias1 = (const float*)(lds + P::NP * plane_bytes(HID, C));
  constexpr float NEUTRAL = RED == RED_MAX ? -__builtin_huge_valf() : 0.f;

  const int piece = blockIdx.x * NW + wave;
  const int n0 = __builtin_amdgcn_readfirstlane(a.wtab[piece]);
  const int n1 = __builtin_amdgcn_readfirstlane(a.wtab[piece + 1]);
  if (n0 >= n1) return;
  const int e0 = __builtin_amdgcn_readfirstlane(a.seg[n0]);
  const int e1 = __builtin_amdgcn_readfirstlane(a.seg[n1]);
  if (e0 >= e1) return;

  // (destination, source) of this lane's row of the tile at position t; dc: a destination
  // with seg[dc] <= t (wave-uniform), advanced to the destination of the tile's last row.
  // Rows past the piece's last edge repeat it (a re-read of cached rows; masked below).
  auto decode = [&](int t, int& dc, int& di, int& sj) {
    const int q = min(t + r, e1 - 1);
    const int qmax = min(t + 31, e1 - 1);
    int base = dc;
    di = -1;
    for (;;) {
      // seg[base .. base + 63], clamped to the piece's end (seg[n1] = e1 > q): the row's
      // destination is the last entry <= q, inside this window when its last entry is > q
      const int wv = a.seg[min(base + lane, n1)];
      const int wlast = __builtin_amdgcn_readlane(wv, 63);
      int lo = 0;
#pragma unroll
      for (int st = 32; st; st >>= 1) {
        const int v = __shfl(wv, lo + st, 64);
        lo += v <= q ? st : 0;
      }
      if (di < 0 && wlast > q) di = base + lo;
      if (wlast > qmax) break;  // wave-uniform: every row resolved
      base += 63;               // seg[base + 63] <= q of every unresolved row
    }
    dc = __builtin_amdgcn_readlane(di, 31);
    const int b = a.beg[di], k = q - a.seg[di];
    sj = min(b + k + (k >= di - b ? 1 : 0), a.n_nodes - 1);
  };

  float run[2] = {0.f, 0.f};  // lane = features lane, lane + 64: the current destination's value
  int crow = a.n_nodes;       // its aggregate row; before the first destination the spare row
  int dc = n0, d_c, s_c, d_n = 0, s_n = 0;
  decode(e0, dc, d_c, s_c);
  for (int t0 = e0; t0 < e1; t0 += 32) {
    const int d = d_c;
    // ---- h = leaky(P[dst] + Q[src]) in accumulator order (features 32m + 8g + 4h .. + 3 at
    //      registers 4g .. 4g + 3 of tile m)
    f32x16 acc1[4];
    {
      const float* pp = a.pq + (size_t)d * PQW + 4 * h;
      const float* pqq = a.pq + (size_t)s_c * PQW + HID + 4 * h;
      f32x4 p[16], q[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) p[i] = *(const f32x4*)(pp + 8 * i);
#pragma unroll
      for (int i = 0; i < 16; ++i) q[i] = *(const f32x4*)(pqq + 8 * i);
      // the next tile's rows while these loads are in flight
      if (t0 + 32 < e1) decode(t0 + 32, dc, d_n, s_n);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc1[m][4 * g + t] = act_t<ACT_LEAKY>(p[4 * m + g][t] + q[4 * m + g][t]);
    }
    // destination-change mask of this tile's edges (bit j: edge t0 + j starts a segment)
    const int dprev = __shfl_up(d, 1, 64);
    const uint32_t smask = (uint32_t)__ballot(r == 0 ? d != crow : d != dprev) &
                           (e1 - t0 >= 32 ? 0xffffffffu : ((1u << (e1 - t0)) - 1u));
    // ---- m = leaky(W_1 h + b_1) (B operand = h's accumulators)
    f32x16 acc2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc2[m] = ld_bias_frag(bias1, m, h);
    layer_x3<8, 4, 4>(acc2, w1, 0, [&](int s) { return split_acc_of<P>(acc1[s >> 1], s & 1); });
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc2[m][i] = act_t<ACT_LEAKY>(acc2[m][i]);
    // ---- segmented reduction in edge order, TR edges per LDS pass: each edge one operation
    //      and one select; a destination change (a set bit of smask, wave-uniform) flushes the
    //      finished value to its row
    const int nv = min(32, e1 - t0);
#pragma unroll
    for (int c = 0; c < 32 / TR; ++c) {
      if (TR * c >= nv) break;  // wave-uniform
      if (r / TR == c) {
        float* row = T + (r % TR) * TS + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(f32x4*)(row + 32 * m + 8 * g) = (f32x4){acc2[m][4 * g], acc2[m][4 * g + 1],
                                                      acc2[m][4 * g + 2], acc2[m][4 * g + 3]};
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __builtin_amdgcn_wave_barrier();
      float v[TR][2];
#pragma unroll
      for (int j = 0; j < TR; ++j) {
        v[j][0] = T[j * TS + lane];
        v[j][1] = T[j * TS + 64 + lane];
      }
      const uint32_t pm = (smask >> (TR * c)) & ((1u << TR) - 1u);
      if (TR * c + TR > nv) {  // rows past the piece's end change nothing
#pragma unroll
        for (int j = 0; j < TR; ++j)
#pragma unroll
          for (int u = 0; u < 2; ++u) v[j][u] = TR * c + j < nv ? v[j][u] : NEUTRAL;
      }
      // rv[j] = the running value after edge TR c + j (a set bit restarts it)
      float rv[TR][2];
#pragma unroll
      for (int j = 0; j < TR; ++j)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float prev = j == 0 ? run[u] : rv[j - 1][u];
          const float nx = RED == RED_MAX ? fmaxf(prev, v[j][u]) : prev + v[j][u];
          rv[j][u] = ((pm >> j) & 1u) ? v[j][u] : nx;
        }
      // at a set bit j the value before it belongs to the destination that ended there
      for (uint32_t m = pm; m; m &= m - 1) {
        const int j = __builtin_ctz(m);
        float fin[2] = {run[0], run[1]};
#pragma unroll
        for (int k = 0; k + 1 < TR; ++k)
#pragma unroll
          for (int u = 0; u < 2; ++u) fin[u] = (j == k + 1) ? rv[k][u] : fin[u];
        a.agg[(size_t)crow * C + lane] = fin[0];
        a.agg[(size_t)crow * C + 64 + lane] = fin[1];
        crow = __builtin_amdgcn_readlane(d, TR * c + j);
      }
      run[0] = rv[TR - 1][0];
      run[1] = rv[TR - 1][1];
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
    d_c = d_n;
    s_c = s_n;
  }
  a.agg[(size_t)crow * C + lane] = run[0];
  a.agg[(size_t)crow * C + 64 + lane] = run[1];
}

// ------------------------------------------------------------------ node launch
// x_out = x + leaky(W_u cat(x, agg) + b_u): W_u packed FAST_IN (K = 256, N = 128), streamed
// from L2; lane r = node, one 32-node tile per wave and step
template <typename P, int RED>
__global__ __launch_bounds__(NFT) void cls_node_kernel(const float* x, int ldx,
                                                       const float* agg,
                                                       const int* siz, int n_nodes,
                                                       const char* wu,
                                                       float* x_out, int ldo) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const WBuf W = wbuf(wu, P::image_bytes(2 * C, C), plane_bytes(2 * C, C), lane);
  const float* bias = (const float*)(wu + P::NP * plane_bytes(2 * C, C));
  const int ntiles = (n_nodes + 31) / 32;
  for (int t = blockIdx.x * (NFT / 64) + wave; t < ntiles; t += gridDim.x * (NFT / 64)) {
    const int node = t * 32 + r;
    const bool valid = node < n_nodes;
    const int nrow = valid ? node : n_nodes - 1;
    const int deg = siz[nrow] - 1;
    const float* px = x + (size_t)nrow * ldx;
    const float* pa = agg + (size_t)nrow * C + 8 * h;
    // x[node] and agg[node] in k order (features 16 s + 8 h .. + 7)
    f32x4 xb[8][2];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      xb[s][0] = *(const f32x4*)(px + 8 * h + 16 * s);
      xb[s][1] = *(const f32x4*)(px + 8 * h + 16 * s + 4);
    }
    // agg[node] is read k-step by k-step beside the MFMAs (its 64 registers would not fit
    // next to x's).  A node without incoming edges (a one-member object) has no row in the
    // scratch: PyG leaves its aggregate at zero
    auto agg_rows = [&](int s, int u) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (deg > 0) v = *(const f32x4*)(pa + 16 * s + 4 * u);
      if (RED == RED_MEAN && deg > 0) {
        const float sc = (float)deg;
        v = (f32x4){div_rn(v.x, sc), div_rn(v.y, sc), div_rn(v.z, sc), div_rn(v.w, sc)};
      }
      return v;
    };
    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = ld_bias_frag(bias, m, h);
    layer_x3<16, 4, 4>(acc, W, 0, [&](int s) {
      return s < 8 ? P::split(xb[s][0], xb[s][1]) : P::split(agg_rows(s - 8, 0), agg_rows(s - 8, 1));
    });
    if (valid) {
      // the residual in accumulator order (features 32m + 8g + 4h .. + 3): a re-read of the
      // row just loaded
      float* po = x_out + (size_t)node * ldo + 4 * h;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 xi = *(const f32x4*)(px + 4 * h + 32 * m + 8 * g);
          f32x4 o;
#pragma unroll
          for (int u = 0; u < 4; ++u) o[u] = xi[u] + act_t<ACT_LEAKY>(acc[m][4 * g + u]);
          *(f32x4*)(po + 32 * m + 8 * g) = o;
        }
    }
  }
}

// the projection and the edge launch: P | Q to pq [N][256], the raw aggregate (a sum or a
// maximum; rows of nodes without edges unwritten) to agg [N + 1][128]
template <typename P, int RED>
static int launch_edge_phase(const rg_layer* layers, const float* x, int ldx, const Tab& tb,
                             int n_nodes, float* pq, float* agg, hipStream_t st) {
  const int tiles = (n_nodes + 31) / 32;
  const int nblk = (tiles + NFT / 64 - 1) / (NFT / 64) < 1024 ? (tiles + NFT / 64 - 1) / (NFT / 64) : 1024;
  cls_proj_kernel<P><<<nblk, NFT, 0, st>>>(x, ldx, n_nodes, (const char*)layers[0].w_packed, pq);
  RG_LAUNCH_CHECK();
  EArgs a;
  a.pq = pq;
  a.seg = tb.seg;
  a.beg = tb.beg;
  a.siz = tb.siz;
  a.wtab = tb.wtab;
  a.agg = agg;
  a.w1 = (const char*)layers[1].w_packed;
  a.n_nodes = n_nodes;
  auto edge = cls_edge_kernel<P, RED == RED_MAX ? RED_MAX : RED_SUM>;
  RG_ENSURE_LDS(edge, Lay<P>::LDS);
  edge<<<edge_groups(n_nodes), FT, Lay<P>::LDS, st>>>(a);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

template <typename P, int RED>
static int launch_layer(const rg_layer* layers, const float* x, int ldx, const Tab& tb, int n_nodes,
                        float* x_out, int ld_out, float* pq, float* agg, hipStream_t st) {
  const int rc = launch_edge_phase<P, RED>(layers, x, ldx, tb, n_nodes, pq, agg, st);
  if (rc != RG_OK) return rc;
  const int tiles = (n_nodes + 31) / 32;
  const int nblk = (tiles + NFT / 64 - 1) / (NFT / 64) < 1024 ? (tiles + NFT / 64 - 1) / (NFT / 64) : 1024;
  cls_node_kernel<P, RED><<<nblk, NFT, 0, st>>>(x, ldx, agg, tb.siz, n_nodes,
                                                (const char*)layers[2].w_packed, x_out, ld_out);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

// The aggregate as the update MLP reads it (cls_node_kernel's agg_rows, written out for the
// training tape): `mean` divided by n_o - 1, a one-member object's row zero.  One thread per
// four features.
template <int RED>
__global__ void cls_agg_finish_kernel(const float* __restrict__ raw, const int* __restrict__ siz,
                                      int n_nodes, float* __restrict__ agg) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_nodes * (C / 4)) return;
  const int node = (int)(t / (C / 4));
  const int deg = siz[node] - 1;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (deg > 0) v = ((const f32x4*)raw)[t];
  if (RED == RED_MEAN && deg > 0) {
    const float sc = (float)deg;
    v = (f32x4){div_rn(v.x, sc), div_rn(v.y, sc), div_rn(v.z, sc), div_rn(v.w, sc)};
  }
  ((f32x4*)agg)[t] = v;
}

}  // namespace clsx3
}  // namespace rg

using namespace rg;
using namespace rg::clsx3;

static size_t align256_t(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" size_t rg_cls_object_table_bytes(int n_nodes, int n_obj) {
  (void)n_obj;
  return tab_ints(n_nodes) * sizeof(int);
}

extern "C" size_t rg_cls_object_table_workspace_size(int n_obj) {
  const size_t n = n_obj > 0 ? n_obj : 0;
  return 4 * align256_t((n + 1) * sizeof(int)) + align256_t(scan_workspace_bytes((long)n));
}

extern "C" int rg_cls_object_table(const int64_t* object_size, int n_obj, int n_nodes, long n_edges,
                                   int* table, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  RG_REQUIRE(n_obj >= 0 && n_nodes >= 0 && n_edges >= 0 && table && (object_size || n_obj == 0),
             RG_ERR_ARG, "rg_cls_object_table: bad arguments");
  RG_REQUIRE(n_edges < (1L << 31), RG_ERR_ARG,
             "rg_cls_object_table: n_edges=%ld does not fit the int32 segment table", n_edges);
  RG_REQUIRE(workspace_bytes >= rg_cls_object_table_workspace_size(n_obj) && (workspace || n_obj == 0),
             RG_ERR_ARG, "rg_cls_object_table: workspace too small");
  if (n_nodes == 0) return RG_OK;
  hipStream_t st = (hipStream_t)stream;
  const Tab tb = tab_of(table, n_nodes);
  char* w = (char*)workspace;
  const size_t a = align256_t(((size_t)n_obj + 1) * sizeof(int));
  int* sz = (int*)w;
  int* pairs = (int*)(w + a);
  int* node_off = (int*)(w + 2 * a);
  int* edge_off = (int*)(w + 3 * a);
  void* sws = w + 4 * a;
  if (n_obj > 0) {
    sizes_kernel<<<ceil_div(n_obj, 256), 256, 0, st>>>(object_size, n_obj, sz, pairs);
    RG_LAUNCH_CHECK();
    int rc = exclusive_scan(sz, n_obj, node_off, nullptr, sws, st);
    if (rc) return rc;
    rc = exclusive_scan(pairs, n_obj, edge_off, nullptr, sws, st);
    if (rc) return rc;
  }
  nodes_kernel<<<ceil_div((long)n_nodes + 1, 256), 256, 0, st>>>(node_off, edge_off, n_obj, n_nodes,
                                                                tb.seg, tb.beg, tb.siz);
  RG_LAUNCH_CHECK();
  const int W = edge_groups(n_nodes) * NW;
  waves_kernel<<<(W + 256) / 256, 256, 0, st>>>(tb.seg, n_nodes, W, tb.wtab);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" size_t rg_cls_conv_layer_x3_workspace_size(int n_nodes, int n_obj) {
  (void)n_obj;
  const size_t n = n_nodes > 0 ? n_nodes : 0;
  // P | Q [N][256] and the aggregate rows [N + 1][128]
  return align256_t(n * PQW * sizeof(float)) + align256_t((n + 1) * C * sizeof(float));
}

extern "C" int rg_cls_conv_layer_x3(const rg_layer* layers, int aggr, const float* x, int ldx,
                                    const int* table, int n_nodes, int n_obj, float* x_out,
                                    int ld_out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  RG_REQUIRE(layers, RG_ERR_ARG, "rg_cls_conv_layer_x3: layers is NULL");
  const rg_layer& pq = layers[0];
  const rg_layer& m1 = layers[1];
  const rg_layer& u = layers[2];
  RG_REQUIRE(pq.in_dim == C && pq.out_dim == PQW && m1.in_dim == HID && m1.out_dim == C &&
                 u.in_dim == 2 * C && u.out_dim == C,
             RG_ERR_UNSUPPORTED,
             "rg_cls_conv_layer_x3: compiled for 128 -> 256 (P | Q), 128 -> 128, 256 -> 128");
  RG_REQUIRE(!pq.norm_mu && !m1.norm_mu && !u.norm_mu && pq.act == ACT_LEAKY &&
                 m1.act == ACT_LEAKY && u.act == ACT_LEAKY,
             RG_ERR_UNSUPPORTED, "rg_cls_conv_layer_x3: un-normalised LeakyReLU layers only");
  RG_REQUIRE(aggr == RG_REDUCE_SUM || aggr == RG_REDUCE_MEAN || aggr == RG_REDUCE_MAX,
             RG_ERR_UNSUPPORTED, "rg_cls_conv_layer_x3: aggregation %d", aggr);
  RG_REQUIRE(!((pq.flags | m1.flags | u.flags) & RG_LAYER_CENTERED), RG_ERR_UNSUPPORTED,
             "rg_cls_conv_layer_x3: images are packed un-centred");
  RG_REQUIRE(ldx % 4 == 0 && ld_out % 4 == 0 && ldx >= C && ld_out >= C, RG_ERR_UNSUPPORTED,
             "rg_cls_conv_layer_x3: row strides must be multiples of 4, at least 128");
  RG_REQUIRE(!((pq.flags | m1.flags | u.flags) & (RG_LAYER_H2 | RG_LAYER_F16)), RG_ERR_ARG,
             "rg_cls_conv_layer_x3: RG_PACK_X3 images only (the classifier's activations leave "
             "the h2 domain)");
  RG_REQUIRE(x != x_out, RG_ERR_ARG, "rg_cls_conv_layer_x3: x_out must not alias x");
  RG_REQUIRE(workspace_bytes >= rg_cls_conv_layer_x3_workspace_size(n_nodes, n_obj), RG_ERR_ARG,
             "rg_cls_conv_layer_x3: workspace too small");
  if (n_nodes <= 0) return RG_OK;
  RG_REQUIRE(x && x_out && table && workspace && pq.w_packed && m1.w_packed && u.w_packed, RG_ERR_ARG,
             "rg_cls_conv_layer_x3: NULL argument");
  const Tab tb = tab_of(const_cast<int*>(table), n_nodes);
  float* pqr = (float*)workspace;
  float* agg = (float*)((char*)workspace + align256_t((size_t)n_nodes * PQW * sizeof(float)));
  hipStream_t st = (hipStream_t)stream;
  if (aggr == RG_REDUCE_MAX)
    return launch_layer<B3, RED_MAX>(layers, x, ldx, tb, n_nodes, x_out, ld_out, pqr, agg, st);
  if (aggr == RG_REDUCE_MEAN)
    return launch_layer<B3, RED_MEAN>(layers, x, ldx, tb, n_nodes, x_out, ld_out, pqr, agg, st);
  return launch_layer<B3, RED_SUM>(layers, x, ldx, tb, n_nodes, x_out, ld_out, pqr, agg, st);
}

extern "C" size_t rg_cls_conv_aggregate_x3_workspace_size(int n_nodes) {
  const size_t n = n_nodes > 0 ? n_nodes : 0;
  return align256_t((n + 1) * C * sizeof(float));  // the edge launch's raw rows [N + 1][128]
}

extern "C" int rg_cls_conv_aggregate_x3(const rg_layer* layers, int aggr, const float* x, int ldx,
                                        const int* table, int n_nodes, float* pq, float* agg,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  RG_REQUIRE(layers, RG_ERR_ARG, "rg_cls_conv_aggregate_x3: layers is NULL");
  const rg_layer& lp = layers[0];
  const rg_layer& m1 = layers[1];
  RG_REQUIRE(lp.in_dim == C && lp.out_dim == PQW && m1.in_dim == HID && m1.out_dim == C,
             RG_ERR_UNSUPPORTED, "rg_cls_conv_aggregate_x3: compiled for 128 -> 256 (P | Q), 128 -> 128");
  RG_REQUIRE(!lp.norm_mu && !m1.norm_mu && lp.act == ACT_LEAKY && m1.act == ACT_LEAKY,
             RG_ERR_UNSUPPORTED, "rg_cls_conv_aggregate_x3: un-normalised LeakyReLU layers only");
  RG_REQUIRE(aggr == RG_REDUCE_SUM || aggr == RG_REDUCE_MEAN, RG_ERR_UNSUPPORTED,
             "rg_cls_conv_aggregate_x3: aggregation %d (sum and mean have a fused backward)", aggr);
  RG_REQUIRE(!((lp.flags | m1.flags) & RG_LAYER_CENTERED), RG_ERR_UNSUPPORTED,
             "rg_cls_conv_aggregate_x3: images are packed un-centred");
  RG_REQUIRE(ldx % 4 == 0 && ldx >= C, RG_ERR_UNSUPPORTED,
             "rg_cls_conv_aggregate_x3: the row stride must be a multiple of 4, at least 128");
  RG_REQUIRE(!((lp.flags | m1.flags) & (RG_LAYER_H2 | RG_LAYER_F16)), RG_ERR_ARG,
             "rg_cls_conv_aggregate_x3: RG_PACK_X3 images only (the classifier's activations "
             "leave the h2 domain)");
  RG_REQUIRE((const void*)x != (const void*)pq && (const void*)x != (const void*)agg &&
                 pq != agg && (void*)pq != workspace && (void*)agg != workspace,
             RG_ERR_ARG, "rg_cls_conv_aggregate_x3: x, pq, agg and the workspace must not alias");
  RG_REQUIRE(workspace_bytes >= rg_cls_conv_aggregate_x3_workspace_size(n_nodes), RG_ERR_ARG,
             "rg_cls_conv_aggregate_x3: workspace too small");
  if (n_nodes <= 0) return RG_OK;
  RG_REQUIRE(x && pq && agg && table && workspace && lp.w_packed && m1.w_packed, RG_ERR_ARG,
             "rg_cls_conv_aggregate_x3: NULL argument");
  const Tab tb = tab_of(const_cast<int*>(table), n_nodes);
  float* raw = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_edge_phase<B3, RED_SUM>(layers, x, ldx, tb, n_nodes, pq, raw, st);
  if (rc != RG_OK) return rc;
  const int nblk = ceil_div((long)n_nodes * (C / 4), 256);
  if (aggr == RG_REDUCE_MEAN)
    cls_agg_finish_kernel<RED_MEAN><<<nblk, 256, 0, st>>>(raw, tb.siz, n_nodes, agg);
  else
    cls_agg_finish_kernel<RED_SUM><<<nblk, 256, 0, st>>>(raw, tb.siz, n_nodes, agg);
  RG_LAUNCH_CHECK();
  return RG_OK;
}
