// Backward of the edge phase of the classifier's conv block over complete object graphs
// (forward: cls_conv_x3.hip), straight from the object table: no edge array, no E-sized tape.
//     m_ij = leaky(W_1 leaky(P[i] + Q[j]) + b_1),  agg_i = AGG_j m_ij
// Given P | Q [N][256] and d agg [N][128], rg_cls_conv_backward_x3 forms d P | d Q [N][256] and
// adds d W_1, d b_1:
//  * cls_bwd_kernel<ROLE>: the skeleton of cls_edge_kernel (pieces of whole owners with equal
//    edge counts, one per wave; 32-edge tiles; the closed-form partner; the wave-private LDS
//    transposition and the in-order running sum that restarts at each owner change).  Per tile
//        z0 = P[i] + Q[j], h = leaky(z0), z1 = W_1 h + b_1                 (recomputed)
//        dm = d agg[i] leaky'(z1)   (mean: times 1 / (n_o - 1))
//        dz0 = (W_1^T dm) leaky'(z0)
//    dm stays in the accumulator registers, the B operand of the second product as h is of the
//    first.  ROLE_DST: owner = destination i, partner = source j, the sum over the owner's
//    tile rows is d P[i].  ROLE_SRC: owner = j, partner = i -- the graph is symmetric, so the
//    source-major walk is the same table with the roles swapped -- and the sum is d Q[j].
//    Every owner lies whole in one wave and is summed in ascending partner order: no atomics,
//    bits independent of the rest of the batch and of where the pieces are cut.
//    W_1's planes sit in LDS; W_1^T's (as large again: both do not fit) are streamed from L2
//    through a buffer resource.  Unlike the forward the pieces are cut inside the kernel (two
//    uniform binary searches per wave over seg_ptr), so that a launch can take a part of the
//    edge sequence.
//  * d W_1 += sum_e dm_e h_e^T, d b_1 += sum_e dm_e contract over edges, which are lanes in
//    the accumulator layout.  The ROLE_DST pass runs in chunks of whole destinations of at most
//    CHUNK + max_degree edges, writes each chunk's dm and h rows to a workspace of that constant
//    size, and rg_linear_grad (exact f32 products, fixed reduction order) adds the chunk's
//    product.
// Scheme b3 only (x3_common.h), as the forward.
#include <type_traits>

#ifndef RG_X3_SPLIT
#define RG_X3_SPLIT 4  // builtin conversions in the splits, as cls_conv_x3.hip
#endif
#include "cls_conv_common.h"
#include "x3_common.h"

namespace rg {
namespace clsx3 {

using namespace ::rg::x3;

static constexpr long CHUNK = 1L << 17;  // edge rows of a dm / h tape chunk, less max_degree
// four waves, one per SIMD: z1 / dm, dz0, the signs of z0 and the gathered rows in flight need
// more than the 256 registers a wave has at two per SIMD (the forward's launch: 6 to 19 spilled)
static constexpr int BFT = 256;
static constexpr int BNW = BFT / 64;
enum { ROLE_DST = 0, ROLE_SRC = 1 };

template <typename P>
struct BLay {
  static constexpr int W1 = P::image_bytes(HID, C);
  static constexpr int LDS = al16(W1) + BNW * T_BYTES;
  static_assert(LDS <= DYN_LDS_MAX, "cls_conv_bwd_x3 LDS");
};

struct BArgs {
  const float* pq;    // [N][256]
  const float* dagg;  // [N][ld_dagg], 128 wide
  const int* seg;     // [N + 1]
  const int* beg;     // [N]
  const int* siz;     // [N]
  float* dpq;         // [N][256]: columns [0, 128) of ROLE_DST, [128, 256) of ROLE_SRC
  float* spare;       // [128]: takes the flush before a piece's first owner
  const char* w1;     // msg1, FAST_CHAIN
  const char* w1t;    // msg1 transposed (128 -> 128, no bias), FAST_CHAIN
  float* tape_h;      // ROLE_DST: [tape_rows][128] h and dm of this launch's edges
  float* tape_dm;
  long tape_rows;
  int ld_dagg;
  int n_nodes;
  int q_lo, q_hi;     // the launch takes the owners whose segment starts in [q_lo, q_hi)
};

// first n in [lo, hi] with seg[n] >= target (hi when none)
__device__ __forceinline__ int lower_seg(const int* seg, int lo, int hi, int target) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename P, int ROLE, bool MEAN>
__global__ __launch_bounds__(BFT) void cls_bwd_kernel(BArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  stage_lds<BFT>(lds, a.w1, BLay<P>::W1);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  float* T = (float*)(lds + al16(BLay<P>::W1) + wave * T_BYTES);  // [TR][TS] dz0 rows
  const WLds w1{lds + lane * 16, plane_bytes(HID, C)};
  const float* bias1 = (const float*)(lds + P::NP * plane_bytes(HID, C));
  const WBuf w1t = wbuf(a.w1t, P::image_bytes(C, HID), plane_bytes(C, HID), lane);
  constexpr int OFF = ROLE == ROLE_SRC ? HID : 0;

  // this launch's owners [na, nb) and this wave's piece of them: equal edge counts, whole owners
  const int na = lower_seg(a.seg, 0, a.n_nodes, a.q_lo);
  const int nb = lower_seg(a.seg, na, a.n_nodes, a.q_hi);
  const int ea = a.seg[na], eb = a.seg[nb];
  if (ea >= eb) return;
  const int W = gridDim.x * BNW, piece = blockIdx.x * BNW + wave;
  const int c0 = ea + (int)((long)(eb - ea) * piece / W);
  const int c1 = ea + (int)((long)(eb - ea) * (piece + 1) / W);
  const int n0 = __builtin_amdgcn_readfirstlane(lower_seg(a.seg, na, nb, c0));
  const int n1 = __builtin_amdgcn_readfirstlane(piece + 1 == W ? nb : lower_seg(a.seg, na, nb, c1));
  if (n0 >= n1) return;
  const int e0 = __builtin_amdgcn_readfirstlane(a.seg[n0]);
  const int e1 = __builtin_amdgcn_readfirstlane(a.seg[n1]);
  if (e0 >= e1) return;

  // (owner, partner) of this lane's row of the tile at position t: cls_edge_kernel's decode
  auto decode = [&](int t, int& dc, int& di, int& sj) {
    const int q = min(t + r, e1 - 1);
    const int qmax = min(t + 31, e1 - 1);
    int base = dc;
    di = -1;
    for (;;) {
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
      base += 63;
    }
    dc = __builtin_amdgcn_readlane(di, 31);
    const int b = a.beg[di], k = q - a.seg[di];
    sj = min(b + k + (k >= di - b ? 1 : 0), a.n_nodes - 1);
  };
  auto out_row = [&](int row) {
    return row == a.n_nodes ? a.spare : a.dpq + (size_t)row * PQW + OFF;
  };

  float run[2] = {0.f, 0.f};  // lane = features lane, lane + 64: the current owner's sum
  int crow = a.n_nodes;       // its row; before the first owner the spare row
  int dc = n0, d_c, s_c, d_n = 0, s_n = 0;
  decode(e0, dc, d_c, s_c);
  for (int t0 = e0; t0 < e1; t0 += 32) {
    const int d = d_c;
    const int ip = ROLE == ROLE_DST ? d : s_c;  // the edge's destination: P and d agg
    const int iq = ROLE == ROLE_DST ? s_c : d;  // its source: Q
    const bool live = t0 + r < e1;              // rows past the piece's last edge repeat it
    // ---- z0 = P[i] + Q[j] and h = leaky(z0) in accumulator order; z0's signs in two masks
    f32x16 acc1[4];
    uint32_t pos0[2] = {0u, 0u};
    {
      const float* pp = a.pq + (size_t)ip * PQW + 4 * h;
      const float* pqq = a.pq + (size_t)iq * PQW + HID + 4 * h;
      f32x4 p[16], q[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) p[i] = *(const f32x4*)(pp + 8 * i);
#pragma unroll
      for (int i = 0; i < 16; ++i) q[i] = *(const f32x4*)(pqq + 8 * i);
      if (t0 + 32 < e1) decode(t0 + 32, dc, d_n, s_n);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float z = p[4 * m + g][t] + q[4 * m + g][t];
            pos0[m >> 1] |= z > 0.f ? 1u << (16 * (m & 1) + 4 * g + t) : 0u;
            acc1[m][4 * g + t] = act_t<ACT_LEAKY>(z);
          }
    }
    const size_t trow = (size_t)(t0 + r - ea);
    const bool taped = ROLE == ROLE_DST && live && (long)trow < a.tape_rows;
    if (ROLE == ROLE_DST && taped) {
      float* ph = a.tape_h + trow * HID + 4 * h;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(f32x4*)(ph + 32 * m + 8 * g) = (f32x4){acc1[m][4 * g], acc1[m][4 * g + 1],
                                                   acc1[m][4 * g + 2], acc1[m][4 * g + 3]};
    }
    // owner-change mask of this tile's edges (bit j: edge t0 + j starts a segment)
    const int dprev = __shfl_up(d, 1, 64);
    const uint32_t smask = (uint32_t)__ballot(r == 0 ? d != crow : d != dprev) &
                           (e1 - t0 >= 32 ? 0xffffffffu : ((1u << (e1 - t0)) - 1u));
    // ---- z1 = W_1 h + b_1 (B operand = h's accumulators)
    f32x16 acc2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc2[m] = ld_bias_frag(bias1, m, h);
    layer_x3<8, 4, 4>(acc2, w1, 0, [&](int s) { return split_acc_of<P>(acc1[s >> 1], s & 1); });
    // ---- dm = d agg[i] leaky'(z1), in place of z1
    {
      const float* pg = a.dagg + (size_t)ip * a.ld_dagg + 4 * h;
      float sc = 1.f;
      if (MEAN) sc = div_rn(1.f, (float)max(a.siz[ip] - 1, 1));
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 gv = *(const f32x4*)(pg + 32 * m + 8 * g);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float gs = MEAN ? gv[t] * sc : gv[t];
            acc2[m][4 * g + t] = acc2[m][4 * g + t] > 0.f ? gs : gs * 0.01f;
          }
        }
    }
    if (ROLE == ROLE_DST && taped) {
      float* pd = a.tape_dm + trow * C + 4 * h;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(f32x4*)(pd + 32 * m + 8 * g) = (f32x4){acc2[m][4 * g], acc2[m][4 * g + 1],
                                                   acc2[m][4 * g + 2], acc2[m][4 * g + 3]};
    }
    // ---- dz0 = (W_1^T dm) leaky'(z0) (B operand = dm's accumulators)
    f32x16 acc3[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc3[m][i] = 0.f;
    layer_x3<8, 4, 4>(acc3, w1t, 0, [&](int s) { return split_acc_of<P>(acc2[s >> 1], s & 1); });
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc3[m][i] = ((pos0[m >> 1] >> (16 * (m & 1) + i)) & 1u) ? acc3[m][i] : acc3[m][i] * 0.01f;
    // ---- segmented sum in edge order, TR edges per LDS pass (cls_edge_kernel's reduction)
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
            *(f32x4*)(row + 32 * m + 8 * g) = (f32x4){acc3[m][4 * g], acc3[m][4 * g + 1],
                                                      acc3[m][4 * g + 2], acc3[m][4 * g + 3]};
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
          for (int u = 0; u < 2; ++u) v[j][u] = TR * c + j < nv ? v[j][u] : 0.f;
      }
      // rv[j] = the running sum after edge TR c + j (a set bit restarts it)
      float rv[TR][2];
#pragma unroll
      for (int j = 0; j < TR; ++j)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float prev = j == 0 ? run[u] : rv[j - 1][u];
          rv[j][u] = ((pm >> j) & 1u) ? v[j][u] : prev + v[j][u];
        }
      // at a set bit j the sum before it belongs to the owner that ended there
      for (uint32_t m = pm; m; m &= m - 1) {
        const int j = __builtin_ctz(m);
        float fin[2] = {run[0], run[1]};
#pragma unroll
        for (int k = 0; k + 1 < TR; ++k)
#pragma unroll
          for (int u = 0; u < 2; ++u) fin[u] = (j == k + 1) ? rv[k][u] : fin[u];
        float* po = out_row(crow);
        po[lane] = fin[0];
        po[64 + lane] = fin[1];
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
  float* po = out_row(crow);
  po[lane] = run[0];
  po[64 + lane] = run[1];
}

static size_t align256_b(size_t v) { return (v + 255) & ~(size_t)255; }

struct BWs {
  size_t spare, tape_h, tape_dm, lgrad, lgrad_bytes, total;
  long rows;  // of a tape
};
static BWs bws_of(int max_degree) {
  BWs w;
  w.rows = CHUNK + (max_degree > 0 ? max_degree : 0);
  w.spare = 0;
  w.tape_h = align256_b(C * sizeof(float));
  w.tape_dm = w.tape_h + align256_b((size_t)w.rows * HID * sizeof(float));
  w.lgrad = w.tape_dm + align256_b((size_t)w.rows * C * sizeof(float));
  // rg_linear_grad's partials: their count is bounded, whatever the rows
  w.lgrad_bytes = align256_b(rg_linear_grad_workspace_size(1L << 30, C, HID));
  w.total = w.lgrad + w.lgrad_bytes;
  return w;
}

template <typename P, int ROLE, bool MEAN>
static int launch_bwd(BArgs a, long n_edges_launch, hipStream_t st) {
  // a piece of >= 4 tiles per wave, one workgroup per CU at most
  long g = (n_edges_launch + (long)BNW * 128 - 1) / ((long)BNW * 128);
  g = g < 1 ? 1 : g > GMAX ? GMAX : g;
  auto k = cls_bwd_kernel<P, ROLE, MEAN>;
  RG_ENSURE_LDS(k, BLay<P>::LDS);
  k<<<(int)g, BFT, BLay<P>::LDS, st>>>(a);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

template <bool MEAN>
static int run_bwd(BArgs a, long n_edges, int max_degree, float* d_w1, float* d_b1, char* ws,
                   const BWs& w, hipStream_t st) {
  RG_CHECK_HIP(hipMemsetAsync(a.dpq, 0, (size_t)a.n_nodes * PQW * sizeof(float), st));
  if (n_edges <= 0) return RG_OK;
  a.spare = (float*)(ws + w.spare);
  a.tape_h = a.tape_dm = nullptr;
  a.tape_rows = 0;
  a.q_lo = 0;
  a.q_hi = (int)n_edges;
  int rc = launch_bwd<B3, ROLE_SRC, MEAN>(a, n_edges, st);
  if (rc != RG_OK) return rc;
  a.tape_h = (float*)(ws + w.tape_h);
  a.tape_dm = (float*)(ws + w.tape_dm);
  for (long q = 0; q < n_edges; q += CHUNK) {
    const long len = n_edges - q < CHUNK ? n_edges - q : CHUNK;
    // the chunk's owners start in [q, q + len): between len - max_degree and len + max_degree
    // of their edges' rows are written; the rows that may stay unwritten are zeroed (dm: no
    // contribution; h: finite)
    const long rows = len + max_degree;
    const long z0 = len - max_degree > 0 ? len - max_degree : 0;
    RG_CHECK_HIP(hipMemsetAsync(a.tape_h + z0 * HID, 0, (size_t)(rows - z0) * HID * sizeof(float), st));
    RG_CHECK_HIP(hipMemsetAsync(a.tape_dm + z0 * C, 0, (size_t)(rows - z0) * C * sizeof(float), st));
    a.tape_rows = rows;
    a.q_lo = (int)q;
    a.q_hi = (int)(q + len);
    rc = launch_bwd<B3, ROLE_DST, MEAN>(a, len, st);
    if (rc != RG_OK) return rc;
    rc = rg_linear_grad(a.tape_dm, C, rows, C, HID, RG_IN_DENSE, a.tape_h, HID, HID, nullptr, 0, 0,
                        nullptr, 0, 0, nullptr, nullptr, d_w1, d_b1, ws + w.lgrad, w.lgrad_bytes, st);
    if (rc != RG_OK) return rc;
  }
  return RG_OK;
}

}  // namespace clsx3
}  // namespace rg

using namespace rg;
using namespace rg::clsx3;

extern "C" size_t rg_cls_conv_backward_x3_workspace_size(int n_nodes, int max_degree) {
  (void)n_nodes;
  return bws_of(max_degree).total;
}

extern "C" int rg_cls_conv_backward_x3(const rg_layer* layers, int aggr, const float* pq,
                                       const float* d_agg, int ld_dagg, const int* table,
                                       int n_nodes, long n_edges, int max_degree, float* d_pq,
                                       float* d_w1, float* d_b1, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  RG_REQUIRE(layers, RG_ERR_ARG, "rg_cls_conv_backward_x3: layers is NULL");
  const rg_layer& m1 = layers[0];
  const rg_layer& m1t = layers[1];
  RG_REQUIRE(m1.in_dim == HID && m1.out_dim == C && m1t.in_dim == C && m1t.out_dim == HID,
             RG_ERR_UNSUPPORTED, "rg_cls_conv_backward_x3: compiled for 128 -> 128 and its transpose");
  RG_REQUIRE(!m1.norm_mu && !m1t.norm_mu && m1.act == ACT_LEAKY, RG_ERR_UNSUPPORTED,
             "rg_cls_conv_backward_x3: an un-normalised LeakyReLU layer only");
  RG_REQUIRE(aggr == RG_REDUCE_SUM || aggr == RG_REDUCE_MEAN, RG_ERR_UNSUPPORTED,
             "rg_cls_conv_backward_x3: aggregation %d (max needs the messages)", aggr);
  RG_REQUIRE(!((m1.flags | m1t.flags) & RG_LAYER_CENTERED), RG_ERR_UNSUPPORTED,
             "rg_cls_conv_backward_x3: images are packed un-centred");
  RG_REQUIRE(ld_dagg % 4 == 0 && ld_dagg >= C, RG_ERR_UNSUPPORTED,
             "rg_cls_conv_backward_x3: d_agg's row stride must be a multiple of 4, at least 128");
  RG_REQUIRE(!((m1.flags | m1t.flags) & (RG_LAYER_H2 | RG_LAYER_F16)), RG_ERR_ARG,
             "rg_cls_conv_backward_x3: RG_PACK_X3 images only (the classifier's activations "
             "leave the h2 domain)");
  RG_REQUIRE(n_nodes >= 0 && n_edges >= 0 && n_edges < (1L << 31) && max_degree >= 0, RG_ERR_ARG,
             "rg_cls_conv_backward_x3: bad counts (n_edges must fit int32)");
  {
    // every output against every input, the other outputs and the workspace
    const void* outs[3] = {d_pq, d_w1, d_b1};
    const void* ins[3] = {pq, d_agg, workspace};
    bool alias = false;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) alias |= outs[i] && outs[i] == ins[j];
      for (int j = i + 1; j < 3; ++j) alias |= outs[i] && outs[i] == outs[j];
    }
    alias |= workspace && (workspace == (const void*)pq || workspace == (const void*)d_agg);
    RG_REQUIRE(!alias, RG_ERR_ARG,
               "rg_cls_conv_backward_x3: outputs must not alias inputs, each other or the "
               "workspace");
  }
  const BWs w = bws_of(max_degree);
  RG_REQUIRE(workspace_bytes >= w.total, RG_ERR_ARG, "rg_cls_conv_backward_x3: workspace too small");
  if (n_nodes <= 0) return RG_OK;
  RG_REQUIRE(pq && d_agg && table && d_pq && d_w1 && d_b1 && workspace && m1.w_packed &&
                 m1t.w_packed,
             RG_ERR_ARG, "rg_cls_conv_backward_x3: NULL argument");
  const Tab tb = tab_of(const_cast<int*>(table), n_nodes);
  BArgs a;
  a.pq = pq;
  a.dagg = d_agg;
  a.seg = tb.seg;
  a.beg = tb.beg;
  a.siz = tb.siz;
  a.dpq = d_pq;
  a.w1 = (const char*)m1.w_packed;
  a.w1t = (const char*)m1t.w_packed;
  a.ld_dagg = ld_dagg;
  a.n_nodes = n_nodes;
  hipStream_t st = (hipStream_t)stream;
  if (aggr == RG_REDUCE_MEAN)
    return run_bwd<true>(a, n_edges, max_degree, d_w1, d_b1, (char*)workspace, w, st);
  return run_bwd<false>(a, n_edges, max_degree, d_w1, d_b1, (char*)workspace, w, st);
}
