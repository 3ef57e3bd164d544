// Graph attention (GATv2Conv as residual_graph_attn_block uses it,
// modules/neural_net/gnn/gnn_attention.py:26-36, 72), forward only, float32.
//
//   m_k   = xl[src[k]] + xr[i] + e_k W_e^T            edge k of destination i, [H][C]
//   a_kh  = sum_c att[h][c] leaky_relu(m_k[h][c])
//   w_kh  = softmax of a_kh over the incoming edges of i (per head)
//   out_i = concat_h sum_k w_kh xl[src[k]][h][:] + bias
//
// PyG evaluates this through three [E][H C] tensors.  Here a layer is two launches and the
// only per-edge buffer is the logits [E][H]:
//
//  1. gat_logits_kernel.  A tile is 32 edges; a wave owns ONE head of it.  Y^T = W_e . e^T on
//     v_mfma_f32_32x32x2_f32 (exact f32 products), so lane (r = lane & 31, h = lane >> 5)
//     holds edge r's channels {32 mm + 8 g + 4 h + t} of its head in accumulator register
//     4 g + t of M-tile mm -- four consecutive channels, one 16-byte gather each from
//     xl[src] and xr[dst], whose sum is the accumulators' START value.  The att contraction
//     is an in-lane sum of 32 terms plus one v_permlane32_swap.  Operand form: a head's W_e
//     (64 x 64 floats) is 64 registers of fragments read once per wave from the float32
//     parameter itself (k order 8 s4 + 4 h + u: a float4 of a row); the workgroups are
//     persistent and walk the tiles, a workgroup is one head GROUP of four heads (four
//     waves, one per SIMD), blockIdx.y the group.  No LDS: all of W_e in f32 would be
//     128 KiB of the CU's 160, in three bf16 planes 192 KiB.
//  2. gat_aggregate_kernel.  One wave per destination, lane l = channels 8 l .. 8 l + 7 (head
//     l >> 3).  The segment's maximum per head, then in ascending edge position
//     p = exp(a - max), den += p, acc += p xl[src] (a 2 KiB row per edge, coalesced), and
//     out = acc / (den + 1e-16) + bias.  No atomics, no online rescale: a destination's
//     result is a fixed sequence of operations over its own segment.
//
// rg_linear_f32 is the block's wide nn.Linear (lin_l | lin_r: 64 -> 2 x 512; the first update
// layer: 64 + 512 -> 256), beyond the chain kernels' 256 features: the same MFMA and lane
// layout, weights read from the parameter, 32 rows per wave.
#include "rg_common.h"

namespace rg {
namespace gat {

static constexpr int C = 64;    // channels per head
static constexpr int CE = 64;   // encoded edge channels
static constexpr int H = 8;     // heads
static constexpr int HC = H * C;
static constexpr int HG = 4;    // heads per workgroup: one wave each
static constexpr int ET = 32;   // edges per tile
static constexpr int LOGIT_BLOCKS = 512;  // persistent workgroups per head group

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int clamp_node(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

struct LogitArgs {
  const float* xlr;
  const float* e;
  const int* seg_ptr;
  const int* src;
  const int* dst;
  const float* w_edge;
  const float* att;
  float* logits;
  int ld_xlr, ld_e, ld_w, n_nodes;
  long cap;
  float slope;
};

__global__ __launch_bounds__(HG * 64) void gat_logits_kernel(const LogitArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y * HG + wave;
  long E = a.seg_ptr[a.n_nodes];
  if (E > a.cap) E = a.cap;
  // this head's W_e fragments and att values, for the whole launch
  f32x4 w[2][CE / 8], at[2][4];
#pragma unroll
  for (int mm = 0; mm < 2; ++mm) {
    const float* wr = a.w_edge + (size_t)(hd * C + 32 * mm + r) * a.ld_w + 4 * h;
#pragma unroll
    for (int s4 = 0; s4 < CE / 8; ++s4) w[mm][s4] = *(const f32x4*)(wr + 8 * s4);
#pragma unroll
    for (int g = 0; g < 4; ++g) at[mm][g] = *(const f32x4*)(a.att + hd * C + 32 * mm + 8 * g + 4 * h);
  }
  for (long t = blockIdx.x; t * ET < E; t += gridDim.x) {
    const long p = t * ET + r;
    const bool ok = p < E;
    f32x16 acc[2];
    f32x4 ev[CE / 8];
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mm][i] = 0.f;
#pragma unroll
    for (int s4 = 0; s4 < CE / 8; ++s4) ev[s4] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const int s = clamp_node(a.src[p], a.n_nodes), d = clamp_node(a.dst[p], a.n_nodes);
      const float* xl = a.xlr + (size_t)s * a.ld_xlr + hd * C + 4 * h;
      const float* xr = a.xlr + (size_t)d * a.ld_xlr + HC + hd * C + 4 * h;
      const float* er = a.e + (size_t)p * a.ld_e + 4 * h;
#pragma unroll
      for (int s4 = 0; s4 < CE / 8; ++s4) ev[s4] = *(const f32x4*)(er + 8 * s4);
#pragma unroll
      for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 u = *(const f32x4*)(xl + 32 * mm + 8 * g);
          const f32x4 v = *(const f32x4*)(xr + 32 * mm + 8 * g);
          acc[mm][4 * g] = u.x + v.x;
          acc[mm][4 * g + 1] = u.y + v.y;
          acc[mm][4 * g + 2] = u.z + v.z;
          acc[mm][4 * g + 3] = u.w + v.w;
        }
    }
#pragma unroll
    for (int s4 = 0; s4 < CE / 8; ++s4)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[0] = mfma(w[0][s4][u], ev[s4][u], acc[0]);
        acc[1] = mfma(w[1][s4][u], ev[s4][u], acc[1]);
      }
    float sum = 0.f;
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float m = acc[mm][4 * g + u];
          sum = fmaf(at[mm][g][u], m > 0.f ? m : m * a.slope, sum);
        }
    sum = add_xor32(sum);
    if (ok && h == 0) a.logits[(size_t)p * H + hd] = sum;
  }
}

struct AggArgs {
  const float* xlr;
  const int* seg_ptr;
  const int* src;
  const float* logits;
  const float* bias;
  float* out;
  int ld_xlr, ld_out, n_nodes;
  long cap;
};

__global__ __launch_bounds__(256) void gat_aggregate_kernel(const AggArgs a) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_nodes) return;
  const int hd = lane >> 3;  // channels 8 lane .. 8 lane + 7
  long p0 = a.seg_ptr[i], p1 = a.seg_ptr[i + 1];
  if (p1 > a.cap) p1 = a.cap;
  if (p0 < 0) p0 = 0;
  float mx = -INFINITY;
  for (long p = p0; p < p1; ++p) mx = fmaxf(mx, a.logits[(size_t)p * H + hd]);
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
#pragma unroll 4
  for (long p = p0; p < p1; ++p) {
    const int s = clamp_node(a.src[p], a.n_nodes);
    const float wgt = expf(a.logits[(size_t)p * H + hd] - mx);
    const float* row = a.xlr + (size_t)s * a.ld_xlr + 8 * lane;
    const f32x4 u = *(const f32x4*)row, v = *(const f32x4*)(row + 4);
    den += wgt;
    a0.x = fmaf(wgt, u.x, a0.x);
    a0.y = fmaf(wgt, u.y, a0.y);
    a0.z = fmaf(wgt, u.z, a0.z);
    a0.w = fmaf(wgt, u.w, a0.w);
    a1.x = fmaf(wgt, v.x, a1.x);
    a1.y = fmaf(wgt, v.y, a1.y);
    a1.z = fmaf(wgt, v.z, a1.z);
    a1.w = fmaf(wgt, v.w, a1.w);
  }
  den += 1e-16f;
  const f32x4 b0 = *(const f32x4*)(a.bias + 8 * lane), b1 = *(const f32x4*)(a.bias + 8 * lane + 4);
  float* o = a.out + (size_t)i * a.ld_out + 8 * lane;
  *(f32x4*)o = (f32x4){a0.x / den + b0.x, a0.y / den + b0.y, a0.z / den + b0.z, a0.w / den + b0.w};
  *(f32x4*)(o + 4) =
      (f32x4){a1.x / den + b1.x, a1.y / den + b1.y, a1.z / den + b1.z, a1.w / den + b1.w};
}

// ------------------------------------------------------------------ wide linear
struct LinArgs {
  const float* w;
  const float* b;
  const float* in;
  float* out;
  const int* rows_dev;
  long rows;
  int K, O, ld_w, ld_in, ld_out, act;
  int vec_w, vec_in, vec_out;  // rows 16-byte aligned: float4 accesses
};

// row[k .. k + 3], zero from K on
__device__ __forceinline__ f32x4 ld4_row(const float* row, int k, int K, bool vec) {
  if (vec && k + 4 <= K) return *(const f32x4*)(row + k);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (k < K) v.x = row[k];
  if (k + 1 < K) v.y = row[k + 1];
  if (k + 2 < K) v.z = row[k + 2];
  if (k + 3 < K) v.w = row[k + 3];
  return v;
}

__global__ __launch_bounds__(256) void linear_f32_kernel(const LinArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  long rows = a.rows;
  if (a.rows_dev) {
    const long rd = *a.rows_dev;
    rows = rd < rows ? (rd < 0 ? 0 : rd) : rows;
  }
  const long row0 = ((long)blockIdx.x * 4 + wave) * 32;
  if (row0 >= rows) return;  // wave-uniform
  const long row = row0 + r;
  const bool ok = row < rows;
  const float* xin = a.in + (size_t)(ok ? row : row0) * a.ld_in;
  float* xo = a.out + (size_t)(ok ? row : row0) * a.ld_out;
  const int MT = (a.O + 31) / 32, S4 = (a.K + 7) / 8;
  for (int m = 0; m < MT; ++m) {
    const int o = 32 * m + r;
    const bool ook = o < a.O;
    const float* wr = a.w + (size_t)(ook ? o : 0) * a.ld_w;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int f = 32 * m + 8 * g + 4 * h + t;
        acc[4 * g + t] = (a.b && f < a.O) ? a.b[f] : 0.f;
      }
    for (int s4 = 0; s4 < S4; ++s4) {
      const int k = 8 * s4 + 4 * h;
      f32x4 av = ld4_row(wr, k, a.K, a.vec_w);
      f32x4 bv = ld4_row(xin, k, a.K, a.vec_in);
      if (!ook) av = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (!ok) bv = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc = mfma(av.x, bv.x, acc);
      acc = mfma(av.y, bv.y, acc);
      acc = mfma(av.z, bv.z, acc);
      acc = mfma(av.w, bv.w, acc);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = apply_act(acc[i], a.act);
    if (ok) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f0 = 32 * m + 8 * g + 4 * h;
        if (a.vec_out && f0 + 4 <= a.O) {
          *(f32x4*)(xo + f0) = (f32x4){acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (f0 + t < a.O) xo[f0 + t] = acc[4 * g + t];
        }
      }
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace gat
}  // namespace rg

using namespace rg;

extern "C" int rg_linear_f32(const float* weight, int ld_w, const float* bias, int in_dim,
                             int out_dim, int act, const float* in, int ld_in, long rows,
                             const int* rows_dev, float* out, int ld_out, void* stream) {
  RG_REQUIRE(in_dim >= 1 && out_dim >= 1, RG_ERR_ARG, "rg_linear_f32: dims %d -> %d", in_dim,
             out_dim);
  RG_REQUIRE(rows >= 0 && rows <= (long)0x7fffffff * 64, RG_ERR_ARG, "rg_linear_f32: rows=%ld",
             rows);
  RG_REQUIRE(act >= RG_ACT_NONE && act <= RG_ACT_SWISH, RG_ERR_ARG, "rg_linear_f32: act=%d", act);
  RG_REQUIRE(ld_w >= in_dim && ld_in >= in_dim, RG_ERR_ARG,
             "rg_linear_f32: ld_w=%d / ld_in=%d shorter than in_dim=%d", ld_w, ld_in, in_dim);
  RG_REQUIRE(ld_out >= out_dim, RG_ERR_ARG, "rg_linear_f32: ld_out=%d shorter than out_dim=%d",
             ld_out, out_dim);
  if (rows == 0) return RG_OK;
  RG_REQUIRE(weight && in && out, RG_ERR_ARG, "rg_linear_f32: null pointer with rows=%ld", rows);
  gat::LinArgs a;
  a.w = weight; a.b = bias; a.in = in; a.out = out; a.rows_dev = rows_dev; a.rows = rows;
  a.K = in_dim; a.O = out_dim; a.ld_w = ld_w; a.ld_in = ld_in; a.ld_out = ld_out; a.act = act;
  a.vec_w = gat::aligned16(weight) && ld_w % 4 == 0;
  a.vec_in = gat::aligned16(in) && ld_in % 4 == 0;
  a.vec_out = gat::aligned16(out) && ld_out % 4 == 0;
  const long blocks = (rows + 127) / 128;
  hipLaunchKernelGGL(gat::linear_f32_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, a);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

extern "C" size_t rg_gat_v2_layer_workspace_size(long n_edges_cap, int heads) {
  if (n_edges_cap <= 0 || heads <= 0) return 0;
  return ((size_t)n_edges_cap * (size_t)heads * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int rg_gat_v2_layer(const float* xlr, int ld_xlr, const float* e, int ld_e,
                               const int* seg_ptr, const int* src, const int* dst, int n_nodes,
                               long n_edges_cap, const float* w_edge, int ld_w, const float* att,
                               const float* bias, int edge_dim, int heads, int head_dim,
                               float negative_slope, float* out, int ld_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
  RG_REQUIRE(n_nodes >= 0 && n_edges_cap >= 0, RG_ERR_ARG,
             "rg_gat_v2_layer: n_nodes=%d n_edges_cap=%ld", n_nodes, n_edges_cap);
  RG_REQUIRE(edge_dim >= 1 && heads >= 1 && head_dim >= 1, RG_ERR_ARG,
             "rg_gat_v2_layer: edge_dim=%d heads=%d head_dim=%d", edge_dim, heads, head_dim);
  RG_REQUIRE(edge_dim == gat::CE && heads == gat::H && head_dim == gat::C, RG_ERR_UNSUPPORTED,
             "rg_gat_v2_layer: compiled for edge_dim=%d heads=%d head_dim=%d, not %d / %d / %d",
             gat::CE, gat::H, gat::C, edge_dim, heads, head_dim);
  RG_REQUIRE(ld_xlr >= 2 * gat::HC && ld_out >= gat::HC && ld_w >= gat::CE, RG_ERR_ARG,
             "rg_gat_v2_layer: short stride (ld_xlr=%d < %d, ld_out=%d < %d or ld_w=%d < %d)",
             ld_xlr, 2 * gat::HC, ld_out, gat::HC, ld_w, gat::CE);
  RG_REQUIRE(n_edges_cap == 0 || ld_e >= gat::CE, RG_ERR_ARG,
             "rg_gat_v2_layer: short stride (ld_e=%d < %d)", ld_e, gat::CE);
  if (n_nodes == 0) return RG_OK;
  RG_REQUIRE(xlr && seg_ptr && w_edge && att && bias && out, RG_ERR_ARG,
             "rg_gat_v2_layer: null pointer with n_nodes=%d", n_nodes);
  RG_REQUIRE(n_edges_cap == 0 || (e && src && dst), RG_ERR_ARG,
             "rg_gat_v2_layer: null e / src / dst with n_edges_cap=%ld", n_edges_cap);
  RG_REQUIRE(ld_xlr % 4 == 0 && ld_out % 4 == 0 && ld_w % 4 == 0 && gat::aligned16(xlr) &&
                 gat::aligned16(out) && gat::aligned16(w_edge) && gat::aligned16(att) &&
                 gat::aligned16(bias),
             RG_ERR_ARG, "rg_gat_v2_layer: misaligned rows (16-byte base and stride)");
  RG_REQUIRE(n_edges_cap == 0 || (ld_e % 4 == 0 && gat::aligned16(e)), RG_ERR_ARG,
             "rg_gat_v2_layer: misaligned rows of e (16-byte base and stride)");
  const size_t need = rg_gat_v2_layer_workspace_size(n_edges_cap, heads);
  RG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && gat::aligned16(workspace)),
             RG_ERR_ARG, "rg_gat_v2_layer: workspace of %zu bytes, %zu needed (16-byte aligned)",
             workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  float* logits = (float*)workspace;
  if (n_edges_cap > 0) {
    gat::LogitArgs a;
    a.xlr = xlr; a.e = e; a.seg_ptr = seg_ptr; a.src = src; a.dst = dst; a.w_edge = w_edge;
    a.att = att; a.logits = logits;
    a.ld_xlr = ld_xlr; a.ld_e = ld_e; a.ld_w = ld_w; a.n_nodes = n_nodes;
    a.cap = n_edges_cap; a.slope = negative_slope;
    const long tiles = (n_edges_cap + gat::ET - 1) / gat::ET;
    const unsigned gx = (unsigned)(tiles < gat::LOGIT_BLOCKS ? tiles : gat::LOGIT_BLOCKS);
    hipLaunchKernelGGL(gat::gat_logits_kernel, dim3(gx, gat::H / gat::HG), dim3(gat::HG * 64), 0,
                       st, a);
    RG_LAUNCH_CHECK();
  }
  gat::AggArgs g;
  g.xlr = xlr; g.seg_ptr = seg_ptr; g.src = src; g.logits = logits; g.bias = bias; g.out = out;
  g.ld_xlr = ld_xlr; g.ld_out = ld_out; g.n_nodes = n_nodes; g.cap = n_edges_cap;
  hipLaunchKernelGGL(gat::gat_aggregate_kernel, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0,
                     st, g);
  RG_LAUNCH_CHECK();
  return RG_OK;
}
