// Everything that writes a packed weight image: rg_pack_linear, rg_pack_linear_ld,
// rg_pack_linear_jobs (and rg_packed_linear_bytes).  Where each element goes and how large an
// image is comes from pack_layout.h; here are only the values: which weight an element holds,
// centring, the bf16 / fp16 planes and their residues, the h2 scale.
// One thread per image element, 256 threads per workgroup.
#include "pack_layout.h"
#include "rg_common.h"

namespace rg {

static constexpr int MAXW = 256;  // the chains' widest layer

// the weight at (o, k), 0 in the padding.  transpose: W holds the [in][out] matrix whose
// transpose is the layer; ld: W's row stride (0: dense) -- a column block of a wider matrix
__device__ inline float weight_at(const float* __restrict__ W, int in, int out, int transpose,
                                  int ld, OK e) {
  if (e.o >= out || e.k >= in) return 0.f;
  const int ldw = ld ? ld : (transpose ? out : in);
  return transpose ? W[(size_t)e.k * ldw + e.o] : W[(size_t)e.o * ldw + e.k];
}

// element t of an f32 image (RG_F32 / RG_PACK_F32_FAST): its `total` weights, then its bias
__device__ inline float f32_image_elem(const float* __restrict__ W, const float* __restrict__ bias,
                                       int in, int out, int fmt, int transpose, int ld, long t,
                                       long total) {
  const bool fast = fmt == RG_PACK_F32_FAST;
  if (t < total)
    return weight_at(W, in, out, transpose, ld, fast ? elem_f32_fast(in, t) : elem_f32(in, t));
  const int f = fast ? bias_acc((int)(t - total)) : bias_plain((int)(t - total));
  return (bias && f < out) ? bias[f] : 0.f;
}
// weights and the nb bias entries that follow them in one launch (nb 0: weights only)
__global__ void pack_f32_kernel(const float* __restrict__ W, const float* __restrict__ bias, int in,
                                int out, int fmt, int transpose, int ld, float* __restrict__ P,
                                long total, int nb) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < total + nb) P[t] = f32_image_elem(W, bias, in, out, fmt, transpose, ld, t, total);
}
// rg_pack_linear_jobs: blockIdx.y = job, a grid-stride loop over its weights then its bias
__global__ void pack_jobs_kernel(const rg_pack_job* __restrict__ jobs) {
  const rg_pack_job j = jobs[blockIdx.y];
  const long total = (long)frag_bytes(j.in_dim, j.out_dim, j.fmt) / sizeof(float);
  const int nb = kpad(j.out_dim, bias_pad(j.fmt));
  float* P = (float*)j.packed;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total + nb;
       t += (long)gridDim.x * blockDim.x)
    P[t] = f32_image_elem(j.weight, j.bias, j.in_dim, j.out_dim, j.fmt, j.transpose, j.ld, t, total);
}

// the mean over the n entries of a column (stride ld): one sequential f32 sum, one divide --
// RG_PACK_CENTERED subtracts it from every weight of column k and from the bias
__device__ inline float column_mean(const float* __restrict__ col, int n, int ld) {
  float cs = 0.f;
  for (int i = 0; i < n; ++i) cs += col[(size_t)i * ld];
  return cs / (float)n;
}
// element t of a plane of a 16-bit format (RG_BF16, RG_PACK_FAST_*): the (centred) weight
__device__ inline float w16_elem(const float* __restrict__ W, int in, int out, int fmt, int center,
                                 int transpose, long t) {
  const OK e = elem_of(fmt, in, t);
  float v = weight_at(W, in, out, transpose, 0, e);
  if (center && e.o < out && e.k < in) v -= column_mean(W + e.k, out, in);
  return v;
}
// plane `plane` of a 16-bit image: bf16, or IEEE fp16 (f16: RG_PACK_F16, RG_PACK_H2), of the
// weight less the planes before it (exact residues); tr (RG_PACK_H2): times the scale tr[1]
__global__ void pack_w16_kernel(const float* __restrict__ W, int in, int out, int fmt, int center,
                                int transpose, int plane, int f16, const float* __restrict__ tr,
                                uint16_t* __restrict__ P, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  float v = w16_elem(W, in, out, fmt, center, transpose, t);
  if (tr) v *= tr[1];
  for (int q = 0; q < plane; ++q)
    v -= f16 ? f16_to_f32(f32_to_f16(v)) : bf16_to_f32(f32_to_bf16(v));
  P[t] = f16 ? f32_to_f16(v) : f32_to_bf16(v);
}

// RG_PACK_H2: the layer's power-of-two scale from max |w| (centred as the planes are), one
// workgroup; tr = {2^-s, 2^s, (int) s, 0} with max |w| 2^s in [2^12, 2^13), |s| <= H2_SMAX
__global__ void h2_scale_kernel(const float* __restrict__ W, int in, int out, int center,
                                float* __restrict__ tr) {
  __shared__ float red[256];
  float mx = 0.f;
  for (int k = threadIdx.x; k < in; k += 256) {
    const float mean = center ? column_mean(W + k, out, in) : 0.f;
    for (int o = 0; o < out; ++o) {
      const float v = center ? W[(size_t)o * in + k] - mean : W[(size_t)o * in + k];
      mx = fmaxf(mx, fabsf(v));
    }
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int s = 0;
    if (red[0] > 0.f && red[0] < INFINITY) {
      int e;
      frexpf(red[0], &e);  // max = m 2^e, m in [0.5, 1): max 2^(13 - e) in [2^12, 2^13)
      s = min(max(13 - e, -H2_SMAX), H2_SMAX);
    }
    tr[0] = ldexpf(1.f, -s);
    tr[1] = ldexpf(1.f, s);
    ((int*)tr)[2] = s;
    tr[3] = 0.f;
  }
}

// the n bias entries of an image: plain or accumulator order (fmt), centred with the weights,
// times the h2 scale tr[1] (exact)
__global__ void pack_bias_kernel(const float* __restrict__ b, int out, int n, int fmt, int center,
                                 const float* __restrict__ tr, float* __restrict__ P) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int f = bias_of(fmt, t);
  float v = 0.f;
  if (b && f < out) v = center ? b[f] - column_mean(b, out, 1) : b[f];
  P[t] = tr ? v * tr[1] : v;
}

// One image.  who: the entry point, for its messages; flags as rg_pack_linear takes them
static int pack_image(const char* who, const float* weight, const float* bias, int in_dim,
                      int out_dim, int flags, int ld, void* packed, hipStream_t st) {
  RG_REQUIRE(in_dim > 0 && out_dim > 0 && in_dim <= MAXW && out_dim <= MAXW, RG_ERR_UNSUPPORTED,
             "%s: dims %dx%d outside 1..%d", who, out_dim, in_dim, MAXW);
  const int fmt = flags & ~(RG_PACK_CENTERED | RG_PACK_TRANSPOSE | RG_PACK_X3 | RG_PACK_F16 | RG_PACK_H2);
  const int center = (flags & RG_PACK_CENTERED) ? 1 : 0, transpose = (flags & RG_PACK_TRANSPOSE) ? 1 : 0;
  const int x3 = (flags & RG_PACK_X3) ? 1 : 0, h2 = (flags & RG_PACK_H2) ? 1 : 0;
  const int f16 = (flags & RG_PACK_F16) ? 1 : 0;
  const bool fast = is_fast16(fmt);
  RG_REQUIRE(ld == 0 || ld >= (transpose ? out_dim : in_dim), RG_ERR_ARG,
             "%s: ld %d shorter than a row", who, ld);
  RG_REQUIRE(!f16 || (!x3 && !h2 && !transpose && (fast || (fmt == RG_BF16 && !center))), RG_ERR_ARG,
             "rg_pack_linear: RG_PACK_F16 applies to RG_BF16 and the RG_PACK_FAST_* formats");
  if (h2) {
    RG_REQUIRE(!x3 && !transpose, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_H2 excludes RG_PACK_X3, RG_PACK_F16 and RG_PACK_TRANSPOSE");
    RG_REQUIRE(fmt == RG_PACK_FAST_IN || fmt == RG_PACK_FAST_CHAIN, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_H2 applies to RG_PACK_FAST_IN and RG_PACK_FAST_CHAIN");
  } else if (x3) {
    RG_REQUIRE(fmt != RG_BF16 || !center, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_CENTERED applies to the fast formats");
    RG_REQUIRE(fmt == RG_BF16 || !transpose, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_X3 with RG_PACK_TRANSPOSE applies to RG_BF16");
    RG_REQUIRE(fmt == RG_BF16 || fast, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_X3 applies to RG_BF16 and the RG_PACK_FAST_* formats");
  } else {
    RG_REQUIRE(!transpose || fmt == RG_F32 || fmt == RG_PACK_F32_FAST, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_TRANSPOSE applies to RG_F32 and RG_PACK_F32_FAST");
    RG_REQUIRE(!center || fast, RG_ERR_ARG,
               "rg_pack_linear: RG_PACK_CENTERED applies to the bf16 RG_PACK_FAST_* formats");
    RG_REQUIRE(fmt == RG_F32 || fmt == RG_BF16 || fast || fmt == RG_PACK_F32_FAST, RG_ERR_ARG,
               "rg_pack_linear: bad dtype %d", fmt);
  }
  RG_REQUIRE(fast_upd_ok(fmt, in_dim), RG_ERR_ARG,
             "RG_PACK_FAST_UPD needs in_dim = 2*C with C a multiple of 32");
  const size_t fb = frag_bytes(in_dim, out_dim, fmt);
  const long total = (long)(fb / elem_size(fmt));
  const int nb = kpad(out_dim, bias_pad(flags));
  const int np = plane_count(flags);
  float* pb = (float*)((char*)packed + np * fb);
  if (fmt == RG_F32 || fmt == RG_PACK_F32_FAST) {
    // RG_F32: weights and bias in one launch (the bias follows the weights)
    const int nb1 = fmt == RG_F32 ? nb : 0;
    pack_f32_kernel<<<ceil_div(total + nb1, 256), 256, 0, st>>>(
        weight, bias, in_dim, out_dim, fmt, transpose, ld, (float*)packed, total, nb1);
    if (fmt == RG_F32) {
      RG_LAUNCH_CHECK();
      return RG_OK;
    }
  } else {
    float* tr = h2 ? pb + nb : nullptr;  // the scale the planes and the bias are packed by
    if (h2) h2_scale_kernel<<<1, 256, 0, st>>>(weight, in_dim, out_dim, center, tr);
    for (int p = 0; p < np; ++p)
      pack_w16_kernel<<<ceil_div(total, 256), 256, 0, st>>>(
          weight, in_dim, out_dim, fmt, center, transpose, p, f16 | h2, tr,
          (uint16_t*)((char*)packed + p * fb), total);
  }
  pack_bias_kernel<<<ceil_div(nb, 256), 256, 0, st>>>(bias, out_dim, nb, fmt, center,
                                                      h2 ? pb + nb : nullptr, pb);
  RG_LAUNCH_CHECK();
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" size_t rg_packed_linear_bytes(int in_dim, int out_dim, int dtype) {
  return image_bytes(in_dim, out_dim, dtype);
}

extern "C" int rg_pack_linear(const float* weight, const float* bias, int in_dim, int out_dim,
                              int dtype, void* packed, void* stream) {
  return pack_image("rg_pack_linear", weight, bias, in_dim, out_dim, dtype, 0, packed,
                    (hipStream_t)stream);
}

extern "C" int rg_pack_linear_ld(const float* weight, const float* bias, int in_dim, int out_dim,
                                 int dtype, int ld, void* packed, void* stream) {
  const int fmt = dtype & ~RG_PACK_TRANSPOSE;
  RG_REQUIRE(fmt == RG_F32 || fmt == RG_PACK_F32_FAST, RG_ERR_ARG,
             "rg_pack_linear_ld: RG_F32 or RG_PACK_F32_FAST (| RG_PACK_TRANSPOSE)");
  return pack_image("rg_pack_linear_ld", weight, bias, in_dim, out_dim, dtype, ld, packed,
                    (hipStream_t)stream);
}

extern "C" int rg_pack_linear_jobs(const rg_pack_job* jobs, int n_jobs, void* stream) {
  RG_REQUIRE(n_jobs >= 0 && n_jobs <= 65535 && (jobs || n_jobs == 0), RG_ERR_ARG,
             "rg_pack_linear_jobs: %d jobs", n_jobs);
  if (n_jobs == 0) return RG_OK;
  // 64 blocks of 256 per job: the largest f32 image (256 x 256 + bias) in four passes
  pack_jobs_kernel<<<dim3(64, n_jobs), 256, 0, (hipStream_t)stream>>>(jobs);
  RG_LAUNCH_CHECK();
  return RG_OK;
}
