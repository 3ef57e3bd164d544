// Float32 arithmetic on the 16-bit matrix cores (conv_x3.hip, chain_x3.hip), under one of
// two TERM SCHEMES (a compile-time policy: plane count, element type, split, MFMA, product
// list), B3 and H2P below.
//
// b3 (B3) -- three bf16 terms, six products (on request: engine.X3_TERMS = 'b3').
// Every f32 operand is split EXACTLY into three bf16 terms, v = v0 + v1 + v2 (round to
// nearest even at each step: v0 = bf16(v), v1 = bf16(v - v0), v2 = bf16(v - v0 - v1); the
// residues are exact in f32, and the third term holds the last 8 significant bits), and a
// product a.b is formed from the six terms of weight <= 2,
//     a0 b0 + a0 b1 + a1 b0 + a0 b2 + a1 b1 + a2 b0,
// on v_mfma_f32_32x32x16_bf16 with f32 accumulation.  The dropped terms a1 b2 + a2 b1 +
// a2 b2 are below 2^-23 |a b|: each product carries about the error of one f32 rounding and
// the accumulation is f32 -- the arithmetic of the reference's fp32 path, not of bf16.
// Six 32-cycle bf16 MFMAs replace eight 64-cycle f32 MFMAs per 16-deep k-step: 2.7x the
// matrix rate of v_mfma_f32_32x32x2_f32.
//
// h2 (H2P) -- two IEEE f16 terms, three products (the default of the chains and the conv layer).
// v = v0 + v1 + r with v0 = f16(v), v1 = f16(v - v0); v - v0 is exact in f32 and |r| <= 2^-21 |v| while v1 is a normal f16.
// A product is a0 w1 + a1 w0 + a0 w0 (small terms first) on v_mfma_f32_32x32x16_f16 with f32
// accumulation; the dropped a1 w1 and the two r terms are each <= 2^-21 |a w|, the size of
// the f32 accumulation error over K = 64..256 that sets the end-to-end error either way
// (DESIGN.md 4.1).  Half the MFMAs of b3 and a 4-instruction split per pair (v_cvt_pk_f16_f32,
// two v_fma_mix_f32 residues read straight from the packed halves, v_cvt_pk_f16_f32).
//  * f16 has 5 exponent bits.  Weights are packed times a power of two 2^s per layer
//    (max |w| 2^s in [2^12, 2^13): the residue plane w1 then keeps its bits down to
//    2^-24, i.e. 2^-36 of the largest weight), the bias as b 2^s, and the kernels descale
//    once per layer: folded into the row scale of a normalised layer, into the activation
//    of an un-normalised one, one multiply at a plain output (power of two: exact).
//  * Activations are NOT scaled: the small residues a1 are f16 subnormals, which the MFMA
//    honours (the kernels run with f16 denormals on; tests/test_h2_gpu.py pins it), and
//    every value an h2 kernel converts must satisfy |a| < 2^15 (f16 overflows above
//    65504).  An overflow gives a0 = inf, a - a0 = -inf: the row comes back non-finite,
//    never wrong and finite.
//
// Packed weights (rg_pack_linear with RG_PACK_X3, or RG_PACK_H2): three (two) planes of a
// 32x32x16 fragment format (RG_PACK_FAST_IN / _CHAIN), back to back, then the f32 bias in
// accumulator order; h2 images end with 16 bytes {2^-s, 2^s, (int) s, 0}.
// Lane (r = lane & 31, h = lane >> 5) of an accumulator tile m holds row r's features
// {32m + 8(q >> 2) + 4h + (q & 3)} in register q.
#pragma once

#include "pack_layout.h"
#include "rg_common.h"

namespace rg {
namespace x3 {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// image sizes (plane_bytes, x3_bytes, h2_bytes and their tails): pack_layout.h
__host__ __device__ constexpr int al16(int b) { return (b + 15) & ~15; }

__device__ __forceinline__ bf16x8_t ld_bf8(const char* p) {
  return __builtin_bit_cast(bf16x8_t, *(const u32x4*)p);
}
__device__ __forceinline__ f32x16 mf(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

struct X3 {
  bf16x8_t p0, p1, p2;
};
struct H2 {
  f16x8_t p0, p1;
};

// v_cvt_pk_bf16_f32 (round to nearest even) as an opaque instruction: through the builtin
// the compiler re-derives each element's bf16 with a second conversion instead of taking
// it from the packed word (two extra instructions per pair)
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

#ifndef RG_X3_PIPE
#define RG_X3_PIPE 1  // layer_x3 computes the B operand of k-step s + 1 beside step s's MFMAs
#endif
#ifndef RG_X3_LASTSB
#define RG_X3_LASTSB 0  // 0: no fence after the last k-step (M edge encoder 1.41 -> 1.38 ms, conv flat)
#endif
#ifndef RG_X3_SPLIT
#define RG_X3_SPLIT 0  // split8: 0 pair by pair through the inline-asm conversion (the chains),
                       // 4 builtin conversions (no asm: no s_nop pads; conv_x3.hip)
#endif

// the two f32 values of a packed bf16 pair
__device__ __forceinline__ f32x2 unpk(uint32_t u) {
  return (f32x2){__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
}

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
// v_cvt_pk_bf16_f32 through the generic conversion: the compiler takes each element's value
// from the packed word (no inline asm: an asm result costs an s_nop before its first reader,
// the hazard recognizer having to assume a transcendental)
__device__ __forceinline__ uint32_t cvt_pk_bf16_c(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2_t));
}
__device__ __forceinline__ f32x2 unpk_c(uint32_t u) {
  return __builtin_convertvector(__builtin_bit_cast(bf16x2_t, u), f32x2);
}

// 8 consecutive k values of one row -> the three exact bf16 terms (the residues of a
// pair in one v_pk_add_f32)
__device__ __forceinline__ X3 split8(const f32x4 lo, const f32x4 hi) {
  const f32x2 v[4] = {{lo.x, lo.y}, {lo.z, lo.w}, {hi.x, hi.y}, {hi.z, hi.w}};
  u32x4 w0, w1, w2;
#if RG_X3_SPLIT == 4
  // builtin conversions, scalar residues: 3 conversions + 4 unpacks + 4 subtractions per pair
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t u0 = cvt_pk_bf16_c(v[i].x, v[i].y);
    const f32x2 u0f = unpk_c(u0);
    const float rx = v[i].x - u0f.x, ry = v[i].y - u0f.y;
    const uint32_t u1 = cvt_pk_bf16_c(rx, ry);
    const f32x2 u1f = unpk_c(u1);
    w0[i] = u0;
    w1[i] = u1;
    w2[i] = cvt_pk_bf16_c(rx - u1f.x, ry - u1f.y);
  }
#else
  // the inline-asm conversion, scalar residues
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t u0 = cvt_pk_bf16(v[i].x, v[i].y);
    const f32x2 u0f = unpk(u0);
    const f32x2 r = {v[i].x - u0f.x, v[i].y - u0f.y};
    const uint32_t u1 = cvt_pk_bf16(r.x, r.y);
    const f32x2 u1f = unpk(u1);
    const f32x2 t = {r.x - u1f.x, r.y - u1f.y};
    w0[i] = u0;
    w1[i] = u1;
    w2[i] = cvt_pk_bf16(t.x, t.y);
  }
#endif
  return X3{__builtin_bit_cast(bf16x8_t, w0), __builtin_bit_cast(bf16x8_t, w1),
            __builtin_bit_cast(bf16x8_t, w2)};
}
// registers 8 hf .. 8 hf + 7 of an accumulator tile (one RG_PACK_FAST_CHAIN k-step)
__device__ __forceinline__ X3 split_acc(const f32x16& t, int hf) {
  const int q = 8 * hf;
  return split8((f32x4){t[q], t[q + 1], t[q + 2], t[q + 3]},
                (f32x4){t[q + 4], t[q + 5], t[q + 6], t[q + 7]});
}

// h2: 8 consecutive k values of one row -> f16(v) and f16(v - f16(v)).  The residue is an
// fma of the packed half itself (v_fma_mix_f32 takes either half of a register as an f16
// source: no unpacking conversion), exact in f32.
// (the -1 is a scalar register the optimiser cannot see through: written as a constant, the
// fma is first rewritten as v - float(h), which selects a conversion and a subtraction per
// value -- 6 instead of 4 VALU per pair)
__device__ __forceinline__ H2 split8_h2(const f32x4 lo, const f32x4 hi) {
  const f32x2 v[4] = {{lo.x, lo.y}, {lo.z, lo.w}, {hi.x, hi.y}, {hi.z, hi.w}};
  float m1 = -1.f;
  asm("" : "+s"(m1));
  u32x4 w0, w1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f16x2_t h0 = __builtin_convertvector(v[i], f16x2_t);
    const f32x2 r = {__builtin_fmaf((float)h0.x, m1, v[i].x), __builtin_fmaf((float)h0.y, m1, v[i].y)};
    w0[i] = __builtin_bit_cast(uint32_t, h0);
    w1[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2_t));
  }
  return H2{__builtin_bit_cast(f16x8_t, w0), __builtin_bit_cast(f16x8_t, w1)};
}

// ---------------------------------------------------------------- term schemes
// NP planes of element vectors `vec`; product i of a k-step multiplies weight plane wp(i)
// by operand term bp(i), small terms first; SCALED: the image carries a power-of-two scale
// (see the header) that the layer's epilogue takes out.
struct B3 {
  static constexpr int NP = 3, NPROD = 6;
  static constexpr bool SCALED = false;
  typedef bf16x8_t vec;
  typedef X3 terms;
  static constexpr int wp(int i) { return i == 0 ? 2 : (i == 1 || i == 3) ? 1 : 0; }
  static constexpr int bp(int i) { return i == 2 ? 2 : (i == 1 || i == 4) ? 1 : 0; }
  static constexpr int image_bytes(int K, int N) { return x3_bytes(K, N); }
  static constexpr int tail_bytes(int N) { return x3_tail_bytes(N); }  // what follows the planes
  static __device__ __forceinline__ vec term(const X3& b, int i) {
    return i == 0 ? b.p0 : i == 1 ? b.p1 : b.p2;
  }
  static __device__ __forceinline__ vec cast(u32x4 u) { return __builtin_bit_cast(vec, u); }
  static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) { return mf(a, b, c); }
  static __device__ __forceinline__ X3 split(const f32x4 lo, const f32x4 hi) { return split8(lo, hi); }
};
struct H2P {
  static constexpr int NP = 2, NPROD = 3;
  static constexpr bool SCALED = true;
  typedef f16x8_t vec;
  typedef H2 terms;
  static constexpr int wp(int i) { return i == 0 ? 1 : 0; }
  static constexpr int bp(int i) { return i == 1 ? 1 : 0; }
  static constexpr int image_bytes(int K, int N) { return h2_bytes(K, N); }
  static constexpr int tail_bytes(int N) { return h2_tail_bytes(N); }
  static __device__ __forceinline__ vec term(const H2& b, int i) { return i == 0 ? b.p0 : b.p1; }
  static __device__ __forceinline__ vec cast(u32x4 u) { return __builtin_bit_cast(vec, u); }
  static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ H2 split(const f32x4 lo, const f32x4 hi) { return split8_h2(lo, hi); }
};
template <typename T> struct scheme_of;
template <> struct scheme_of<X3> { typedef B3 type; };
template <> struct scheme_of<H2> { typedef H2P type; };

// the NPROD products of one k-step, M-tile by M-tile within each product
template <typename P, int MT>
__device__ __forceinline__ void products(f32x16 (&acc)[MT], const typename P::vec (&A)[MT][P::NP],
                                         const typename P::terms& b) {
#pragma unroll
  for (int i = 0; i < P::NPROD; ++i)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = P::mfma(A[m][P::wp(i)], P::term(b, P::bp(i)), acc[m]);
}

// ---------------------------------------------------------------- weight sources
// W(p, off): the 16 bytes of this lane in plane p at byte offset off of the plane.
// LDS-staged images, or global memory / L2 through a buffer resource (one lane-offset
// register, the fragment offset as a scalar: plain global pointers make the compiler hoist
// one 64-bit address per fragment out of a persistent loop and spill them).
struct WLds {
  const char* p;  // image base + lane * 16
  int pl;         // plane stride
  __device__ __forceinline__ bf16x8_t operator()(int plane, int off) const {
    return ld_bf8(p + plane * pl + off);
  }
  __device__ __forceinline__ u32x4 raw(int plane, int off) const {
    return *(const u32x4*)(p + plane * pl + off);
  }
};
struct WBuf {
  __amdgpu_buffer_rsrc_t rs;
  int voff;  // lane * 16
  int pl;
  __device__ __forceinline__ bf16x8_t operator()(int plane, int off) const {
    return __builtin_bit_cast(bf16x8_t,
                              __builtin_amdgcn_raw_buffer_load_b128(rs, voff, plane * pl + off, 0));
  }
  __device__ __forceinline__ u32x4 raw(int plane, int off) const {
    return __builtin_bit_cast(u32x4,
                              __builtin_amdgcn_raw_buffer_load_b128(rs, voff, plane * pl + off, 0));
  }
};
__device__ __forceinline__ WBuf wbuf(const void* img, int bytes, int pl, int lane) {
  return WBuf{__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(img), 0, bytes, 0x00020000),
              lane * 16, pl};
}
// planes in LDS for bit p of MASK, else global
template <int MASK>
struct WMix {
  WLds l;
  WBuf g;
  __device__ __forceinline__ bf16x8_t operator()(int plane, int off) const {
    return ((MASK >> plane) & 1) ? l(plane, off) : g(plane, off);
  }
  __device__ __forceinline__ u32x4 raw(int plane, int off) const {
    return ((MASK >> plane) & 1) ? l.raw(plane, off) : g.raw(plane, off);
  }
};

struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// acc[t][m] += W[m-tile m0 + m] . B_t over KS k-steps for RT row tiles t; W an image of
// MTW M-tiles; bop(s, t) returns the split B operand of k-step s, row tile t, and its type
// (X3 or H2) selects the term scheme.  Per k-step
// the A fragments are issued first and the B operands are split while they arrive; the
// small terms go first.
// DB: the A fragments of k-step s + 1 are issued before the MFMAs of step s (double
// buffer: MT * 12 more registers, no wait on the fragment loads between k-steps).
// pre1 (RT = 2): the previous layer's epilogue of row tile 1, run after row tile 0's first
// MFMAs are issued instead of before the layer -- a one-k-step skew of the two row tiles at
// the layer boundary, so that epilogue (row statistics, a dependent reduction) issues while
// the matrix pipe works on tile 0 rather than in front of an idle pipe.
template <int KS, int MT, int MTW, int RT, int DB = 0, typename WSrc, typename BOp,
          typename Hook = NoHook>
__device__ __forceinline__ void layer_x3(f32x16 (&acc)[RT][MT], const WSrc& W, int m0, BOp&& bop,
                                         Hook&& pre1 = Hook{}) {
  constexpr bool LAZY = RT == 2 && !std::is_same<std::decay_t<Hook>, NoHook>::value;
  typedef std::decay_t<decltype(bop(0, 0))> T;
  typedef typename scheme_of<T>::type P;
  typedef typename P::vec vec;
  // DB: A fragments read DB k-steps ahead (a ring of DB + 1 buffers); 0: at their step
  constexpr int NBUF = DB + 1;
  vec Ab[NBUF][MT][P::NP];
  auto lda = [&](int s, vec (&d)[MT][P::NP]) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int p = 0; p < P::NP; ++p) d[m][p] = P::cast(W.raw(p, ((m0 + m) * KS + s) * 1024));
  };
  if constexpr (DB > 0) {
#pragma unroll
    for (int q = 0; q < DB && q < KS; ++q) lda(q, Ab[q % NBUF]);
  }
  // B operands one k-step ahead (RG_X3_PIPE): the split of step s + 1 is independent of
  // step s's MFMAs, so its VALU work can issue in their shadow instead of between them
  T bq[RG_X3_PIPE ? RT : 1];
  if constexpr (RG_X3_PIPE) {
#pragma unroll
    for (int t = 0; t < (LAZY ? 1 : RT); ++t) bq[t] = bop(0, t);
  } else if constexpr (LAZY) {
    static_assert(!LAZY, "pre1 needs the B-operand pipeline");
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if constexpr (DB > 0) {
      if (s + DB < KS) lda(s + DB, Ab[(s + DB) % NBUF]);
    } else {
      lda(s, Ab[0]);
    }
    const vec(&A)[MT][P::NP] = Ab[DB > 0 ? s % NBUF : 0];
    T bn[RG_X3_PIPE ? RT : 1];
    if constexpr (RG_X3_PIPE) {
      if (s + 1 < KS) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
          if (!(LAZY && s == 0 && t == 1)) bn[t] = bop(s + 1, t);
      }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      if constexpr (LAZY) {
        if (s == 0 && t == 1) {  // tile 0's first MFMAs are issued: tile 1's epilogue now
          pre1();
          bq[1] = bop(0, 1);
          if (s + 1 < KS) bn[1] = bop(1, 1);
        }
      }
      const T b = RG_X3_PIPE ? bq[t] : bop(s, t);
      products<P, MT>(acc[t], A, b);
    }
    if constexpr (RG_X3_PIPE) {
      if (s + 1 < KS) {
#pragma unroll
        for (int t = 0; t < RT; ++t) bq[t] = bn[t];
      }
    }
    // RG_X3_LASTSB 0: no fence after the last k-step, so the caller's epilogue of row tile 0
    // may interleave with the last MFMAs of the other row tiles
    if (RG_X3_LASTSB || s + 1 < KS) __builtin_amdgcn_sched_barrier(0);
  }
}
// The same products in the same order per accumulator as layer_x3 (one row tile), issued
// M-tile by M-tile: the six MFMAs of tile m chain on acc[m] back to back, and only two
// M-tiles' A fragments are live (the next tile's three are read while the current tile's
// MFMAs run: 24 registers instead of MT * 12).  Bit-identical to layer_x3.
template <int KS, int MT, typename WSrc, typename BOp>
__device__ __forceinline__ void layer_x3_mo(f32x16 (&acc)[MT], const WSrc& W, int m0, BOp&& bop) {
  typedef std::decay_t<decltype(bop(0))> T;
  typedef typename scheme_of<T>::type P;
  typedef typename P::vec vec;
  auto lda = [&](int s, int m, vec (&d)[1][P::NP]) {
#pragma unroll
    for (int p = 0; p < P::NP; ++p) d[0][p] = P::cast(W.raw(p, ((m0 + m) * KS + s) * 1024));
  };
  T bq = bop(0);
  vec A[2][1][P::NP];
  lda(0, 0, A[0]);
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    T bn;
    if (s + 1 < KS) bn = bop(s + 1);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int u = (s * MT + m) & 1;
      if (m + 1 < MT) lda(s, m + 1, A[u ^ 1]);
      else if (s + 1 < KS) lda(s + 1, 0, A[u ^ 1]);
      products<P, 1>(*reinterpret_cast<f32x16(*)[1]>(&acc[m]), A[u], bq);
    }
    if (s + 1 < KS) bq = bn;
    __builtin_amdgcn_sched_barrier(0);
  }
}

// one row tile
template <int KS, int MT, int MTW, int DB = 0, typename WSrc, typename BOp>
__device__ __forceinline__ void layer_x3(f32x16 (&acc)[MT], const WSrc& W, int m0, BOp&& bop) {
  layer_x3<KS, MT, MTW, 1, DB>(*reinterpret_cast<f32x16(*)[1][MT]>(&acc), W, m0,
                               [&](int s, int) { return bop(s); });
}

static constexpr float X3_NORM_EPS = 1e-5f;  // constants.py:9
static constexpr float X3_LEAKY_PRE = 0.505f;
static constexpr float X3_LEAKY_C = 0.495f / 0.505f;

// row statistics of channel_normalization over the 32 MT features of a lane pair: eight
// independent partial sums per statistic (short dependent chains: the epilogue sits on the
// critical path between two layers), then one v_permlane32_swap each.  1 / (std + eps)
// from the hardware sqrt and reciprocal (~1 ulp each, 2e-7 relative on the scale; the
// float32 MFMA path keeps the correctly rounded sequences).  CENT: the layer's weights and
// bias were packed zero-mean over the outputs (RG_LAYER_CENTERED), so the row mean of the
// pre-activations is zero up to f32 rounding and its pass is skipped -- the normalisation
// is invariant to the shift, and the centred form avoids the cancellation of x - mean.
// SC (h2): acc holds the pre-activations times 2^s and ds = 2^-s; the value returned is
// 2^-s / (std + eps) with std the true deviation, so that acc times it is the normalised row
template <int MT, bool CENT, bool SC = false>
__device__ __forceinline__ float row_inv_std(f32x16 (&acc)[MT], float ds = 1.f) {
  constexpr int N = 32 * MT;
  if constexpr (!CENT) {
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = acc[0][i] + acc[0][i + 8];
#pragma unroll
    for (int m = 1; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < 16; ++q) s[q & 7] += acc[m][q];
    const float mean =
        add_xor32(((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) * (1.f / N);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[m][q] -= mean;
  }
  float u[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) u[i] = acc[0][i] * acc[0][i];
#pragma unroll
  for (int i = 0; i < 8; ++i) u[i] = fmaf(acc[0][i + 8], acc[0][i + 8], u[i]);
#pragma unroll
  for (int m = 1; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < 16; ++q) u[q & 7] = fmaf(acc[m][q], acc[m][q], u[q & 7]);
  const float ss = add_xor32(((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7])));
  if constexpr (SC)
    return ds * __builtin_amdgcn_rcpf(
                    fmaf(__builtin_amdgcn_sqrtf(ss * (1.f / (float)(N - 1))), ds, X3_NORM_EPS));
  return __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(ss * (1.f / (float)(N - 1))) + X3_NORM_EPS);
}

// channel_normalization (common.py:208-220) + LeakyReLU (common.py:256-267, constants.py:10):
// after the statistics, two fmas per feature -- y' = x a + b with the 0.505 of
// leaky(y) = 0.505 y + 0.495 |y| folded into a and b, then |y'| C + y'
template <int MT, bool CENT = false, bool SC = false>
__device__ __forceinline__ void norm_leaky(f32x16 (&acc)[MT], float mu, float sd, float ds = 1.f) {
  const float inv = row_inv_std<MT, CENT, SC>(acc, ds);  // acc now centred
  const float ga = X3_LEAKY_PRE * (sd * inv), gb = X3_LEAKY_PRE * mu;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x2 y = {fmaf(acc[m][2 * i], ga, gb), fmaf(acc[m][2 * i + 1], ga, gb)};
      set_pair(acc[m], i, (f32x2){fmaf(fabsf(y.x), X3_LEAKY_C, y.x), fmaf(fabsf(y.y), X3_LEAKY_C, y.y)});
    }
}

// channel_normalization without activation
template <int MT, bool CENT = false, bool SC = false>
__device__ __forceinline__ void norm_only(f32x16 (&acc)[MT], float mu, float sd, float ds = 1.f) {
  const float ga = sd * row_inv_std<MT, CENT, SC>(acc, ds);
  const f32x2 ga2 = {ga, ga}, mu2 = {mu, mu};
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 8; ++i) set_pair(acc[m], i, fma2(pair(acc[m], i), ga2, mu2));
}

// A normalised layer's scale and activation applied when the NEXT layer reads it, eight
// values per k-step (its B operand), instead of over the whole tile between the layers:
// that VALU work then issues beside the next layer's MFMAs (layer_x3's one-step-ahead B).
// PEND 1: norm + LeakyReLU (ga, gb as in norm_leaky), 2: norm only, 0: nothing pending.
struct Pend {
  float ga, gb;
};
template <int MT, bool CENT, bool SC = false>
__device__ __forceinline__ Pend pend_norm_leaky(f32x16 (&acc)[MT], float mu, float sd, float ds = 1.f) {
  const float inv = row_inv_std<MT, CENT, SC>(acc, ds);
  return Pend{X3_LEAKY_PRE * (sd * inv), X3_LEAKY_PRE * mu};
}
template <int MT, bool CENT, bool SC = false>
__device__ __forceinline__ Pend pend_norm_only(f32x16 (&acc)[MT], float mu, float sd, float ds = 1.f) {
  return Pend{sd * row_inv_std<MT, CENT, SC>(acc, ds), mu};
}
// registers 8 hf .. 8 hf + 7 of an accumulator tile under scheme P
template <typename P>
__device__ __forceinline__ typename P::terms split_acc_of(const f32x16& t, int hf) {
  const int q = 8 * hf;
  return P::split((f32x4){t[q], t[q + 1], t[q + 2], t[q + 3]},
                  (f32x4){t[q + 4], t[q + 5], t[q + 6], t[q + 7]});
}
template <int PEND, typename P = B3>
__device__ __forceinline__ typename P::terms split_acc_pend(const f32x16& t, int hf, Pend p) {
  if constexpr (PEND == 0) {
    return split_acc_of<P>(t, hf);
  } else {
    const int q = 8 * hf;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float y = fmaf(t[q + i], p.ga, p.gb);
      if constexpr (PEND == 1) y = fmaf(fabsf(y), X3_LEAKY_C, y);
      v[i] = y;
    }
    return P::split((f32x4){v[0], v[1], v[2], v[3]}, (f32x4){v[4], v[5], v[6], v[7]});
  }
}

// an un-normalised layer under a scaled scheme: the descale and the LeakyReLU of 16
// accumulators (a power of two commutes with max(v, 0.01 v): the values of the unscaled form)
template <bool SC, bool ACT>
__device__ __forceinline__ void plain_epilogue(f32x16& y, float ds) {
  if constexpr (SC && ACT) {
    const float d1 = 0.01f * ds;
#pragma unroll
    for (int q = 0; q < 16; ++q) y[q] = fmaxf(y[q] * ds, y[q] * d1);
  } else if constexpr (SC) {
#pragma unroll
    for (int q = 0; q < 16; ++q) y[q] *= ds;
  } else if constexpr (ACT) {
#pragma unroll
    for (int q = 0; q < 16; ++q) y[q] = act_t<ACT_LEAKY>(y[q]);
  }
}

}  // namespace x3
}  // namespace rg
