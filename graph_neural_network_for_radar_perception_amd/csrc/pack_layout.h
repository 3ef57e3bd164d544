// The packed weight formats of rg_pack_linear (include/radar_gnn.h): THE definition of which
// element goes where, how many bytes a plane and an image have, and where the bias and the h2
// trailer sit.  pack.hip writes images by these maps, the kernels size and address theirs by
// these functions, and tests/abi_sanitize_main.cpp checks them on the CPU -- so no HIP types
// here, and everything is constexpr.
//
// An image is NP planes of fragments, then the float32 bias, then (RG_PACK_H2) a trailer:
//   format             plane element t = ((m S + s) 64 + lane) E + e holds W[o][k]   bias
//   RG_F32             E 4, S = kpad(in, 16) / 16: o = 16m + lane % 16,              plain, to 16
//                           k = 16s + 4 (lane / 16) + e
//   RG_BF16            E 8, S = kpad(in, 32) / 32: o = 16m + lane % 16,              plain, to 16
//                           k = 32s + 8 (lane / 16) + e                              (X3: to 32)
//   RG_PACK_F32_FAST   E 4, S = kpad(in, 8) / 8:   o = 32m + lane % 32,              acc, to 32
//                           k = 8s + 4 (lane / 32) + e
//   RG_PACK_FAST_*     E 8, S = kpad(in, 16) / 16: o = 32m + lane % 32, h = lane / 32 acc, to 32
//     k-step s < mem_steps   k = 16s + 8h + e                (operand loaded from memory)
//     the others, s' = s - mem_steps
//                            k = 16 mem_steps + 32 (s' / 2) + 16 (s' % 2) + 8 (e / 4) + 4h + e % 4
//                            (operand = accumulator registers 8 (s' % 2) .. + 7 of the previous
//                            layer's M-tile s' / 2: no lane movement)
//     mem_steps: FAST_IN all, FAST_CHAIN 0, FAST_UPD half (x[node] from memory, the aggregate
//     from accumulators: in = 2C with C a multiple of 32)
// "acc": the 32x32 accumulator order [m][h][16], entry 4g + j = bias[32m + 8g + 4h + j], so
// lane half h of M-tile m initialises its 16 accumulators with four 16-byte reads.
// Planes: 1; RG_PACK_X3 3 (bf16(w), bf16(w - p0), bf16(w - p0 - p1)); RG_PACK_H2 2
// (fp16(w 2^s), fp16(w 2^s - p0)), the bias times 2^s, the trailer {2^-s, 2^s, (int) s, 0}.
// RG_PACK_F16 / _CENTERED / _TRANSPOSE change values, never sizes or places.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/radar_gnn.h"

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ inline
#else
#define RG_HD inline
#endif

namespace rg {

RG_HD constexpr int kpad(int k, int p) { return (k + p - 1) / p * p; }

RG_HD constexpr bool is_fast16(int fmt) {
  return fmt == RG_PACK_FAST_IN || fmt == RG_PACK_FAST_CHAIN || fmt == RG_PACK_FAST_UPD;
}
// 32-row M-tiles (the 32x32 MFMAs) and the accumulator-order bias; else 16-row tiles
RG_HD constexpr bool is_wide(int fmt) { return is_fast16(fmt) || fmt == RG_PACK_F32_FAST; }

// bytes of one plane of fragments of base format fmt (no flags): M-tiles x k-steps x 64 lanes x
// the lane's elements, 1 KiB per fragment in every format
RG_HD constexpr size_t frag_bytes(int in_dim, int out_dim, int fmt) {
  if (fmt == RG_PACK_F32_FAST)
    return (size_t)((out_dim + 31) / 32) * ((in_dim + 7) / 8) * 1024;
  if (is_fast16(fmt))
    return (size_t)((out_dim + 31) / 32) * ((in_dim + 15) / 16) * 64 * 8 * sizeof(uint16_t);
  const size_t mt = (size_t)(out_dim + 15) / 16;
  if (fmt == RG_F32) return mt * (kpad(in_dim, 16) / 16) * 64 * 4 * sizeof(float);
  return mt * (kpad(in_dim, 32) / 32) * 64 * 8 * sizeof(uint16_t);
}
RG_HD constexpr int elem_size(int fmt) { return (fmt == RG_F32 || fmt == RG_PACK_F32_FAST) ? 4 : 2; }

static constexpr int H2_TRAILER = 16;  // {2^-s, 2^s, (int) s, 0}
static constexpr int H2_SMAX = 64;     // |s| <= H2_SMAX

// flags: a base format with RG_PACK_X3 or RG_PACK_H2 (the other flags change no size)
RG_HD constexpr int plane_count(int flags) {
  return (flags & RG_PACK_H2) ? 2 : (flags & RG_PACK_X3) ? 3 : 1;
}
RG_HD constexpr int base_format(int flags) { return flags & 0xff; }
RG_HD constexpr int bias_pad(int flags) {
  return (is_wide(base_format(flags)) || (flags & (RG_PACK_X3 | RG_PACK_H2))) ? 32 : 16;
}
RG_HD constexpr size_t tail_bytes(int out_dim, int flags) {  // what follows the planes
  return (size_t)kpad(out_dim, bias_pad(flags)) * sizeof(float) +
         ((flags & RG_PACK_H2) ? H2_TRAILER : 0);
}
RG_HD constexpr size_t image_bytes(int in_dim, int out_dim, int flags) {
  return plane_count(flags) * frag_bytes(in_dim, out_dim, base_format(flags)) +
         tail_bytes(out_dim, flags);
}

// The kernels' template arithmetic, views of the functions above.  A kernel that takes its
// padded width N as the layer's (N % 32 == 0) says so with a static_assert where it
// instantiates these.
RG_HD constexpr int plane_bytes(int K, int N) { return (int)frag_bytes(K, N, RG_PACK_FAST_IN); }
RG_HD constexpr int fast_bytes(int K, int N) { return (int)image_bytes(K, N, RG_PACK_FAST_IN); }
RG_HD constexpr int f32_fast_bytes(int K, int N) { return (int)image_bytes(K, N, RG_PACK_F32_FAST); }
RG_HD constexpr int x3_bytes(int K, int N) { return (int)image_bytes(K, N, RG_PACK_FAST_IN | RG_PACK_X3); }
RG_HD constexpr int h2_bytes(int K, int N) { return (int)image_bytes(K, N, RG_PACK_FAST_IN | RG_PACK_H2); }
RG_HD constexpr int x3_tail_bytes(int N) { return (int)tail_bytes(N, RG_PACK_FAST_IN | RG_PACK_X3); }
RG_HD constexpr int h2_tail_bytes(int N) { return (int)tail_bytes(N, RG_PACK_FAST_IN | RG_PACK_H2); }

// ------------------------------------------------------------------ element maps
struct OK {
  int o, k;
};
// k-steps of a RG_PACK_FAST_* layer whose operand comes from memory
RG_HD constexpr int mem_steps(int fmt, int in_dim) {
  const int ks = (in_dim + 15) / 16;
  return fmt == RG_PACK_FAST_IN ? ks : fmt == RG_PACK_FAST_CHAIN ? 0 : ks / 2;
}
RG_HD constexpr bool fast_upd_ok(int fmt, int in_dim) {
  return fmt != RG_PACK_FAST_UPD || in_dim % 64 == 0;
}

// element t of a plane: t = ((m S + s) 64 + lane) E + e, E = 2^LE elements per lane
struct Frag {
  int m, s, lane, e;
};
RG_HD constexpr Frag frag_of(long t, int LE, int S) {
  const int ms = (int)(t >> (LE + 6));  // the fragment: 32-bit, its division runs per element
  return Frag{ms / S, ms % S, (int)((t >> LE) & 63), (int)(t & ((1 << LE) - 1))};
}
RG_HD constexpr OK elem_f32(int in_dim, long t) {
  const Frag f = frag_of(t, 2, kpad(in_dim, 16) / 16);
  return OK{16 * f.m + (f.lane & 15), 16 * f.s + 4 * (f.lane >> 4) + f.e};
}
RG_HD constexpr OK elem_bf16(int in_dim, long t) {
  const Frag f = frag_of(t, 3, kpad(in_dim, 32) / 32);
  return OK{16 * f.m + (f.lane & 15), 32 * f.s + 8 * (f.lane >> 4) + f.e};
}
RG_HD constexpr OK elem_f32_fast(int in_dim, long t) {
  const Frag f = frag_of(t, 2, (in_dim + 7) / 8);
  return OK{32 * f.m + (f.lane & 31), 8 * f.s + 4 * (f.lane >> 5) + f.e};
}
RG_HD constexpr OK elem_fast16(int in_dim, int mem, long t) {
  const Frag f = frag_of(t, 3, (in_dim + 15) / 16);
  const int h = f.lane >> 5, sc = f.s - mem;
  return OK{32 * f.m + (f.lane & 31),
            f.s < mem ? 16 * f.s + 8 * h + f.e
                      : 16 * mem + 32 * (sc >> 1) + 16 * (sc & 1) + 8 * (f.e >> 2) + 4 * h + (f.e & 3)};
}
RG_HD constexpr OK elem_of(int fmt, int in_dim, long t) {
  return fmt == RG_F32 ? elem_f32(in_dim, t)
         : fmt == RG_BF16 ? elem_bf16(in_dim, t)
         : fmt == RG_PACK_F32_FAST ? elem_f32_fast(in_dim, t)
                                   : elem_fast16(in_dim, mem_steps(fmt, in_dim), t);
}

// bias entry t of the image holds bias[f] (0 beyond out_dim)
RG_HD constexpr int bias_plain(int t) { return t; }
RG_HD constexpr int bias_acc(int t) {
  const int m = t >> 5, h = (t >> 4) & 1, g = (t >> 2) & 3, j = t & 3;
  return 32 * m + 8 * g + 4 * h + j;
}
RG_HD constexpr int bias_of(int fmt, int t) { return is_wide(fmt) ? bias_acc(t) : bias_plain(t); }

// ------------------------------------------------------------------ split rows
// A SPLIT ROW holds the two h2 terms of a row of 64 float32 values v in the 256 bytes of the
// float32 row itself (rg_mlp_chain_x3_split writes it, rg_conv_layer_x3_split_for reads it):
// each aligned 32-byte group of eight values (features 8j .. 8j + 7) is the eight fp16 heads
// a0 = fp16(v), 16 bytes, then the eight fp16 residues a1 = fp16(v - a0), 16 bytes.  Lane
// (r, h) of the conv's edge launch reads the 16-byte pieces at float offsets 8h + 16i and
// 8h + 16i + 4 of its row per k-step i -- group 2i + h: its heads and its residues, the MFMA B
// operands of planes 0 and 1 as loaded.
static constexpr int SPLIT_ROW_W = 64;                    // values per row
static constexpr int SPLIT_ROW_BYTES = 4 * SPLIT_ROW_W;   // = the float32 row
// byte offset in the row of the head / the residue of feature f
RG_HD constexpr int split_row_head(int f) { return 32 * (f >> 3) + 2 * (f & 7); }
RG_HD constexpr int split_row_res(int f) { return split_row_head(f) + 16; }

}  // namespace rg
