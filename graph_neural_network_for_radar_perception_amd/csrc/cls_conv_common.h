// What the classifier conv layer's forward (cls_conv_x3.hip) and backward (cls_conv_bwd_x3.hip)
// share: the compiled widths, the edge launches' tile geometry and the object table's layout.
#pragma once

#include <cstddef>

namespace rg {
namespace clsx3 {

static constexpr int C = 128;     // node / message / output channels
static constexpr int HID = 128;   // msg hidden width
static constexpr int PQW = 2 * HID;
static constexpr int FT = 512;    // edge launch: 8 waves, two per SIMD
static constexpr int NW = FT / 64;
static constexpr int GMAX = 256;  // workgroups of the edge launch at most (one per CU)
static constexpr int TR = 8;      // message rows per LDS transposition pass
static constexpr int TS = C + 4;  // LDS row stride (floats) of the message tile
static constexpr int T_BYTES = TR * TS * 4;

// ------------------------------------------------------------------ the object table
// int32 [seg_ptr N + 1 | begin N | size N | wave table W + 1], each part padded to 16 bytes
__host__ __device__ inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }
static int edge_groups(int n_nodes) {
  const int g = (n_nodes + 63) / 64;
  return g < 1 ? 1 : g > GMAX ? GMAX : g;
}
struct Tab {
  int *seg, *beg, *siz, *wtab;
};
static Tab tab_of(int* t, int n_nodes) {
  const size_t n = n_nodes > 0 ? n_nodes : 0;
  Tab r;
  r.seg = t;
  r.beg = r.seg + al4(n + 1);
  r.siz = r.beg + al4(n);
  r.wtab = r.siz + al4(n);
  return r;
}
static size_t tab_ints(int n_nodes) {
  const size_t n = n_nodes > 0 ? n_nodes : 0;
  return al4(n + 1) + 2 * al4(n) + al4((size_t)GMAX * NW + 1);
}

}  // namespace clsx3
}  // namespace rg
