// The split-row format of csrc/pack_layout.h on the CPU: split_row_head / split_row_res map the
// 64 features of a row one to one onto the 128 fp16 slots of its 256 bytes, group by group
// (heads of features 8j .. 8j + 7 in the first 16 bytes of group j's 32, residues in the second),
// and the two 16-byte pieces a lane of the conv's edge launch loads per k-step are exactly one
// group's heads and residues in k order.  Prints every (feature, head offset, residue offset)
// for tests/test_split_rows_layout.py to compare with its numpy reference; exits non-zero on a
// violation.  Built with the host compiler alone (no HIP, no GPU).
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../graph_neural_network_for_radar_perception_amd/csrc/pack_layout.h"

static int fail(const char* what, int a, int b) {
  std::fprintf(stderr, "split_rows_layout: %s (%d, %d)\n", what, a, b);
  return 1;
}

int main() {
  static_assert(rg::SPLIT_ROW_BYTES == 256 && rg::SPLIT_ROW_W == 64, "a float32 row of 64");
  static_assert(rg::split_row_head(0) == 0 && rg::split_row_res(0) == 16, "constexpr maps");
  unsigned char used[rg::SPLIT_ROW_BYTES];
  std::memset(used, 0, sizeof(used));
  for (int f = 0; f < rg::SPLIT_ROW_W; ++f) {
    const int hb = rg::split_row_head(f), rb = rg::split_row_res(f);
    for (int b : {hb, hb + 1, rb, rb + 1}) {
      if (b < 0 || b >= rg::SPLIT_ROW_BYTES) return fail("offset outside the row", f, b);
      if (used[b]++) return fail("byte used twice", f, b);
    }
    if (hb % 2 || rb % 2) return fail("unaligned fp16", f, hb);
    if (hb / 32 != f / 8 || rb / 32 != f / 8) return fail("outside the feature's group", f, hb);
    if (hb % 32 != 2 * (f % 8) || rb % 32 != 16 + 2 * (f % 8)) return fail("order in group", f, hb);
    std::printf("%d %d %d\n", f, hb, rb);
  }
  for (int b = 0; b < rg::SPLIT_ROW_BYTES; ++b)
    if (used[b] != 1) return fail("byte not covered", b, used[b]);
  // the edge launch's loads: lane half h, k-step i reads float offsets 8h + 16i (.. + 3) and
  // 8h + 16i + 4 (.. + 7); its MFMA B operand of k-step i is features 16i + 8h + 0 .. 7
  for (int h = 0; h < 2; ++h)
    for (int i = 0; i < 4; ++i)
      for (int e = 0; e < 8; ++e) {
        const int f = 16 * i + 8 * h + e;
        if (rg::split_row_head(f) != 4 * (8 * h + 16 * i) + 2 * e) return fail("plane 0 piece", f, e);
        if (rg::split_row_res(f) != 4 * (8 * h + 16 * i + 4) + 2 * e) return fail("plane 1 piece", f, e);
      }
  return 0;
}
