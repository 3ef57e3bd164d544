// Host-side sanitizer driver for the graph attention C ABI (csrc/attention.hip), run by
// tests/test_attention_host.py::test_attention_host_code_under_asan_ubsan on the CPU.
//
// The library's host code is compiled with -fsanitize=address,undefined (host side only) and
// linked into this executable (build.build_sanitized_driver).  It drives the host paths of
// rg_gat_v2_layer, its workspace query and rg_linear_f32: null pointers with non-zero counts,
// zero counts (no-ops), short and misaligned workspaces, short and misaligned strides, shapes
// the kernel is not compiled for, and the workspace arithmetic at the M batch's size
// (64 x 3000 nodes, 20 edges each) and past 2^31 bytes.  Every rejected call must return an
// RG_ERR_* code with a message before touching device memory; no GPU is needed, nothing here
// reaches a kernel launch.  Any sanitizer report fails the test (the runtime aborts with a
// nonzero exit status), as does a failed CHECK.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "radar_gnn.h"

static int g_fail = 0;
#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) {                                                            \
      std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #c); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

static void expect(int rc, int code, const char* what) {
  const char* msg = rg_last_error();
  if (rc != code || !msg || !msg[0]) {
    std::fprintf(stderr, "%s: expected rc %d, got %d (%s)\n", what, code, rc, msg ? msg : "null");
    ++g_fail;
  }
}

struct Gat {
  // never dereferenced: every call below fails its checks first (or has nothing to do)
  const float* xlr = (const float*)(uintptr_t)4096;
  int ld_xlr = 1024;
  const float* e = (const float*)(uintptr_t)4096;
  int ld_e = 64;
  const int* seg_ptr = (const int*)(uintptr_t)4096;
  const int* src = (const int*)(uintptr_t)4096;
  const int* dst = (const int*)(uintptr_t)4096;
  int n_nodes = 64 * 3000;
  long cap = 64L * 3000 * 20;
  const float* w = (const float*)(uintptr_t)4096;
  int ld_w = 64;
  const float* att = (const float*)(uintptr_t)4096;
  const float* bias = (const float*)(uintptr_t)4096;
  int edge_dim = 64, heads = 8, head_dim = 64;
  float* out = (float*)(uintptr_t)4096;
  int ld_out = 512;
  void* ws = (void*)(uintptr_t)4096;
  long ws_bytes = -1;  // -1: exactly what the query asks for

  int call() const {
    const size_t need = rg_gat_v2_layer_workspace_size(cap, heads);
    return rg_gat_v2_layer(xlr, ld_xlr, e, ld_e, seg_ptr, src, dst, n_nodes, cap, w, ld_w, att,
                           bias, edge_dim, heads, head_dim, 0.2f, out, ld_out, ws,
                           ws_bytes < 0 ? need : (size_t)ws_bytes, nullptr);
  }
};

int main() {
  // ---- workspace-size arithmetic
  const long caps[] = {1, 31, 32, 33, 636, 64L * 3000 * 20, 1L << 27, 1L << 31, 1L << 36};
  size_t prev = 0;
  for (long c : caps) {
    const size_t b = rg_gat_v2_layer_workspace_size(c, 8);
    CHECK(b >= sizeof(float) * 8 * (size_t)c);
    CHECK(b < sizeof(float) * 8 * (size_t)c + 256);
    CHECK(b % 256 == 0);
    CHECK(b >= prev);
    prev = b;
  }
  CHECK(rg_gat_v2_layer_workspace_size(0, 8) == 0);
  CHECK(rg_gat_v2_layer_workspace_size(-1, 8) == 0);
  CHECK(rg_gat_v2_layer_workspace_size(100, 0) == 0);
  CHECK(rg_gat_v2_layer_workspace_size(100, -3) == 0);

  // ---- rg_gat_v2_layer
  { Gat g; g.n_nodes = -1; expect(g.call(), RG_ERR_ARG, "gat n_nodes < 0"); }
  { Gat g; g.cap = -1; expect(g.call(), RG_ERR_ARG, "gat cap < 0"); }
  { Gat g; g.heads = 0; expect(g.call(), RG_ERR_ARG, "gat 0 heads"); }
  { Gat g; g.head_dim = -64; expect(g.call(), RG_ERR_ARG, "gat head_dim < 0"); }
  { Gat g; g.heads = 4; expect(g.call(), RG_ERR_UNSUPPORTED, "gat 4 heads"); }
  { Gat g; g.head_dim = 32; expect(g.call(), RG_ERR_UNSUPPORTED, "gat 32 channels"); }
  { Gat g; g.edge_dim = 128; expect(g.call(), RG_ERR_UNSUPPORTED, "gat edge_dim 128"); }
  { Gat g; g.ld_xlr = 1020; expect(g.call(), RG_ERR_ARG, "gat short ld_xlr"); }
  { Gat g; g.ld_out = 256; expect(g.call(), RG_ERR_ARG, "gat short ld_out"); }
  { Gat g; g.ld_e = 32; expect(g.call(), RG_ERR_ARG, "gat short ld_e"); }
  { Gat g; g.ld_w = 0; expect(g.call(), RG_ERR_ARG, "gat short ld_w"); }
  { Gat g; g.ld_xlr = 1025; expect(g.call(), RG_ERR_ARG, "gat odd ld_xlr"); }
  { Gat g; g.ld_e = 66; expect(g.call(), RG_ERR_ARG, "gat ld_e not a multiple of 4"); }
  { Gat g; g.xlr = (const float*)(uintptr_t)4100; expect(g.call(), RG_ERR_ARG, "gat xlr + 4"); }
  { Gat g; g.out = (float*)(uintptr_t)4104; expect(g.call(), RG_ERR_ARG, "gat out + 8"); }
  { Gat g; g.att = (const float*)(uintptr_t)4108; expect(g.call(), RG_ERR_ARG, "gat att + 12"); }
  { Gat g; g.e = (const float*)(uintptr_t)4100; expect(g.call(), RG_ERR_ARG, "gat e + 4"); }
  { Gat g; g.xlr = nullptr; expect(g.call(), RG_ERR_ARG, "gat null xlr"); }
  { Gat g; g.seg_ptr = nullptr; expect(g.call(), RG_ERR_ARG, "gat null seg_ptr"); }
  { Gat g; g.w = nullptr; expect(g.call(), RG_ERR_ARG, "gat null w_edge"); }
  { Gat g; g.att = nullptr; expect(g.call(), RG_ERR_ARG, "gat null att"); }
  { Gat g; g.bias = nullptr; expect(g.call(), RG_ERR_ARG, "gat null bias"); }
  { Gat g; g.out = nullptr; expect(g.call(), RG_ERR_ARG, "gat null out"); }
  { Gat g; g.e = nullptr; expect(g.call(), RG_ERR_ARG, "gat null e"); }
  { Gat g; g.src = nullptr; expect(g.call(), RG_ERR_ARG, "gat null src"); }
  { Gat g; g.dst = nullptr; expect(g.call(), RG_ERR_ARG, "gat null dst"); }
  { Gat g; g.ws = nullptr; expect(g.call(), RG_ERR_ARG, "gat null workspace"); }
  { Gat g; g.ws = (void*)(uintptr_t)4100; expect(g.call(), RG_ERR_ARG, "gat workspace + 4"); }
  { Gat g; g.ws_bytes = 0; expect(g.call(), RG_ERR_ARG, "gat empty workspace"); }
  for (long c : {1L, 636L, 64L * 3000 * 20, 1L << 31}) {
    Gat g;
    g.cap = c;
    g.ws_bytes = (long)rg_gat_v2_layer_workspace_size(c, 8) - 1;
    expect(g.call(), RG_ERR_ARG, "gat workspace one byte short");
  }
  {  // nothing to do: no node (no pointer is looked at)
    Gat g;
    g.n_nodes = 0;
    g.xlr = nullptr;
    g.seg_ptr = nullptr;
    g.out = nullptr;
    g.ws = nullptr;
    CHECK(g.call() == RG_OK);
  }

  // ---- rg_linear_f32
  const float* ff = (const float*)(uintptr_t)4096;
  float* fo = (float*)(uintptr_t)4096;
  expect(rg_linear_f32(nullptr, 576, ff, 576, 256, RG_ACT_LEAKY, ff, 576, 64L * 3000, nullptr, fo,
                       256, nullptr),
         RG_ERR_ARG, "linear null weight");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, RG_ACT_LEAKY, nullptr, 576, 64L * 3000, nullptr, fo,
                       256, nullptr),
         RG_ERR_ARG, "linear null input");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, RG_ACT_LEAKY, ff, 576, 64L * 3000, nullptr, nullptr,
                       256, nullptr),
         RG_ERR_ARG, "linear null output");
  expect(rg_linear_f32(ff, 575, ff, 576, 256, RG_ACT_LEAKY, ff, 576, 10, nullptr, fo, 256, nullptr),
         RG_ERR_ARG, "linear short ld_w");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, RG_ACT_LEAKY, ff, 64, 10, nullptr, fo, 256, nullptr),
         RG_ERR_ARG, "linear short ld_in");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, RG_ACT_LEAKY, ff, 576, 10, nullptr, fo, 255, nullptr),
         RG_ERR_ARG, "linear short ld_out");
  expect(rg_linear_f32(ff, 576, ff, 0, 256, RG_ACT_LEAKY, ff, 576, 10, nullptr, fo, 256, nullptr),
         RG_ERR_ARG, "linear in_dim 0");
  expect(rg_linear_f32(ff, 576, ff, 576, -1, RG_ACT_LEAKY, ff, 576, 10, nullptr, fo, 256, nullptr),
         RG_ERR_ARG, "linear out_dim < 0");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, 17, ff, 576, 10, nullptr, fo, 256, nullptr),
         RG_ERR_ARG, "linear bad act");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, RG_ACT_NONE, ff, 576, -1, nullptr, fo, 256, nullptr),
         RG_ERR_ARG, "linear rows < 0");
  expect(rg_linear_f32(ff, 576, ff, 576, 256, RG_ACT_NONE, ff, 576, (1L << 62), nullptr, fo, 256,
                       nullptr),
         RG_ERR_ARG, "linear rows past the grid");
  CHECK(rg_linear_f32(nullptr, 576, nullptr, 576, 256, RG_ACT_NONE, nullptr, 576, 0, nullptr,
                      nullptr, 256, nullptr) == RG_OK);
  return g_fail ? 1 : 0;
}
