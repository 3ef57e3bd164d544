// Host-side sanitizer driver for the object stage's C ABI (csrc/objects.hip), run by
// tests/test_objects_host.py::test_object_host_code_under_asan_ubsan on the CPU.
//
// The library's host code is compiled with -fsanitize=address,undefined (host side only) and
// linked into this executable (build.build_sanitized_driver).  It drives the host paths of the
// new entry points: null pointers with non-zero counts, zero counts (no-ops), short
// workspaces, out-of-range arguments, and the workspace-size arithmetic at the M batch's size
// (64 x 3000 nodes, every node its own cluster), at one 20 000-node frame and at the int32
// limit.  Every rejected call must return an RG_ERR_* code with a message before touching
// device memory; no GPU is needed, nothing here reaches a kernel launch.  Any sanitizer report
// fails the test (the runtime aborts with a nonzero exit status), as does a failed CHECK.
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

static void expect_error(int rc, const char* what) {
  const char* msg = rg_last_error();
  if (rc == RG_OK || !msg || !msg[0]) {
    std::fprintf(stderr, "%s: expected an error, got rc %d (%s)\n", what, rc, msg ? msg : "null");
    ++g_fail;
  }
}

int main() {
  // never dereferenced: every call below fails its checks first (or has nothing to do)
  float* ff = (float*)(uintptr_t)4096;
  int* fi = (int*)(uintptr_t)4096;
  int64_t* fl = (int64_t*)(uintptr_t)4096;
  void* fv = (void*)(uintptr_t)4096;
  const float noise[4] = {0.5f, 0.f, 0.f, 0.5f};
  const float skew[4] = {0.5f, 0.1f, 0.2f, 0.5f};

  // ---- workspace-size arithmetic
  const int counts[] = {1, 2, 63, 64, 65, 300, 20000, 64 * 3000, 1 << 24, 1 << 30};
  size_t prev = 0;
  for (int k : counts) {
    const size_t b = rg_object_select_workspace_size(k);
    CHECK(b >= 4 * sizeof(int) * (size_t)k);
    CHECK(b % 256 == 0);
    CHECK(b >= prev);
    prev = b;
  }
  CHECK(rg_object_select_workspace_size(0) == 0);
  CHECK(rg_object_select_workspace_size(-1) == 0);
  CHECK(rg_object_select_workspace_size((1 << 30) + 1) == 0);

  // ---- rg_cluster_stats
  expect_error(rg_cluster_stats(ff, 2, -1, fi, fi, 1, noise, fi, ff, ff, ff, ff, fi, nullptr),
               "stats n_nodes < 0");
  expect_error(rg_cluster_stats(ff, 2, 10, fi, fi, -1, noise, fi, ff, ff, ff, ff, fi, nullptr),
               "stats n_clusters < 0");
  expect_error(rg_cluster_stats(ff, 2, 10, fi, fi, 11, noise, fi, ff, ff, ff, ff, fi, nullptr),
               "stats more clusters than nodes");
  expect_error(rg_cluster_stats(ff, 2, 10, fi, fi, 4, nullptr, fi, ff, ff, ff, ff, fi, nullptr),
               "stats null noise");
  expect_error(rg_cluster_stats(ff, 2, 10, fi, fi, 4, skew, fi, ff, ff, ff, ff, fi, nullptr),
               "stats asymmetric noise");
  expect_error(rg_cluster_stats(nullptr, 2, 64 * 3000, fi, fi, 64 * 3000, noise, fi, ff, ff, ff,
                                ff, fi, nullptr),
               "stats null xy");
  expect_error(rg_cluster_stats(ff, 2, 20000, nullptr, fi, 1, noise, fi, ff, ff, ff, ff, fi,
                                nullptr),
               "stats null cluster_ptr");
  expect_error(rg_cluster_stats(ff, 2, 20000, fi, fi, 1, noise, nullptr, ff, ff, ff, ff, fi,
                                nullptr),
               "stats null size");
  expect_error(rg_cluster_stats(ff, 1, 20000, fi, fi, 1, noise, fi, ff, ff, ff, ff, fi, nullptr),
               "stats ld_xy < 2");
  CHECK(rg_cluster_stats(nullptr, 2, 0, nullptr, nullptr, 0, noise, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr) == RG_OK);
  CHECK(rg_cluster_stats(nullptr, 2, 64 * 3000, nullptr, nullptr, 0, noise, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr) == RG_OK);

  // ---- rg_cov_ellipse
  expect_error(rg_cov_ellipse(ff, ff, ff, 4, 2.f, 0, ff, ff, nullptr), "ellipse n_points 0");
  expect_error(rg_cov_ellipse(ff, ff, ff, 4, 2.f, -7, ff, ff, nullptr), "ellipse n_points < 0");
  expect_error(rg_cov_ellipse(ff, ff, ff, -1, 2.f, 100, ff, ff, nullptr), "ellipse clusters < 0");
  expect_error(rg_cov_ellipse(nullptr, ff, ff, 64 * 3000, 2.f, 100, ff, ff, nullptr),
               "ellipse null eigval");
  expect_error(rg_cov_ellipse(ff, ff, ff, 64 * 3000, 2.f, 100, nullptr, ff, nullptr),
               "ellipse null abt");
  expect_error(rg_cov_ellipse(ff, ff, nullptr, 4, 2.f, 100, ff, ff, nullptr),
               "ellipse points without mu");
  CHECK(rg_cov_ellipse(nullptr, nullptr, nullptr, 0, 2.f, 100, nullptr, nullptr, nullptr) == RG_OK);

  // ---- rg_softmax_max
  expect_error(rg_softmax_max(ff, 7, -1, 7, fl, ff, nullptr), "softmax rows < 0");
  expect_error(rg_softmax_max(ff, 7, 10, 0, fl, ff, nullptr), "softmax 0 classes");
  expect_error(rg_softmax_max(ff, 40, 10, 33, fl, ff, nullptr), "softmax 33 classes");
  expect_error(rg_softmax_max(ff, 3, 10, 7, fl, ff, nullptr), "softmax ld < classes");
  expect_error(rg_softmax_max(nullptr, 7, 64L * 3000, 7, fl, ff, nullptr), "softmax null x");
  expect_error(rg_softmax_max(ff, 7, 10, 7, nullptr, nullptr, nullptr), "softmax no output");
  CHECK(rg_softmax_max(nullptr, 7, 0, 7, nullptr, nullptr, nullptr) == RG_OK);

  // ---- rg_object_select
  for (int k : {1, 20000, 64 * 3000}) {
    const size_t need = rg_object_select_workspace_size(k);
    expect_error(rg_object_select(fi, fi, k, fi, 64, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl, fv,
                                  need - 1, nullptr),
                 "select short workspace");
    expect_error(rg_object_select(fi, fi, k, fi, 64, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl, fv, 0,
                                  nullptr),
                 "select empty workspace");
    expect_error(rg_object_select(fi, fi, k, fi, 64, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl,
                                  nullptr, need, nullptr),
                 "select null workspace");
    expect_error(rg_object_select(nullptr, fi, k, fi, 64, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl, fv,
                                  need, nullptr),
                 "select null cluster_ptr");
    expect_error(rg_object_select(fi, fi, k, fi, 64, nullptr, 7, 0, 6, fi, fi, fi, fi, fi, fl, fv,
                                  need, nullptr),
                 "select drop_class without classes");
  }
  expect_error(rg_object_select(fi, fi, -1, fi, 1, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl, fv, 4096,
                                nullptr),
               "select clusters < 0");
  expect_error(rg_object_select(fi, fi, 10, fi, -1, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl, fv, 4096,
                                nullptr),
               "select frames < 0");
  expect_error(rg_object_select(fi, fi, 10, fi, 1, fl, 7, -1, -1, fi, fi, fi, fi, fi, fl, fv, 4096,
                                nullptr),
               "select min_meas < 0");
  expect_error(rg_object_select(fi, fi, 10, fi, 1, fl, 0, 2, -1, fi, fi, fi, fi, fi, fl, fv, 4096,
                                nullptr),
               "select 0 classes");
  expect_error(rg_object_select(fi, fi, 10, fi, 1, fl, 33, 2, -1, fi, fi, fi, fi, fi, fl, fv, 4096,
                                nullptr),
               "select 33 classes");
  expect_error(rg_object_select(fi, fi, 10, fi, 1, fl, 7, 2, 7, fi, fi, fi, fi, fi, fl, fv, 4096,
                                nullptr),
               "select drop_class out of range");
  expect_error(rg_object_select(fi, fi, 10, fi, 1, fl, 7, 2, -1, fi, fi, fi, fi, fi, nullptr, fv,
                                4096, nullptr),
               "select null counts");
  expect_error(rg_object_select(fi, fi, 10, fi, 1, fl, 7, 2, -1, fi, fi, fi, fi, nullptr, fl, fv,
                                4096, nullptr),
               "select one frame range only");
  expect_error(rg_object_select(fi, fi, 10, nullptr, 1, fl, 7, 2, -1, fi, fi, fi, fi, fi, fl, fv,
                                4096, nullptr),
               "select frame ranges without frame_ptr");

  // ---- rg_object_gather
  expect_error(rg_object_gather(fi, fl, -1, fi, fl, ff, ff, ff, ff, fi, fi, fi, 4, fl, fl, ff, ff,
                                ff, ff, fi, nullptr),
               "gather clusters < 0");
  expect_error(rg_object_gather(nullptr, fl, 10, fi, fl, ff, ff, ff, ff, fi, fi, fi, 4, fl, fl, ff,
                                ff, ff, ff, fi, nullptr),
               "gather null obj_cluster");
  expect_error(rg_object_gather(fi, fl, 10, nullptr, fl, ff, ff, ff, ff, fi, fi, fi, 4, fl, fl, ff,
                                ff, ff, ff, fi, nullptr),
               "gather size output without source");
  expect_error(rg_object_gather(fi, fl, 10, fi, fl, ff, ff, ff, nullptr, fi, fi, fi, 4, fl, fl, ff,
                                ff, ff, ff, fi, nullptr),
               "gather ellipse output without source");
  expect_error(rg_object_gather(fi, fl, 10, fi, fl, ff, ff, ff, ff, fi, fi, nullptr, 4, fl, fl, ff,
                                ff, ff, ff, fi, nullptr),
               "gather frames without frame_ptr");
  expect_error(rg_object_gather(fi, fl, 10, fi, fl, ff, ff, ff, ff, fi, fi, fi, 0, fl, fl, ff, ff,
                                ff, ff, fi, nullptr),
               "gather frames with n_frames 0");
  CHECK(rg_object_gather(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr) == RG_OK);

  // ---- rg_object_features
  expect_error(rg_object_features(ff, 2, ff, 1, -1, fi, fi, 1, fi, ff, ff, ff, nullptr),
               "features nodes < 0");
  expect_error(rg_object_features(ff, 2, ff, 1, 10, fi, fi, -1, fi, ff, ff, ff, nullptr),
               "features clusters < 0");
  expect_error(rg_object_features(nullptr, 2, ff, 1, 64 * 3000, fi, fi, 64 * 3000, fi, ff, ff, ff,
                                  nullptr),
               "features null xy");
  expect_error(rg_object_features(ff, 2, nullptr, 1, 20000, fi, fi, 1, fi, ff, ff, ff, nullptr),
               "features null rcs");
  expect_error(rg_object_features(ff, 2, ff, 1, 20000, fi, fi, 1, fi, ff, ff, nullptr, nullptr),
               "features null output");
  expect_error(rg_object_features(ff, 1, ff, 1, 10, fi, fi, 4, fi, ff, ff, ff, nullptr),
               "features ld_xy < 2");
  expect_error(rg_object_features(ff, 2, ff, 0, 10, fi, fi, 4, fi, ff, ff, ff, nullptr),
               "features ld_rcs < 1");
  CHECK(rg_object_features(nullptr, 2, nullptr, 1, 0, nullptr, nullptr, 0, nullptr, nullptr,
                           nullptr, nullptr, nullptr) == RG_OK);
  CHECK(rg_object_features(nullptr, 2, nullptr, 1, 20000, nullptr, nullptr, 0, nullptr, nullptr,
                           nullptr, nullptr, nullptr) == RG_OK);
  return g_fail ? 1 : 0;
}
