// Host-side sanitizer driver for the training feed's C ABI (csrc/training_feed.hip), run by
// tests/test_training_feed_host.py::test_training_feed_host_code_under_asan_ubsan on the CPU.
//
// The library's host code is compiled with -fsanitize=address,undefined (host side only) and
// linked into this executable (build.build_sanitized_driver).  It drives every argument check
// of rg_frontend_flip, rg_train_labels and rg_train_offsets -- null arrays, negative sizes, several windows
// without win_ptr, n_nodes * 2 and pair_capacity at and past int32, a misaligned offsets
// array, a short or misaligned workspace -- each of which must return RG_ERR_ARG with a message before anything is launched,
// and the empty calls that are valid and launch nothing; no GPU is needed.  Any sanitizer
// report fails the test (the runtime aborts), as does a failed check.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "radar_gnn.h"

static int g_fail = 0;

static void expect_arg_error(int rc, const char* what, const char* needle) {
  const char* msg = rg_last_error();
  if (rc != RG_ERR_ARG || !msg || !std::strstr(msg, needle)) {
    std::fprintf(stderr, "%s: expected RG_ERR_ARG mentioning '%s', got rc %d (%s)\n", what, needle,
                 rc, msg ? msg : "null");
    ++g_fail;
  }
}

static void expect_ok(int rc, const char* what) {
  if (rc != RG_OK) {
    std::fprintf(stderr, "%s: expected RG_OK, got rc %d (%s)\n", what, rc, rg_last_error());
    ++g_fail;
  }
}

int main() {
  // never dereferenced: every call below fails its checks first or has nothing to do
  float* f = (float*)(uintptr_t)4096;
  int* i = (int*)(uintptr_t)4096;
  uint8_t* u = (uint8_t*)(uintptr_t)4096;
  int64_t* l = (int64_t*)(uintptr_t)4096;

  // ---- rg_frontend_flip
  expect_arg_error(rg_frontend_flip(f, f, i, 4, u, -1, nullptr), "n_meas < 0", "n_meas=-1");
  expect_arg_error(rg_frontend_flip(f, f, i, -2, u, 100, nullptr), "n_windows < 0",
                   "n_windows=-2");
  expect_arg_error(rg_frontend_flip(f, f, nullptr, 2, u, 100, nullptr), "windows without win_ptr",
                   "win_ptr");
  expect_arg_error(rg_frontend_flip(nullptr, f, i, 4, u, 100, nullptr), "null py", "null");
  expect_arg_error(rg_frontend_flip(f, nullptr, i, 4, u, 100, nullptr), "null vy", "null");
  expect_arg_error(rg_frontend_flip(f, f, i, 4, nullptr, 100, nullptr), "null flip", "null");
  expect_arg_error(rg_frontend_flip(f, f, nullptr, 1, nullptr, 100, nullptr),
                   "null flip, one window", "null");
  expect_ok(rg_frontend_flip(nullptr, nullptr, nullptr, 1, nullptr, 0, nullptr), "no measurement");
  expect_ok(rg_frontend_flip(f, f, i, 0, u, 100, nullptr), "no window");

  // ---- rg_train_labels
  const long cap = 64L * 2000;
  expect_arg_error(rg_train_labels(f, f, f, -1, i, i, i, i, cap, l, f, l, nullptr), "N < 0",
                   "n_nodes=-1");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, -1, l, f, l, nullptr), "capacity < 0",
                   "pair_capacity=-1");
  expect_arg_error(rg_train_labels(f, f, f, 1 << 30, i, i, i, i, cap, l, f, l, nullptr),
                   "N * 2 at 2^31", "int32");
  expect_arg_error(rg_train_labels(f, f, f, 0x7fffffff, i, i, i, i, cap, l, f, l, nullptr),
                   "N * 2 far past int32", "int32");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, 1L << 31, l, f, l, nullptr),
                   "capacity at 2^31", "int32");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, 0x7fffffffffffffffL, l, f, l, nullptr),
                   "capacity far past int32", "int32");
  expect_arg_error(rg_train_labels(nullptr, f, f, 100, i, i, i, i, cap, l, f, l, nullptr),
                   "null class_labels", "null node");
  expect_arg_error(rg_train_labels(f, nullptr, f, 100, i, i, i, i, cap, l, f, l, nullptr),
                   "null offset_x", "null node");
  expect_arg_error(rg_train_labels(f, f, nullptr, 100, i, i, i, i, cap, l, f, l, nullptr),
                   "null offset_y", "null node");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, cap, nullptr, f, l, nullptr),
                   "null node_class", "null node");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, cap, l, nullptr, l, nullptr),
                   "null node_offsets", "null node");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, 0, l, nullptr, l, nullptr),
                   "null node_offsets, no pair", "null node");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, nullptr, i, i, cap, l, f, l, nullptr),
                   "null pair_src", "null pair");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, nullptr, i, cap, l, f, l, nullptr),
                   "null pair_dst", "null pair");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, nullptr, cap, l, f, l, nullptr),
                   "null n_pairs", "null pair");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, cap, l, f, nullptr, nullptr),
                   "null edge_class", "null pair");
  expect_arg_error(rg_train_labels(f, f, f, 0, i, i, i, i, cap, l, f, nullptr, nullptr),
                   "null edge_class, no node", "null pair");
  expect_arg_error(rg_train_labels(f, f, f, 100, nullptr, i, i, i, cap, l, f, l, nullptr),
                   "null track_key", "track_key");
  expect_arg_error(rg_train_labels(f, f, f, 100, i, i, i, i, cap, l, (float*)(uintptr_t)4100, l,
                                   nullptr),
                   "misaligned node_offsets", "aligned");
  expect_ok(rg_train_labels(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0,
                            nullptr, nullptr, nullptr, nullptr),
            "no node, no pair");

  // ---- rg_train_offsets
  void* ws = (void*)(uintptr_t)4096;
  const size_t need = rg_train_offsets_workspace_size(1000);
  if (need < 1001 * (2 * sizeof(int) + 2 * sizeof(float)) ||
      rg_train_offsets_workspace_size(0) == 0 || rg_train_offsets_workspace_size(-1) != 0) {
    std::fprintf(stderr, "rg_train_offsets_workspace_size: %zu for 1000 tracks\n", need);
    ++g_fail;
  }
  (void)rg_train_offsets_workspace_size(0x7ffffffe);  // no overflow on the way
  expect_arg_error(rg_train_offsets(i, -1, f, f, 100, f, f, ws, need, nullptr), "n_tracks < 0",
                   "n_tracks=-1");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, -1, f, f, ws, need, nullptr), "n_meas < 0",
                   "n_meas=-1");
  expect_arg_error(rg_train_offsets(i, 0x7fffffff, f, f, 100, f, f, ws, (size_t)1 << 40, nullptr),
                   "n_tracks + 1 past int32", "too large");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, 0x7fffffff, f, f, ws, need, nullptr),
                   "n_meas past the first-index sentinel", "too large");
  expect_arg_error(rg_train_offsets(nullptr, 1000, f, f, 100, f, f, ws, need, nullptr),
                   "null track_key", "null");
  expect_arg_error(rg_train_offsets(i, 1000, nullptr, f, 100, f, f, ws, need, nullptr), "null px",
                   "null");
  expect_arg_error(rg_train_offsets(i, 1000, f, nullptr, 100, f, f, ws, need, nullptr), "null py",
                   "null");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, 100, nullptr, f, ws, need, nullptr),
                   "null offset_x", "null");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, 100, f, nullptr, ws, need, nullptr),
                   "null offset_y", "null");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, 100, f, f, nullptr, need, nullptr),
                   "null workspace", "workspace");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, 100, f, f, ws, need - 1, nullptr),
                   "workspace one byte short", "workspace");
  expect_arg_error(rg_train_offsets(i, 1000, f, f, 100, f, f, (void*)(uintptr_t)4100, need, nullptr),
                   "misaligned workspace", "aligned");
  expect_ok(rg_train_offsets(nullptr, 1000, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0,
                             nullptr),
            "no measurement");
  return g_fail ? 1 : 0;
}
