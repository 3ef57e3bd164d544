// Host-side sanitizer driver for the sequence set's C ABI (csrc/sequence.hip), run by
// tests/test_sequence_set_host.py::test_sequence_set_host_code_under_asan_ubsan on the CPU.
//
// The library's host code is compiled with -fsanitize=address,undefined (host side only) and
// linked into this executable (build.build_sanitized_driver).  It drives the argument checks of
// rg_sequence_set_windows -- null table, windows and outputs, n_seq < 1, key_stride < 0, W < 1,
// negative sizes, n_windows * W and n_windows * key_stride at and past int32, a misaligned
// descriptor table -- each of which must return RG_ERR_ARG with a message before anything is
// launched; no GPU is needed.  The descriptors lie in device memory and are never read by the
// host, so the table pointer here is never dereferenced.  Any sanitizer report fails the test
// (the runtime aborts), as does a failed check.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "radar_gnn.h"

static int g_fail = 0;

static void expect_arg_error(int rc, const char* what, const char* needle) {
  const char* msg = rg_last_error();
  if (rc != RG_ERR_ARG || !msg || !std::strstr(msg, needle) ||
      !std::strstr(msg, "rg_sequence_set_windows")) {
    std::fprintf(stderr, "%s: expected RG_ERR_ARG mentioning '%s', got rc %d (%s)\n", what, needle,
                 rc, msg ? msg : "null");
    ++g_fail;
  }
}

static rg_window_batch outputs() {
  rg_window_batch o;
  void* f = (void*)(uintptr_t)4096;
  o.scan_ptr = o.scan_ref = o.win_ptr = o.meas_scan = o.src_row = o.track_key = (int*)f;
  o.mount = o.odometry = (double*)f;
  o.x_cc = o.y_cc = o.azimuth_sc = o.vr = o.vr_compensated = o.rcs = (float*)f;
  o.timestamp = o.sensor_id = o.label_id = (int64_t*)f;
  return o;
}

int main() {
  const rg_sequence* seqs = (const rg_sequence*)(uintptr_t)4096;
  const int* win = (const int*)(uintptr_t)4096;
  const long cap = 64L * 10 * 134;
  const int n_seq = 158, T = 500, big = 0x7fffffff;
  rg_window_batch o = outputs();
  expect_arg_error(rg_sequence_set_windows(nullptr, n_seq, T, win, 64, 10, cap, &o, nullptr),
                   "null seqs", "null");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, nullptr, 64, 10, cap, &o, nullptr),
                   "null win", "null");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 64, 10, cap, nullptr, nullptr),
                   "null out", "null");
  expect_arg_error(rg_sequence_set_windows(seqs, 0, T, win, 64, 10, cap, &o, nullptr), "n_seq = 0",
                   "n_seq=0");
  expect_arg_error(rg_sequence_set_windows(seqs, -1, T, win, 64, 10, cap, &o, nullptr),
                   "n_seq < 0", "n_seq=-1");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, -1, win, 64, 10, cap, &o, nullptr),
                   "key_stride < 0", "key_stride=-1");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 64, 0, cap, &o, nullptr), "W = 0",
                   "W=0");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 64, -1, cap, &o, nullptr), "W < 0",
                   "W=-1");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, -1, 10, cap, &o, nullptr),
                   "windows < 0", "n_windows=-1");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 64, 10, -1, &o, nullptr),
                   "capacity < 0", "capacity=-1");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 1 << 30, 2, cap, &o, nullptr),
                   "window-scans at 2^31", "windows of");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, big, big, cap, &o, nullptr),
                   "window-scans far past int32", "windows of");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, 1 << 25, win, 64, 10, cap, &o, nullptr),
                   "keys at 2^31", "int32");
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, big, win, big / 10, 10, cap, &o, nullptr),
                   "keys far past int32", "int32");
  expect_arg_error(rg_sequence_set_windows((const rg_sequence*)(uintptr_t)4100, n_seq, T, win, 64,
                                           10, cap, &o, nullptr),
                   "misaligned table", "aligned");
  o = outputs();
  o.win_ptr = nullptr;
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 64, 10, cap, &o, nullptr),
                   "null win_ptr", "per-scan");
  o = outputs();
  o.src_row = nullptr;
  expect_arg_error(rg_sequence_set_windows(seqs, n_seq, T, win, 64, 10, cap, &o, nullptr),
                   "null src_row", "per-measurement");
  return g_fail ? 1 : 0;
}
