// Host-side sanitizer driver for the sequence store's C ABI (csrc/sequence.hip), run by
// tests/test_sequence_host.py::test_sequence_host_code_under_asan_ubsan on the CPU.
//
// The library's host code is compiled with -fsanitize=address,undefined (host side only) and
// linked into this executable (build.build_sanitized_driver).  It drives the argument checks of
// rg_sequence_windows -- null structs, tables, fields and outputs, W < 1, negative sizes,
// n_windows * W and n_windows * n_tracks at and past int32, a misaligned scene table -- each of
// which must return RG_ERR_ARG with a message before anything is launched; no GPU is needed.
// Any sanitizer report fails the test (the runtime aborts), as does a failed check.
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

static rg_sequence sequence() {
  // never dereferenced: every call below fails its checks first
  rg_sequence s;
  const void* f = (const void*)(uintptr_t)4096;
  s.scenes = (const int*)f;
  s.mount = (const double*)f;
  s.odometry = (const double*)f;
  s.x_cc = s.y_cc = s.azimuth_sc = s.vr = s.vr_compensated = s.rcs = (const float*)f;
  s.timestamp = (const int64_t*)f;
  s.sensor_id = s.label_id = (const uint8_t*)f;
  s.track_key = (const int*)f;
  s.n_scenes = 6011;
  s.n_sensors = 4;
  s.n_odometry = 7000;
  s.n_meas = 803760;
  s.n_tracks = 500;
  return s;
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
  const int* first = (const int*)(uintptr_t)4096;
  const long cap = 64L * 10 * 134;
  rg_sequence s = sequence();
  rg_window_batch o = outputs();
  expect_arg_error(rg_sequence_windows(nullptr, first, 64, 10, cap, &o, nullptr), "null seq", "null");
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, nullptr, nullptr), "null out", "null");
  expect_arg_error(rg_sequence_windows(&s, nullptr, 64, 10, cap, &o, nullptr), "null win_first",
                   "null");
  expect_arg_error(rg_sequence_windows(&s, first, 64, 0, cap, &o, nullptr), "W = 0", "W=0");
  expect_arg_error(rg_sequence_windows(&s, first, 64, -1, cap, &o, nullptr), "W < 0", "W=-1");
  expect_arg_error(rg_sequence_windows(&s, first, -1, 10, cap, &o, nullptr), "windows < 0",
                   "n_windows=-1");
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, -1, &o, nullptr), "capacity < 0",
                   "capacity=-1");
  expect_arg_error(rg_sequence_windows(&s, first, 1 << 30, 2, cap, &o, nullptr),
                   "window-scans at 2^31", "windows of");
  expect_arg_error(rg_sequence_windows(&s, first, 0x7fffffff, 0x7fffffff, cap, &o, nullptr),
                   "window-scans far past int32", "windows of");
  s = sequence();
  s.n_tracks = 1 << 25;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "keys at 2^31", "int32");
  s.n_tracks = 0x7fffffff;
  expect_arg_error(rg_sequence_windows(&s, first, 0x7fffffff / 10, 10, cap, &o, nullptr),
                   "keys far past int32", "int32");
  for (int which = 0; which < 5; ++which) {
    s = sequence();
    (which == 0 ? s.n_scenes : which == 1 ? s.n_sensors : which == 2 ? s.n_odometry
     : which == 3 ? s.n_meas : s.n_tracks) = -1;
    expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "negative size",
                     "negative");
  }
  s = sequence();
  s.scenes = nullptr;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "null scenes", "table");
  s = sequence();
  s.mount = nullptr;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "null mount", "table");
  s = sequence();
  s.odometry = nullptr;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "null odometry",
                   "table");
  s = sequence();
  s.label_id = nullptr;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "null field",
                   "measurement");
  s = sequence();
  s.scenes = (const int*)(uintptr_t)4100;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "misaligned scenes",
                   "aligned");
  s = sequence();
  o = outputs();
  o.win_ptr = nullptr;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "null win_ptr",
                   "per-scan");
  o = outputs();
  o.src_row = nullptr;
  expect_arg_error(rg_sequence_windows(&s, first, 64, 10, cap, &o, nullptr), "null src_row",
                   "per-measurement");
  return g_fail ? 1 : 0;
}
