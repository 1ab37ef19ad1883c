// The table walk of a PACK of recordings (include/vqvs.h "Packed window steps"), shared by the kernels that run
// on one: the packed steps and the packed keep region (sampler_kernels.hip), the pause detector and the kept-window test
// (pause_kernels.hip).  `first` [R + 1] holds the prefix sums of the window counts: recording r owns windows first[r] ..
// first[r + 1] - 1 and starts at sample first[r] * H + r * V of the long arrays (every row is n_r * H + V long).  Table entries are
// clamped to 0..N and N to 1..65535, so a malformed table cannot send an access outside N * H + R * V samples or N windows.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vqvs {

struct PackRow {
  int r, fb, n, q;  // recording, its first window, its window count, the quad's index in the recording's own row
  bool ok;          // the quad lies in that row: a quad that a malformed table puts nowhere is left alone
  size_t off;       // the recording's first sample in the long arrays
};
struct PackTable {
  const int* first;
  int R, N, H, V;
  __device__ __forceinline__ int at(int i) const { return i <= 0 ? 0 : i >= R ? N : min(max(first[i], 0), N); }
  __device__ __forceinline__ int64_t off(int i, int f) const { return (int64_t)f * H + (int64_t)i * V; }
  __device__ __forceinline__ int64_t total() const { return min(off(R, N), ((int64_t)1 << 31) - 4); }
};
__device__ __forceinline__ PackTable pack_table(const int* first, int R, int W, int H) {
  return PackTable{first, R, min(max(first[R], 1), 65535), H, W - H};
}
// p0: a position at or before p that is uniform over the workgroup (its first thread's)
__device__ __forceinline__ PackRow pack_row(const PackTable& t, int64_t p0, int64_t p) {
  int lo = 0, hi = t.R;  // off(lo) <= p0 < off(hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.off(mid, t.at(mid)) <= p0) lo = mid; else hi = mid;
  }
  int r = lo, f0 = t.at(r), f1 = t.at(r + 1);
  while (r + 1 < t.R && t.off(r + 1, f1) <= p) {
    ++r;
    f0 = f1;
    f1 = t.at(r + 1);
  }
  PackRow w;
  w.r = r;
  w.n = f1 - f0;
  w.fb = f0;
  w.off = (size_t)t.off(r, f0);
  const int64_t u = p - t.off(r, f0);
  w.ok = w.n >= 1 && u >= 0 && u < (int64_t)w.n * t.H + t.V;  // (always, unless the table is not one of prefix sums)
  w.q = (int)(u / 4);
  return w;
}
// window b's recording: the last r with first[r] <= b (b uniform over the workgroup: scalar loads again)
__device__ __forceinline__ int pack_window_row(const PackTable& t, int b) {
  int lo = 0, hi = t.R;  // at(lo) <= b < at(hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.at(mid) <= b) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace vqvs
