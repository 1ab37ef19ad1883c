// Pauses of a pack of recordings (include/vqvs.h, vqvs_pause_mask and vqvs_windows_kept): which samples of
// the padded source rows lie in a pause, as the uint8 mask the keep region takes, and which windows such a mask covers whole.  The
// definition is in integers, as the YIN kernel's is: samples are quantised to the 16 bits a WAV would hold, a frame's energy is an
// exact integer sum, and a frame is quiet iff E <= thr * (its sample count).  Integer sums are the same in any order, so a
// recording's mask depends on its own samples alone: not on R, on its place in the pack, or on the run.
//
// A recording's frames are cut into CHUNKS of PM_CH; chunk c of recording r owns slot floor(off_r / S) + r + c of the scratch
// (S = PM_CH * frame samples), which no other chunk can own since consecutive recordings' first slots differ by floor(L_r / S) + 1
// or more, and which the host can bound without knowing N.  Three launches, the first and third on a grid of (chunk stride,
// recording) -- a recording is found by its index, not by a search:
//   pause_energy_kernel  per frame E and the quiet flag, parked in the FIRST byte of the frame's span of the mask; per chunk the last
//                        and the first loud frame (-1 / INT_MAX without one) into the chunk's slot
//   pause_carry_kernel   one wave per recording: exclusive forward max-scan of the last loud frames and backward min-scan of the first
//                        ones over the recording's slots, in place -- what a chunk needs to know of the frames outside it
//   pause_expand_kernel  per chunk the flags back from the mask, left(f) / right(f) from the wave ballots and the carries, the
//                        four conditions of the scan form, the counts, and the chunk's span of the mask written whole
// A frame is kept iff quiet(f), right - left - 1 >= min_frames, (left < 0 or f - left > guard) and (right >= F or right - f > guard),
// with left(f) the last loud frame <= f or -1 and right(f) the first loud frame >= f or F.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "kernels.hpp"
#include "pack_table.hpp"

namespace vqvs {

namespace {

constexpr int PM_CH = 256;  // frames per chunk: one per thread of the expansion's workgroup

struct PauseArgs {
  const float* x;
  uint8_t* keep;
  const int* first;
  int *last_loud, *first_loud;  // scratch, one entry per slot
  long long* counts;            // [R, 2] or nullptr
  int R, W, H, frame, g;        // g: lanes per frame of the energy pass, a power of two <= min(frame / 4, 64)
  long long thr;
  int min_frames, guard;
  bool x_vec, keep_vec;  // 16-byte loads of x / 4-byte stores of the mask are aligned
};

struct PauseRow {
  int64_t off, L;  // first sample in the pack, samples
  int F, C;        // frames, chunks
  int64_t slot;    // the first chunk's slot
  bool ok;         // (always, unless the table is not one of prefix sums)
};
__device__ __forceinline__ PauseRow pause_row(const PackTable& t, int r, int frame) {
  const int f0 = t.at(r), f1 = t.at(r + 1);
  PauseRow w;
  w.off = t.off(r, f0);
  w.L = (int64_t)(f1 - f0) * t.H + t.V;
  w.ok = f1 > f0 && w.off + w.L <= t.total();
  w.F = (int)((w.L + frame - 1) / frame);
  w.C = (w.F + PM_CH - 1) / PM_CH;
  w.slot = w.off / ((int64_t)PM_CH * frame) + r;
  return w;
}

__device__ __forceinline__ long long wave_sum(long long v, int width) {
  for (int o = 1; o < width; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void pause_energy_kernel(const PauseArgs a) {
  __shared__ int s_last, s_first;
  const PackTable t = pack_table(a.first, a.R, a.W, a.H);
  const PauseRow w = pause_row(t, blockIdx.y, a.frame);
  if (!w.ok) return;  // (uniform)
  const int tid = threadIdx.x, sub = tid / a.g, li = tid % a.g, per = 256 / a.g;
  const float* x = a.x + w.off;
  for (int c = blockIdx.x; c < w.C; c += gridDim.x) {
    if (tid == 0) s_last = -1, s_first = INT_MAX;
    __syncthreads();
    for (int fb = 0; fb < PM_CH; fb += per) {
      const int f = c * PM_CH + fb + sub;
      const bool valid = f < w.F;
      const int64_t start = (int64_t)f * a.frame;
      const int cnt = valid ? (int)min((int64_t)a.frame, w.L - start) : 0;  // a multiple of 4, as L and frame are
      long long e = 0;
      for (int j = li * 4; j < cnt; j += a.g * 4) {
        int q[4];
        if (a.x_vec) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + start + j);
          for (int k = 0; k < 4; ++k) q[k] = quantise(v[k]);
        } else {
          for (int k = 0; k < 4; ++k) q[k] = quantise(x[start + j + k]);
        }
        for (int k = 0; k < 4; ++k) e += (long long)q[k] * q[k];
      }
      e = wave_sum(e, a.g);
      if (valid && li == 0) {
        const bool quiet = e <= a.thr * cnt;
        a.keep[w.off + start] = quiet ? 1 : 0;
        if (!quiet) atomicMax(&s_last, f), atomicMin(&s_first, f);
      }
    }
    __syncthreads();
    if (tid == 0) a.last_loud[w.slot + c] = s_last, a.first_loud[w.slot + c] = s_first;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void pause_carry_kernel(const PauseArgs a) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.R) return;  // (uniform over the wave)
  if (a.counts && lane < 2) a.counts[2 * (size_t)r + lane] = 0;
  const PackTable t = pack_table(a.first, a.R, a.W, a.H);
  const PauseRow w = pause_row(t, r, a.frame);
  if (!w.ok) return;
  int* last = a.last_loud + w.slot;
  int* first = a.first_loud + w.slot;
  int carry = -1;  // the last loud frame of the chunks before `base`
  for (int base = 0; base < w.C; base += 64) {
    const int c = base + lane;
    int v = c < w.C ? last[c] : -1;
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(v, o, 64);
      if (lane >= o) v = max(v, up);
    }
    const int before = __shfl_up(v, 1, 64);
    if (c < w.C) last[c] = lane ? max(carry, before) : carry;
    carry = max(carry, __shfl(v, 63, 64));
  }
  carry = INT_MAX;  // the first loud frame of the chunks behind `base` + 63
  for (int base = (w.C - 1) / 64 * 64; base >= 0; base -= 64) {
    const int c = base + lane;
    int v = c < w.C ? first[c] : INT_MAX;
    for (int o = 1; o < 64; o <<= 1) {
      const int dn = __shfl_down(v, o, 64);
      if (lane + o < 64) v = min(v, dn);
    }
    const int after = __shfl_down(v, 1, 64);
    if (c < w.C) first[c] = lane < 63 ? min(carry, after) : carry;
    carry = min(carry, __shfl(v, 0, 64));
  }
}

__global__ __launch_bounds__(256) void pause_expand_kernel(const PauseArgs a) {
  __shared__ unsigned long long s_loud[4];
  __shared__ uint8_t s_kept[PM_CH];
  const PackTable t = pack_table(a.first, a.R, a.W, a.H);
  const int r = blockIdx.y;
  const PauseRow w = pause_row(t, r, a.frame);
  if (!w.ok) return;  // (uniform)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint8_t* keep = a.keep + w.off;
  for (int c = blockIdx.x; c < w.C; c += gridDim.x) {
    const int f0 = c * PM_CH, f = f0 + tid;
    const bool valid = f < w.F;
    const bool quiet = valid && keep[(int64_t)f * a.frame] != 0;
    const unsigned long long loud = __ballot(valid && !quiet);
    if (lane == 0) s_loud[wave] = loud;
    __syncthreads();
    int left = a.last_loud[w.slot + c], right = min(a.first_loud[w.slot + c], w.F);
    for (int v = 0; v < wave; ++v)
      if (s_loud[v]) left = f0 + v * 64 + 63 - __clzll((long long)s_loud[v]);
    for (int v = 3; v > wave; --v)
      if (s_loud[v]) right = f0 + v * 64 + __ffsll((long long)s_loud[v]) - 1;
    const unsigned long long upto = loud & (lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull), from = loud & (~0ull << lane);
    if (upto) left = f0 + wave * 64 + 63 - __clzll((long long)upto);
    if (from) right = f0 + wave * 64 + __ffsll((long long)from) - 1;
    const bool pause = quiet && right - left - 1 >= a.min_frames;
    const bool kept = pause && (left < 0 || f - left > a.guard) && (right >= w.F || right - f > a.guard);
    s_kept[tid] = kept ? 1 : 0;
    if (a.counts) {
      const long long samples = wave_sum(kept ? min((int64_t)a.frame, w.L - (int64_t)f * a.frame) : 0, 64);
      const long long pauses = wave_sum(pause && left == f - 1 ? 1 : 0, 64);  // (a pause is counted at its first frame)
      if (lane == 0) {
        if (samples) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + 2 * (size_t)r), (unsigned long long)samples);
        if (pauses) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + 2 * (size_t)r + 1), (unsigned long long)pauses);
      }
    }
    __syncthreads();
    const int64_t base = (int64_t)f0 * a.frame;
    const int span = (int)min((int64_t)PM_CH * a.frame, w.L - base);  // a multiple of 4
    for (int j = tid * 4; j < span; j += 1024) {
      const uint8_t v = s_kept[j / a.frame];  // (frame % 4 == 0: the four bytes lie in one frame)
      if (a.keep_vec) {
        *reinterpret_cast<uint32_t*>(keep + base + j) = v ? 0x01010101u : 0u;
      } else {
        for (int k = 0; k < 4; ++k) keep[base + j + k] = v;
      }
    }
    __syncthreads();
  }
}

// out[b] = every byte of window b's span of the mask is non-zero; one window per workgroup and stride
__global__ __launch_bounds__(256) void windows_kept_kernel(const uint8_t* keep, uint8_t* out, const int* first, int R, int W, int H, bool vec) {
  const PackTable t = pack_table(first, R, W, H);
  for (int b = blockIdx.x; b < t.N; b += gridDim.x) {
    const int64_t start = t.off(pack_window_row(t, b), b);
    const bool inside = start + W <= t.total();  // (always, unless the table is not one of prefix sums)
    bool all = inside;
    if (inside) {
      const uint8_t* m = keep + start;
      for (int j = threadIdx.x * 4; j < W; j += 1024) {
        if (vec) {
          const uint32_t v = *reinterpret_cast<const uint32_t*>(m + j);
          all = all && (v & 0xffu) && (v & 0xff00u) && (v & 0xff0000u) && (v & 0xff000000u);
        } else {
          for (int k = 0; k < 4; ++k) all = all && m[j + k];
        }
      }
    }
    const int every = __syncthreads_and(all ? 1 : 0);
    if (threadIdx.x == 0) out[b] = every ? 1 : 0;
  }
}

// the most slots a pack of this geometry can own: its samples are at most min(65535 H + R V, 2^31)
size_t pause_slots(int R, int W, int H, int frame) {
  const int64_t most = std::min<int64_t>((int64_t)65535 * H + (int64_t)R * (W - H), (int64_t)1 << 31);
  return (size_t)(most / ((int64_t)PM_CH * frame) + R + 1);
}

}  // namespace

size_t pause_mask_scratch_bytes(int R, int W, int H, int frame) { return pause_slots(R, W, H, frame) * 2 * sizeof(int); }

int run_pause_mask(const float* x, uint8_t* keep, long long* counts, const int* first, void* scratch, int R, int W, int H, int frame,
                   long long thr, int min_frames, int guard_frames, hipStream_t st) {
  if (R < 1 || R > 65535 || frame < 4 || frame > 4096 || frame % 4 || thr < 0 || thr > (1ll << 30))
    VQVS_FAIL(-1, "pause mask: R=%d frame=%d thr=%lld outside the kernel's limits", R, frame, thr);
  PauseArgs a;
  a.x = x, a.keep = keep, a.first = first, a.counts = counts;
  a.last_loud = static_cast<int*>(scratch);
  a.first_loud = a.last_loud + pause_slots(R, W, H, frame);
  a.R = R, a.W = W, a.H = H, a.frame = frame, a.thr = thr, a.min_frames = min_frames, a.guard = guard_frames;
  a.g = 1;
  while (a.g * 2 <= std::min(frame / 4, 64)) a.g *= 2;
  a.x_vec = reinterpret_cast<uintptr_t>(x) % 16 == 0;
  a.keep_vec = reinterpret_cast<uintptr_t>(keep) % 4 == 0;
  const dim3 grid(std::max(1, 2048 / R), R);  // about 2048 workgroups or one per recording, whichever is more
  hipLaunchKernelGGL(pause_energy_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(pause_carry_kernel, dim3((R + 3) / 4), dim3(256), 0, st, a);
  hipLaunchKernelGGL(pause_expand_kernel, grid, dim3(256), 0, st, a);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_windows_kept(const uint8_t* keep, uint8_t* out, const int* first, int R, int W, int H, hipStream_t st) {
  hipLaunchKernelGGL(windows_kept_kernel, dim3(2048), dim3(256), 0, st, keep, out, first, R, W, H, reinterpret_cast<uintptr_t>(keep) % 4 == 0);
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
