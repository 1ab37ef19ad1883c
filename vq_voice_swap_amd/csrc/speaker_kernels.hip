// Speaker mix (include/vqvs.h, vqvs_speaker_mix): conditioning vectors made on the device from rows of a table,
//   out[b][e] = sum over the used slots j, in slot order, of w[b][j] * table[idx[b][j]][e].
// A voice has to be reproducible from its spec, so the arithmetic is fixed: every product and every sum is an fp32 operation rounded
// on its own (contraction off, the rule of the guidance mix in sampler_kernels.hip), and the first used slot's product is the initial
// value -- nothing is added to a zero, so one slot of weight 1 copies its row bit for bit (-0.0 and NaN payloads included).
//
// One thread per four entries of a row; blockIdx.y strides over the rows of the batch.  A thread reads its row's J indices and
// weights (wave-uniform addresses) and J quads of the table, and writes one quad.  Runs once per conversion: no tuning beyond 16-byte
// accesses where the shapes and pointers allow them.
#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace vqvs {

namespace {

constexpr int MIX_NT = 256;

// the row a slot names: negative = unused (the caller skips it), anything past the table is clamped to its last row
__device__ __forceinline__ int mix_row(int idx, int K) { return idx >= K ? K - 1 : idx; }

__device__ __forceinline__ float mix_mul(float w, float v) {
#pragma clang fp contract(off)
  return w * v;
}

__device__ __forceinline__ float mix_add(float acc, float p) {
#pragma clang fp contract(off)
  return acc + p;
}

// VEC: E % 4 == 0 and table / out on 16 bytes (the launcher checks): a thread owns quad q of a row.  Otherwise a thread owns the (up
// to) four floats [4 q, 4 q + 4) of the row one at a time.
template <bool VEC>
__global__ __launch_bounds__(MIX_NT) void speaker_mix_kernel(const float* table, int K, int E, const int* idx, const float* w, int J, float* out, int B) {
  const int q = blockIdx.x * MIX_NT + threadIdx.x;
  const int e0 = q * 4;
  if (e0 >= E) return;
  const int ne = VEC ? 4 : min(4, E - e0);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
    for (int j = 0; j < J; ++j) {
      const int id = idx[(size_t)b * J + j];
      if (id < 0) continue;
      const float wj = w[(size_t)b * J + j];
      const float* row = table + (size_t)mix_row(id, K) * E + e0;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (VEC) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(row);
        v[0] = r[0], v[1] = r[1], v[2] = r[2], v[3] = r[3];
      } else {
        for (int k = 0; k < ne; ++k) v[k] = row[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float p = mix_mul(wj, v[k]);
        acc[k] = any ? mix_add(acc[k], p) : p;
      }
      any = true;
    }
    float* o = out + (size_t)b * E + e0;
    if (VEC) {
      *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    } else {
      for (int k = 0; k < ne; ++k) o[k] = acc[k];
    }
  }
}

}  // namespace

int run_speaker_mix(const float* table, int K, int E, const int* idx, const float* w, int J, float* out, int B, hipStream_t st) {
  const bool vec = E % 4 == 0 && (reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
  const int quads = (E + 3) / 4;
  const dim3 grid((quads + MIX_NT - 1) / MIX_NT, std::min(B, 1024));
  if (vec)
    hipLaunchKernelGGL((speaker_mix_kernel<true>), grid, dim3(MIX_NT), 0, st, table, K, E, idx, w, J, out, B);
  else
    hipLaunchKernelGGL((speaker_mix_kernel<false>), grid, dim3(MIX_NT), 0, st, table, K, E, idx, w, J, out, B);
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
