// The counter-based normal generator shared by every kernel that draws noise (sampler_kernels.hip, loss_kernels.hip).
#pragma once
#include "common.hpp"

namespace vqvs {

// stream ids in use (the last counter word): 0 = the reverse step's noise, 1 = x_T, 2 = the forward process' epsilon
// (vqvs_ddpm_noise / vqvs_ddpm_sqerr), 3 = the noise that puts a kept region back on the source's forward process (vqvs_keep_region)
constexpr uint32_t PHILOX_STREAM_STEP = 0u, PHILOX_STREAM_XT = 1u, PHILOX_STREAM_LOSS = 2u, PHILOX_STREAM_KEEP = 3u;

// ---------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011), keyed by the sampler seed; the counter carries
// (quad index within the clip, GLOBAL clip index, step index, stream id) so a clip's noise
// does not depend on which GPU or batch slot it is sampled in.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0;
  c[1] = (uint32_t)p1;
  c[2] = n2;
  c[3] = (uint32_t)p0;
}

__device__ __forceinline__ f32x4 philox_normal4(uint64_t seed, uint32_t quad, uint64_t clip, uint32_t step, uint32_t stream_id) {
  uint32_t c[4] = {quad, (uint32_t)clip, step, stream_id ^ ((uint32_t)(clip >> 32) << 8)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  // Box-Muller on (0,1] x [0,1)
  const float u0 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
  const float u2 = ((float)(c[2] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u3 = (float)(c[3] >> 8) * (1.0f / 16777216.0f);
  const float r0 = sqrtf(-2.0f * logf(u0));
  const float r1 = sqrtf(-2.0f * logf(u2));
  float s0, c0, s1, c1;
  sincosf(6.28318530717958647692f * u1, &s0, &c0);
  sincosf(6.28318530717958647692f * u3, &s1, &c1);
  return f32x4{r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}

}  // namespace vqvs
