// Counter-based random numbers for the training step's noise (K12) and augmentation (K17): Philox4x32-10 as Random123 /
// cuRAND define it, and the one draw layout every consumer and its "draws written out" twin share.
//
// A draw is a pure function of (seed, offset, image b, group g): nothing depends on the batch size, the grid or the
// launch.   key     = (seed & 0xffffffff, seed >> 32)
//           counter = (g, b, offset & 0xffffffff, offset >> 32)
//   g < 0xFFFFFFFD  normals: the four words x0..x3 of block g are elements 4g .. 4g+3 of image b,
//                   ua = ((x0 >> 9) + 0.5) * 2^-23 in (0,1), ub = (x1 >> 8) * 2^-24, R = sqrt(-2 ln ua),
//                   z0 = R cos(2 pi ub), z1 = R sin(2 pi ub); x2, x3 give z2, z3 the same way  (Box-Muller, fp32)
//   g = 0xFFFFFFFF  word 0: the per-image uniform y of the exponential sampler, y = (x0 >> 8) * 2^-24 in [0,1)
//   g = 0xFFFFFFFE  words 0..3: the augmentation uniforms u0..u3 of image b (same conversion as y)
//   g = 0xFFFFFFFD  word 0: u4, the augmentation's Bernoulli draw (apply = u4 < p)
//                   words 1, 2: balanced sampling's index of image b (pointwise.h: balanced_index_rng), integers only:
//                   class j = (x1 * Kn) >> 32 among the Kn non-empty classes, member m = (x2 * cnt_j) >> 32 of its cnt_j.
//                   Multiply-high maps 2^32 words onto cnt values: each value gets floor or ceil of 2^32 / cnt words,
//                   so a probability is off from 1 / cnt by less than 2^-32 (relative bias at most cnt / 2^32)
//                   word 3: free
// The image word b is the image's place in the batch for the training step's consumers.  Held-out validation
// (noise_blend_fixed_index_rng_kernel, loss.hip) puts the image's place in its DATASET there instead, b = index[b] in
// [0, 2^32): the draws of a held-out image then depend on nothing but (seed, offset, the image), not on the batch size or
// the batch it arrives in.  The layout of the groups g is the same.
// The python side packs offset = global_step << 24 | rank << 8 | stream (rng.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define D3F_HD __host__ __device__ __forceinline__
#else
#define D3F_HD inline
#endif

namespace d3f {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;  // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;  // Weyl key increments
constexpr uint32_t RNG_G_Y = 0xFFFFFFFFu, RNG_G_AUG = 0xFFFFFFFEu, RNG_G_APPLY = 0xFFFFFFFDu;

struct Philox4 {
  uint32_t x[4];
};

D3F_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += PHILOX_W0;  // the key is bumped after every round
    k1 += PHILOX_W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// block g of image b in the stream (seed, offset)
D3F_HD Philox4 rng_block(uint64_t seed, uint64_t offset, uint32_t b, uint32_t g) {
  return philox4x32_10(g, b, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// [0, 1) on the 2^-24 grid, as torch.rand
D3F_HD float rng_uniform24(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }

#if defined(__HIPCC__)
// the four standard normals of block g: accurate logf / sqrtf / sincospif, every step rounded to fp32
__device__ __forceinline__ float4 rng_normal4(uint64_t seed, uint64_t offset, uint32_t b, uint32_t g) {
  const Philox4 p = rng_block(seed, offset, b, g);
  const float ua0 = ((float)(p.x[0] >> 9) + 0.5f) * 0x1p-23f, ua1 = ((float)(p.x[2] >> 9) + 0.5f) * 0x1p-23f;
  const float r0 = sqrtf(-2.0f * logf(ua0)), r1 = sqrtf(-2.0f * logf(ua1));
  float s0, c0, s1, c1;
  sincospif(2.0f * rng_uniform24(p.x[1]), &s0, &c0);
  sincospif(2.0f * rng_uniform24(p.x[3]), &s1, &c1);
  return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}
__device__ __forceinline__ float rng_y(uint64_t seed, uint64_t offset, uint32_t b) {
  return rng_uniform24(rng_block(seed, offset, b, RNG_G_Y).x[0]);
}
#endif

}  // namespace d3f
