// What the SSIM kernels of loss.hip (the criterion and its gradient) and quality.hip (the per-image, forward-only
// scores) share: the tile geometry, the 11 fp32 taps and the [0, 1] normalisation of
// d3f/loss_functions/structural_similarity_loss.py:14-26 (piqa.SSIM defaults).
#pragma once
#include <math.h>

#include "common.h"

namespace d3f {

constexpr int SS_T = 32;            // tile edge (outputs)
constexpr int SS_K = 11;            // window
constexpr int SS_IN = SS_T + SS_K - 1;  // 42
constexpr int SS_LD = SS_IN + 1;        // 43: odd stride -> conflict-free column walks
constexpr int SS_FILL = (SS_IN * SS_IN + 255) / 256;  // 7: elements of the input tile per thread

struct GaussK {
  float g[SS_K];
};
typedef float f32x2 __attribute__((ext_vector_type(2)));  // a register pair for the packed fp32 instructions

static GaussK make_gauss() {
  GaussK k;
  // same arithmetic as the oracle (float32 throughout)
  float s = 0.f;
  for (int i = 0; i < SS_K; ++i) {
    const float d = (float)i - (float)(SS_K - 1) / 2.f;
    k.g[i] = expf(-(d * d) / (2.f * 1.5f * 1.5f));
    s += k.g[i];
  }
  for (int i = 0; i < SS_K; ++i) k.g[i] /= s;
  return k;
}

__device__ __forceinline__ float norm01(float v, float lo, float range) {
  const float t = (v - lo) / range;  // same op order as structural_similarity_loss.py:24
  return fminf(fmaxf(t, 0.f), 1.f);
}

}  // namespace d3f
