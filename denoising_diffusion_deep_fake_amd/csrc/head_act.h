// The activation behind the segmentation head: smp's Activation module, which smp.Unet applies last in
// segmentation_head (the reference passes activation=None, d3f/train_denoiser/lit_module.py:46-52).  One __device__
// function per activation and direction over the channel vector of ONE pixel; every kernel of head_act.hip inlines
// them, so the stand-alone forward kernel and the fused uint8 epilogue produce the same bits.  All arithmetic is fp32.
#pragma once
#include "common.h"

namespace d3f {

// (the values of D3F_ACT_* in include/d3f_hip.h)
enum HeadAct { HEAD_ACT_IDENTITY, HEAD_ACT_SIGMOID, HEAD_ACT_TANH, HEAD_ACT_SOFTMAX, HEAD_ACT_LOGSOFTMAX, HEAD_ACT_CLAMP,
               HEAD_ACT_COUNT };
constexpr int HEAD_ACT_MAXC = 16;  // the engine's limit on `classes`

// The channel loops run over all HEAD_ACT_MAXC slots under `c < C`, fully unrolled: the vector stays in registers.

// ---- forward: v = z on entry, a on return ---------------------------------------------------------------------------
__device__ __forceinline__ void head_sigmoid_fwd(float (&v)[HEAD_ACT_MAXC], int C) {
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) v[c] = 1.f / (1.f + expf(-v[c]));  // (expf overflows to inf for z < -88.7: 1 / inf = 0)
}
__device__ __forceinline__ void head_tanh_fwd(float (&v)[HEAD_ACT_MAXC], int C) {
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) v[c] = tanhf(v[c]);
}
// m = the channel maximum, then v = exp(z - m); returns the sum of those over the channels (in channel order)
__device__ __forceinline__ float head_exp_shifted(float (&v)[HEAD_ACT_MAXC], int C, float& m) {
  m = v[0];
#pragma unroll
  for (int c = 1; c < HEAD_ACT_MAXC; ++c)
    if (c < C) m = fmaxf(m, v[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) {
      v[c] = expf(v[c] - m);
      s += v[c];
    }
  return s;
}
__device__ __forceinline__ void head_softmax_fwd(float (&v)[HEAD_ACT_MAXC], int C) {
  float m;
  const float s = head_exp_shifted(v, C, m);
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) v[c] = v[c] / s;
}
__device__ __forceinline__ void head_logsoftmax_fwd(float (&v)[HEAD_ACT_MAXC], int C) {
  float e[HEAD_ACT_MAXC], m;
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c) e[c] = v[c];
  const float ls = logf(head_exp_shifted(e, C, m));
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) v[c] = (v[c] - m) - ls;
}
__device__ __forceinline__ void head_clamp_fwd(float (&v)[HEAD_ACT_MAXC], int C) {
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) v[c] = fminf(fmaxf(v[c], 0.f), 1.f);
}

// ---- backward: z as the forward saw it, g = the upstream gradient on entry, dz on return ----------------------------
// (a is recomputed from z by the forward function above: the engine keeps z, not a)
__device__ __forceinline__ void head_sigmoid_bwd(float (&z)[HEAD_ACT_MAXC], float (&g)[HEAD_ACT_MAXC], int C) {
  head_sigmoid_fwd(z, C);
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) g[c] = g[c] * z[c] * (1.f - z[c]);
}
__device__ __forceinline__ void head_tanh_bwd(float (&z)[HEAD_ACT_MAXC], float (&g)[HEAD_ACT_MAXC], int C) {
  head_tanh_fwd(z, C);
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) g[c] = g[c] * (1.f - z[c] * z[c]);
}
__device__ __forceinline__ void head_softmax_bwd(float (&z)[HEAD_ACT_MAXC], float (&g)[HEAD_ACT_MAXC], int C) {
  head_softmax_fwd(z, C);
  float dot = 0.f;  // sum_k g_k a_k
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) dot += g[c] * z[c];
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) g[c] = z[c] * (g[c] - dot);
}
__device__ __forceinline__ void head_logsoftmax_bwd(float (&z)[HEAD_ACT_MAXC], float (&g)[HEAD_ACT_MAXC], int C) {
  head_logsoftmax_fwd(z, C);
  float sum = 0.f;  // sum_k g_k
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) sum += g[c];
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) g[c] = g[c] - expf(z[c]) * sum;
}
// torch's rule for clamp: the gradient passes where lo <= z <= hi, bounds included
__device__ __forceinline__ void head_clamp_bwd(float (&z)[HEAD_ACT_MAXC], float (&g)[HEAD_ACT_MAXC], int C) {
#pragma unroll
  for (int c = 0; c < HEAD_ACT_MAXC; ++c)
    if (c < C) g[c] = (z[c] >= 0.f && z[c] <= 1.f) ? g[c] : 0.f;
}

template <int ACT> __device__ __forceinline__ void head_act_fwd(float (&v)[HEAD_ACT_MAXC], int C) {
  if constexpr (ACT == HEAD_ACT_SIGMOID) head_sigmoid_fwd(v, C);
  if constexpr (ACT == HEAD_ACT_TANH) head_tanh_fwd(v, C);
  if constexpr (ACT == HEAD_ACT_SOFTMAX) head_softmax_fwd(v, C);
  if constexpr (ACT == HEAD_ACT_LOGSOFTMAX) head_logsoftmax_fwd(v, C);
  if constexpr (ACT == HEAD_ACT_CLAMP) head_clamp_fwd(v, C);
}
template <int ACT>
__device__ __forceinline__ void head_act_bwd(float (&z)[HEAD_ACT_MAXC], float (&g)[HEAD_ACT_MAXC], int C) {
  if constexpr (ACT == HEAD_ACT_SIGMOID) head_sigmoid_bwd(z, g, C);
  if constexpr (ACT == HEAD_ACT_TANH) head_tanh_bwd(z, g, C);
  if constexpr (ACT == HEAD_ACT_SOFTMAX) head_softmax_bwd(z, g, C);
  if constexpr (ACT == HEAD_ACT_LOGSOFTMAX) head_logsoftmax_bwd(z, g, C);
  if constexpr (ACT == HEAD_ACT_CLAMP) head_clamp_bwd(z, g, C);
}

// ---- launches (head_act.hip) -------------------------------------------------------------------------------------------
// host-side argument check of the two launches below (nothing is enqueued)
int head_act_check(int act, int C, int Cpad);
// a = act(z), both NCHW fp32 [B][C][H][W].  Two networks in one launch (common.h, NetSplit): z is a workspace tensor
// (ns->ws), a the caller's prediction (ns->out).
int head_act_forward_launch(int act, const float* z, float* a, int B, int C, int H, int W, hipStream_t stream,
                            const NetSplit* ns = nullptr);
// (z, g) NCHW fp32 -> dz twice: NCHW fp32 (the bias gradient's channel sum reads it) and NHWC in the storage dtype
// [B][H][W][Cpad], rounded once from the fp32 dz, padding channels zero (the head's data and weight gradients read it).
// dz_nchw may be z itself (in place); no other two of the buffers may overlap.
// Two networks: z, dz_nchw and dy_nhwc are workspace tensors (ns->ws), g is the caller's output gradient (ns->in).
int head_act_backward_launch(int act, int dtype, const float* z, const float* g, float* dz_nchw, void* dy_nhwc, int B, int C,
                             int H, int W, int Cpad, hipStream_t stream, const NetSplit* ns = nullptr);
// nchw_to_u8bgr_launch (pointwise.h, K16) with the activation applied to the three channels first
int head_act_to_u8bgr_launch(int act, const float* z, uint8_t* out, int B, int H, int W, long out_row_stride,
                             const float mean255[3], const float std255[3], hipStream_t stream);

}  // namespace d3f
