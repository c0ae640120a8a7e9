// Kernels of the segmentation head's activation (head_act.h): the forward a = act(z), the head of the backward pass
// (z, g) -> dz in the two layouts its consumers read, and the uint8 epilogue of the inference entries with the
// activation applied first.  One thread owns a pixel and walks its C <= 16 channels in registers: loads and stores of
// the NCHW tensors are coalesced along HW, and the channel softmax needs no cross-lane work.
#include "head_act.h"

#include <type_traits>

#include "vec16.h"

namespace d3f {

// z, a: [B][C][HW] fp32.  Two networks in one launch (common.h, NetSplit): blockIdx.z = network
template <int ACT>
__global__ __launch_bounds__(256) void head_act_fwd_kernel(const float* __restrict__ z, float* __restrict__ a, int B, int C,
                                                           long HW, long net_ws, long net_out) {
  if (blockIdx.z != 0) {  // workspace tensor in, boundary tensor out
    net_shift(z, net_ws); net_shift(a, net_out);
  }
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    const long base = b * C * HW + pix;
    float v[HEAD_ACT_MAXC];
#pragma unroll
    for (int c = 0; c < HEAD_ACT_MAXC; ++c) v[c] = c < C ? z[base + c * HW] : 0.f;
    head_act_fwd<ACT>(v, C);
#pragma unroll
    for (int c = 0; c < HEAD_ACT_MAXC; ++c)
      if (c < C) a[base + c * HW] = v[c];
  }
}

// z, g, dz_nchw: [B][C][HW] fp32; dy: [B][HW][Cpad] T, rounded once from the fp32 dz, channels [C, Cpad) zero.
// dz_nchw may BE z (the engine's in-place form; neither is __restrict__): a thread reads its pixel's z before it writes
template <int ACT, typename T>
__global__ __launch_bounds__(256) void head_act_bwd_kernel(const float* z, const float* __restrict__ g, float* dz_nchw,
                                                           T* __restrict__ dy, int B, int C, long HW, int Cpad, long net_in,
                                                           long net_ws) {
  if (blockIdx.z != 0) {  // the output gradient is the boundary tensor; z, dz and dY live in the workspace
    net_shift(g, net_in); net_shift(z, net_ws); net_shift(dz_nchw, net_ws); net_shift(dy, net_ws);
  }
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    const long base = b * C * HW + pix;
    float v[HEAD_ACT_MAXC], d[HEAD_ACT_MAXC];
#pragma unroll
    for (int c = 0; c < HEAD_ACT_MAXC; ++c) {
      v[c] = c < C ? z[base + c * HW] : 0.f;
      d[c] = c < C ? g[base + c * HW] : 0.f;
    }
    head_act_bwd<ACT>(v, d, C);
#pragma unroll
    for (int c = 0; c < HEAD_ACT_MAXC; ++c)
      if (c < C) {
        dz_nchw[base + c * HW] = d[c];
        dy[i * Cpad + c] = from_f32<T>(d[c]);
      }
    for (int c = C; c < Cpad; ++c) dy[i * Cpad + c] = from_f32<T>(0.f);
  }
}

// nchw_to_u8bgr_kernel (pointwise.hip, K16) behind the activation: y*std*255 + mean*255 in two roundings, .int()
// truncation, clamp(0, 255), RGB -> BGR
template <int ACT>
__global__ __launch_bounds__(256) void head_act_to_u8bgr_kernel(const float* __restrict__ z, uint8_t* __restrict__ out, int B,
                                                                long HW, int W, long out_row_stride, float m0, float m1,
                                                                float m2, float s0, float s1, float s2) {
  const long total = (long)B * HW, H = HW / W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    const float* src = z + b * 3 * HW + pix;
    float v[HEAD_ACT_MAXC];
#pragma unroll
    for (int c = 0; c < HEAD_ACT_MAXC; ++c) v[c] = c < 3 ? src[c * HW] : 0.f;
    head_act_fwd<ACT>(v, 3);
    auto q = [](float y, float s, float m) {
      const float t = y * s + m;
      int k = (int)t;
      k = k < 0 ? 0 : (k > 255 ? 255 : k);
      return (uint8_t)k;
    };
    const long y = pix / W, x = pix - y * W;
    uint8_t* o = out + (b * H + y) * out_row_stride + x * 3;
    o[2] = q(v[0], s0, m0);
    o[1] = q(v[1], s1, m1);
    o[0] = q(v[2], s2, m2);
  }
}

int head_act_check(int act, int C, int Cpad) {
  D3F_CHECK(act >= 0 && act < HEAD_ACT_COUNT, "head activation: unknown code %d (D3F_ACT_IDENTITY .. D3F_ACT_CLAMP)", act);
  D3F_CHECK(C >= 1 && C <= HEAD_ACT_MAXC, "head activation: %d channels (1 .. %d)", C, HEAD_ACT_MAXC);
  D3F_CHECK(Cpad >= C, "head activation: padded channels %d < channels %d", Cpad, C);
  return 0;
}

// the launch body `F(std::integral_constant<int, ACT>)` for the runtime code `act` (checked by the caller)
template <typename F> static void head_act_dispatch(int act, F&& f) {
  switch (act) {
    case HEAD_ACT_IDENTITY: f(std::integral_constant<int, HEAD_ACT_IDENTITY>()); break;
    case HEAD_ACT_SIGMOID: f(std::integral_constant<int, HEAD_ACT_SIGMOID>()); break;
    case HEAD_ACT_TANH: f(std::integral_constant<int, HEAD_ACT_TANH>()); break;
    case HEAD_ACT_SOFTMAX: f(std::integral_constant<int, HEAD_ACT_SOFTMAX>()); break;
    case HEAD_ACT_LOGSOFTMAX: f(std::integral_constant<int, HEAD_ACT_LOGSOFTMAX>()); break;
    default: f(std::integral_constant<int, HEAD_ACT_CLAMP>()); break;
  }
}

int head_act_forward_launch(int act, const float* z, float* a, int B, int C, int H, int W, hipStream_t stream,
                            const NetSplit* ns) {
  if (int rc = head_act_check(act, C, C)) return rc;
  const long HW = (long)H * W, total = (long)B * HW;
  D3F_CHECK(B >= 0 && H >= 0 && W >= 0, "head activation: extent B=%d H=%d W=%d", B, H, W);
  if (total == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid(grid_for(total), 1, nv.nets);
  head_act_dispatch(act, [&](auto A) {
    hipLaunchKernelGGL(head_act_fwd_kernel<decltype(A)::value>, grid, dim3(256), 0, stream, z, a, B, C, HW, nv.ws, nv.out);
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

int head_act_backward_launch(int act, int dtype, const float* z, const float* g, float* dz_nchw, void* dy_nhwc, int B, int C,
                             int H, int W, int Cpad, hipStream_t stream, const NetSplit* ns) {
  if (int rc = head_act_check(act, C, Cpad)) return rc;
  D3F_CHECK(dtype == D3F_F32 || dtype == D3F_BF16, "head activation: storage dtype %d", dtype);
  D3F_CHECK(B >= 0 && H >= 0 && W >= 0, "head activation: extent B=%d H=%d W=%d", B, H, W);
  const long HW = (long)H * W, total = (long)B * HW;
  if (total == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid(grid_for(total), 1, nv.nets);
  head_act_dispatch(act, [&](auto A) {
    if (dtype == D3F_F32)
      hipLaunchKernelGGL((head_act_bwd_kernel<decltype(A)::value, float>), grid, dim3(256), 0, stream, z, g, dz_nchw,
                         (float*)dy_nhwc, B, C, HW, Cpad, nv.in, nv.ws);
    else
      hipLaunchKernelGGL((head_act_bwd_kernel<decltype(A)::value, bf16_t>), grid, dim3(256), 0, stream, z, g, dz_nchw,
                         (bf16_t*)dy_nhwc, B, C, HW, Cpad, nv.in, nv.ws);
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

int head_act_to_u8bgr_launch(int act, const float* z, uint8_t* out, int B, int H, int W, long out_row_stride,
                             const float mean255[3], const float std255[3], hipStream_t stream) {
  if (int rc = head_act_check(act, 3, 3)) return rc;
  const long HW = (long)H * W;
  if ((long)B * HW == 0) return 0;
  head_act_dispatch(act, [&](auto A) {
    hipLaunchKernelGGL(head_act_to_u8bgr_kernel<decltype(A)::value>, dim3(grid_for((long)B * HW)), dim3(256), 0, stream, z,
                       out, B, HW, W, out_row_stride, mean255[0], mean255[1], mean255[2], std255[0], std255[1], std255[2]);
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
