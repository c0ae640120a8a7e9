// HBM-bound kernels of the U-Net hot path: 3x3/s2 max-pool, 2x2 sum (backward of nearest
// up-sampling), layout conversion at the NCHW boundary and weight packing (BatchNorm, ReLU and
// the residual add: batchnorm.hip).  All activations NHWC, every access a 16-byte vector per
// lane, grid-stride over at most 2048 workgroups.
//
// These replace the ATen max_pool2d / upsample_nearest2d / cat kernels (forward and autograd
// backward) the reference's U-Net dispatches (semantics: SURVEY.md
// Appendix A.1).
#include "pointwise.h"
#include "philox.h"
#include "vec16.h"

#include <type_traits>

namespace d3f {

// ------------------------------------------------------------------------------------------
// MaxPool2d(3, stride 2, padding 1): first maximum in (kh, kw) scan order wins, like ATen.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                          uint8_t* __restrict__ idx, int B, int H,
                                                          int W, int C, long net_ws) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit)
    net_shift(in, net_ws); net_shift(out, net_ws); net_shift(idx, net_ws);
  }
  constexpr int N = V16<T>::N;
  const int Ho = H / 2, Wo = W / 2, VC = C / N;
  const long total = (long)B * Ho * Wo * VC;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % VC);
    long t = i / VC;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float best[N];
    int bi[N];
    bool first = true;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = 2 * oy - 1 + kh;
      if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = 2 * ox - 1 + kw;
        if ((unsigned)ix >= (unsigned)W) continue;
        float v[N];
        V16<T>::load(in + (((long)b * H + iy) * W + ix) * C + cv * N, v);
        if (first) {
#pragma unroll
          for (int k = 0; k < N; ++k) { best[k] = v[k]; bi[k] = kh * 3 + kw; }
          first = false;
        } else {
#pragma unroll
          for (int k = 0; k < N; ++k)
            if (v[k] > best[k] || v[k] != v[k]) { best[k] = v[k]; bi[k] = kh * 3 + kw; }
        }
      }
    }
    const long o = (((long)b * Ho + oy) * Wo + ox) * C + cv * N;
    V16<T>::store(out + o, best);
#pragma unroll
    for (int k = 0; k < N; ++k) idx[o + k] = (uint8_t)bi[k];
  }
}

// grid = (blocks over one input row's W * C/N vectors, blocks of MPB_PAIRS row pairs): the column decode is one
// multiply-high; the argmax bytes of a vector are one load.
// (r03: the first form decoded a flat index with four 64-bit divisions and walked all 9 taps under branches: ~600
// vector instructions per 16 bytes written -- the pass was ALU-bound at 2.6 TB/s.)
// A thread owns its column of MPB_PAIRS pairs of input rows (2m, 2m + 1).  Window row oy covers input rows 2*oy-1 ..
// 2*oy+1, so the even row lies in window row m alone (as its filter row 1) and the odd row in window rows m + 1 (filter
// row 0) and m (filter row 2): the pair needs the two window rows m, m + 1 once, where one row per thread fetched three.
// The same holds for columns: candidates ox0 = (ix + 1) / 2 and, for odd ix, ox0 - 1 with filter column 2.  Every
// candidate is loaded from a clamped (always valid) address in front of all arithmetic and enters under a select, in
// the order the taps have always been added: window row m + 1 before m, column ox0 before ox0 - 1.
constexpr int MPB_PAIRS = 2;
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dout,
                                                          const uint8_t* __restrict__ idx,
                                                          T* __restrict__ din, int npairs,
                                                          int H, int W, int C, unsigned vc_mul, unsigned vc_shr,
                                                          long net_ws) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit)
    net_shift(dout, net_ws); net_shift(idx, net_ws); net_shift(din, net_ws);
  }
  constexpr int N = V16<T>::N;
  const int Ho = H / 2, Wo = W / 2, VC = C / N;
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;  // (ix, cv) in the row
  if (j >= W * VC) return;
  const int ix = fast_div(j, vc_mul, vc_shr), cv = j - ix * VC;
  const int ox0 = (ix + 1) >> 1;
  const bool okc[2] = {ox0 < Wo, (ix & 1) != 0};
  const int oxc[2] = {ox0 < Wo ? ox0 : Wo - 1, ox0 > 0 ? ox0 - 1 : 0};
  const unsigned kwc[2] = {(ix & 1) ? 0u : 1u, 2u};
  float d[MPB_PAIRS][2][2][N], old[MPB_PAIRS][2][N];  // [pair][window row m, m + 1][candidate column]
  uint32_t w[MPB_PAIRS][2][2][N / 4];
  bool next[MPB_PAIRS];
#pragma unroll
  for (int u = 0; u < MPB_PAIRS; ++u) {
    int p = (int)blockIdx.y * MPB_PAIRS + u;  // b * Ho + m  (block-uniform)
    if (p >= npairs) p = npairs - 1;          // (loaded again, not stored)
    next[u] = p % Ho + 1 < Ho;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const long prow = a && next[u] ? p + 1 : p;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const long o = (prow * Wo + oxc[c]) * C + cv * N;
        V16<T>::load(dout + o, d[u][a][c]);
        if constexpr (N == 4) {
          w[u][a][c][0] = *reinterpret_cast<const uint32_t*>(idx + o);
        } else {
          const uint2 t = *reinterpret_cast<const uint2*>(idx + o);
          w[u][a][c][0] = t.x;
          w[u][a][c][1] = t.y;
        }
      }
    }
    if constexpr (ACC) {
#pragma unroll
      for (int e = 0; e < 2; ++e) V16<T>::load(din + ((2L * p + e) * W * VC + j) * N, old[u][e]);
    }
  }
#pragma unroll
  for (int u = 0; u < MPB_PAIRS; ++u) {
    const int p = (int)blockIdx.y * MPB_PAIRS + u;
    if (p >= npairs) break;
    float g[2][N];  // the even row, the odd row
#pragma unroll
    for (int k = 0; k < N; ++k) g[0][k] = g[1][k] = 0.f;
    auto add = [&](float (&gr)[N], int a, unsigned kh, bool row_ok) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const unsigned tap = kh * 3 + kwc[c];
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const bool hit = row_ok && okc[c] && ((w[u][a][c][k >> 2] >> (8 * (k & 3))) & 0xffu) == tap;
          gr[k] = hit ? gr[k] + d[u][a][c][k] : gr[k];
        }
      }
    };
    add(g[0], 0, 1, true);
    add(g[1], 1, 0, next[u]);
    add(g[1], 0, 2, true);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      if constexpr (ACC) {
#pragma unroll
        for (int k = 0; k < N; ++k) g[e][k] += old[u][e][k];
      }
      V16<T>::store(din + ((2L * p + e) * W * VC + j) * N, g[e]);
    }
  }
}

int maxpool3x3s2_fwd_launch(int dtype, const void* in, void* out, uint8_t* idx, int B, int H, int W,
                            int C, hipStream_t stream, const NetSplit* ns) {
  const int ve = dtype == D3F_F32 ? 4 : 8;
  D3F_CHECK(C % ve == 0 && H % 2 == 0 && W % 2 == 0, "maxpool: shape (%d,%d,%d)", H, W, C);
  const long total = (long)B * (H / 2) * (W / 2) * (C / ve);
  if (total == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid(grid_for(total), 1, nv.nets);
  if (dtype == D3F_F32)
    hipLaunchKernelGGL(maxpool_fwd_kernel<float>, grid, dim3(256), 0, stream,
                       (const float*)in, (float*)out, idx, B, H, W, C, nv.ws);
  else
    hipLaunchKernelGGL(maxpool_fwd_kernel<bf16_t>, grid, dim3(256), 0, stream,
                       (const bf16_t*)in, (bf16_t*)out, idx, B, H, W, C, nv.ws);
  D3F_HIP(hipGetLastError());
  return 0;
}

int maxpool3x3s2_bwd_launch(int dtype, const void* dout, const uint8_t* idx, void* din, int accumulate,
                            int B, int H, int W, int C, hipStream_t stream, const NetSplit* ns) {
  const int ve = dtype == D3F_F32 ? 4 : 8;
  D3F_CHECK(C % ve == 0 && H % 2 == 0 && W % 2 == 0, "maxpool: shape (%d,%d,%d)", H, W, C);
  const NetSplit nv = net_split_or_single(ns);
  const long total = (long)B * H * W * (C / ve);
  if (total == 0) return 0;
  const int vc = C / ve;
  unsigned vc_mul, vc_shr;
  fast_div_setup((unsigned)vc, &vc_mul, &vc_shr);
  D3F_CHECK((long)B * H <= 65535, "maxpool backward: %d rows exceed the grid", B * H);
  const int npairs = B * (H / 2);
  const dim3 grid((unsigned)cdiv((long)W * vc, 256), (unsigned)cdiv(npairs, MPB_PAIRS), (unsigned)nv.nets);
  auto go = [&](auto kernel, auto* typed) {
    typedef std::remove_pointer_t<decltype(typed)> T;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (const T*)dout, idx, (T*)din, npairs, H, W, C, vc_mul, vc_shr,
                       nv.ws);
  };
  if (dtype == D3F_F32) {
    if (accumulate) go(maxpool_bwd_kernel<float, true>, (float*)nullptr);
    else go(maxpool_bwd_kernel<float, false>, (float*)nullptr);
  } else {
    if (accumulate) go(maxpool_bwd_kernel<bf16_t, true>, (bf16_t*)nullptr);
    else go(maxpool_bwd_kernel<bf16_t, false>, (bf16_t*)nullptr);
  }
  D3F_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// backward of F.interpolate(scale_factor=2, mode="nearest"): sum each 2x2 block
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sum2x2_kernel(const T* __restrict__ dfull, T* __restrict__ dlow,
                                                     int B, int Hl, int Wl, int C, long net_ws) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit)
    net_shift(dfull, net_ws); net_shift(dlow, net_ws);
  }
  constexpr int N = V16<T>::N;
  const int VC = C / N;
  const long total = (long)B * Hl * Wl * VC;
  const int Wf = 2 * Wl;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % VC);
    long t = i / VC;
    const int x = (int)(t % Wl);
    t /= Wl;  // t = b*Hl + y
    const long base = ((t * 2) * Wf + 2 * x) * (long)C + cv * N;
    float s[N], v[N];
    V16<T>::load(dfull + base, s);
    V16<T>::load(dfull + base + C, v);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += v[k];
    V16<T>::load(dfull + base + (long)Wf * C, v);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += v[k];
    V16<T>::load(dfull + base + (long)Wf * C + C, v);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += v[k];
    V16<T>::store(dlow + i * N, s);
  }
}

int sum2x2_launch(int dtype, const void* dfull, void* dlow, int B, int Hl, int Wl, int C,
                  hipStream_t stream, const NetSplit* ns) {
  const int ve = dtype == D3F_F32 ? 4 : 8;
  D3F_CHECK(C % ve == 0, "sum2x2: C=%d", C);
  const long total = (long)B * Hl * Wl * (C / ve);
  if (total == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid(grid_for(total), 1, nv.nets);
  if (dtype == D3F_F32)
    hipLaunchKernelGGL(sum2x2_kernel<float>, grid, dim3(256), 0, stream,
                       (const float*)dfull, (float*)dlow, B, Hl, Wl, C, nv.ws);
  else
    hipLaunchKernelGGL(sum2x2_kernel<bf16_t>, grid, dim3(256), 0, stream,
                       (const bf16_t*)dfull, (bf16_t*)dlow, B, Hl, Wl, C, nv.ws);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// boundary layout conversion
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in,
                                                           T* __restrict__ out, int B, int C, long HW,
                                                           int Cpad, long net_in, long net_ws) {
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): boundary tensor in, workspace tensor out
    net_shift(in, net_in); net_shift(out, net_ws);
  }
  const long total = (long)B * HW;
  constexpr int N = V16<T>::N;
  if (Cpad == N && C <= N && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    // the stem's case (3 channels padded to one vector): a pixel is ONE 16-byte store, not Cpad stores 16 bytes apart
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
      const long b = i / HW, pix = i - b * HW;
      alignas(16) T px[N];
#pragma unroll
      for (int c = 0; c < N; ++c) px[c] = from_f32<T>(c < C ? in[(b * C + c) * HW + pix] : 0.f);
      *reinterpret_cast<uint4*>(out + i * N) = *reinterpret_cast<const uint4*>(px);
    }
    return;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    for (int c = 0; c < Cpad; ++c) {
      const float v = c < C ? in[(b * C + c) * HW + pix] : 0.f;
      out[i * Cpad + c] = from_f32<T>(v);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* __restrict__ in,
                                                           float* __restrict__ out, int B, int C,
                                                           long HW, int Cpad) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    for (int c = 0; c < C; ++c) out[(b * C + c) * HW + pix] = to_f32<T>(in[i * Cpad + c]);
  }
}

// K16 (inference boundary, d3f/train_deep_fake/lit_module.py:272-300): uint8 BGR frames [B][H][W][3] ->
// normalised NHWC activations in RGB order, (float(u8) - mean*255) / (std*255) in the reference's order of
// fp32 operations; and the way back: y*std*255 + mean*255, .int() truncation, clamp(0, 255), RGB -> BGR.
template <typename T>
__global__ __launch_bounds__(256) void u8bgr_to_nhwc_kernel(const uint8_t* __restrict__ in, T* __restrict__ out,
                                                            long npix, int Cpad, float m0, float m1, float m2,
                                                            float s0, float s1, float s2) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    const uint8_t* px = in + i * 3;
    const float r = ((float)px[2] - m0) / s0, g = ((float)px[1] - m1) / s1, b = ((float)px[0] - m2) / s2;
    T* o = out + i * Cpad;
    o[0] = from_f32<T>(r);
    o[1] = from_f32<T>(g);
    o[2] = from_f32<T>(b);
    for (int c = 3; c < Cpad; ++c) o[c] = from_f32<T>(0.f);
  }
}

__global__ __launch_bounds__(256) void nchw_to_u8bgr_kernel(const float* __restrict__ in, uint8_t* __restrict__ out,
                                                            int B, long HW, int W, long out_row_stride, float m0,
                                                            float m1, float m2, float s0, float s1, float s2) {
  const long total = (long)B * HW, H = HW / W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    const float* src = in + b * 3 * HW + pix;
    auto q = [](float y, float s, float m) {
      const float v = y * s + m;      // two roundings, like the reference's in-place mul then add
      int t = (int)v;                 // .int(): truncation toward zero
      t = t < 0 ? 0 : (t > 255 ? 255 : t);
      return (uint8_t)t;
    };
    const long y = pix / W, x = pix - y * W;
    uint8_t* o = out + (b * H + y) * out_row_stride + x * 3;
    o[2] = q(src[0], s0, m0);
    o[1] = q(src[HW], s1, m1);
    o[0] = q(src[2 * HW], s2, m2);
  }
}

// Input pipeline: uint8 RGB frames [B][H][W][3] as PIL decodes them -> normalised NCHW fp32 training batch,
// ((float)u8 / 255 - mean) / std in the order of fp32 operations of albumentations.Normalize(max_pixel_value=255) +
// ToTensorV2 (d3f/train_deep_fake/lit_module.py:100-110) -- bit-identical to the host transform, but the batch crosses
// worker IPC and PCIe as 1 byte per value instead of 4.
__global__ __launch_bounds__(256) void u8rgb_to_nchw_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                            int B, long HW, U8Normalise norm) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / HW, pix = i - b * HW;
    const uint8_t* px = in + i * 3;
    float* o = out + b * 3 * HW + pix;
    o[0] = norm(px[0], 0);
    o[HW] = norm(px[1], 1);
    o[2 * HW] = norm(px[2], 2);
  }
}

// K17: batched affine warp of NCHW fp32 images -- affine_grid + grid_sample(bilinear, zeros, align_corners=False)
// in one pass (the GPU-side augmentation of train_denoiser, d3f/train_denoiser/lit_module.py:55-65,113).
// theta [B][2][3] maps normalised output coordinates to normalised input coordinates.
// (the sampling: affine_warp_pixel, pointwise.h)
__global__ __launch_bounds__(256) void affine_warp_kernel(const float* __restrict__ in, const float* __restrict__ theta,
                                                          float* __restrict__ out, int B, int C, int H, int W) {
  const long HW = (long)H * W, total = (long)B * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / HW);
    affine_warp_pixel(PlaneTexels{in + (long)b * C * HW, HW}, out + (long)b * C * HW, theta + b * 6,
                      (int)(i - (long)b * HW), C, H, W);
  }
}

int affine_warp_launch(const float* in, const float* theta, float* out, int B, int C, int H, int W,
                       hipStream_t stream) {
  const long total = (long)B * H * W;
  if (total == 0) return 0;
  hipLaunchKernelGGL(affine_warp_kernel, dim3(grid_for(total, 256, 8192)), dim3(256), 0, stream, in, theta, out, B, C,
                     H, W);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ---- K17 with its parameters drawn inside (affine_theta_rng, pointwise.h) ---------------------------------------------
// one image per blockIdx.y; thread 0 draws the image's theta, the workgroup samples with it (or copies the image)
__global__ __launch_bounds__(256) void affine_warp_rng_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              uint64_t seed, uint64_t offset, AffineRngParams q, int C,
                                                              int H, int W) {
  __shared__ float th[6];
  __shared__ int warped;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    float t[6];
    warped = affine_theta_rng(seed, offset, b, q, t) ? 1 : 0;
    for (int k = 0; k < 6; ++k) th[k] = t[k];
  }
  __syncthreads();
  const long HW = (long)H * W;
  if (warped) {
    float t[6];
    for (int k = 0; k < 6; ++k) t[k] = th[k];
    const PlaneTexels src{in + (long)b * C * HW, HW};
    for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (long)gridDim.x * 256)
      affine_warp_pixel(src, out + (long)b * C * HW, t, (int)pix, C, H, W);
  } else {
    const long n = (long)C * HW;
    const float* __restrict__ src = in + (long)b * n;
    float* __restrict__ dst = out + (long)b * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(64) void affine_theta_draw_kernel(uint64_t seed, uint64_t offset, AffineRngParams q,
                                                               float* __restrict__ theta, uint8_t* __restrict__ apply,
                                                               int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float t[6];
  const bool w = affine_theta_rng(seed, offset, b, q, t);
  if (theta != nullptr)
    for (int k = 0; k < 6; ++k) theta[(long)b * 6 + k] = t[k];
  if (apply != nullptr) apply[b] = w ? 1 : 0;
}

int affine_rng_params(int kind, const float params[5], int H, int W, AffineRngParams& q) {
  D3F_CHECK(kind == 0 || kind == 1, "affine rng: kind %d is neither 0 (RandomAffine) nor 1 (ShiftScaleRotate)", kind);
  D3F_CHECK(H > 0 && W > 0, "affine rng: bad shape");
  q = AffineRngParams{};
  q.kind = kind;
  q.deg2rad = (float)(M_PI / 180.0);
  q.h_over_w = (float)((double)H / (double)W);
  q.w_over_h = (float)((double)W / (double)H);
  if (kind == 0) {  // degrees, translate_x, translate_y, scale_lo, scale_hi
    D3F_CHECK(params[3] > 0.f && params[4] >= params[3], "affine rng: scale range [%g, %g]", params[3], params[4]);
    q.angle_unit = (float)((double)params[0] * (M_PI / 180.0));  // math.radians(degrees)
    q.shift_x = params[1], q.shift_y = params[2];
    q.scale_lo = params[3];
    q.scale_span = (float)((double)params[4] - (double)params[3]);
    q.p = 1.0f;
  } else {  // shift_limit, scale_limit, rotate_limit, p
    D3F_CHECK(params[1] >= 0.f && params[1] < 1.f, "affine rng: scale_limit %g outside [0, 1)", params[1]);
    q.shift_x = q.shift_y = params[0];
    q.scale_span = params[1];
    q.angle_unit = params[2];
    q.p = params[3];
  }
  return 0;
}

int affine_warp_rng_launch(const float* in, float* out, uint64_t seed, uint64_t offset, const AffineRngParams& q, int B,
                           int C, int H, int W, hipStream_t stream) {
  const long HW = (long)H * W;
  if ((long)B * HW == 0) return 0;
  D3F_CHECK((long)C * HW < (1L << 31), "affine_warp_rng: image of %ld elements", (long)C * HW);
  long bx = (HW + 255) / 256;
  if (bx > 128) bx = 128;
  hipLaunchKernelGGL(affine_warp_rng_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, stream, in, out, seed, offset,
                     q, C, H, W);
  D3F_HIP(hipGetLastError());
  return 0;
}

int affine_theta_draw_launch(uint64_t seed, uint64_t offset, const AffineRngParams& q, float* theta, uint8_t* apply, int B,
                             hipStream_t stream) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(affine_theta_draw_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, seed, offset, q,
                     theta, apply, B);
  D3F_HIP(hipGetLastError());
  return 0;
}

int u8bgr_to_nhwc_launch(int dtype, const uint8_t* in, void* out, long npix, int Cpad, const float mean255[3],
                         const float std255[3], hipStream_t stream) {
  if (npix == 0) return 0;
  if (dtype == D3F_F32)
    hipLaunchKernelGGL(u8bgr_to_nhwc_kernel<float>, dim3(grid_for(npix)), dim3(256), 0, stream, in, (float*)out, npix,
                       Cpad, mean255[0], mean255[1], mean255[2], std255[0], std255[1], std255[2]);
  else
    hipLaunchKernelGGL(u8bgr_to_nhwc_kernel<bf16_t>, dim3(grid_for(npix)), dim3(256), 0, stream, in, (bf16_t*)out,
                       npix, Cpad, mean255[0], mean255[1], mean255[2], std255[0], std255[1], std255[2]);
  D3F_HIP(hipGetLastError());
  return 0;
}

int u8rgb_to_nchw_launch(const uint8_t* in, float* out, int B, long HW, const float mean[3], const float stdv[3],
                         hipStream_t stream) {
  if ((long)B * HW == 0) return 0;
  hipLaunchKernelGGL(u8rgb_to_nchw_kernel, dim3(grid_for((long)B * HW)), dim3(256), 0, stream, in, out, B, HW,
                     U8Normalise{mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]});
  D3F_HIP(hipGetLastError());
  return 0;
}

int nchw_to_u8bgr_launch(const float* in, uint8_t* out, int B, int H, int W, long out_row_stride, const float mean255[3],
                         const float std255[3], hipStream_t stream) {
  const long HW = (long)H * W;
  if ((long)B * HW == 0) return 0;
  hipLaunchKernelGGL(nchw_to_u8bgr_kernel, dim3(grid_for((long)B * HW)), dim3(256), 0, stream, in, out, B, HW, W,
                     out_row_stride, mean255[0], mean255[1], mean255[2], std255[0], std255[1], std255[2]);
  D3F_HIP(hipGetLastError());
  return 0;
}

int nchw_to_nhwc_launch(int dtype, const float* in, void* out, int B, int C, int H, int W, int Cpad,
                        hipStream_t stream, const NetSplit* ns) {
  const long total = (long)B * H * W;
  if (total == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid(grid_for(total), 1, nv.nets);
  if (dtype == D3F_F32)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, grid, dim3(256), 0, stream, in,
                       (float*)out, B, C, (long)H * W, Cpad, nv.in, nv.ws);
  else
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, grid, dim3(256), 0, stream, in,
                       (bf16_t*)out, B, C, (long)H * W, Cpad, nv.in, nv.ws);
  D3F_HIP(hipGetLastError());
  return 0;
}

int nhwc_to_nchw_launch(int dtype, const void* in, float* out, int B, int C, int H, int W, int Cpad,
                        hipStream_t stream) {
  const long total = (long)B * H * W;
  if (total == 0) return 0;
  if (dtype == D3F_F32)
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(grid_for(total)), dim3(256), 0, stream,
                       (const float*)in, out, B, C, (long)H * W, Cpad);
  else
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, stream,
                       (const bf16_t*)in, out, B, C, (long)H * W, Cpad);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// weight packing (fp32 master in PyTorch layout -> kernel layouts)
// ------------------------------------------------------------------------------------------
// forward:  wf[n][(kh*KW + kw)*Cin + c]                     = w[n][c][kh][kw]
// dgrad:    wd[c][slot*CoutD + n]                            = w[n][c][kh][kw], flipped tap f = (KH-1-kh)*KW + (KW-1-kw)
//           stride 1: slot = f.  3x3 stride 2: the flipped taps are stored output-parity class by class,
//           (odd,odd) (odd,even) (even,odd) (even,even) = f in {0,2,6,8} {1,7} {3,5} {4}, so that each class of the
//           parity-decomposed data gradient (conv_igemm.hip) is one contiguous k-range of the same rows.
__device__ __forceinline__ int dgrad_tap_slot_to_flipped(int slot, int taps, int stride) {
  if (stride == 2 && taps == 9) return (int)((0x453718620ull >> (4 * slot)) & 15);  // 0,2,6,8,1,7,3,5,4
  return slot;
}
// store one packed weight: plain T, or (X3) its exact 3-way bf16 split into three planes `plane` elements apart
template <typename T, bool X3>
__device__ __forceinline__ void pack_store(T* __restrict__ base, long idx, long plane, float v) {
  if constexpr (X3) {
    const uint32_t xb = __float_as_uint(v), hb = xb & 0xffff0000u;
    const float r1 = v - __uint_as_float(hb);
    const uint32_t mb = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(mb);
    base[idx] = (T)(hb >> 16);
    base[plane + idx] = (T)(mb >> 16);
    base[2 * plane + idx] = (T)(__float_as_uint(r2) >> 16);  // exact: r2 has at most 8 significant bits
  } else {
    base[idx] = from_f32<T>(v);
  }
}

// ------------------------------------------------------------------------------------------
// "Up-sample folded into the weights" layouts for the decoder's conv(cat(upsample2x(x), skip)), 3x3 pad 1:
// nearest x2 up-sampling repeats every low-resolution pixel 2x2 times, so inside an output-parity class (py, px)
// the 3x3 taps on the up-sampled operand touch only a 2x2 neighbourhood of x, each low-resolution pixel through
// 1, 2 or 4 taps whose weights can be summed ONCE per step instead of multiplied separately for every pixel:
// 4 MACs per (pixel, channel pair) instead of 9 on the up-sampled channels, forward and data gradient.
//   forward, per class z = 2*py + px:  wfc[z][n][(a*2+b)*C0 + c]      = sum_{kh in S(py,a), kw in S(px,b)} w[n][c][kh][kw]
//                                      wfc[z][n][4*C0 + (kh*3+kw)*C1 + c1] = w[n][C0 + c1][kh][kw]          (skip taps)
//     S(0,0) = {0}, S(0,1) = {1,2}, S(1,0) = {0,1}, S(1,1) = {2}; low-resolution row of tap a is j + a + py - 1
//   data gradient w.r.t. x (a 4x4 stride-2 pad-1 convolution over dY, written at low resolution):
//                                      wd4[c][(u*4+v)*CoutD + n]      = sum_{kh in T(u), kw in T(v)} w[n][c][kh][kw]
//     T(0) = {2}, T(1) = {1,2}, T(2) = {0,1}, T(3) = {0}
//   data gradient w.r.t. the skip tensor (an ordinary 3x3 data gradient with C1 outputs, flipped taps):
//                                      wds[c1][f*CoutD + n]            = w[n][C0 + c1][8 - f]
// The sums are formed in fp32 from the fp32 masters (one rounding per sum: the same order of error as the fp32
// accumulation order inside any conv kernel).  One thread per output element; ~9 M elements per step in total.
__device__ __forceinline__ unsigned up_fwd_set(int parity, int a) {  // bitmask over kh / kw
  return parity == 0 ? (a == 0 ? 1u : 6u) : (a == 0 ? 3u : 4u);
}
__device__ __forceinline__ unsigned up_bwd_set(int u) { return u == 0 ? 4u : u == 1 ? 6u : u == 2 ? 3u : 1u; }

// (the element decode divides by seven run-time constants: multiply-high pairs from the host, fast_div in common.h)
struct UpDiv {
  unsigned fplane[2], kc[2], c0[2], c1[2], k9[2], cd[2], k4[2];
};
template <typename T, bool X3>
__global__ __launch_bounds__(256) void pack_up_kernel(const float* __restrict__ w, int Cout, int C0, int C1,
                                                      T* __restrict__ wfc, int CoutPad, T* __restrict__ wd4,
                                                      int C0Rows, T* __restrict__ wds, int C1Rows, int CoutD,
                                                      int K9, UpDiv dv) {  // K9: wds row length, 9*CoutD padded to whole k-tiles
  const int Cin = C0 + C1;
  const int Kc = 4 * C0 + 9 * C1, K4 = 16 * CoutD;
  const int nf = 4 * CoutPad * Kc, nd = C0Rows * K4, ns = C1Rows * K9;  // (< 2^31 in all: pack_up_launch)
  const int fplane = CoutPad * Kc;  // x3: planes of one class
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < nf + nd + ns; i += (int)gridDim.x * 256) {
    if (i < nf) {
      const int z = fast_div(i, dv.fplane[0], dv.fplane[1]);
      const int r = i - z * fplane;
      const int n = fast_div(r, dv.kc[0], dv.kc[1]), k = r - n * Kc;
      float v = 0.f;
      if (n < Cout) {
        if (k < 4 * C0) {
          const int ab = fast_div(k, dv.c0[0], dv.c0[1]), c = k - ab * C0;
          const unsigned sh = up_fwd_set(z >> 1, ab >> 1), sw = up_fwd_set(z & 1, ab & 1);
          const float* __restrict__ wp = w + ((long)n * Cin + c) * 9;
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
              if (((sh >> kh) & 1u) && ((sw >> kw) & 1u)) v += wp[kh * 3 + kw];
        } else {
          const int kk = k - 4 * C0, tap = fast_div(kk, dv.c1[0], dv.c1[1]), c1 = kk - tap * C1;
          v = w[((long)n * Cin + C0 + c1) * 9 + tap];
        }
      }
      // class blocks are [z][plane][CoutPad][Kc] in x3 mode, [z][CoutPad][Kc] otherwise
      pack_store<T, X3>(wfc + (X3 ? 3L * z * fplane : (long)z * fplane), r, fplane, v);
    } else if (i >= nf + nd) {
      const int j = i - nf - nd;
      const int c1 = fast_div(j, dv.k9[0], dv.k9[1]), k = j - c1 * K9;
      const int f = fast_div(k, dv.cd[0], dv.cd[1]), n = k - f * CoutD;
      float v = 0.f;
      if (c1 < C1 && n < Cout && f < 9) v = w[((long)n * Cin + C0 + c1) * 9 + (8 - f)];
      pack_store<T, X3>(wds, j, ns, v);
    } else {
      const int j = i - nf;
      const int c = fast_div(j, dv.k4[0], dv.k4[1]), k = j - c * K4;
      const int uv = fast_div(k, dv.cd[0], dv.cd[1]), n = k - uv * CoutD;
      float v = 0.f;
      if (c < C0 && n < Cout) {
        const unsigned sh = up_bwd_set(uv >> 2), sw = up_bwd_set(uv & 3);
        const float* __restrict__ wp = w + ((long)n * Cin + c) * 9;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw)
            if (((sh >> kh) & 1u) && ((sw >> kw) & 1u)) v += wp[kh * 3 + kw];
      }
      pack_store<T, X3>(wd4, j, nd, v);
    }
  }
}

int pack_up_launch(int dtype, const float* w, int Cout, int C0, int C1, void* wfc, int CoutPad, void* wd4,
                   int C0Rows, void* wds, int C1Rows, hipStream_t stream) {
  const int ve = dtype == D3F_BF16 ? 8 : 4;
  const int CoutD = (int)round_up(Cout, ve);
  if (wd4 == nullptr) C0Rows = 0;
  if (wds == nullptr) C1Rows = 0;
  const int K9 = (int)round_up(9L * CoutD, dtype == D3F_BF16 ? 64 : 32);  // = the data gradient's KpadD
  const long total = 4L * CoutPad * (4 * C0 + 9 * C1) + (long)C0Rows * 16 * CoutD + (long)C1Rows * K9;
  if (total == 0) return 0;
  D3F_CHECK(total < (1L << 31) - 2048L * 256, "pack_up: %ld elements exceed the 32-bit element index", total);
  UpDiv dv;
  auto setup = [](long d, unsigned (&o)[2]) { fast_div_setup((unsigned)(d > 0 ? d : 1), &o[0], &o[1]); };
  setup((long)CoutPad * (4 * C0 + 9 * C1), dv.fplane);
  setup(4 * C0 + 9 * C1, dv.kc);
  setup(C0, dv.c0);
  setup(C1, dv.c1);
  setup(K9, dv.k9);
  setup(CoutD, dv.cd);
  setup(16 * CoutD, dv.k4);
  if (dtype == D3F_F32)
    hipLaunchKernelGGL((pack_up_kernel<float, false>), dim3(grid_for(total)), dim3(256), 0, stream, w, Cout, C0, C1,
                       (float*)wfc, CoutPad, (float*)wd4, C0Rows, (float*)wds, C1Rows, CoutD, K9, dv);
  else if (dtype == D3F_F32X3)
    hipLaunchKernelGGL((pack_up_kernel<bf16_t, true>), dim3(grid_for(total)), dim3(256), 0, stream, w, Cout, C0, C1,
                       (bf16_t*)wfc, CoutPad, (bf16_t*)wd4, C0Rows, (bf16_t*)wds, C1Rows, CoutD, K9, dv);
  else
    hipLaunchKernelGGL((pack_up_kernel<bf16_t, false>), dim3(grid_for(total)), dim3(256), 0, stream, w, Cout, C0, C1,
                       (bf16_t*)wfc, CoutPad, (bf16_t*)wd4, C0Rows, (bf16_t*)wds, C1Rows, CoutD, K9, dv);
  D3F_HIP(hipGetLastError());
  return 0;
}

// All layers of a network in one launch: the table travels as a kernel argument (no device-side state) and a
// block looks its layer up by its first block index.  A block transposes one [32 filters][CT channels][taps]
// tile through LDS: the torch layout [n][c][tap] is read in contiguous runs of CT*taps floats and the packed
// layouts the entry asks for ([n][tap][c] and / or [c][flipped tap][n]) are written in contiguous runs; padding
// rows/columns of the packed matrices are (re)written as zeros by the edge tiles, so the workspace needs no
// initialisation.
template <typename T, bool X3>
__global__ __launch_bounds__(256) void pack_all_kernel(const float* __restrict__ params, char* __restrict__ ws,
                                                       PackTable t) {
  __shared__ float tile[PACK_NT * (PACK_LDS_ROW + 1)];
  int l = 0;
  while (l + 1 < t.n && blockIdx.x >= t.e[l + 1].block0) ++l;
  const PackEntry e = t.e[l];
  const float* __restrict__ w = params + e.w_off;
  T* __restrict__ wf = reinterpret_cast<T*>(ws + (size_t)e.wf_off16 * 16);
  T* __restrict__ wd = reinterpret_cast<T*>(ws + (size_t)e.wd_off16 * 16);
  const int taps = e.taps, Cin = e.Cin, CinReal = e.CinReal, Cout = e.Cout, Kpad = e.Kpad, KpadD = e.KpadD,
            CoutD = e.CoutD, CT = e.CT, CoutPad = e.CoutPad, CinRows = e.CinRows;
  const int rel = (int)(blockIdx.x - e.block0);
  const int nt = rel / e.ctiles, ct = rel % e.ctiles;  // (block-uniform)
  const int n0 = nt * PACK_NT, c0 = ct * CT;
  const int run = CT * taps, stride = run + 1;  // LDS row: [c_l][tap]
  // per-element index arithmetic: CT and the filter tile are powers of two, the only real division is by the tap count
  // (multiply-high, PackEntry) -- with five integer divisions per element and phase the pass was ALU-bound (r03: 193 us
  // alone for 265 MB)
  const unsigned tmul = e.taps_mul, tshr = e.taps_shr, lgct = e.ct_log2;
  // ---- load: contiguous runs of the torch layout, zero outside the real filter ----
  // (eight loads per thread are issued before the first LDS store: the stem's entry runs as two workgroups on the
  // caller's stream, and 25 load -> store rounds of one element each were 25 dependent memory round trips)
  constexpr int LU = 8;
  for (int i0 = threadIdx.x; i0 < PACK_NT * run; i0 += 256 * LU) {
    float v[LU];
    int dst[LU];
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int i = i0 + u * 256;
      const int nl = fast_div(i >> lgct, tmul, tshr), r = i - nl * run;
      const int n = n0 + nl, c = c0 + fast_div(r, tmul, tshr);
      dst[u] = i < PACK_NT * run ? nl * stride + r : -1;
      const bool real = dst[u] >= 0 && n < Cout && c < CinReal;
      const float x = w[real ? (unsigned)((n * CinReal + c0) * taps + r) : 0u];  // (branch-free: element 0 stands in)
      v[u] = real ? x : 0.f;
    }
#pragma unroll
    for (int u = 0; u < LU; ++u)
      if (dst[u] >= 0) tile[dst[u]] = v[u];
  }
  __syncthreads();
  // ---- forward layout wf[n][tap*Cin + c] ----
  if (e.has_f) {
    for (int i = threadIdx.x; i < PACK_NT * run; i += 256) {
      const int cl = i & (CT - 1), q = i >> lgct;
      const int nl = fast_div(q, tmul, tshr), tap = q - nl * taps;
      const int n = n0 + nl, c = c0 + cl;
      if (n < CoutPad && c < Cin)
        pack_store<T, X3>(wf, (long)(unsigned)(n * Kpad + tap * Cin + c), (long)CoutPad * Kpad, tile[nl * stride + cl * taps + tap]);
    }
    if (ct == 0) {  // zero tail of each row: k in [taps*Cin, Kpad)
      const int k0 = taps * Cin, tail = Kpad - k0;
      for (int i = threadIdx.x; i < PACK_NT * tail; i += 256) {
        const int n = n0 + i / tail;
        if (n < CoutPad) pack_store<T, X3>(wf, (long)n * Kpad + k0 + i % tail, (long)CoutPad * Kpad, 0.f);
      }
    }
  }
  // ---- data-gradient layout wd[c][tapf*CoutD + n], taps flipped ----
  if (e.has_d) {
    for (int i = threadIdx.x; i < PACK_NT * run; i += 256) {
      const int nl = i & (PACK_NT - 1), q = i / PACK_NT;
      const int cl = fast_div(q, tmul, tshr), slot = q - cl * taps;
      const int n = n0 + nl, c = c0 + cl;
      if (c < CinRows && n < CoutD)
        pack_store<T, X3>(wd, (long)(unsigned)(c * KpadD + slot * CoutD + n), (long)CinRows * KpadD,
                          tile[nl * stride + cl * taps + (taps - 1 - dgrad_tap_slot_to_flipped(slot, taps, e.conv_stride))]);
    }
    if (nt == 0) {
      const int k0 = taps * CoutD, tail = KpadD - k0;
      for (int i = threadIdx.x; i < CT * tail; i += 256) {
        const int c = c0 + i / tail;
        if (c < CinRows) pack_store<T, X3>(wd, (long)c * KpadD + k0 + i % tail, (long)CinRows * KpadD, 0.f);
      }
    }
  }
}

int pack_all_launch(int dtype, const float* params, void* ws, const PackTable& t, int blocks,
                    hipStream_t stream) {
  if (t.n == 0 || blocks == 0) return 0;
  if (dtype == D3F_F32)
    hipLaunchKernelGGL((pack_all_kernel<float, false>), dim3(blocks), dim3(256), 0, stream, params, (char*)ws, t);
  else if (dtype == D3F_F32X3)
    hipLaunchKernelGGL((pack_all_kernel<bf16_t, true>), dim3(blocks), dim3(256), 0, stream, params, (char*)ws, t);
  else
    hipLaunchKernelGGL((pack_all_kernel<bf16_t, false>), dim3(blocks), dim3(256), 0, stream, params, (char*)ws, t);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
