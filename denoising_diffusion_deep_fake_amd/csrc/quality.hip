// Held-out validation's scores: per-image MSE, SSIM, PSNR and criterion value of a prediction, forward only.
//
// criterion : d3f/loss_functions/structural_similarity_loss.py:14-26 with piqa.SSIM defaults, restricted to one image:
//               mse  = mean over the image's 3*H*W raw elements of (p - t)^2
//               ssim = mean over its 3*(H-10)*(W-10) valid positions of the SSIM map -- the arithmetic of ssim_fwd_kernel
//                      (loss.hip): norm01, the 11 fp32 taps of make_gauss, columns then rows, taps summed in the order
//                      i = 0 .. 10, the same c1 and c2, never a fused multiply-add
//               loss = (mse + (1.0f - ssim)) / 2.0f
//               psnr = -10 log10(mse01), mse01 = mean of (norm01(p) - norm01(t))^2; +inf when mse01 is 0
//
// The training criterion gets these numbers only together with the gradient (three derivative maps written and read
// back, an adjoint pass) and only as one value per batch.  Here ONE stencil pass reads prediction and target once per tile
// (the 10-element halo apart) and keeps three sums per workgroup; a second, small kernel adds an image's partials in a
// fixed order in float64 and writes the four values where `index` says.  Nothing depends on the batch an image is
// scored in, or on its place in it: an image's four values have the same bits whatever the call.
//
// The grid covers the INPUT extent, tiles(W) x tiles(H) x 3B, as ssim_mse_bwd_kernel's does: the tile at (ty, tx) owns
// the squared errors of the input pixels [32 ty, 32 ty + 32) x [32 tx, 32 tx + 32) and the SSIM outputs of the same
// index range.  The last ten rows and columns of the image have no SSIM output; a tile that lies wholly inside them
// skips the filter stage (one branch for the whole workgroup) and loads its own 32 x 32 pixels only.
#include "pointwise.h"
#include "ssim_common.h"

namespace d3f {

constexpr int Q_SUMS = 3;  // per tile: sum of ss, of (p - t)^2, of (norm01(p) - norm01(t))^2

static inline int tiles(int n) { return (n + SS_T - 1) / SS_T; }

// 104 VGPRs, no scratch, 42 KB of LDS (ssim_fwd_kernel: 102 and the same LDS): three workgroups per CU, bounded by the LDS
__global__ __launch_bounds__(256) void quality_partial_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ target, float lo, float range,
                                                              GaussK gk, int H, int W, float* __restrict__ partial) {
  __shared__ float tx[SS_IN * SS_LD], ty[SS_IN * SS_LD];
  __shared__ float vv[5][SS_T * SS_LD];
  __shared__ float wsum[Q_SUMS][4];
  const int Hv = H - (SS_K - 1), Wv = W - (SS_K - 1);
  const int plane = blockIdx.z;
  const int oy0 = blockIdx.y * SS_T, ox0 = blockIdx.x * SS_T;
  const bool has_out = oy0 < Hv && ox0 < Wv;  // the same for every thread of the workgroup
  const float* __restrict__ px = pred + (long)plane * H * W;
  const float* __restrict__ py = target + (long)plane * H * W;
  const int tid = threadIdx.x;
  float se = 0.f, se01 = 0.f, local = 0.f;
  // the fill of ssim_fwd_kernel (all loads in flight before the first is used), which also takes the squared errors of
  // the 32 x 32 pixels this tile owns from the registers it already holds
  {
    float ra[SS_FILL], rb[SS_FILL];
#pragma unroll
    for (int k = 0; k < SS_FILL; ++k) {
      const int e = tid + k * 256, r = e / SS_IN, c = e - r * SS_IN;
      const int iy = oy0 + r, ix = ox0 + c;
      const bool wanted = has_out || (r < SS_T && c < SS_T);
      const long off = (e < SS_IN * SS_IN && iy < H && ix < W && wanted) ? (long)iy * W + ix : 0;
      ra[k] = px[off];
      rb[k] = py[off];
    }
#pragma unroll
    for (int k = 0; k < SS_FILL; ++k) {
      const int e = tid + k * 256, r = e / SS_IN, c = e - r * SS_IN;
      const int iy = oy0 + r, ix = ox0 + c;
      if (e < SS_IN * SS_IN) {
        const bool in = iy < H && ix < W;
        const float xh = norm01(ra[k], lo, range), yh = norm01(rb[k], lo, range);
        if (in && r < SS_T && c < SS_T) {
          const float d = ra[k] - rb[k], dn = xh - yh;
          se += d * d;
          se01 += dn * dn;
        }
        if (has_out) {
          tx[r * SS_LD + c] = in ? xh : 0.f;
          ty[r * SS_LD + c] = in ? yh : 0.f;
        }
      }
    }
  }
  if (has_out) {
    __syncthreads();
    // filter along H, then along W: ssim_fwd_kernel's two passes (register-blocked, packed fp32 pairs, every output
    // summed over the taps in the order i = 0 .. 10)
    constexpr int RB = 8;
    if (tid < SS_IN * (SS_T / RB)) {
      const int c = tid % SS_IN, r0 = (tid / SS_IN) * RB;
      f32x2 xy[RB + SS_K - 1], sq[RB + SS_K - 1];
      float ab[RB + SS_K - 1];
#pragma unroll
      for (int i = 0; i < RB + SS_K - 1; ++i) {
        xy[i] = f32x2{tx[(r0 + i) * SS_LD + c], ty[(r0 + i) * SS_LD + c]};
        sq[i] = xy[i] * xy[i];
        ab[i] = xy[i].x * xy[i].y;
      }
#pragma unroll
      for (int r = 0; r < RB; r += 2) {
        f32x2 s01[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, s23[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, s4 = f32x2{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < SS_K; ++i) {
          const f32x2 g = f32x2{gk.g[i], gk.g[i]};
          s01[0] += g * xy[r + i];
          s23[0] += g * sq[r + i];
          s01[1] += g * xy[r + 1 + i];
          s23[1] += g * sq[r + 1 + i];
          s4 += g * f32x2{ab[r + i], ab[r + 1 + i]};
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          vv[0][(r0 + r + e) * SS_LD + c] = s01[e].x;
          vv[1][(r0 + r + e) * SS_LD + c] = s01[e].y;
          vv[2][(r0 + r + e) * SS_LD + c] = s23[e].x;
          vv[3][(r0 + r + e) * SS_LD + c] = s23[e].y;
          vv[4][(r0 + r + e) * SS_LD + c] = e ? s4.y : s4.x;
        }
      }
    }
    __syncthreads();
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    constexpr int CBk = 4;
    const int rr = tid / (SS_T / CBk), cq = (tid % (SS_T / CBk)) * CBk;
    f32x2 w01[CBk + SS_K - 1], w23[CBk + SS_K - 1];
    float w4[CBk + SS_K - 1];
#pragma unroll
    for (int j = 0; j < CBk + SS_K - 1; ++j) {
      w01[j] = f32x2{vv[0][rr * SS_LD + cq + j], vv[1][rr * SS_LD + cq + j]};
      w23[j] = f32x2{vv[2][rr * SS_LD + cq + j], vv[3][rr * SS_LD + cq + j]};
      w4[j] = vv[4][rr * SS_LD + cq + j];
    }
    float mm[CBk][5];
#pragma unroll
    for (int cc = 0; cc < CBk; cc += 2) {
      f32x2 s01[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, s23[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, s4 = f32x2{0.f, 0.f};
#pragma unroll
      for (int j = 0; j < SS_K; ++j) {
        const f32x2 g = f32x2{gk.g[j], gk.g[j]};
        s01[0] += g * w01[cc + j];
        s23[0] += g * w23[cc + j];
        s01[1] += g * w01[cc + 1 + j];
        s23[1] += g * w23[cc + 1 + j];
        s4 += g * f32x2{w4[cc + j], w4[cc + 1 + j]};
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        mm[cc + e][0] = s01[e].x; mm[cc + e][1] = s01[e].y; mm[cc + e][2] = s23[e].x; mm[cc + e][3] = s23[e].y;
        mm[cc + e][4] = e ? s4.y : s4.x;
      }
    }
#pragma unroll
    for (int cc = 0; cc < CBk; ++cc) {
      if (oy0 + rr >= Hv || ox0 + cq + cc >= Wv) continue;
      const float (&m)[5] = mm[cc];
      const float mux = m[0], muy = m[1];
      const float sxx = m[2] - mux * mux, syy = m[3] - muy * muy, sxy = m[4] - mux * muy;
      const float a1 = 2.f * mux * muy + c1, b1 = mux * mux + muy * muy + c1;
      const float a2 = 2.f * sxy + c2, b2 = sxx + syy + c2;
      const float l = a1 / b1, cs = a2 / b2;
      local += l * cs;
    }
  }
  // a tile's three sums: at most seven adds in a thread, six shuffle steps, a tree of four
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    local += __shfl_xor(local, o);
    se += __shfl_xor(se, o);
    se01 += __shfl_xor(se01, o);
  }
  if ((tid & 63) == 0) {
    wsum[0][tid >> 6] = local;
    wsum[1][tid >> 6] = se;
    wsum[2][tid >> 6] = se01;
  }
  __syncthreads();
  if (tid < Q_SUMS)
    partial[(((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * Q_SUMS + tid] =
        (wsum[tid][0] + wsum[tid][1]) + (wsum[tid][2] + wsum[tid][3]);
}

// one wavefront per image: lane l adds the partials of tiles l, l + 64, ... of the image's three planes in that order in
// float64, six xor steps fold the lanes (both partners form the same sum), lane 0 writes the four values
__global__ __launch_bounds__(64) void quality_finalize_kernel(const float* __restrict__ partial, int tiles_per_image,
                                                              double n_elems, double n_ssim,
                                                              const int64_t* __restrict__ index, float* __restrict__ metrics,
                                                              int N) {
  const int b = blockIdx.x;
  const float* __restrict__ p = partial + (long)b * tiles_per_image * Q_SUMS;
  double ss = 0.0, se = 0.0, se01 = 0.0;
  for (int i = threadIdx.x; i < tiles_per_image; i += 64) {
    const float v0 = p[(long)i * Q_SUMS], v1 = p[(long)i * Q_SUMS + 1], v2 = p[(long)i * Q_SUMS + 2];
    ss += (double)v0;
    se += (double)v1;
    se01 += (double)v2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o);
    se += __shfl_xor(se, o);
    se01 += __shfl_xor(se01, o);
  }
  if (threadIdx.x != 0) return;
  const int64_t dst = index != nullptr ? index[b] : (int64_t)b;
  if (dst < 0 || dst >= (int64_t)N) return;  // outside the buffer: nothing is written
  const float mse = (float)(se / n_elems);
  const float ssim = (float)(ss / n_ssim);
  const float mse01 = (float)(se01 / n_elems);
  metrics[dst] = mse;
  metrics[(long)N + dst] = ssim;
  // log10 in double, rounded once (the device's fp32 log10f is a few ulp off); log10(0) = -inf gives +inf
  metrics[2 * (long)N + dst] = (float)(-10.0 * log10((double)mse01));
  metrics[3 * (long)N + dst] = (mse + (1.0f - ssim)) / 2.0f;
}

size_t quality_per_image_workspace_bytes(int B, int H, int W) {
  if (B < 0 || H < SS_K || W < SS_K) return 0;
  return (size_t)B * 3 * tiles(H) * tiles(W) * Q_SUMS * sizeof(float) + 64;
}

int quality_per_image_scatter_launch(const float* pred, const float* target, float in_min, float in_max,
                                     const int64_t* index_or_null, float* metrics, int N, void* workspace, int B, int H,
                                     int W, hipStream_t stream) {
  D3F_CHECK(H >= SS_K && W >= SS_K, "quality_per_image: image %dx%d smaller than the 11x11 SSIM window", H, W);
  D3F_CHECK(in_max > in_min, "quality_per_image: input range");
  D3F_CHECK(N >= 1, "quality_per_image: N = %d", N);
  D3F_CHECK(B >= 0 && (long)B * 3 <= 65535, "quality_per_image: %d images in one call (at most 21845)", B);
  D3F_CHECK((long)3 * tiles(H) * tiles(W) <= INT32_MAX, "quality_per_image: image %dx%d too large", H, W);
  if (B == 0) return 0;
  static const GaussK gk = make_gauss();
  float* partial = reinterpret_cast<float*>(workspace);
  const int Hv = H - SS_K + 1, Wv = W - SS_K + 1;
  hipLaunchKernelGGL(quality_partial_kernel, dim3(tiles(W), tiles(H), (unsigned)(B * 3)), dim3(256), 0, stream, pred,
                     target, in_min, in_max - in_min, gk, H, W, partial);
  D3F_HIP(hipGetLastError());
  hipLaunchKernelGGL(quality_finalize_kernel, dim3((unsigned)B), dim3(64), 0, stream, partial, 3 * tiles(H) * tiles(W),
                     3.0 * (double)H * (double)W, 3.0 * (double)Hv * (double)Wv, index_or_null, metrics, N);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
