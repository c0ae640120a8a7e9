// Noise blend (K12) and the (MSE + 1 - SSIM)/2 criterion with its gradient (K13).
//
// noise blend  : d3f/train_denoiser/lit_module.py:128-153 == d3f/train_deep_fake/lit_module.py:208-233
//                r = (1/lam) * log(1 / (y*(1-c) + c)), c = exp(-lam);  out = sqrt(1-r)*x + sqrt(r)*noise
//                (same operation order and roundings as the torch expression: no FMA contraction).
// criterion    : d3f/loss_functions/structural_similarity_loss.py:14-26 with piqa.SSIM defaults
//                (11-tap sigma-1.5 separable Gaussian, valid filtering, k1=.01, k2=.03, value range 1).
// Tensors here are the NCHW fp32 boundary tensors (prediction / target images), 3 channels.
//
// SSIM forward is one LDS-tiled pass per (image, channel, 32x32 output tile): it filters
// x, y, x^2, y^2, xy (columns then rows), evaluates the SSIM map and at the same time the
// three derivative maps d ss / d(mu_x, E[x^2], E[xy]); the backward pass filters those three
// maps with the adjoint (zero-padded) Gaussian and adds the MSE gradient, so the loss and
// d loss / d prediction cost 2 stencil passes over the images instead of ~15 torch kernels.
#include "pointwise.h"
#include "philox.h"
#include "ssim_common.h"  // the tile geometry, GaussK / make_gauss, norm01 (shared with quality.hip)

namespace d3f {

__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ pred,
                                                       const float* __restrict__ target, float lo,
                                                       float range, GaussK gk, int H, int W,
                                                       float* __restrict__ dA, float* __restrict__ dB,
                                                       float* __restrict__ dC,
                                                       float* __restrict__ partial) {
  chain_priority();
  __shared__ float tx[SS_IN * SS_LD], ty[SS_IN * SS_LD];
  __shared__ float vv[5][SS_T * SS_LD];
  __shared__ float wsum[4];
  const int Hv = H - (SS_K - 1), Wv = W - (SS_K - 1);
  const int plane = blockIdx.z;
  const int oy0 = blockIdx.y * SS_T, ox0 = blockIdx.x * SS_T;
  const float* __restrict__ px = pred + (long)plane * H * W;
  const float* __restrict__ py = target + (long)plane * H * W;
  const int tid = threadIdx.x;
  // the tile's seven elements per thread are all loaded (branch-free, from a clamped address) before the first is used:
  // as a rolled load -> normalise -> store loop the fill was seven dependent memory round trips per workgroup, at three
  // workgroups per CU
  {
    float ra[SS_FILL], rb[SS_FILL];
#pragma unroll
    for (int k = 0; k < SS_FILL; ++k) {
      const int e = tid + k * 256, r = e / SS_IN, c = e - r * SS_IN;
      const int iy = oy0 + r, ix = ox0 + c;
      const long off = (e < SS_IN * SS_IN && iy < H && ix < W) ? (long)iy * W + ix : 0;
      ra[k] = px[off];
      rb[k] = py[off];
    }
#pragma unroll
    for (int k = 0; k < SS_FILL; ++k) {
      const int e = tid + k * 256, r = e / SS_IN, c = e - r * SS_IN;
      const int iy = oy0 + r, ix = ox0 + c;
      if (e < SS_IN * SS_IN) {
        const bool in = iy < H && ix < W;
        tx[r * SS_LD + c] = in ? norm01(ra[k], lo, range) : 0.f;
        ty[r * SS_LD + c] = in ? norm01(rb[k], lo, range) : 0.f;
      }
    }
  }
  __syncthreads();
  // filter along H (piqa filters dim -2 first): vv[q][r][c], r < 32 output rows, c < 42 columns.  Register-blocked:
  // a thread owns column c and 8 consecutive output rows, reads its 18 input rows ONCE (the products a*a, b*b, a*b
  // are formed once per input instead of once per tap) -- 36 LDS reads instead of 176; every output is still summed
  // over the taps in the order i = 0 .. 10.
  // The taps run as packed fp32 pairs (v_pk_mul_f32 + v_pk_add_f32, two IEEE operations per instruction: the same
  // products and sums, rounded the same way, as the scalar form -- never a fused multiply-add): (x, y) and (x^2, y^2)
  // of one row pair up, xy pairs up across two neighbouring output rows.
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
  float local = 0.f;
  // row filter, register-blocked the same way: a thread owns row r and 4 consecutive output columns (14 reads per map
  // instead of 44)
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
  float mm[CBk][5];  // (packed like the column pass; the fifth map pairs up across two neighbouring columns)
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
    const int r = rr, c = cq + cc;
    const int oy = oy0 + r, ox = ox0 + c;
    if (oy >= Hv || ox >= Wv) continue;
    const float (&m)[5] = mm[cc];
    const float mux = m[0], muy = m[1];
    const float sxx = m[2] - mux * mux, syy = m[3] - muy * muy, sxy = m[4] - mux * muy;
    const float a1 = 2.f * mux * muy + c1, b1 = mux * mux + muy * muy + c1;
    const float a2 = 2.f * sxy + c2, b2 = sxx + syy + c2;
    const float l = a1 / b1, cs = a2 / b2;
    const float ss = l * cs;
    local += ss;
    const long o = ((long)plane * Hv + oy) * Wv + ox;
    const float dl_dmux = 2.f * (muy - l * mux) / b1;
    const float dcs_dmux = (2.f * mux * cs - 2.f * muy) / b2;
    dA[o] = cs * dl_dmux + l * dcs_dmux;   // d ss / d mu_x   (total)
    dB[o] = -l * cs / b2;                  // d ss / d E[x^2]
    dC[o] = 2.f * l / b2;                  // d ss / d E[xy]
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
  if ((tid & 63) == 0) wsum[tid >> 6] = local;
  __syncthreads();
  if (tid == 0)
    partial[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
        (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void ssim_mse_bwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, float lo, float range, GaussK gk,
    int H, int W, const float* __restrict__ dA, const float* __restrict__ dB,
    const float* __restrict__ dC, float ssim_coef, float mse_coef, float* __restrict__ grad,
    float* __restrict__ partial_mse) {
  chain_priority();
  __shared__ float t3[3][SS_IN * SS_LD];
  __shared__ float vv[3][SS_T * SS_LD];
  __shared__ float wsum[4];
  const int Hv = H - (SS_K - 1), Wv = W - (SS_K - 1);
  const int plane = blockIdx.z;
  const int py0 = blockIdx.y * SS_T, px0 = blockIdx.x * SS_T;
  const int tid = threadIdx.x;
  // derivative maps at outputs o = p - k, k in [0,10]: tile origin (py0-10, px0-10)
  // (all loads of the fill before its first LDS store, as in ssim_fwd_kernel; and the four pixels this thread finishes
  // are fetched here too, so that they travel during the two filter passes)
  constexpr int CBk = 4;  // row r, 4 consecutive columns per thread
  const int rr = tid / (SS_T / CBk), cq = (tid % (SS_T / CBk)) * CBk;
  float pv4[CBk], tv4[CBk];
  {
    float ra[SS_FILL], rb[SS_FILL], rd[SS_FILL];
#pragma unroll
    for (int k = 0; k < SS_FILL; ++k) {
      const int e = tid + k * 256, r = e / SS_IN, c = e - r * SS_IN;
      const int oy = py0 - (SS_K - 1) + r, ox = px0 - (SS_K - 1) + c;
      const bool in = e < SS_IN * SS_IN && oy >= 0 && oy < Hv && ox >= 0 && ox < Wv;
      const long o = (long)plane * Hv * Wv + (in ? (long)oy * Wv + ox : 0);
      ra[k] = dA[o];
      rb[k] = dB[o];
      rd[k] = dC[o];
    }
#pragma unroll
    for (int cc = 0; cc < CBk; ++cc) {
      const int iy = py0 + rr, ix = px0 + cq + cc;
      const long p = (long)plane * H * W + ((iy < H && ix < W) ? (long)iy * W + ix : 0);
      pv4[cc] = pred[p];
      tv4[cc] = target[p];
    }
#pragma unroll
    for (int k = 0; k < SS_FILL; ++k) {
      const int e = tid + k * 256, r = e / SS_IN, c = e - r * SS_IN;
      const int oy = py0 - (SS_K - 1) + r, ox = px0 - (SS_K - 1) + c;
      if (e < SS_IN * SS_IN) {
        const bool in = oy >= 0 && oy < Hv && ox >= 0 && ox < Wv;
        t3[0][r * SS_LD + c] = in ? ra[k] : 0.f;
        t3[1][r * SS_LD + c] = in ? rb[k] : 0.f;
        t3[2][r * SS_LD + c] = in ? rd[k] : 0.f;
      }
    }
  }
  __syncthreads();
  // adjoint filter: G(p) = sum_k g[k] * D[p - k] = sum_i g[10 - i] * tile[r + i]; register-blocked like the forward
  // pass (column c, 8 consecutive output rows per thread; same summation order per output)
  constexpr int RB = 8;
  if (tid < SS_IN * (SS_T / RB)) {
    const int c = tid % SS_IN, r0 = (tid / SS_IN) * RB;
    f32x2 v01[RB + SS_K - 1];  // (packed pairs as in ssim_fwd_kernel: maps 0 and 1 of a row, map 2 of two rows)
    float v2[RB + SS_K - 1];
#pragma unroll
    for (int i = 0; i < RB + SS_K - 1; ++i) {
      v01[i] = f32x2{t3[0][(r0 + i) * SS_LD + c], t3[1][(r0 + i) * SS_LD + c]};
      v2[i] = t3[2][(r0 + i) * SS_LD + c];
    }
#pragma unroll
    for (int r = 0; r < RB; r += 2) {
      f32x2 s01[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, s2 = f32x2{0.f, 0.f};
#pragma unroll
      for (int i = 0; i < SS_K; ++i) {
        const f32x2 g = f32x2{gk.g[SS_K - 1 - i], gk.g[SS_K - 1 - i]};
        s01[0] += g * v01[r + i];
        s01[1] += g * v01[r + 1 + i];
        s2 += g * f32x2{v2[r + i], v2[r + 1 + i]};
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        vv[0][(r0 + r + e) * SS_LD + c] = s01[e].x;
        vv[1][(r0 + r + e) * SS_LD + c] = s01[e].y;
        vv[2][(r0 + r + e) * SS_LD + c] = e ? s2.y : s2.x;
      }
    }
  }
  __syncthreads();
  const float inv_range = 1.f / range;
  float local = 0.f;
  f32x2 w01[CBk + SS_K - 1];
  float w2[CBk + SS_K - 1];
#pragma unroll
  for (int j = 0; j < CBk + SS_K - 1; ++j) {
    w01[j] = f32x2{vv[0][rr * SS_LD + cq + j], vv[1][rr * SS_LD + cq + j]};
    w2[j] = vv[2][rr * SS_LD + cq + j];
  }
  float gg[CBk][3];
#pragma unroll
  for (int cc = 0; cc < CBk; cc += 2) {
    f32x2 s01[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}, s2 = f32x2{0.f, 0.f};
#pragma unroll
    for (int j = 0; j < SS_K; ++j) {
      const f32x2 g = f32x2{gk.g[SS_K - 1 - j], gk.g[SS_K - 1 - j]};
      s01[0] += g * w01[cc + j];
      s01[1] += g * w01[cc + 1 + j];
      s2 += g * f32x2{w2[cc + j], w2[cc + 1 + j]};
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      gg[cc + e][0] = s01[e].x; gg[cc + e][1] = s01[e].y; gg[cc + e][2] = e ? s2.y : s2.x;
    }
  }
#pragma unroll
  for (int cc = 0; cc < CBk; ++cc) {
    const int r = rr, c = cq + cc;
    const int iy = py0 + r, ix = px0 + c;
    if (iy >= H || ix >= W) continue;
    const float ga = gg[cc][0], gb = gg[cc][1], gc = gg[cc][2];
    const long p = (long)plane * H * W + (long)iy * W + ix;
    const float pv = pv4[cc], tv = tv4[cc];
    const float rawx = (pv - lo) / range;
    const float xh = fminf(fmaxf(rawx, 0.f), 1.f);
    const float yh = norm01(tv, lo, range);
    float gx = ga + 2.f * xh * gb + yh * gc;       // d(sum ss)/d xhat
    gx = (rawx >= 0.f && rawx <= 1.f) ? gx * inv_range : 0.f;  // through clip and affine
    const float diff = pv - tv;
    local += diff * diff;
    grad[p] = ssim_coef * gx + mse_coef * diff;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
  if ((tid & 63) == 0) wsum[tid >> 6] = local;
  __syncthreads();
  if (tid == 0)
    partial_mse[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
        (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ part_ss, int n_ss,
                                                            const float* __restrict__ part_mse,
                                                            int n_mse, double n_ssim_elems,
                                                            double n_elems, float* __restrict__ out) {
  chain_priority();
  __shared__ double red[2][256];
  // a thread adds elements tid, tid + 256, ... in that order; four loads are issued in front of their adds (one block
  // walks 3072 + 3072 partials at the headline shape: twelve dependent round trips per array otherwise)
  auto strided_sum = [](const float* __restrict__ p, int n) {
    double s = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * 256 < n; i += 4 * 256) {
      const float v0 = p[i], v1 = p[i + 256], v2 = p[i + 512], v3 = p[i + 768];
      s += (double)v0; s += (double)v1; s += (double)v2; s += (double)v3;
    }
    for (; i < n; i += 256) s += (double)p[i];
    return s;
  };
  const double a = strided_sum(part_ss, n_ss), b = strided_sum(part_mse, n_mse);
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float ssim = (float)(red[0][0] / n_ssim_elems);
    const float mse = (float)(red[1][0] / n_elems);
    out[0] = (mse + (1.0f - ssim)) / 2.0f;
    out[1] = mse;
    out[2] = ssim;
  }
}

static inline int tiles(int n) { return (n + SS_T - 1) / SS_T; }

size_t loss_workspace_floats(int B, int H, int W) {
  if (H < SS_K || W < SS_K) return 0;
  const long planes = (long)B * 3;
  const long maps = 3 * planes * (H - SS_K + 1) * (W - SS_K + 1);
  const long p1 = planes * tiles(H - SS_K + 1) * tiles(W - SS_K + 1);
  const long p2 = planes * tiles(H) * tiles(W);
  return (size_t)(maps + p1 + p2 + 16);
}

int mse_ssim_loss_launch(const float* pred, const float* target, float in_min, float in_max,
                         float* loss_out, float* grad_pred, float* workspace, int B, int H, int W,
                         hipStream_t stream) {
  D3F_CHECK(H >= SS_K && W >= SS_K, "loss: image %dx%d smaller than the 11x11 SSIM window", H, W);
  D3F_CHECK(in_max > in_min, "loss: input range");
  static const GaussK gk = make_gauss();
  const int Hv = H - SS_K + 1, Wv = W - SS_K + 1;
  const long planes = (long)B * 3;
  const long map = planes * Hv * Wv;
  float* dA = workspace;
  float* dB = dA + map;
  float* dC = dB + map;
  float* part_ss = dC + map;
  const int n_ss = (int)(planes * tiles(Hv) * tiles(Wv));
  float* part_mse = part_ss + n_ss;
  const int n_mse = (int)(planes * tiles(H) * tiles(W));
  const float range = in_max - in_min;
  hipLaunchKernelGGL(ssim_fwd_kernel, dim3(tiles(Wv), tiles(Hv), (unsigned)planes), dim3(256), 0, stream,
                     pred, target, in_min, range, gk, H, W, dA, dB, dC, part_ss);
  D3F_HIP(hipGetLastError());
  const double n_elems = (double)planes * H * W;
  const double n_ssim = (double)planes * Hv * Wv;
  // loss = (mse + 1 - mean(ss)) / 2
  const float ssim_coef = (float)(-0.5 / n_ssim);
  const float mse_coef = (float)(1.0 / n_elems);  // 0.5 * 2 * diff / N
  hipLaunchKernelGGL(ssim_mse_bwd_kernel, dim3(tiles(W), tiles(H), (unsigned)planes), dim3(256), 0,
                     stream, pred, target, in_min, range, gk, H, W, dA, dB, dC, ssim_coef, mse_coef,
                     grad_pred, part_mse);
  D3F_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, stream, part_ss, n_ss, part_mse, n_mse,
                     n_ssim, n_elems, loss_out);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// the blend's per-image coefficients and its four-element body: ONE expression for the kernel that loads its draws and
// for the ones that draw inside (noise_blend_rng_kernel), so that the same z and y give the same bits
struct BlendCoef {
  float r, sa, sb;
};
__device__ __forceinline__ BlendCoef blend_coef(float y, float c, float one_minus_c, float inv_lam) {
  // x = 1/lam * log(1 / (y*(1-c) + c))   -- every step rounded to f32 like the torch expression
  const float t = __fadd_rn(__fmul_rn(y, one_minus_c), c);
  // log / sqrt evaluated in double and rounded once: correctly rounded f32 results (the device's
  // f32 logf / sqrtf are 1-2 ulp off the host libm the reference's CPU path uses); 3 ops per image
  // inv_lam <= 0: fixed-ratio mode (balance_training_images), y holds r itself
  const float r = inv_lam > 0.f ? __fmul_rn(inv_lam, (float)log((double)__fdiv_rn(1.0f, t))) : y;
  // __fsqrt_rn: IEEE correctly rounded f32 square root
  return BlendCoef{r, __fsqrt_rn(__fsub_rn(1.0f, r)), __fsqrt_rn(r)};
}
__device__ __forceinline__ float4 blend4(const BlendCoef k, const float4 a, const float4 n) {
  float4 o;
  o.x = __fadd_rn(__fmul_rn(k.sa, a.x), __fmul_rn(k.sb, n.x));
  o.y = __fadd_rn(__fmul_rn(k.sa, a.y), __fmul_rn(k.sb, n.y));
  o.z = __fadd_rn(__fmul_rn(k.sa, a.z), __fmul_rn(k.sb, n.z));
  o.w = __fadd_rn(__fmul_rn(k.sa, a.w), __fmul_rn(k.sb, n.w));
  return o;
}

__global__ __launch_bounds__(256) void noise_blend_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ noise,
                                                          const float* __restrict__ y_uniform,
                                                          float c, float one_minus_c, float inv_lam,
                                                          float* __restrict__ out,
                                                          float* __restrict__ r_out, long per_image) {
  const int b = blockIdx.y;
  const BlendCoef k = blend_coef(y_uniform[b], c, one_minus_c, inv_lam);
  if (r_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) r_out[b] = k.r;
  const long nvec = per_image / 4;
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + (long)b * per_image);
  const float4* __restrict__ nv = reinterpret_cast<const float4*>(noise + (long)b * per_image);
  float4* __restrict__ ov = reinterpret_cast<float4*>(out + (long)b * per_image);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) ov[i] = blend4(k, xv[i], nv[i]);
}

int noise_blend_launch(const float* x, const float* noise, const float* y_uniform, float lam,
                       float* out, float* r_out, int B, long per_image, hipStream_t stream) {
  D3F_CHECK(per_image % 4 == 0, "noise_blend: per-image element count %ld not a multiple of 4", per_image);
  D3F_CHECK(lam > 0.f, "noise_blend: lambda must be positive");
  if (B == 0 || per_image == 0) return 0;
  const double c = 1.0 / exp((double)lam);
  long bx = (per_image / 4 + 255) / 256;
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(noise_blend_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, stream, x, noise,
                     y_uniform, (float)c, (float)(1.0 - c), (float)(1.0 / (double)lam), out, r_out,
                     per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

// fixed-ratio blend (d3f/balance_training_images/lit_module.py:109-121): out = sqrt(1-r[b])*x + sqrt(r[b])*noise
int noise_blend_fixed_launch(const float* x, const float* noise, const float* r, float* out, int B, long per_image,
                             hipStream_t stream) {
  D3F_CHECK(per_image % 4 == 0, "noise_blend: per-image element count %ld not a multiple of 4", per_image);
  if (B == 0 || per_image == 0) return 0;
  long bx = (per_image / 4 + 255) / 256;
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(noise_blend_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, stream, x, noise, r, 0.f, 0.f,
                     -1.f, out, (float*)nullptr, per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ---- K12 with its draws made inside (philox.h: the draw layout) ------------------------------------------------------
// d3f/train_denoiser/lit_module.py:128-153 == d3f/train_deep_fake/lit_module.py:208-233 (randn_like + rand + blend) and
// d3f/balance_training_images/lit_module.py:109-121 (randn_like + fixed-ratio blend) as ONE kernel: block g of image b
// gives the four normals of float4 g, the image's y comes from block 0xFFFFFFFF; no noise tensor goes through HBM.
// y_or_r == nullptr: y is drawn (exponential sampler); otherwise y_or_r[b] is the fixed ratio r (inv_lam <= 0).
__global__ __launch_bounds__(256) void noise_blend_rng_kernel(const float* __restrict__ x, uint64_t seed, uint64_t offset,
                                                              const float* __restrict__ y_or_r, float c,
                                                              float one_minus_c, float inv_lam, float* __restrict__ out,
                                                              float* __restrict__ r_out, long per_image) {
  chain_priority();
  const int b = blockIdx.y;
  const BlendCoef k = blend_coef(y_or_r != nullptr ? y_or_r[b] : rng_y(seed, offset, b), c, one_minus_c, inv_lam);
  if (r_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) r_out[b] = k.r;
  const long nvec = per_image / 4;
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + (long)b * per_image);
  float4* __restrict__ ov = reinterpret_cast<float4*>(out + (long)b * per_image);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256)
    ov[i] = blend4(k, xv[i], rng_normal4(seed, offset, b, (uint32_t)i));
}

// the draws of noise_blend_rng_kernel written out (either pointer may be null): the same device functions
__global__ __launch_bounds__(256) void noise_draw_kernel(uint64_t seed, uint64_t offset, float* __restrict__ noise,
                                                         float* __restrict__ y, long per_image) {
  const int b = blockIdx.y;
  if (y != nullptr && blockIdx.x == 0 && threadIdx.x == 0) y[b] = rng_y(seed, offset, b);
  if (noise == nullptr) return;
  const long nvec = per_image / 4;
  float4* __restrict__ nv = reinterpret_cast<float4*>(noise + (long)b * per_image);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256)
    nv[i] = rng_normal4(seed, offset, b, (uint32_t)i);
}

static int rng_shape_check(const char* what, long per_image) {
  D3F_CHECK(per_image % 4 == 0, "%s: per-image element count %ld not a multiple of 4", what, per_image);
  // groups 0xFFFFFFFD .. 0xFFFFFFFF of every image hold the augmentation draws and y
  D3F_CHECK(per_image / 4 < (long)RNG_G_APPLY, "%s: per-image element count %ld leaves no room for the reserved groups",
            what, per_image);
  return 0;
}
static unsigned rng_blocks(long per_image) {
  const long bx = (per_image / 4 + 255) / 256;
  return (unsigned)(bx > 256 ? 256 : (bx < 1 ? 1 : bx));
}

int noise_blend_rng_launch(const float* x, uint64_t seed, uint64_t offset, float lam, float* out, float* r_out, int B,
                           long per_image, hipStream_t stream) {
  if (int rc = rng_shape_check("noise_blend_rng", per_image)) return rc;
  D3F_CHECK(lam > 0.f, "noise_blend_rng: lambda must be positive");
  if (B == 0 || per_image == 0) return 0;
  const double c = 1.0 / exp((double)lam);
  hipLaunchKernelGGL(noise_blend_rng_kernel, dim3(rng_blocks(per_image), (unsigned)B), dim3(256), 0, stream, x, seed,
                     offset, (const float*)nullptr, (float)c, (float)(1.0 - c), (float)(1.0 / (double)lam), out, r_out,
                     per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

int noise_blend_fixed_rng_launch(const float* x, uint64_t seed, uint64_t offset, const float* r, float* out, int B,
                                 long per_image, hipStream_t stream) {
  if (int rc = rng_shape_check("noise_blend_fixed_rng", per_image)) return rc;
  if (B == 0 || per_image == 0) return 0;
  hipLaunchKernelGGL(noise_blend_rng_kernel, dim3(rng_blocks(per_image), (unsigned)B), dim3(256), 0, stream, x, seed,
                     offset, r, 0.f, 0.f, -1.f, out, (float*)nullptr, per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

// the fixed-ratio blend with the counter's image word taken from index[b] instead of b (held-out validation: an image
// meets the same noise whatever batch it arrives in, and wherever in it).  A kernel of its own next to
// noise_blend_rng_kernel, whose launches stay as they are; the same device functions, so index = 0 .. B-1 gives that
// kernel's bits.  An index outside [0, 2^32) names no counter: the image is written as NaN.
__global__ __launch_bounds__(256) void noise_blend_fixed_index_rng_kernel(const float* __restrict__ x, uint64_t seed,
                                                                          uint64_t offset, const float* __restrict__ r,
                                                                          const int64_t* __restrict__ index,
                                                                          float* __restrict__ out, long per_image) {
  const int b = blockIdx.y;
  const int64_t word = index[b];
  const bool named = word >= 0 && word <= (int64_t)0xFFFFFFFFll;
  const BlendCoef k = blend_coef(r[b], 0.f, 0.f, -1.f);
  const long nvec = per_image / 4;
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + (long)b * per_image);
  float4* __restrict__ ov = reinterpret_cast<float4*>(out + (long)b * per_image);
  if (!named) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256)
      ov[i] = make_float4(NAN, NAN, NAN, NAN);
    return;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256)
    ov[i] = blend4(k, xv[i], rng_normal4(seed, offset, (uint32_t)word, (uint32_t)i));
}

int noise_blend_fixed_index_rng_launch(const float* x, uint64_t seed, uint64_t offset, const float* r,
                                       const int64_t* index, float* out, int B, long per_image, hipStream_t stream) {
  if (int rc = rng_shape_check("noise_blend_fixed_index_rng", per_image)) return rc;
  if (B == 0 || per_image == 0) return 0;
  D3F_CHECK(B <= 65535, "noise_blend_fixed_index_rng: %d images in one call (at most 65535)", B);
  hipLaunchKernelGGL(noise_blend_fixed_index_rng_kernel, dim3(rng_blocks(per_image), (unsigned)B), dim3(256), 0, stream,
                     x, seed, offset, r, index, out, per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

int noise_draw_launch(uint64_t seed, uint64_t offset, float* noise, float* y, int B, long per_image,
                      hipStream_t stream) {
  if (int rc = rng_shape_check("noise_draw", per_image)) return rc;
  if (B == 0 || (noise == nullptr && y == nullptr)) return 0;
  const unsigned bx = (noise != nullptr && per_image > 0) ? rng_blocks(per_image) : 1u;
  hipLaunchKernelGGL(noise_draw_kernel, dim3(bx, (unsigned)B), dim3(256), 0, stream, seed, offset,
                     per_image > 0 ? noise : (float*)nullptr, y, per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

// per-image mean absolute error (compute_difficulty_loss, d3f/balance_training_images/lit_module.py:139-142):
// L1_PARTS partial sums per image, then one thread block per image adds them in a fixed order (f64; l1_image_mean)
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                         double* __restrict__ partial, long per_image) {
  __shared__ double red[256];
  const int b = blockIdx.y;
  const float* pp = p + (long)b * per_image;
  const float* tt = t + (long)b * per_image;
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per_image; i += (long)gridDim.x * 256)
    s += (double)fabsf(pp[i] - tt[i]);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(long)b * L1_PARTS + blockIdx.x] = red[0];
}
__global__ void l1_finalize_kernel(const double* __restrict__ partial, float* __restrict__ out, int B, long per_image) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  out[b] = l1_image_mean(partial, b, per_image);
}
size_t l1_per_image_workspace_bytes(int B) { return (size_t)B * L1_PARTS * sizeof(double) + 64; }
// the first stage alone: partial [B][L1_PARTS] (l1_per_image_scatter_launch, difficulty.hip, shares it)
int l1_partials_launch(const float* pred, const float* target, double* partial, int B, long per_image,
                       hipStream_t stream) {
  hipLaunchKernelGGL(l1_partial_kernel, dim3(L1_PARTS, (unsigned)B), dim3(256), 0, stream, pred, target, partial,
                     per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}
int l1_per_image_launch(const float* pred, const float* target, float* out, void* workspace, int B, long per_image,
                        hipStream_t stream) {
  if (B == 0) return 0;
  double* partial = reinterpret_cast<double*>(workspace);
  if (int rc = l1_partials_launch(pred, target, partial, B, per_image, stream)) return rc;
  hipLaunchKernelGGL(l1_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, partial, out, B, per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
