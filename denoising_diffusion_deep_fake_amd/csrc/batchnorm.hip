// BatchNorm2d layers: train mode forward / backward with the ReLU and the residual add, and the eval-mode coefficients.
// Replaces ATen's batch_norm / batch_norm_backward / relu / add under segmentation_models_pytorch.Unet
// (d3f/train_denoiser/lit_module.py:46-52).  A layer is described and planned once (BnLayer, bn_layer_plan) and runs as
// one call per pass (bn_layer_forward / bn_layer_backward), the same way for the engine and the C API.
//
// The split form runs BatchNorm forward as   partial statistics (conv epilogue) -> bn_finalize (one tiny launch) ->
// bn_apply (streaming pass), and backward as   partial sums (bn_bwd_reduce, or the data-gradient epilogue) ->
// bn_bwd_finalize -> bn_bwd_apply.  On the training step's critical path every one of those 92 finalize launches costs
// its dispatch latency plus 5-14 us of a kernel that keeps 64-512 workgroups busy for a few hundred loads each.  The
// fused form (bn_finalize_apply, bn_bwd_finalize_apply) folds the finalize step into the streaming pass that needs its
// result: the streaming kernel's workgroups REDUNDANTLY reduce the partial rows of their own 32-channel slab first (f64,
// fixed order, 8-256 KB of L2-resident partials per workgroup), derive the slab's coefficients in LDS and go straight on
// to the streaming pass: no second launch, no atomics, no fences, and every workgroup computes bit-identical
// coefficients.  Row block 0 of each slab also writes the coefficients (the backward pass and the data-gradient
// epilogues read them) and updates the running statistics / dgamma, dbeta.  fp32 or bf16 tensors (statistics,
// coefficients and arithmetic are fp32 / f64 in both; bf16 rows are 8-byte vectors per thread), channel counts that are
// a multiple of 32, at most BNF_MAX_ROWS partial rows; the split form serves the rest and synchronised statistics.
#include "common.h"
#include "pointwise.h"
#include "vec16.h"

#include <algorithm>
#include <type_traits>

namespace d3f {

constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;  // torch.nn.BatchNorm2d's defaults

constexpr int BNF_SC = 32;         // channels per slab = one 128-byte line per tensor row
constexpr int BNF_MAX_ROWS = 1024;  // partial rows a workgroup is asked to reduce (x 256 B): 512 / 1024 / 2048 within 0.2 % of each other; 2048 would take in the stem, whose 512 KB prologue per workgroup makes the pass 3x longer
#ifndef BNF_FWD_U_F32
#define BNF_FWD_U_F32 4  // fp32 rows per batch in the forward streaming pass (8: 7.855 / 7.831 / 7.856 ms against 7.866 / 7.860 / 7.843 with 4 -- no gain, 176 instead of 128 VGPRs)
#endif
#ifndef BNF_BWD_U
#define BNF_BWD_U 2  // rows in flight per thread in the backward streaming pass (4: +0.4 % step time -- 142 VGPRs leave one workgroup per CU next to the weight-gradient stream)
#endif  // partial rows a workgroup is asked to reduce (x 256 B)

// Forward coefficients of channel c from its f64 (sum, sum of squares) over `count` rows: mean, invstd and the folded
// scale / shift, returned as (scale, shift); with `store` also written to the coefficient rows, and the running
// statistics (if any) take their momentum step with the unbiased variance.
__device__ __forceinline__ float2 bn_fwd_coef(double s1, double s2, double count, int c, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, float momentum, bool store,
                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                              float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                              float* __restrict__ scale_o, float* __restrict__ shift_o) {
  const double mean = s1 / count;
  double var = s2 / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const double invstd = 1.0 / sqrt(var + (double)eps);
  const float g = gamma[c], bt = beta[c];
  const float sc = (float)((double)g * invstd), sf = (float)((double)bt - mean * (double)g * invstd);
  if (store) {
    mean_o[c] = (float)mean; invstd_o[c] = (float)invstd; scale_o[c] = sc; shift_o[c] = sf;
    if (running_mean != nullptr) {
      const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
      running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
      running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
    }
  }
  return make_float2(sc, sf);
}

// Backward coefficients of channel c from the f64 sums s1 = sum dz, s2 = sum dz * xhat over `count` rows, returned as
// (k0, k1, k2) = (gamma * invstd, s1 / count, s2 / count); with `store` also written to k[3][C], and the sums to dbeta /
// dgamma (null: not wanted).
__device__ __forceinline__ float3 bn_bwd_coef(double s1, double s2, double count, int c, int C,
                                              const float* __restrict__ gamma, const float* __restrict__ invstd, bool store,
                                              float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ k) {
  const float k0 = gamma[c] * invstd[c], k1 = (float)(s1 / count), k2 = (float)(s2 / count);
  if (store) {
    if (dgamma != nullptr) { dgamma[c] = (float)s2; dbeta[c] = (float)s1; }
    k[c] = k0; k[C + c] = k1; k[2 * C + c] = k2;
  }
  return make_float3(k0, k1, k2);
}

// runs f((T*)nullptr), T = the tensors' element type of a storage dtype
template <typename F> static void by_dtype(int dtype, F&& f) {
  if (dtype == D3F_F32) f((float*)nullptr);
  else f((bf16_t*)nullptr);
}

// ------------------------------------------------------------------------------------------
// BatchNorm forward
// ------------------------------------------------------------------------------------------
// one workgroup per channel: 256 lanes stride over the m-tile partials (up to 8192 of them for the
// 256x16 tiles), f64 accumulation, wave shuffle + LDS tree
__device__ __forceinline__ void block_sum2(double& s1, double& s2) {
  __shared__ double red[2][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s1;
    red[1][threadIdx.x >> 6] = s2;
  }
  __syncthreads();
  s1 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  s2 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// a thread's share of one channel's partial rows (rows tid, tid + 256, ... of [rows][ld / 2][2]), added in that order;
// the loads of eight rows (then four) are issued in front of their adds -- a C = 16 layer brings 4096 rows to 16
// workgroups, and with one load in flight per thread the kernel was sixteen dependent L2 round trips long
__device__ __forceinline__ void column_sum2(const float* __restrict__ col, int rows, long ld, double& s1, double& s2) {
  int t = threadIdx.x;
  for (; t + 7 * 256 < rows; t += 8 * 256) {
    float2 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float2*>(col + (long)(t + j * 256) * ld);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1 += (double)v[j].x; s2 += (double)v[j].y; }
  }
  for (; t + 3 * 256 < rows; t += 4 * 256) {
    float2 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float2*>(col + (long)(t + j * 256) * ld);
#pragma unroll
    for (int j = 0; j < 4; ++j) { s1 += (double)v[j].x; s2 += (double)v[j].y; }
  }
  for (; t < rows; t += 256) {
    const float2 v = *reinterpret_cast<const float2*>(col + (long)t * ld);
    s1 += (double)v.x;
    s2 += (double)v.y;
  }
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(
    const float* __restrict__ stats, int tiles, int C, int Cpad, double count,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
    float* __restrict__ running_mean, float* __restrict__ running_var, float* __restrict__ mean_o,
    float* __restrict__ invstd_o, float* __restrict__ scale_o, float* __restrict__ shift_o, NetSplit ns) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): blockIdx.z = net
    net_shift(stats, ns.ws); net_shift(gamma, ns.par); net_shift(beta, ns.par);
    net_shift(running_mean, ns.bn); net_shift(running_var, ns.bn);
    net_shift(mean_o, ns.ws); net_shift(invstd_o, ns.ws); net_shift(scale_o, ns.ws); net_shift(shift_o, ns.ws);
  }
  const int c = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  column_sum2(stats + (long)c * 2, tiles, (long)Cpad * 2, s1, s2);
  block_sum2(s1, s2);
  if (threadIdx.x == 0)
    bn_fwd_coef(s1, s2, count, c, gamma, beta, eps, momentum, true, running_mean, running_var, mean_o, invstd_o, scale_o,
                shift_o);
}

// every BatchNorm of the network in one launch (eval forward): block = layer, table as kernel argument
__global__ __launch_bounds__(256) void bn_eval_coeff_all_kernel(const float* __restrict__ params,
                                                                const float* __restrict__ bnstats,
                                                                char* __restrict__ ws, float eps, BnEvalTable t) {
  const BnEvalEntry e = t.e[blockIdx.x];
  float* __restrict__ coef = reinterpret_cast<float*>(ws + (size_t)e.coef_off16 * 16);
  for (int c = threadIdx.x; c < e.C; c += 256) {
    const float invstd = 1.0f / sqrtf(bnstats[e.rv_off + c] + eps);
    const float sc = params[e.g_off + c] * invstd;
    coef[2 * e.C + c] = sc;
    coef[3 * e.C + c] = params[e.b_off + c] - bnstats[e.rm_off + c] * sc;
  }
}

static_assert(BN_SCALE == 2 && BN_SHIFT == 3, "bn_eval_coeff_all_kernel writes the scale / shift rows");
int bn_eval_coeff_all_launch(const float* params, const float* bnstats, void* ws, const BnEvalTable& t,
                             hipStream_t stream) {
  if (t.n == 0) return 0;
  hipLaunchKernelGGL(bn_eval_coeff_all_kernel, dim3(t.n), dim3(256), 0, stream, params, bnstats, (char*)ws, BN_EPS, t);
  D3F_HIP(hipGetLastError());
  return 0;
}

// out = [relu](y * scale + shift [+ residual]).  RES: 0 no residual, 1 a tensor, 2 another layer's y under its own
// coefficients.  A thread's vectors are a whole number of tensor rows apart (256 * N % C == 0: bn_layer_apply), so its N
// channels and their coefficients are loop invariants held in registers; U vectors per trip, every load of a trip in
// front of its arithmetic.
template <typename T, int RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(
    const T* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
    const T* __restrict__ res, const T* __restrict__ yr, const float* __restrict__ scale_r,
    const float* __restrict__ shift_r, int relu, T* __restrict__ out, long nvec, int C, long net_ws) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): every operand lives in the workspace
    net_shift(y, net_ws); net_shift(scale, net_ws); net_shift(shift, net_ws); net_shift(res, net_ws); net_shift(yr, net_ws);
    net_shift(scale_r, net_ws); net_shift(shift_r, net_ws); net_shift(out, net_ws);
  }
  constexpr int N = V16<T>::N, U = N == 4 ? 4 : 2;  // (bf16: 8 floats per vector; U = 4 takes up to 98 VGPRs here, 5 waves per SIMD with U = 2)
  const int c0 = ((int)threadIdx.x * N) % C;
  float sc[N], sf[N], scr[N], sfr[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    sc[k] = scale[c0 + k];
    sf[k] = shift[c0 + k];
    scr[k] = RES == 2 ? scale_r[c0 + k] : 0.f;
    sfr[k] = RES == 2 ? shift_r[c0 + k] : 0.f;
  }
  const T* __restrict__ rsrc = RES == 2 ? yr : res;
  auto one = [&](float (&v)[N], const float (&r)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] * sc[k] + sf[k];
    if constexpr (RES == 1) {
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] += r[k];
    } else if constexpr (RES == 2) {
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] += r[k] * scr[k] + sfr[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = fmaxf(v[k], 0.f);
    }
  };
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + (U - 1) * stride < nvec; i += U * stride) {
    float v[U][N], r[U][N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      V16<T>::load(y + (i + u * stride) * N, v[u]);
      if constexpr (RES != 0) V16<T>::load(rsrc + (i + u * stride) * N, r[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      one(v[u], r[u]);
      V16<T>::store(out + (i + u * stride) * N, v[u]);
    }
  }
  for (; i < nvec; i += stride) {
    float v[N], r[N];
    V16<T>::load(y + i * N, v);
    if constexpr (RES != 0) V16<T>::load(rsrc + i * N, r);
    one(v, r);
    V16<T>::store(out + i * N, v);
  }
}


// ------------------------------------------------------------------------------------------
// BatchNorm backward.  dz = dA * [a > 0];  dbeta = sum dz;  dgamma = sum dz * xhat;
// dy = gamma*invstd * (dz - dbeta/N - xhat * dgamma/N)
// ------------------------------------------------------------------------------------------

// ReLU mask: from the saved activation `a` (a > 0), or -- for layers without a residual, mask_scale !=
// null -- recomputed from y with the forward's own arithmetic (y*scale + shift > 0), which saves reading `a`.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(
    const T* __restrict__ dA, const T* __restrict__ a, const T* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ partial,
    long rows, int C, const float* __restrict__ mask_scale, const float* __restrict__ mask_shift, long net_ws) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): every operand lives in the workspace
    net_shift(dA, net_ws); net_shift(a, net_ws); net_shift(y, net_ws); net_shift(mean, net_ws); net_shift(invstd, net_ws);
    net_shift(partial, net_ws); net_shift(mask_scale, net_ws); net_shift(mask_shift, net_ws);
  }
  constexpr int N = V16<T>::N;
  __shared__ float red[256 * N * 2];
  const int VC = C / N;        // vectors per row (power of two, <= 256)
  const int RP = 256 / VC;     // rows per pass
  const int cv = threadIdx.x % VC, r0 = threadIdx.x / VC;
  const long rows_per_block = (rows + gridDim.x - 1) / gridDim.x;
  const long rbeg = (long)blockIdx.x * rows_per_block;
  long rend = rbeg + rows_per_block;
  if (rend > rows) rend = rows;
  float mu[N], is[N], s1[N], s2[N], msc[N], msf[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    mu[k] = mean[cv * N + k];
    is[k] = invstd[cv * N + k];
    msc[k] = mask_scale ? mask_scale[cv * N + k] : 0.f;
    msf[k] = mask_scale ? mask_shift[cv * N + k] : 0.f;
    s1[k] = 0.f;
    s2[k] = 0.f;
  }
  // U rows per trip: all loads of a trip are issued before any arithmetic (memory-level parallelism)
  constexpr int U = 4;
  const bool from_y = mask_scale != nullptr, from_a = !from_y && a != nullptr;
  long r = rbeg + r0;
  for (; r + (U - 1) * RP < rend; r += U * RP) {
    float g[U][N], yy[U][N], aa[U][N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long off = (r + u * RP) * C + cv * N;
      V16<T>::load(dA + off, g[u]);
      V16<T>::load(y + off, yy[u]);
      if (from_a) V16<T>::load(a + off, aa[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const float keep = from_y ? yy[u][k] * msc[k] + msf[k] : (from_a ? aa[u][k] : 1.f);
        const float gz = keep > 0.f ? g[u][k] : 0.f;
        s1[k] += gz;
        s2[k] += gz * ((yy[u][k] - mu[k]) * is[k]);
      }
    }
  }
  for (; r < rend; r += RP) {
    const long off = r * C + cv * N;
    float g[N], yy[N], aa[N];
    V16<T>::load(dA + off, g);
    V16<T>::load(y + off, yy);
    if (from_a) V16<T>::load(a + off, aa);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float keep = from_y ? yy[k] * msc[k] + msf[k] : (from_a ? aa[k] : 1.f);
      const float gz = keep > 0.f ? g[k] : 0.f;
      s1[k] += gz;
      s2[k] += gz * ((yy[k] - mu[k]) * is[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    red[(threadIdx.x * N + k) * 2 + 0] = s1[k];
    red[(threadIdx.x * N + k) * 2 + 1] = s2[k];
  }
  __syncthreads();
  // thread t < 2*C sums column t over the RP row groups
  for (int t = threadIdx.x; t < 2 * C; t += 256) {
    const int c = t >> 1, which = t & 1;
    const int v = c / N, k = c % N;
    float s = 0.f;
    for (int rr = 0; rr < RP; ++rr) s += red[((rr * VC + v) * N + k) * 2 + which];
    partial[((long)blockIdx.x * C + c) * 2 + which] = s;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(
    const float* __restrict__ partial, int nblocks, int C, double count,
    const float* __restrict__ gamma, const float* __restrict__ invstd, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ coef, NetSplit ns) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit)
    net_shift(partial, ns.ws); net_shift(gamma, ns.par); net_shift(invstd, ns.ws);
    net_shift(dgamma, ns.grad); net_shift(dbeta, ns.grad); net_shift(coef, ns.ws);
  }
  const int c = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  column_sum2(partial + (long)c * 2, nblocks, (long)C * 2, s1, s2);
  block_sum2(s1, s2);
  if (threadIdx.x == 0) bn_bwd_coef(s1, s2, count, c, C, gamma, invstd, true, dgamma, dbeta, coef);
}

// MASK: 0 none, 1 recomputed from y, 2 read from a.  DRES: 0 none, 1 written, 2 accumulated.  As bn_apply_kernel: the
// thread's channels and their seven coefficient vectors are loop invariants, U vectors per trip with every load of a
// trip in front of its arithmetic.
template <typename T, int MASK, int DRES>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    const T* __restrict__ dA, const T* __restrict__ a, const T* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ coef,
    T* __restrict__ dy, T* __restrict__ dres, long nvec, int C,
    const float* __restrict__ mask_scale, const float* __restrict__ mask_shift, long net_ws) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): every operand lives in the workspace
    net_shift(dA, net_ws); net_shift(a, net_ws); net_shift(y, net_ws); net_shift(mean, net_ws); net_shift(invstd, net_ws);
    net_shift(coef, net_ws); net_shift(dy, net_ws); net_shift(dres, net_ws); net_shift(mask_scale, net_ws);
    net_shift(mask_shift, net_ws);
  }
  constexpr int N = V16<T>::N, U = N == 4 ? 4 : 2;  // (bf16: 8 floats per vector: U = 2 already takes 127-202 VGPRs, 2-4 waves per SIMD -- 101 MB in 20 us all the same; U = 4: 160-236)
  const int c0 = ((int)threadIdx.x * N) % C;
  float mu[N], is[N], k0[N], k1[N], k2[N], msc[N], msf[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int c = c0 + k;
    mu[k] = mean[c];
    is[k] = invstd[c];
    k0[k] = coef[c];
    k1[k] = coef[C + c];
    k2[k] = coef[2 * C + c];
    msc[k] = MASK == 1 ? mask_scale[c] : 0.f;
    msf[k] = MASK == 1 ? mask_shift[c] : 0.f;
  }
  auto one = [&](float (&g)[N], const float (&yy)[N], const float (&aa)[N], float (&o)[N]) {
    if constexpr (MASK == 1) {
#pragma unroll
      for (int k = 0; k < N; ++k) g[k] = (yy[k] * msc[k] + msf[k]) > 0.f ? g[k] : 0.f;
    } else if constexpr (MASK == 2) {
#pragma unroll
      for (int k = 0; k < N; ++k) g[k] = aa[k] > 0.f ? g[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float xhat = (yy[k] - mu[k]) * is[k];
      o[k] = k0[k] * (g[k] - k1[k] - xhat * k2[k]);
    }
  };
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + (U - 1) * stride < nvec; i += U * stride) {
    float g[U][N], yy[U][N], aa[U][N], d[U][N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long e = (i + u * stride) * N;
      V16<T>::load(dA + e, g[u]);
      V16<T>::load(y + e, yy[u]);
      if constexpr (MASK == 2) V16<T>::load(a + e, aa[u]);
      if constexpr (DRES == 2) V16<T>::load(dres + e, d[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long e = (i + u * stride) * N;
      float o[N];
      one(g[u], yy[u], aa[u], o);
      V16<T>::store(dy + e, o);
      if constexpr (DRES == 2) {
#pragma unroll
        for (int k = 0; k < N; ++k) g[u][k] += d[u][k];
      }
      if constexpr (DRES != 0) V16<T>::store(dres + e, g[u]);
    }
  }
  for (; i < nvec; i += stride) {
    float g[N], yy[N], aa[N], d[N], o[N];
    V16<T>::load(dA + i * N, g);
    V16<T>::load(y + i * N, yy);
    if constexpr (MASK == 2) V16<T>::load(a + i * N, aa);
    if constexpr (DRES == 2) V16<T>::load(dres + i * N, d);
    one(g, yy, aa, o);
    V16<T>::store(dy + i * N, o);
    if constexpr (DRES == 2) {
#pragma unroll
      for (int k = 0; k < N; ++k) g[k] += d[k];
    }
    if constexpr (DRES != 0) V16<T>::store(dres + i * N, g);
  }
}

// four channels of one tensor row as they sit in memory (fp32: 16 bytes, bf16: 8 bytes): what a prefetched batch keeps in
// registers until its turn
template <typename T> struct Raw4;
template <> struct Raw4<float> { typedef float4 type; };
template <> struct Raw4<bf16_t> { typedef uint2 type; };
__device__ __forceinline__ float4 ldraw(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint2 ldraw(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ float4 cvt4(const float4& v) { return v; }
__device__ __forceinline__ float4 cvt4(const uint2& v) {
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                     __uint_as_float(v.y & 0xffff0000u));
}

// sums the partial rows [rows][ld][2] of channels [c0, c0 + 32) in f64: thread (rl = tid / 16, q = tid % 16) owns the
// float4 q of the slab (channels c0 + 2q, c0 + 2q + 1; sum, second sum each) of rows rl, rl + 16, ...; the 16 row
// lanes are then added in lane order.  tot[2 * ch + which] for ch < 32.  `behind_first_loads()` runs once, right behind
// the issue of the first batch of partial-row loads: the streaming pass puts the loads of its first rows there, so that
// they travel while the reduce waits for its own (the coefficients do not depend on them).
template <typename F>
__device__ __forceinline__ void slab_reduce(const float* __restrict__ partial, int rows, int ld, int c0,
                                            double (&red)[16][64], double (&tot)[64], F behind_first_loads) {
  const int tid = threadIdx.x, q = tid & 15, rl = tid >> 4;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  const float* base = partial + ((long)c0 * 2 + q * 4);
  int r = rl;
  bool hooked = false;
  for (; r + 112 < rows; r += 128) {  // eight rows in flight (layer1-type layers bring 512 partial rows)
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float4*>(base + (long)(r + 16 * j) * ld * 2);
    if (!hooked) { behind_first_loads(); hooked = true; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a0 += (double)v[j].x; a1 += (double)v[j].y; a2 += (double)v[j].z; a3 += (double)v[j].w;
    }
  }
  for (; r + 48 < rows; r += 64) {  // four rows in flight
    const float4 v0 = *reinterpret_cast<const float4*>(base + (long)r * ld * 2);
    const float4 v1 = *reinterpret_cast<const float4*>(base + (long)(r + 16) * ld * 2);
    const float4 v2 = *reinterpret_cast<const float4*>(base + (long)(r + 32) * ld * 2);
    const float4 v3 = *reinterpret_cast<const float4*>(base + (long)(r + 48) * ld * 2);
    if (!hooked) { behind_first_loads(); hooked = true; }
    a0 += (double)v0.x; a1 += (double)v0.y; a2 += (double)v0.z; a3 += (double)v0.w;
    a0 += (double)v1.x; a1 += (double)v1.y; a2 += (double)v1.z; a3 += (double)v1.w;
    a0 += (double)v2.x; a1 += (double)v2.y; a2 += (double)v2.z; a3 += (double)v2.w;
    a0 += (double)v3.x; a1 += (double)v3.y; a2 += (double)v3.z; a3 += (double)v3.w;
  }
  if (!hooked) behind_first_loads();  // (fewer than 64 partial rows: in front of the tail's loads)
  for (; r < rows; r += 16) {
    const float4 v = *reinterpret_cast<const float4*>(base + (long)r * ld * 2);
    a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
  }
  red[rl][q * 4 + 0] = a0;
  red[rl][q * 4 + 1] = a1;
  red[rl][q * 4 + 2] = a2;
  red[rl][q * 4 + 3] = a3;
  __syncthreads();
  if (tid < 64) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][tid];
    tot[tid] = s;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// forward: statistics -> (mean, invstd, scale, shift, running stats) -> out = [relu](y * scale + shift [+ residual])
// grid = (row blocks, C / 32); residual forms as bn_apply_kernel
// ------------------------------------------------------------------------------------------
// The streaming pass keeps TWO batches of U rows per thread in flight: the loads of batch i + 1 are issued in front of the
// arithmetic and the stores of batch i, and batch 0 travels during the slab reduce -- the pass was latency-bound (a
// layer1-type fp32 launch: 16 rows per thread = four dependent load -> store rounds behind the reduce, 10-13 us for 34 MB).
template <typename T, bool HAS2>
__global__ __launch_bounds__(256) void bn_finalize_apply_kernel(
    const float* __restrict__ stats, int stat_rows, int C, int Cpad, double count,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
    float* __restrict__ running_mean, float* __restrict__ running_var, float* __restrict__ mean_o,
    float* __restrict__ invstd_o, float* __restrict__ scale_o, float* __restrict__ shift_o,
    const T* __restrict__ y, const T* __restrict__ res, const T* __restrict__ yr,
    const float* __restrict__ scale_r, const float* __restrict__ shift_r, int relu, T* __restrict__ out,
    long rows, long rows_per_block, NetSplit ns) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): blockIdx.z = net
    net_shift(stats, ns.ws); net_shift(gamma, ns.par); net_shift(beta, ns.par);
    net_shift(running_mean, ns.bn); net_shift(running_var, ns.bn);
    net_shift(mean_o, ns.ws); net_shift(invstd_o, ns.ws); net_shift(scale_o, ns.ws); net_shift(shift_o, ns.ws);
    net_shift(y, ns.ws); net_shift(res, ns.ws); net_shift(yr, ns.ws); net_shift(scale_r, ns.ws); net_shift(shift_r, ns.ws);
    net_shift(out, ns.ws);
  }
  __shared__ double red[16][64];
  __shared__ double tot[64];
  __shared__ float cf[2][BNF_SC];
  typedef typename Raw4<T>::type raw_t;
  constexpr int U = sizeof(T) == 4 ? BNF_FWD_U_F32 : 8;  // rows per batch: 2 x U x 16 (8) bytes per thread in flight
  const int tid = threadIdx.x, c0 = blockIdx.y * BNF_SC;
  // streaming pass: thread (rr = tid / 8, v = tid % 8) owns channels c0 + 4v .. + 3 of rows rr, rr + 32, ...
  const int v = tid & 7, rr = tid >> 3, cc = c0 + v * 4;
  const long r0 = (long)blockIdx.x * rows_per_block;
  long r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  const T* __restrict__ second = res != nullptr ? res : yr;
  raw_t a[U], b[U], an[U], bn[U];
  auto load = [&](raw_t (&ya)[U], raw_t (&yb)[U], long r) {
#pragma unroll
    for (int u = 0; u < U; ++u) {  // rows past the block's end re-read its last row (never stored): straight-line loads
      const long row = r + 32 * u < r1 ? r + 32 * u : r1 - 1;
      ya[u] = ldraw(y + row * C + cc);
      if (HAS2) yb[u] = ldraw(second + row * C + cc);
    }
  };
  slab_reduce(stats, stat_rows, Cpad, c0, red, tot, [&]() { load(a, b, r0 + rr); });
  if (tid < BNF_SC) {
    const float2 f = bn_fwd_coef(tot[2 * tid], tot[2 * tid + 1], count, c0 + tid, gamma, beta, eps, momentum,
                                 blockIdx.x == 0, running_mean, running_var, mean_o, invstd_o, scale_o, shift_o);
    cf[0][tid] = f.x;
    cf[1][tid] = f.y;
  }
  __syncthreads();
  float sc[4], sf[4], scr[4] = {0.f, 0.f, 0.f, 0.f}, sfr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sc[k] = cf[0][v * 4 + k];
    sf[k] = cf[1][v * 4 + k];
    if (HAS2 && res == nullptr) {
      scr[k] = scale_r[cc + k];
      sfr[k] = shift_r[cc + k];
    }
  }
  for (long r = r0 + rr; r < r1; r += 32 * U) {
    if (r + 32 * U < r1) load(an, bn, r + 32 * U);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = r + 32 * u;
      if (row >= r1) continue;
      const float4 ya = cvt4(a[u]);
      float x[4] = {ya.x, ya.y, ya.z, ya.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = x[k] * sc[k] + sf[k];
      if (HAS2) {
        const float4 yb = cvt4(b[u]);
        if (res != nullptr) {
          x[0] += yb.x; x[1] += yb.y; x[2] += yb.z; x[3] += yb.w;
        } else {
          const float t[4] = {yb.x, yb.y, yb.z, yb.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) x[k] += t[k] * scr[k] + sfr[k];
        }
      }
      if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = fmaxf(x[k], 0.f);
      }
      st4<T>(out + row * C + cc, make_float4(x[0], x[1], x[2], x[3]));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = an[u];
      if (HAS2) b[u] = bn[u];
    }
  }
}

// rows per workgroup, whole passes of 32 rows.  Workgroups in all: ~256 for fp32 tensors, ~512 for bf16 (r03 sweep of
// 64 ... 1024 with the chain's kernels at wave priority 3: fp32 256x256 8.88 / 8.38 / 8.30 / 8.24 / 8.28 / 8.30 / 8.35 ms
// per step at 64 / 128 / 192 / 256 / 320 / 512 / 768 -- every workgroup repeats the slab reduce, fewer of them repeat it
// less; bf16 4.83 / 4.58 / 4.55 at 128 / 256 / 512: half the bytes per row, the streaming part wants the parallelism;
// re-swept in round 4 with two batches in flight: fp32 7.87 / 7.91 / 7.94 / 7.94 / 8.02 ms at 256 / 384 / 512 / 768 / 1024,
// bf16 4.09 / 4.09 / 4.12 / 4.18 at 384 / 512 / 768 / 1024 -- unchanged optimum; 512 / 768 / 1024 only for the tensors of 32 MB
// and more (stem, decoder block 3): 7.89 / 7.91 / 7.90 against 7.87 / 7.89 -- no gain either)
static long rows_per_block_for(long rows, int slabs, int dtype, int plan_nets) {
  const long wgs = (dtype == D3F_F32 ? 256 : 512) / plan_nets_for(plan_nets, 64);  // (two networks in one launch share the count)
  long rb = std::max(1L, wgs / slabs);
  long rpb = (rows + rb - 1) / rb;
  rpb = (rpb + 31) / 32 * 32;
  return std::max(32L, rpb);
}

// the residual operands of a = act(y*scale + shift + residual): an activation (res), or another layer's y (yr) with its
// scale / shift
struct BnResidualOps {
  const void *res = nullptr, *yr = nullptr;
  const float *scale_r = nullptr, *shift_r = nullptr;
};
static BnResidualOps residual_ops(const BnLayer& L, const BnBufs& b) {
  if (L.res == BN_RES_TENSOR) return {b.res, nullptr, nullptr, nullptr};
  if (L.res == BN_RES_LAYER) return {nullptr, b.res, bn_coef(b.res_coef, L.C, BN_SCALE), bn_coef(b.res_coef, L.C, BN_SHIFT)};
  return {};
}

static int bn_finalize_apply_launch(const BnLayer& L, const BnBufs& b, hipStream_t stream, const NetSplit* ns) {
  if (L.rows == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid((unsigned)((L.rows + L.rows_per_block - 1) / L.rows_per_block), (unsigned)(L.C / BNF_SC),
                  (unsigned)nv.nets);
  const BnResidualOps r = residual_ops(L, b);
  by_dtype(L.dtype, [&](auto* typed) {
    typedef std::remove_pointer_t<decltype(typed)> T;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, b.stats, L.fwd_rows, L.C, L.Cpad, (double)L.rows, b.gamma,
                         b.beta, BN_EPS, BN_MOMENTUM, b.running_mean, b.running_var, bn_coef(b.coef, L.C, BN_MEAN),
                         bn_coef(b.coef, L.C, BN_INVSTD), bn_coef(b.coef, L.C, BN_SCALE), bn_coef(b.coef, L.C, BN_SHIFT),
                         (const T*)b.y, (const T*)r.res, (const T*)r.yr, r.scale_r, r.shift_r, L.relu ? 1 : 0, (T*)b.a,
                         L.rows, L.rows_per_block, nv);
    };
    if (L.res != BN_RES_NONE) go(bn_finalize_apply_kernel<T, true>);
    else go(bn_finalize_apply_kernel<T, false>);
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// backward: partial sums of dz, dz * xhat -> (dgamma, dbeta, coefficients) ->
//   dy = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)),  dz = dA * [a > 0]   (as bn_bwd_apply_kernel)
// ------------------------------------------------------------------------------------------
// FROM_A: the ReLU mask is read from the stored activation (layers with a residual add; else it is recomputed from
// y * mask_scale + mask_shift, or there is no ReLU); RD_DRES: dres is accumulated into.  Template flags so that a launch
// keeps only the tensors it reads in registers: two batches of U rows per thread in flight as in the forward pass.
template <typename T, bool FROM_A, bool RD_DRES>
__global__ __launch_bounds__(256) void bn_bwd_finalize_apply_kernel(
    const float* __restrict__ partial, int nblocks, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ coef, const T* __restrict__ dA,
    const T* __restrict__ a, const T* __restrict__ y, T* __restrict__ dy, T* __restrict__ dres,
    long rows, long rows_per_block, const float* __restrict__ mask_scale,
    const float* __restrict__ mask_shift, NetSplit ns) {
  chain_priority();
  if (blockIdx.z != 0) {  // two networks in one launch (common.h, NetSplit): blockIdx.z = net
    net_shift(partial, ns.ws); net_shift(gamma, ns.par); net_shift(mean, ns.ws); net_shift(invstd, ns.ws);
    net_shift(dgamma, ns.grad); net_shift(dbeta, ns.grad); net_shift(coef, ns.ws);
    net_shift(dA, ns.ws); net_shift(a, ns.ws); net_shift(y, ns.ws); net_shift(dy, ns.ws); net_shift(dres, ns.ws);
    net_shift(mask_scale, ns.ws); net_shift(mask_shift, ns.ws);
  }
  __shared__ double red[16][64];
  __shared__ double tot[64];
  __shared__ float cf[3][BNF_SC];
  typedef typename Raw4<T>::type raw_t;
  constexpr int U = BNF_BWD_U;
  const int tid = threadIdx.x, c0 = blockIdx.y * BNF_SC;
  const int v = tid & 7, rr = tid >> 3, cc = c0 + v * 4;
  const long r0 = (long)blockIdx.x * rows_per_block;
  long r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  raw_t g4[U], y4[U], a4[U], d4[U], g4n[U], y4n[U], a4n[U], d4n[U];
  auto load = [&](raw_t (&gg)[U], raw_t (&yy)[U], raw_t (&aa)[U], raw_t (&dd)[U], long r) {
#pragma unroll
    for (int u = 0; u < U; ++u) {  // rows past the block's end re-read its last row (never stored): straight-line loads
      const long row = r + 32 * u < r1 ? r + 32 * u : r1 - 1;
      gg[u] = ldraw(dA + row * C + cc);
      yy[u] = ldraw(y + row * C + cc);
      if (FROM_A) aa[u] = ldraw(a + row * C + cc);
      if (RD_DRES) dd[u] = ldraw(dres + row * C + cc);
    }
  };
  slab_reduce(partial, nblocks, C, c0, red, tot, [&]() { load(g4, y4, a4, d4, r0 + rr); });
  if (tid < BNF_SC) {
    const float3 k = bn_bwd_coef(tot[2 * tid], tot[2 * tid + 1], count, c0 + tid, C, gamma, invstd, blockIdx.x == 0,
                                 dgamma, dbeta, coef);
    cf[0][tid] = k.x;
    cf[1][tid] = k.y;
    cf[2][tid] = k.z;
  }
  __syncthreads();
  float k0[4], k1[4], k2[4], mu[4], is[4], msc[4] = {0.f, 0.f, 0.f, 0.f}, msf[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    k0[k] = cf[0][v * 4 + k];
    k1[k] = cf[1][v * 4 + k];
    k2[k] = cf[2][v * 4 + k];
    mu[k] = mean[cc + k];
    is[k] = invstd[cc + k];
    if (!FROM_A && mask_scale != nullptr) {
      msc[k] = mask_scale[cc + k];
      msf[k] = mask_shift[cc + k];
    }
  }
  for (long r = r0 + rr; r < r1; r += 32 * U) {
    if (r + 32 * U < r1) load(g4n, y4n, a4n, d4n, r + 32 * U);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = r + 32 * u;
      if (row >= r1) continue;
      const float4 gv = cvt4(g4[u]), yv = cvt4(y4[u]);
      float g[4] = {gv.x, gv.y, gv.z, gv.w};
      const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
      if (FROM_A) {
        const float4 av = cvt4(a4[u]);
        const float aa[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = aa[k] > 0.f ? g[k] : 0.f;
      } else if (mask_scale != nullptr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = (yy[k] * msc[k] + msf[k]) > 0.f ? g[k] : 0.f;
      }
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xhat = (yy[k] - mu[k]) * is[k];
        o[k] = k0[k] * (g[k] - k1[k] - xhat * k2[k]);
      }
      st4<T>(dy + row * C + cc, make_float4(o[0], o[1], o[2], o[3]));
      if (dres != nullptr) {
        if (RD_DRES) {
          const float4 dv = cvt4(d4[u]);
          g[0] += dv.x; g[1] += dv.y; g[2] += dv.z; g[3] += dv.w;
        }
        st4<T>(dres + row * C + cc, make_float4(g[0], g[1], g[2], g[3]));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      g4[u] = g4n[u];
      y4[u] = y4n[u];
      if (FROM_A) a4[u] = a4n[u];
      if (RD_DRES) d4[u] = d4n[u];
    }
  }
}

// the backward's operands besides dA and y: the coefficient rows (k: the block's own, or the caller's) and the ReLU mask,
// read from the stored activation (a) or recomputed from y with the forward's own scale / shift (mask_scale / mask_shift)
struct BnBwdOps {
  const float *mean, *invstd;
  float* k;
  const void* a;
  const float *mask_scale, *mask_shift;
};
static BnBwdOps bwd_ops(const BnLayer& L, const BnBufs& b) {
  const bool from_y = L.mask == BN_MASK_FROM_Y;
  return {bn_coef(b.coef, L.C, BN_MEAN), bn_coef(b.coef, L.C, BN_INVSTD), b.k != nullptr ? b.k : bn_coef(b.coef, L.C, BN_K),
          L.mask == BN_MASK_FROM_A ? b.a : nullptr, from_y ? bn_coef(b.coef, L.C, BN_SCALE) : nullptr,
          from_y ? bn_coef(b.coef, L.C, BN_SHIFT) : nullptr};
}

static int bn_bwd_finalize_apply_launch(const BnLayer& L, const BnBufs& b, const BnBwdOps& o, hipStream_t stream,
                                        const NetSplit* ns) {
  if (L.rows == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const dim3 grid((unsigned)((L.rows + L.rows_per_block - 1) / L.rows_per_block), (unsigned)(L.C / BNF_SC),
                  (unsigned)nv.nets);
  const bool from_a = o.mask_scale == nullptr && o.a != nullptr;
  const bool rd_dres = b.dres != nullptr && b.dres_acc;
  by_dtype(L.dtype, [&](auto* typed) {
    typedef std::remove_pointer_t<decltype(typed)> T;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, b.stats, L.bwd_rows, L.C, (double)L.rows, b.gamma, o.mean,
                         o.invstd, b.dgamma, b.dbeta, o.k, (const T*)b.dA, (const T*)o.a, (const T*)b.y, (T*)b.dy,
                         (T*)b.dres, L.rows, L.rows_per_block, o.mask_scale, o.mask_shift, nv);
    };
    if (from_a && rd_dres) go(bn_bwd_finalize_apply_kernel<T, true, true>);
    else if (from_a) go(bn_bwd_finalize_apply_kernel<T, true, false>);
    else if (rd_dres) go(bn_bwd_finalize_apply_kernel<T, false, true>);
    else go(bn_bwd_finalize_apply_kernel<T, false, false>);
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// the layer: planned once, one call per pass
// ------------------------------------------------------------------------------------------
void bn_layer_plan(BnLayer& L) {
  // fallback knob, read by the shipped library too (the suite runs the network with it): separate launches everywhere
  static const bool no_fused = getenv("D3F_NO_BN_FUSED_FINALIZE") != nullptr;
  auto fused_ok = [&](int rows) {  // fp32 / bf16 tensors, whole slabs, at most BNF_MAX_ROWS partial rows
    return L.allow_fused && !no_fused && (L.dtype == D3F_F32 || L.dtype == D3F_BF16) && L.C % BNF_SC == 0 && rows >= 1 &&
           rows <= BNF_MAX_ROWS;
  };
  // bn_bwd_reduce: a block covers at least one unrolled trip (4 passes of 256 threads) and 16 rows; small tensors then
  // still spread over enough CUs to hide the load latency
  const long min_rows = std::max(16L, 4L * (256 / std::max(1, std::min(256, L.C / (L.dtype == D3F_F32 ? 4 : 8)))));
  L.reduce_blocks = (int)std::clamp((L.rows + min_rows - 1) / min_rows, 1L, 1024L);
  L.bwd_rows = L.fused_rows > 0 ? L.fused_rows : L.reduce_blocks;
  L.fwd_fused = L.apply && fused_ok(L.fwd_rows);
  L.bwd_fused = fused_ok(L.bwd_rows);
  L.rows_per_block = L.fwd_fused || L.bwd_fused ? rows_per_block_for(L.rows, L.C / BNF_SC, L.dtype, L.plan_nets) : 0;
  L.stat_floats = (size_t)L.fwd_rows * L.Cpad * 2;
  L.part_floats = (size_t)std::max(L.reduce_blocks, L.fused_rows) * L.C * 2;
}

int bn_layer_finalize(const BnLayer& L, const BnBufs& b, long count, hipStream_t stream, const NetSplit* ns) {
  const NetSplit nv = net_split_or_single(ns);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(L.C, 1, nv.nets), dim3(256), 0, stream, b.stats, L.fwd_rows, L.C, L.Cpad,
                     (double)count, b.gamma, b.beta, BN_EPS, BN_MOMENTUM, b.running_mean, b.running_var,
                     bn_coef(b.coef, L.C, BN_MEAN), bn_coef(b.coef, L.C, BN_INVSTD), bn_coef(b.coef, L.C, BN_SCALE),
                     bn_coef(b.coef, L.C, BN_SHIFT), nv);
  D3F_HIP(hipGetLastError());
  return 0;
}

int bn_layer_apply(const BnLayer& L, const BnBufs& b, hipStream_t stream, const NetSplit* ns) {
  const int ve = L.dtype == D3F_F32 ? 4 : 8;
  D3F_CHECK(L.C % ve == 0 && (256 * ve) % L.C == 0, "bn_apply: C=%d must divide %d", L.C, 256 * ve);
  const long nvec = L.rows * L.C / ve;
  if (nvec == 0) return 0;
  const NetSplit nv = net_split_or_single(ns);
  const BnResidualOps r = residual_ops(L, b);
  by_dtype(L.dtype, [&](auto* typed) {
    typedef std::remove_pointer_t<decltype(typed)> T;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid_for(nvec), 1, nv.nets), dim3(256), 0, stream, (const T*)b.y,
                         bn_coef(b.coef, L.C, BN_SCALE), bn_coef(b.coef, L.C, BN_SHIFT), (const T*)r.res, (const T*)r.yr,
                         r.scale_r, r.shift_r, L.relu ? 1 : 0, (T*)b.a, nvec, L.C, nv.ws);
    };
    if (r.res != nullptr) go(bn_apply_kernel<T, 1>);  // (the order the kernel used to test the two pointers in)
    else if (r.yr != nullptr) go(bn_apply_kernel<T, 2>);
    else go(bn_apply_kernel<T, 0>);
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

int bn_layer_forward(const BnLayer& L, const BnBufs& b, const BnSync* sync, hipStream_t stream, const NetSplit* ns) {
  long count = L.rows;
  if (sync != nullptr) {  // statistics over every rank's batch: the partial rows are summed across ranks in place
    if (int rc = sync->fn(sync->ctx, b.stats, (int64_t)L.fwd_rows * L.Cpad * 2, (void*)stream))
      return set_error(rc, "BatchNorm statistics all-reduce failed in the forward pass (%s)", L.name.c_str());
    count *= sync->world;
  } else if (L.fwd_fused) {
    return bn_finalize_apply_launch(L, b, stream, ns);
  }
  if (int rc = bn_layer_finalize(L, b, count, stream, ns)) return rc;
  return L.apply ? bn_layer_apply(L, b, stream, ns) : 0;
}

int bn_layer_backward(const BnLayer& L, const BnBufs& b, const BnSync* sync, hipStream_t stream, const NetSplit* ns) {
  const int C = L.C, ve = L.dtype == D3F_F32 ? 4 : 8, vc = C / ve;
  const NetSplit nv = net_split_or_single(ns);
  const BnBwdOps o = bwd_ops(L, b);
  if (L.fused_rows == 0) {  // (else the producing data gradient already left the partial sums in b.stats)
    D3F_CHECK(C % ve == 0 && vc >= 1 && vc <= 256 && (256 % vc) == 0, "bn_bwd_reduce: unsupported channel count %d", C);
    by_dtype(L.dtype, [&](auto* typed) {
      typedef std::remove_pointer_t<decltype(typed)> T;
      hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(L.reduce_blocks, 1, nv.nets), dim3(256), 0, stream,
                         (const T*)b.dA, (const T*)o.a, (const T*)b.y, o.mean, o.invstd, b.stats, L.rows, C, o.mask_scale,
                         o.mask_shift, nv.ws);
    });
    D3F_HIP(hipGetLastError());
  }
  auto finalize = [&](long count, float* dgamma, float* dbeta) -> int {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C, 1, nv.nets), dim3(256), 0, stream, b.stats, L.bwd_rows, C,
                       (double)count, b.gamma, o.invstd, dgamma, dbeta, o.k, nv);
    D3F_HIP(hipGetLastError());
    return 0;
  };
  if (sync != nullptr) {
    // synchronised statistics: dgamma / dbeta from the LOCAL sums (they are summed over ranks with the other
    // gradients), the coefficients of dy from the sums over every rank's batch
    if (int rc = finalize(L.rows, b.dgamma, b.dbeta)) return rc;
    if (int rc = sync->fn(sync->ctx, b.stats, (int64_t)L.bwd_rows * C * 2, (void*)stream))
      return set_error(rc, "BatchNorm statistics all-reduce failed in the backward pass (%s)", L.name.c_str());
    if (int rc = finalize(L.rows * sync->world, nullptr, nullptr)) return rc;
  } else if (L.bwd_fused) {
    return bn_bwd_finalize_apply_launch(L, b, o, stream, ns);
  } else if (int rc = finalize(L.rows, b.dgamma, b.dbeta)) {
    return rc;
  }
  D3F_CHECK(C % ve == 0 && (256 * ve) % C == 0, "bn_bwd_apply: C=%d must divide %d", C, 256 * ve);
  const long nvec = L.rows * C / ve;
  if (nvec == 0) return 0;
  by_dtype(L.dtype, [&](auto* typed) {
    typedef std::remove_pointer_t<decltype(typed)> T;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid_for(nvec), 1, nv.nets), dim3(256), 0, stream, (const T*)b.dA, (const T*)o.a,
                         (const T*)b.y, o.mean, o.invstd, o.k, (T*)b.dy, (T*)b.dres, nvec, C, o.mask_scale, o.mask_shift,
                         nv.ws);
    };
    const int mask = o.mask_scale != nullptr ? 1 : (o.a != nullptr ? 2 : 0);
    const int dres = b.dres == nullptr ? 0 : (b.dres_acc ? 2 : 1);
    auto by_dres = [&](auto m) {
      constexpr int M = decltype(m)::value;
      if (dres == 0) go(bn_bwd_apply_kernel<T, M, 0>);
      else if (dres == 1) go(bn_bwd_apply_kernel<T, M, 1>);
      else go(bn_bwd_apply_kernel<T, M, 2>);
    };
    if (mask == 0) by_dres(std::integral_constant<int, 0>());
    else if (mask == 1) by_dres(std::integral_constant<int, 1>());
    else by_dres(std::integral_constant<int, 2>());
  });
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
