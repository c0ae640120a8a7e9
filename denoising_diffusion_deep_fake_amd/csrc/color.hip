// Colour match of the full-frame output (include/d3f_hip.h: d3f_channel_sums_u8, d3f_color_match_coef; the colour form of the
// paste kernel is in resize.hip): mean / std (Reinhard) matching of the fake to the resized real crop, per frame and per
// byte-in-pixel.  Both images are bytes, so the statistics are integer sums -- exact, and the same in any order of addition;
// tests/color_match_restatement.py restates them with Python integers and the coefficients in float64.
//
// channel_sums_kernel: S = sum p and Q = sum p^2 of the three bytes-in-pixel of [H][W][3] images whose rows lie `stride` bytes
// apart, from any byte address.  A row is read as the aligned 12-byte groups that cover its 3 W bytes (three dwords: four
// pixels, so a group's byte t has channel (t - al) mod 3 with al the row's offset past a dword -- one rotation per group and
// no division per byte); a group's bytes outside the row are masked, and a group that would reach outside the images' bytes
// is read byte by byte.  A workgroup takes `rpw` whole rows of one image, a lane SUMS_UNROLL groups at a time so that their
// loads are in flight together: lanes accumulate in 32 bits (at most 65 536 pixels
// a lane, below the 66 051 that p^2 <= 65 025 allows), widen, reduce across the wave with shuffles and across the four
// waves through LDS, and lanes 0..5 of the workgroup either add the six values to the image's sums with one 64-bit vector
// atomic each (the operator: a launch in front has zeroed them) or store them as the workgroup's row of a slab that
// color_match_coef_kernel adds up in a fixed order (the engine: both halves of pair_out in one launch, nothing to reset).
#include "../../include/d3f_hip.h"
#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int SUMS_THREADS = 256;
constexpr int SUMS_UNROLL = 4;       // groups a lane has in flight
constexpr int SUMS_MIN_ITEMS = 512;  // 12-byte groups a workgroup takes at least (a small image gets fewer workgroups)
constexpr double COLOR_GAIN_MIN = D3F_COLOR_GAIN_MIN, COLOR_GAIN_MAX = D3F_COLOR_GAIN_MAX;

typedef unsigned long long u64;

struct SumsGeom {
  int B, H, W;
  long stride;     // bytes between rows
  long img_delta;  // bytes from image set 0 to image set 1 (blockIdx.z)
  int gpr;         // 12-byte groups per row: ceil((3 W + 3) / 12), the 3 for a row that starts 3 bytes past a dword
  int rpw;         // rows per workgroup
  int slabs;       // != 0: store the workgroup's sums as row blockIdx.x of its image's slab; 0: atomic adds
};

__global__ __launch_bounds__(64) void sums_zero_kernel(u64* __restrict__ sums, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) sums[i] = 0;
}

__global__ __launch_bounds__(SUMS_THREADS) void channel_sums_kernel(const uint8_t* __restrict__ img, SumsGeom g,
                                                                    u64* __restrict__ out) {
  const int tid = threadIdx.x, wg = blockIdx.x, b = blockIdx.y, im = blockIdx.z;
  const uint8_t* base = img + (long)im * g.img_delta;
  // a dword is loaded whole only inside the bytes from the first image's first pixel to the last one's last
  const uint8_t* lo = base;
  const uint8_t* hi = base + ((long)g.B * g.H - 1) * g.stride + 3L * g.W;
  const int r0 = wg * g.rpw, rows = min(g.rpw, g.H - r0), n3 = 3 * g.W;
  uint32_t S[3] = {0, 0, 0}, Q[3] = {0, 0, 0};
  const int items = rows * g.gpr;
  for (int i0 = tid; i0 < items; i0 += SUMS_UNROLL * SUMS_THREADS) {
    uint32_t d[SUMS_UNROLL][3];
    int al[SUMS_UNROLL], k0[SUMS_UNROLL];
    // the loads of SUMS_UNROLL groups first, so that they are in flight together
#pragma unroll
    for (int u = 0; u < SUMS_UNROLL; ++u) {
      const int i = i0 + u * SUMS_THREADS;
      d[u][0] = d[u][1] = d[u][2] = 0;
      al[u] = 0;
      k0[u] = n3;  // nothing of the row
      if (i >= items) continue;
      const int r = i / g.gpr, k = i - r * g.gpr;
      const uint8_t* row = base + ((long)b * g.H + r0 + r) * g.stride;
      al[u] = (int)(reinterpret_cast<uintptr_t>(row) & 3);
      k0[u] = 12 * k - al[u];  // the group's first byte, as an offset into the row
      if (k0[u] >= n3) continue;
      const uint8_t* p = row + k0[u];  // dword aligned
      if (p >= lo && p + 12 <= hi) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        d[u][0] = q[0];
        d[u][1] = q[1];
        d[u][2] = q[2];
      } else {
        for (int w = 0; w < 3; ++w)
          for (int j = 0; j < 4; ++j) {
            const uint8_t* a = p + 4 * w + j;
            if (a >= lo && a < hi) d[u][w] |= (uint32_t)*a << (8 * j);
          }
      }
    }
#pragma unroll
    for (int u = 0; u < SUMS_UNROLL; ++u) {
      if (k0[u] >= n3) continue;
      if (k0[u] < 0 || k0[u] + 12 > n3) {  // a group over an end of the row: its bytes outside the row count as 0
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          uint32_t m = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int kk = k0[u] + 4 * w + j;
            if (kk >= 0 && kk < n3) m |= 0xffu << (8 * j);
          }
          d[u][w] &= m;
        }
      }
      uint32_t ps[3] = {0, 0, 0}, pq[3] = {0, 0, 0};  // by t mod 3
#pragma unroll
      for (int t = 0; t < 12; ++t) {
        const uint32_t v = (d[u][t >> 2] >> (8 * (t & 3))) & 255u;
        ps[t % 3] += v;
        pq[t % 3] += v * v;
      }
      // byte t of the group is byte k0 + t of the row: channel (t - al) mod 3, so channel c is phase (c + al) mod 3
      if (al[u] == 0 || al[u] == 3) {
        S[0] += ps[0], S[1] += ps[1], S[2] += ps[2];
        Q[0] += pq[0], Q[1] += pq[1], Q[2] += pq[2];
      } else if (al[u] == 1) {
        S[0] += ps[1], S[1] += ps[2], S[2] += ps[0];
        Q[0] += pq[1], Q[1] += pq[2], Q[2] += pq[0];
      } else {
        S[0] += ps[2], S[1] += ps[0], S[2] += ps[1];
        Q[0] += pq[2], Q[1] += pq[0], Q[2] += pq[1];
      }
    }
  }
  u64 v[6] = {S[0], Q[0], S[1], Q[1], S[2], Q[2]};  // the layout of sums: [3][2]
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += __shfl_down(v[k], off, 64);
  __shared__ u64 red[SUMS_THREADS / 64][6];
  if ((tid & 63) == 0)
    for (int k = 0; k < 6; ++k) red[tid >> 6][k] = v[k];
  __syncthreads();
  if (tid < 6) {
    u64 t = 0;
    for (int w = 0; w < SUMS_THREADS / 64; ++w) t += red[w][tid];
    const long image = (long)im * g.B + b;
    if (g.slabs)
      out[(image * gridDim.x + wg) * 6 + tid] = t;
    else
      atomicAdd(out + image * 6 + tid, t);
  }
}

// One wave per frame.  from / to: [B][parts][3][2]; the lanes add the frame's rows (parts == 1: the sums themselves; integer
// sums, the same in any order) and the wave's totals go through LDS to lanes 0..2, one per byte-in-pixel.  float64 from
// there on, product and difference rounded separately (-ffp-contract=off).
__global__ __launch_bounds__(64) void color_match_coef_kernel(const u64* __restrict__ from, const u64* __restrict__ to,
                                                              int parts, u64 n, float* __restrict__ coef) {
  const int b = blockIdx.x, lane = threadIdx.x;
  u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // from [3][2], then to [3][2]
  for (int p = lane; p < parts; p += 64) {
    const long at = ((long)b * parts + p) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += from[at + k], s[6 + k] += to[at + k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] += __shfl_down(s[k], off, 64);
  __shared__ u64 total[12];
  if (lane == 0)
    for (int k = 0; k < 12; ++k) total[k] = s[k];
  __syncthreads();
  if (lane >= 3) return;
  const int c = lane;
  const u64 s_from = total[2 * c], q_from = total[2 * c + 1], s_to = total[6 + 2 * c], q_to = total[6 + 2 * c + 1];
  const u64 d_from = n * q_from - s_from * s_from, d_to = n * q_to - s_to * s_to;  // below 2^60 for n <= 2^22: exact
  const double m_from = (double)s_from / (double)n, m_to = (double)s_to / (double)n;
  double gain = 1.0;
  if (d_from != 0 && d_to != 0) gain = sqrt((double)d_to / (double)d_from);
  gain = fmin(fmax(gain, COLOR_GAIN_MIN), COLOR_GAIN_MAX);
  const double scaled = gain * m_from;
  const double offset = m_to - scaled;
  coef[((long)b * 3 + c) * 2] = (float)gain;
  coef[((long)b * 3 + c) * 2 + 1] = (float)offset;
}

// Temporal smoothing of the coefficients (include/d3f_hip.h: d3f_color_coef_smooth).  One wave for the whole batch, the
// frames in order: the lanes add a frame's rows of `to` sums (parts == 1: the sums themselves) with shuffles, every lane
// then holds the three S and decides the cut in exact 64-bit integers, and lanes 0..5 carry one coefficient each from
// frame to frame in a register.  valid is read here and set by the launch function's flag launch behind this one.
__global__ __launch_bounds__(64) void color_coef_smooth_kernel(float* __restrict__ coef, const u64* __restrict__ to, int parts,
                                                               int B, u64 n, float strength, float* __restrict__ state_coef,
                                                               u64* __restrict__ state_sum, const int* __restrict__ valid) {
  const int lane = threadIdx.x;
  bool have_prev = *valid != 0;
  u64 sp[3] = {0, 0, 0};
  float cp = 0.f;
  if (have_prev) {
    for (int c = 0; c < 3; ++c) sp[c] = state_sum[c];
    if (lane < 6) cp = state_coef[lane];
  }
  const u64 limit = (u64)D3F_TEMPORAL_CUT_LEVELS * n;
  for (int b = 0; b < B; ++b) {
    u64 s[3] = {0, 0, 0};
    for (int p = lane; p < parts; p += 64)
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += to[(((long)b * parts + p) * 3 + c) * 2];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += __shfl_xor(s[c], off, 64);
    bool cut = !have_prev;
    if (have_prev)
      for (int c = 0; c < 3; ++c) {
        const u64 d = s[c] > sp[c] ? s[c] - sp[c] : sp[c] - s[c];
        if (d > limit) cut = true;
      }
    if (lane < 6) {
      const float cn = coef[(long)b * 6 + lane];
      float v = cn;
      if (!cut) {  // c' + a * (c_prev - c'), three roundings; at a cut c' itself, and the state is not read
        const float d = __fsub_rn(cp, cn);
        const float q = __fmul_rn(strength, d);
        v = __fadd_rn(cn, q);
      }
      coef[(long)b * 6 + lane] = v;
      cp = v;
    }
    for (int c = 0; c < 3; ++c) sp[c] = s[c];
    have_prev = true;
  }
  if (lane < 6) state_coef[lane] = cp;
  if (lane < 3) state_sum[lane] = sp[lane];
}

int color_coef_smooth_launch(float* coef, const uint64_t* sums_to, int parts, int B, long n, float strength, float* state_coef,
                             uint64_t* state_sum, int* state_valid, hipStream_t stream) {
  D3F_CHECK(B >= 0 && B <= 65535, "color_coef_smooth: B %d outside 0..65535 frames per call", B);
  D3F_CHECK(n > 0 && n <= COLOR_MAX_PIXELS, "color_coef_smooth: n %ld outside 1..%ld pixels per frame", n, COLOR_MAX_PIXELS);
  D3F_CHECK(parts >= 1 && parts <= COLOR_SUMS_MAX_PARTS, "color_coef_smooth: %d rows per frame", parts);
  D3F_CHECK(strength >= 0.f && strength < 1.f, "color_coef_smooth: strength %g outside [0, 1)", (double)strength);  // (NaN fails)
  if (B == 0) return 0;
  hipLaunchKernelGGL(color_coef_smooth_kernel, dim3(1), dim3(64), 0, stream, coef, reinterpret_cast<const u64*>(sums_to), parts,
                     B, (u64)n, strength, state_coef, reinterpret_cast<u64*>(state_sum), state_valid);
  D3F_HIP(hipGetLastError());
  // behind the kernel on the stream (temporal.hip)
  return temporal_flag_set_launch(state_valid, 1, stream);
}

int channel_sums_check(int B, int H, int W, long row_stride) {
  D3F_CHECK(B >= 0 && B <= 65535, "channel_sums: B %d outside 0..65535 frames per call", B);
  D3F_CHECK(H > 0 && W > 0, "channel_sums: non-positive size (%d x %d)", H, W);
  D3F_CHECK((long)H * W <= COLOR_MAX_PIXELS, "channel_sums: %d x %d is above %ld pixels per frame (64-bit n * Q and S * S)",
            H, W, COLOR_MAX_PIXELS);
  D3F_CHECK(row_stride >= 3L * W, "channel_sums: row stride %ld below 3 * W = %ld bytes", row_stride, 3L * W);
  return 0;
}

// Rows per workgroup and, returned, workgroups per image: at most COLOR_SUMS_MAX_PARTS of them, each with SUMS_MIN_ITEMS
// groups or more.  For what channel_sums_check lets through (H W <= 2^22) a workgroup's rpw * gpr groups stay far below the
// 16384 * SUMS_THREADS = 2^22 at which a lane (at most four pixels a group) could pass 65 536 pixels: gpr <= W / 4 + 2, so
// H gpr <= 2^20 + 2 H <= 2^20 + 2^23 and gpr <= 2^20 + 2; rpw * gpr <= max(H gpr / 64 + gpr, SUMS_MIN_ITEMS + gpr)
// <= 2^14 + 2^17 + 2^20 + 2 < 2^21.
static int sums_geometry(SumsGeom& g, int B, int H, int W, long row_stride, long img_delta, int slabs) {
  const int gpr = (3 * W + 3 + 11) / 12;
  const int rpw = max((H + COLOR_SUMS_MAX_PARTS - 1) / COLOR_SUMS_MAX_PARTS, (SUMS_MIN_ITEMS + gpr - 1) / gpr);
  g = SumsGeom{B, H, W, row_stride, img_delta, gpr, rpw, slabs};
  return (H + rpw - 1) / rpw;
}

int channel_sums_u8_launch(const uint8_t* img, int B, int H, int W, long row_stride, uint64_t* sums, hipStream_t stream) {
  if (int rc = channel_sums_check(B, H, W, row_stride)) return rc;
  if (B == 0) return 0;
  SumsGeom g;
  const int parts = sums_geometry(g, B, H, W, row_stride, 0, 0);
  hipLaunchKernelGGL(sums_zero_kernel, dim3((B * 6 + 63) / 64), dim3(64), 0, stream, reinterpret_cast<u64*>(sums), B * 6);
  hipLaunchKernelGGL(channel_sums_kernel, dim3(parts, B, 1), dim3(SUMS_THREADS), 0, stream, img, g,
                     reinterpret_cast<u64*>(sums));
  D3F_HIP(hipGetLastError());
  return 0;
}

int channel_sums_pair_slabs_launch(const uint8_t* img, long img_delta, int B, int H, int W, long row_stride, uint64_t* slabs,
                                   int* parts_out, hipStream_t stream) {
  if (int rc = channel_sums_check(B, H, W, row_stride)) return rc;
  SumsGeom g;
  const int parts = sums_geometry(g, B, H, W, row_stride, img_delta, 1);
  *parts_out = parts;
  if (B == 0) return 0;
  hipLaunchKernelGGL(channel_sums_kernel, dim3(parts, B, 2), dim3(SUMS_THREADS), 0, stream, img, g,
                     reinterpret_cast<u64*>(slabs));
  D3F_HIP(hipGetLastError());
  return 0;
}

int color_match_coef_launch(const uint64_t* sums_from, const uint64_t* sums_to, int parts, int B, long n, float* coef,
                            hipStream_t stream) {
  D3F_CHECK(B >= 0 && B <= 65535, "color_match_coef: B %d outside 0..65535 frames per call", B);
  D3F_CHECK(n > 0 && n <= COLOR_MAX_PIXELS, "color_match_coef: n %ld outside 1..%ld pixels per frame", n, COLOR_MAX_PIXELS);
  D3F_CHECK(parts >= 1 && parts <= COLOR_SUMS_MAX_PARTS, "color_match_coef: %d rows per frame", parts);
  if (B == 0) return 0;
  hipLaunchKernelGGL(color_match_coef_kernel, dim3(B), dim3(64), 0, stream, reinterpret_cast<const u64*>(sums_from),
                     reinterpret_cast<const u64*>(sums_to), parts, (u64)n, coef);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
