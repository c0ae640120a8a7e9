// Temporal filter of the fake video (include/d3f_hip.h: d3f_temporal_filter_u8): a motion-gated recursive filter on the fake's
// bytes.  The gate is the 3 x 3 sum of absolute differences of the REAL crop against its predecessor (the fake changing where
// its input stood still is the flicker; where the input moved it is the signal), the state is fp32, and every operation is
// fixed, so tests/temporal_restatement.py restates it bit for bit.
//
// temporal_filter_kernel: one workgroup per TF_TW x TF_TH tile of pixels, one lane per pixel, and the loop over the frames of
// the call INSIDE the kernel: a lane's three S values stay in registers from frame to frame, state_fake is read and written
// once per call, state_real read once (written by the launch behind, below).  Per frame
//   - the tile of the real frame with its one-pixel halo (clipped to the image: the replicated border is a clamp of the
//     coordinates at read time) and the tile of the fake are staged in LDS as the aligned dwords that cover each row's bytes,
//     as resize_stage does (byte k of a row sits at its dword alignment + k; a dword is loaded whole only inside the
//     buffer's own bytes).  The real tile stays in LDS as the next frame's predecessor (two buffers, swapped), so each real
//     byte comes from memory once per frame;
//   - the loads of frame b + 1 are issued, into registers, before the arithmetic of frame b;
//   - the per-pixel sum of the three absolute differences goes through LDS once (340 halo pixels), each lane adds its nine;
//   - the lane filters its three bytes in LDS, and the tile goes back as whole dwords where a dword lies inside the tile's
//     row, as bytes at the ragged ends (those dwords are shared with the neighbouring tile's workgroup).
// state_valid is read by every workgroup and written by none, and a workgroup reads its halo of state_real from its
// neighbours' tiles: the launch function enqueues temporal_state_kernel behind this one, which copies the call's last real
// frame into state_real and sets the flag.
#include "../../include/d3f_hip.h"
#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int TF_TW = 32, TF_TH = 8, TF_THREADS = TF_TW * TF_TH;
constexpr int TF_HW = TF_TW + 2, TF_HH = TF_TH + 2;  // the tile with its halo
constexpr int TF_RDW = (TF_HW * 3 + 3 + 3) / 4;      // dwords of a staged real row: 102 bytes and up to 3 of alignment
constexpr int TF_FDW = (TF_TW * 3 + 3 + 3) / 4;      // dwords of a staged fake row: 96 bytes and up to 3 of alignment
constexpr int TF_RITEMS = TF_HH * TF_RDW, TF_FITEMS = TF_TH * TF_FDW;
static_assert(TF_RITEMS <= 2 * TF_THREADS && TF_FITEMS <= TF_THREADS && TF_HW * TF_HH <= 2 * TF_THREADS,
              "a lane stages two real dwords, one fake dword and two halo pixels");

struct TemporalGeom {
  int B, H, W;
  long rstride, fstride;  // bytes between rows of real and of fake
  int T;                  // 27 * threshold
  float strength;
};

__device__ __forceinline__ int tf_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// dword k of the aligned dwords that cover the seg_bytes bytes at seg; whole only inside [lo, hi), 0 past the segment
__device__ __forceinline__ uint32_t tf_load_dword(const uint8_t* seg, int seg_bytes, int k, const uint8_t* lo,
                                                  const uint8_t* hi) {
  const int al = (int)(reinterpret_cast<uintptr_t>(seg) & 3);
  if (4 * k >= al + seg_bytes) return 0;
  const uint8_t* p = seg - al + 4 * k;
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (p + j >= lo && p + j < hi) v |= (uint32_t)p[j] << (8 * j);
  return v;
}

// dword k of the aligned dwords that cover the seg_bytes bytes at seg, from LDS bytes src (src[t] is byte t of the segment):
// a whole dword where all four bytes belong to the segment, single bytes otherwise
__device__ __forceinline__ void tf_store_dword(uint8_t* seg, int seg_bytes, int k, const uint8_t* src) {
  const int al = (int)(reinterpret_cast<uintptr_t>(seg) & 3);
  const int t0 = 4 * k - al;
  if (t0 >= seg_bytes) return;
  if (t0 >= 0 && t0 + 4 <= seg_bytes) {
    const uint32_t v = (uint32_t)src[t0] | (uint32_t)src[t0 + 1] << 8 | (uint32_t)src[t0 + 2] << 16 | (uint32_t)src[t0 + 3] << 24;
    *reinterpret_cast<uint32_t*>(seg + t0) = v;
    return;
  }
  for (int j = 0; j < 4; ++j)
    if (t0 + j >= 0 && t0 + j < seg_bytes) seg[t0 + j] = src[t0 + j];
}

// the part of an image a tile's real buffer holds, and where: rows ry0 .. ry0 + rows - 1, columns from cx0, row_bytes bytes of
// each; row cy of an image whose first pixel is at img, rows `stride` apart, lies at staged row cy - ry0 behind its alignment
struct TfHalo {
  int ry0, cx0, rows, row_bytes;
};

__device__ __forceinline__ const uint8_t* tf_staged_row(const uint8_t* buf, const TfHalo& h, const uint8_t* img, long stride,
                                                        int cy) {
  const uint8_t* seg = img + (long)cy * stride + 3L * h.cx0;
  return buf + (cy - h.ry0) * (TF_RDW * 4) + (reinterpret_cast<uintptr_t>(seg) & 3);
}

__global__ __launch_bounds__(TF_THREADS) void temporal_filter_kernel(const uint8_t* real, uint8_t* fake,
                                                                     TemporalGeom g, float* __restrict__ state_fake,
                                                                     const uint8_t* __restrict__ state_real,
                                                                     const int* __restrict__ state_valid) {
  __shared__ uint32_t lds_r[2][TF_RITEMS];
  __shared__ uint32_t lds_f[2][TF_FITEMS];
  __shared__ uint32_t sadpix[TF_HW * TF_HH];
  const int tid = threadIdx.x, lx = tid % TF_TW, ly = tid / TF_TW;
  const int x0 = blockIdx.x * TF_TW, y0 = blockIdx.y * TF_TH, x = x0 + lx, y = y0 + ly;
  const int tw = min(TF_TW, g.W - x0), th = min(TF_TH, g.H - y0);
  const bool active = lx < tw && ly < th;
  TfHalo h;
  h.ry0 = max(y0 - 1, 0), h.cx0 = max(x0 - 1, 0);
  h.rows = min(y0 + TF_TH, g.H - 1) - h.ry0 + 1;
  h.row_bytes = (min(x0 + TF_TW, g.W - 1) - h.cx0 + 1) * 3;
  // the bytes a dword may be loaded whole from: first pixel of the first frame to last pixel of the last
  const uint8_t* r_lo = real;
  const uint8_t* r_hi = real + ((long)g.B * g.H - 1) * g.rstride + 3L * g.W;
  const uint8_t* f_lo = fake;
  const uint8_t* f_hi = fake + ((long)g.B * g.H - 1) * g.fstride + 3L * g.W;
  // what this lane stages: real items tid and tid + TF_THREADS, fake item tid
  const int rr0 = tid / TF_RDW, rk0 = tid % TF_RDW;
  const int rr1 = (tid + TF_THREADS) / TF_RDW, rk1 = (tid + TF_THREADS) % TF_RDW;
  const bool has_r0 = rr0 < h.rows, has_r1 = tid + TF_THREADS < TF_RITEMS && rr1 < h.rows;
  const int fr = tid / TF_FDW, fk = tid % TF_FDW;
  const bool has_f = tid < TF_FITEMS && fr < th;

  bool have_prev = *state_valid != 0;
  const uint8_t* prev_img = state_real;  // the image lds_r[cur ^ 1] was staged from
  long prev_stride = 3L * g.W;
  float S[3] = {0.f, 0.f, 0.f};
  int cur = 0;
  if (have_prev) {  // the state: the real tile as frame 0's predecessor, and the lane's S
    const uint8_t* s_hi = state_real + (long)g.H * prev_stride;
    if (has_r0)
      lds_r[1][tid] = tf_load_dword(state_real + (long)(h.ry0 + rr0) * prev_stride + 3L * h.cx0, h.row_bytes, rk0, state_real,
                                    s_hi);
    if (has_r1)
      lds_r[1][tid + TF_THREADS] =
          tf_load_dword(state_real + (long)(h.ry0 + rr1) * prev_stride + 3L * h.cx0, h.row_bytes, rk1, state_real, s_hi);
    if (active)
      for (int c = 0; c < 3; ++c) S[c] = state_fake[((long)y * g.W + x) * 3 + c];
  }
  uint32_t vr0 = 0, vr1 = 0, vf = 0;
  {
    if (has_r0) vr0 = tf_load_dword(real + (long)(h.ry0 + rr0) * g.rstride + 3L * h.cx0, h.row_bytes, rk0, r_lo, r_hi);
    if (has_r1) vr1 = tf_load_dword(real + (long)(h.ry0 + rr1) * g.rstride + 3L * h.cx0, h.row_bytes, rk1, r_lo, r_hi);
    if (has_f) vf = tf_load_dword(fake + (long)(y0 + fr) * g.fstride + 3L * x0, tw * 3, fk, f_lo, f_hi);
  }
  for (int b = 0; b < g.B; ++b) {
    const uint8_t* rimg = real + (long)b * g.H * g.rstride;
    uint8_t* fimg = fake + (long)b * g.H * g.fstride;
    uint8_t* fbuf = reinterpret_cast<uint8_t*>(lds_f[b & 1]);
    if (has_r0) lds_r[cur][tid] = vr0;
    if (has_r1) lds_r[cur][tid + TF_THREADS] = vr1;
    if (has_f) lds_f[b & 1][tid] = vf;
    __syncthreads();
    if (b + 1 < g.B) {  // the next frame's loads, in flight during this frame's arithmetic
      const uint8_t* rn = rimg + (long)g.H * g.rstride;
      const uint8_t* fn = fimg + (long)g.H * g.fstride;
      if (has_r0) vr0 = tf_load_dword(rn + (long)(h.ry0 + rr0) * g.rstride + 3L * h.cx0, h.row_bytes, rk0, r_lo, r_hi);
      if (has_r1) vr1 = tf_load_dword(rn + (long)(h.ry0 + rr1) * g.rstride + 3L * h.cx0, h.row_bytes, rk1, r_lo, r_hi);
      if (has_f) vf = tf_load_dword(fn + (long)(y0 + fr) * g.fstride + 3L * x0, tw * 3, fk, f_lo, f_hi);
    }
    if (have_prev) {  // |r - r_prev| summed over a pixel's three bytes, for every pixel of the tile and its halo
      const uint8_t* cbuf = reinterpret_cast<const uint8_t*>(lds_r[cur]);
      const uint8_t* pbuf = reinterpret_cast<const uint8_t*>(lds_r[cur ^ 1]);
      for (int i = tid; i < TF_HW * TF_HH; i += TF_THREADS) {
        const int hy = i / TF_HW, hx = i - hy * TF_HW;
        const int cy = tf_clamp(y0 - 1 + hy, 0, g.H - 1), cx = tf_clamp(x0 - 1 + hx, 0, g.W - 1);
        const uint8_t* pc = tf_staged_row(cbuf, h, rimg, g.rstride, cy) + 3 * (cx - h.cx0);
        const uint8_t* pp = tf_staged_row(pbuf, h, prev_img, prev_stride, cy) + 3 * (cx - h.cx0);
        int sad = 0;
        for (int c = 0; c < 3; ++c) sad += abs((int)pc[c] - (int)pp[c]);
        sadpix[i] = (uint32_t)sad;
      }
    }
    __syncthreads();
    if (active) {
      const uint8_t* fseg = fimg + (long)y * g.fstride + 3L * x0;
      uint8_t* fb = fbuf + ly * (TF_FDW * 4) + (reinterpret_cast<uintptr_t>(fseg) & 3) + 3 * lx;
      float k = 0.f;
      if (have_prev) {
        int sad = 0;
        for (int dy = 0; dy < 3; ++dy)
          for (int dx = 0; dx < 3; ++dx) sad += (int)sadpix[(ly + dy) * TF_HW + lx + dx];
        const float q = __fdiv_rn((float)max(g.T - sad, 0), (float)g.T);
        k = __fmul_rn(g.strength, q);
      }
      for (int c = 0; c < 3; ++c) {
        const float f = (float)fb[c];
        if (have_prev) {
          const float d = __fsub_rn(S[c], f);
          const float p = __fmul_rn(k, d);
          S[c] = __fadd_rn(f, p);
        } else {
          S[c] = f;
        }
        const float r = rintf(S[c]);
        fb[c] = (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
      }
    }
    __syncthreads();
    if (has_f) {
      uint8_t* fseg = fimg + (long)(y0 + fr) * g.fstride + 3L * x0;
      tf_store_dword(fseg, tw * 3, fk, fbuf + fr * (TF_FDW * 4) + (reinterpret_cast<uintptr_t>(fseg) & 3));
    }
    have_prev = true;
    prev_img = rimg;
    prev_stride = g.rstride;
    cur ^= 1;
  }
  // the state: the lane's S.  state_real is NOT written here: this workgroup read its halo from its neighbours' part of it,
  // and a neighbour may be through the whole call before this workgroup has started -- temporal_state_kernel, behind
  if (active)
    for (int c = 0; c < 3; ++c) state_fake[((long)y * g.W + x) * 3 + c] = S[c];
}

// Behind temporal_filter_kernel: state_real := the call's last real frame (rows `stride` apart -> packed) and *flag := 1.
// A lane takes one of the aligned dwords that cover state_real's n = 3 H W bytes: a whole dword store where all four bytes
// are the state's, single bytes at the two ends.
__global__ __launch_bounds__(256) void temporal_state_kernel(const uint8_t* __restrict__ last, long stride,
                                                             uint8_t* __restrict__ state_real, int W, int n,
                                                             int* __restrict__ flag) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) *flag = 1;
  const int al = (int)(reinterpret_cast<uintptr_t>(state_real) & 3);
  const int t0 = 4 * k - al;
  if (t0 >= n) return;
  const int row_bytes = 3 * W;
  uint32_t v = 0;
  uint8_t byte[4];
  for (int j = 0; j < 4; ++j) {
    const int t = t0 + j;
    byte[j] = 0;
    if (t >= 0 && t < n) {
      const int r = t / row_bytes;
      byte[j] = last[(long)r * stride + (t - r * row_bytes)];
    }
    v |= (uint32_t)byte[j] << (8 * j);
  }
  if (t0 >= 0 && t0 + 4 <= n) {
    *reinterpret_cast<uint32_t*>(state_real + t0) = v;
    return;
  }
  for (int j = 0; j < 4; ++j)
    if (t0 + j >= 0 && t0 + j < n) state_real[t0 + j] = byte[j];
}

__global__ __launch_bounds__(64) void flag_set_kernel(int* __restrict__ flag, int value) {
  if (threadIdx.x == 0) *flag = value;
}

int temporal_flag_set_launch(int* flag, int value, hipStream_t stream) {
  D3F_CHECK(flag != nullptr, "temporal flag: null argument");
  hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(64), 0, stream, flag, value);
  D3F_HIP(hipGetLastError());
  return 0;
}

namespace {
struct Span {
  const uint8_t* lo;
  const uint8_t* hi;
};
bool spans_meet(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }
}  // namespace

int temporal_filter_check(const uint8_t* real, const uint8_t* fake, int B, int H, int W, long real_stride, long fake_stride,
                          const float* state_fake, const uint8_t* state_real, const int* state_valid, float strength,
                          int threshold) {
  D3F_CHECK(B >= 0 && B <= 65535, "temporal_filter: B %d outside 0..65535 frames per call", B);
  D3F_CHECK(H > 0 && W > 0 && H <= 16384 && W <= 16384, "temporal_filter: size %d x %d outside 1..16384", H, W);
  D3F_CHECK(strength >= 0.f && strength < 1.f, "temporal_filter: strength %g outside [0, 1)", (double)strength);  // (NaN fails)
  D3F_CHECK(threshold >= 1 && threshold <= 255, "temporal_filter: threshold %d outside 1..255", threshold);
  D3F_CHECK(real_stride >= 3L * W && fake_stride >= 3L * W, "temporal_filter: row stride (%ld, %ld) below 3 * W = %ld bytes",
            real_stride, fake_stride, 3L * W);
  D3F_CHECK((reinterpret_cast<uintptr_t>(state_fake) & 3) == 0 && (reinterpret_cast<uintptr_t>(state_valid) & 3) == 0,
            "temporal_filter: state_fake and state_valid must be aligned to 4 bytes");
  const long frames = B > 0 ? B : 1;
  const Span r = {real, real + (frames * H - 1) * real_stride + 3L * W};
  const Span f = {fake, fake + (frames * H - 1) * fake_stride + 3L * W};
  const Span sf = {reinterpret_cast<const uint8_t*>(state_fake), reinterpret_cast<const uint8_t*>(state_fake) + 12L * H * W};
  const Span sr = {state_real, state_real + 3L * H * W};
  const Span sv = {reinterpret_cast<const uint8_t*>(state_valid), reinterpret_cast<const uint8_t*>(state_valid) + 4};
  // real and fake may be interleaved row by row (the halves of a pair buffer): one stride, and the fake's rows inside the
  // gap the real's rows leave
  if (spans_meet(r, f)) {
    bool apart = false;
    if (real_stride == fake_stride) {
      long d = (long)(fake - real) % real_stride;
      if (d < 0) d += real_stride;
      apart = d >= 3L * W && d + 3L * W <= real_stride;
    }
    D3F_CHECK(apart, "temporal_filter: real and fake overlap");
  }
  const Span state[3] = {sf, sr, sv};
  for (int i = 0; i < 3; ++i) {
    D3F_CHECK(!spans_meet(state[i], r) && !spans_meet(state[i], f), "temporal_filter: a state buffer overlaps real or fake");
    for (int j = i + 1; j < 3; ++j) D3F_CHECK(!spans_meet(state[i], state[j]), "temporal_filter: the state buffers overlap");
  }
  return 0;
}

int temporal_filter_u8_launch(const uint8_t* real, uint8_t* fake, int B, int H, int W, long real_stride, long fake_stride,
                              float* state_fake, uint8_t* state_real, int* state_valid, float strength, int threshold,
                              hipStream_t stream) {
  if (int rc = temporal_filter_check(real, fake, B, H, W, real_stride, fake_stride, state_fake, state_real, state_valid,
                                     strength, threshold))
    return rc;
  if (B == 0) return 0;
  const TemporalGeom g = {B, H, W, real_stride, fake_stride, 27 * threshold, strength};
  hipLaunchKernelGGL(temporal_filter_kernel, dim3((W + TF_TW - 1) / TF_TW, (H + TF_TH - 1) / TF_TH), dim3(TF_THREADS), 0,
                     stream, real, fake, g, state_fake, state_real, state_valid);
  D3F_HIP(hipGetLastError());
  // behind the kernel on the stream, never from inside it: its other workgroups may not have read the flag, or their halo
  // of state_real, yet
  const int n = 3 * H * W;  // at most 3 * 2^28
  const int dwords = (int)(((reinterpret_cast<uintptr_t>(state_real) & 3) + n + 3) / 4);
  hipLaunchKernelGGL(temporal_state_kernel, dim3((dwords + 255) / 256), dim3(256), 0, stream,
                     real + ((long)B * H - H) * real_stride, real_stride, state_real, W, n, state_valid);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
