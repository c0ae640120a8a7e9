// Frame path of script_tools (d3f/script_tools/put_video_through_fake_model.py:111-145,
// video_to_center_cropped_images.py:73-107): centre crop + cv2.resize(..., INTER_CUBIC) of uint8 BGR frames, on the
// device, optionally with the K16 normalisation (u8bgr_to_nhwc_kernel) of the resized frame fused in.
//
// Definition (the acceptance contract; tests/resize_restatement.py restates it in float64):
//   * source coordinate of output index d on an axis n_in -> n_out: f = (d + 0.5) * n_in / n_out - 0.5, s = floor(f),
//     t = f - s -- computed EXACTLY in integers: num = (2d + 1) * n_in - n_out, den = 2 * n_out, s = floor(num / den),
//     t = (float)(num - s * den) / (float)den (one fp32 division of two exactly represented integers).  f itself is
//     never formed in fp32: at 1080 -> 448 an fp32 coordinate moves thousands of bytes;
//   * taps s-1 .. s+2, indices clamped to [0, n_in - 1] INSIDE THE CROP (replicate border), no antialiasing;
//   * Keys weights with A = -0.75 evaluated at t+1, t, 1-t, 2-t;
//   * horizontal pass, then vertical pass, in fp32 without intermediate rounding (and without fma: -ffp-contract=off),
//     then rintf (half to even) and clamp to 0..255.
// OpenCV's own 8-bit path works with 11-bit fixed-point coefficients and can differ from this float definition by one
// level on some pixels: byte equality with OpenCV is not claimed (and cannot be checked without cv2).
//
// Form: one workgroup per 32 x 8 tile of output pixels, one lane per pixel.  The tile's source patch (its rows and
// columns inside the crop, 3-byte pixels) is staged in LDS with aligned dword loads -- a lane's 16 taps are 48 byte
// gathers that would otherwise each be a global transaction -- and both passes read from there.  A crop so much larger
// than the output that a tile's patch exceeds RESIZE_LDS_BYTES takes the same arithmetic with the taps read from global
// memory (STAGED = false).
#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int RESIZE_TW = 32, RESIZE_TH = 8;
constexpr int RESIZE_LDS_BYTES = 32 * 1024;
constexpr int RESIZE_MAX_EXTENT = 16384;  // (2d + 1) * n_in stays below 2^31

struct ResizeGeom {
  int src_h, src_w, x1, y1, cw, ch, H, W;
  long dst_row_stride;
  int pitch;  // bytes of one staged patch row (a multiple of 4)
};

// s = floor(f) and the four tap weights of output index d (n_in -> n_out)
__device__ __forceinline__ int cubic_taps(int d, int n_in, int n_out, float w[4]) {
  const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;
  int s = num / den, rem = num - s * den;
  if (rem < 0) {  // floor division
    rem += den;
    s -= 1;
  }
  const float t = (float)rem / (float)den;
  const float A = -0.75f;
  auto inner = [A](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };       // |x| <= 1
  auto outer = [A](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };  // 1 < |x| < 2
  w[0] = outer(t + 1.f);
  w[1] = inner(t);
  w[2] = inner(1.f - t);
  w[3] = outer(2.f - t);
  return s;
}

__device__ __forceinline__ int floor_src(int d, int n_in, int n_out) {
  const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;
  int s = num / den;
  if (num - s * den < 0) s -= 1;
  return s;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T, bool ACT, bool STAGED>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void crop_resize_cubic_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, T* __restrict__ act, ResizeGeom g, int Cpad, float m0,
    float m1, float m2, float s0, float s1, float s2) {
  extern __shared__ __attribute__((aligned(16))) uint8_t patch[];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * RESIZE_TW, oy0 = blockIdx.y * RESIZE_TH, b = blockIdx.z;
  const long frame_bytes = (long)g.src_h * g.src_w * 3;
  const uint8_t* frame = src + b * frame_bytes;
  // the crop's first pixel, and the patch of it this tile reads: rows [ry0, ry1], columns [cx0, cx1] of the crop
  const uint8_t* crop = frame + ((long)g.y1 * g.src_w + g.x1) * 3;
  const long src_pitch = (long)g.src_w * 3;
  int ry0 = 0, cx0 = 0;
  unsigned align0 = 0, align_step = 0;
  if (STAGED) {
    const int oxl = min(ox0 + RESIZE_TW, g.W) - 1, oyl = min(oy0 + RESIZE_TH, g.H) - 1;
    cx0 = max(floor_src(ox0, g.cw, g.W) - 1, 0);
    ry0 = max(floor_src(oy0, g.ch, g.H) - 1, 0);
    const int cx1 = min(floor_src(oxl, g.cw, g.W) + 2, g.cw - 1);
    const int ry1 = min(floor_src(oyl, g.ch, g.H) + 2, g.ch - 1);
    const int row_bytes = (cx1 - cx0 + 1) * 3, rows = ry1 - ry0 + 1, pitch_dw = g.pitch >> 2;
    // patch row r holds the aligned dwords that cover its bytes: byte k of the row sits at r * pitch + align_r + k
    const uint8_t* first = crop + (long)ry0 * src_pitch + (long)cx0 * 3;
    align0 = (unsigned)(reinterpret_cast<uintptr_t>(first) & 3);
    align_step = (unsigned)(src_pitch & 3);
    const uint8_t* lo = src;                                  // a dword is loaded whole only inside the batch's bytes
    const uint8_t* hi = src + (long)gridDim.z * frame_bytes;
    for (int i = tid; i < rows * pitch_dw; i += RESIZE_TW * RESIZE_TH) {
      const int r = i / pitch_dw, k = i - r * pitch_dw;
      const unsigned al = (align0 + (unsigned)r * align_step) & 3;
      if (k * 4 >= (int)al + row_bytes) continue;
      const uint8_t* p = first + (long)r * src_pitch - al + k * 4;
      uint32_t v;
      if (p >= lo && p + 4 <= hi) {
        v = *reinterpret_cast<const uint32_t*>(p);
      } else {
        v = 0;
        for (int j = 0; j < 4; ++j)
          if (p + j >= lo && p + j < hi) v |= (uint32_t)p[j] << (8 * j);
      }
      *reinterpret_cast<uint32_t*>(patch + (long)r * g.pitch + k * 4) = v;
    }
    __syncthreads();
  }
  const int ox = ox0 + (tid % RESIZE_TW), oy = oy0 + (tid / RESIZE_TW);
  if (ox >= g.W || oy >= g.H) return;
  float wx[4], wy[4];
  const int sx = cubic_taps(ox, g.cw, g.W, wx), sy = cubic_taps(oy, g.ch, g.H, wy);
  int col[4];
  for (int k = 0; k < 4; ++k) col[k] = (clampi(sx - 1 + k, 0, g.cw - 1) - cx0) * 3;
  float acc[3];
  float hrow[4][3];
  for (int r = 0; r < 4; ++r) {
    const int cy = clampi(sy - 1 + r, 0, g.ch - 1) - ry0;
    const uint8_t* row;
    if (STAGED)
      row = patch + (long)cy * g.pitch + ((align0 + (unsigned)cy * align_step) & 3);
    else
      row = crop + (long)cy * src_pitch;
    for (int c = 0; c < 3; ++c) {  // horizontal pass
      float h = wx[0] * (float)row[col[0] + c];
      h = h + wx[1] * (float)row[col[1] + c];
      h = h + wx[2] * (float)row[col[2] + c];
      h = h + wx[3] * (float)row[col[3] + c];
      hrow[r][c] = h;
    }
  }
  uint8_t px[3];
  for (int c = 0; c < 3; ++c) {  // vertical pass, rintf, clamp
    float v = wy[0] * hrow[0][c];
    v = v + wy[1] * hrow[1][c];
    v = v + wy[2] * hrow[2][c];
    v = v + wy[3] * hrow[3][c];
    acc[c] = rintf(v);
    px[c] = (uint8_t)(acc[c] < 0.f ? 0.f : (acc[c] > 255.f ? 255.f : acc[c]));
  }
  uint8_t* o = dst + ((long)b * g.H + oy) * g.dst_row_stride + (long)ox * 3;
  o[0] = px[0];
  o[1] = px[1];
  o[2] = px[2];
  if (ACT) {  // u8bgr_to_nhwc_kernel on the rounded byte, operation for operation
    const float r = ((float)px[2] - m0) / s0, gg = ((float)px[1] - m1) / s1, bb = ((float)px[0] - m2) / s2;
    T* a = act + (((long)b * g.H + oy) * g.W + ox) * Cpad;
    a[0] = from_f32<T>(r);
    a[1] = from_f32<T>(gg);
    a[2] = from_f32<T>(bb);
    for (int c = 3; c < Cpad; ++c) a[c] = from_f32<T>(0.f);
  }
}

template <typename T, bool ACT>
static int resize_launch(const uint8_t* src, uint8_t* dst, T* act, const ResizeGeom& g0, int B, int Cpad,
                         const float mean255[3], const float std255[3], hipStream_t stream) {
  ResizeGeom g = g0;
  // the largest patch a tile can need: floor(a + n r) - floor(a) <= floor(n r) + 1 source steps over n output steps,
  // plus the three taps around them, plus up to 3 bytes of dword alignment in front
  const long cols = (long)(RESIZE_TW - 1) * g.cw / g.W + 1 + 4, rows = (long)(RESIZE_TH - 1) * g.ch / g.H + 1 + 4;
  const long pitch = (cols * 3 + 3 + 3) / 4 * 4;
  const bool staged = rows * pitch <= RESIZE_LDS_BYTES;
  g.pitch = staged ? (int)pitch : 0;
  const dim3 grid((g.W + RESIZE_TW - 1) / RESIZE_TW, (g.H + RESIZE_TH - 1) / RESIZE_TH, B), block(RESIZE_TW * RESIZE_TH);
  const float z[3] = {0.f, 0.f, 0.f}, one[3] = {1.f, 1.f, 1.f};
  const float* m = mean255 ? mean255 : z;
  const float* s = std255 ? std255 : one;
  if (staged)
    hipLaunchKernelGGL((crop_resize_cubic_kernel<T, ACT, true>), grid, block, (size_t)(rows * pitch), stream, src, dst, act,
                       g, Cpad, m[0], m[1], m[2], s[0], s[1], s[2]);
  else
    hipLaunchKernelGGL((crop_resize_cubic_kernel<T, ACT, false>), grid, block, 0, stream, src, dst, act, g, Cpad, m[0],
                       m[1], m[2], s[0], s[1], s[2]);
  D3F_HIP(hipGetLastError());
  return 0;
}

static int resize_geometry(ResizeGeom& g, int B, int src_h, int src_w, int x1, int y1, int cw, int ch, int H, int W,
                           long dst_row_stride) {
  D3F_CHECK(B >= 0 && src_h > 0 && src_w > 0 && cw > 0 && ch > 0 && H > 0 && W > 0,
            "crop_resize_cubic: non-positive size (B %d, frame %dx%d, crop %dx%d, output %dx%d)", B, src_h, src_w, ch, cw,
            H, W);
  D3F_CHECK(x1 >= 0 && y1 >= 0 && (long)x1 + cw <= src_w && (long)y1 + ch <= src_h,
            "crop_resize_cubic: crop box (x1 %d, y1 %d, %d x %d) outside the %d x %d frame", x1, y1, cw, ch, src_w, src_h);
  D3F_CHECK(src_h <= RESIZE_MAX_EXTENT && src_w <= RESIZE_MAX_EXTENT && H <= RESIZE_MAX_EXTENT && W <= RESIZE_MAX_EXTENT,
            "crop_resize_cubic: extents up to %d (32-bit source coordinates)", RESIZE_MAX_EXTENT);
  D3F_CHECK(B <= 65535, "crop_resize_cubic: at most 65535 frames per call (B %d)", B);
  D3F_CHECK(dst_row_stride >= 3L * W, "crop_resize_cubic: output row stride %ld below 3 * W = %ld bytes", dst_row_stride,
            3L * W);
  g = ResizeGeom{src_h, src_w, x1, y1, cw, ch, H, W, dst_row_stride, 0};
  return 0;
}

int crop_resize_cubic_check(int B, int src_h, int src_w, int x1, int y1, int cw, int ch, int H, int W, long dst_row_stride) {
  ResizeGeom g;
  return resize_geometry(g, B, src_h, src_w, x1, y1, cw, ch, H, W, dst_row_stride);
}

int crop_resize_cubic_u8_launch(const uint8_t* src, int B, int src_h, int src_w, int x1, int y1, int cw, int ch,
                                uint8_t* dst, int H, int W, long dst_row_stride, hipStream_t stream) {
  ResizeGeom g;
  if (int rc = resize_geometry(g, B, src_h, src_w, x1, y1, cw, ch, H, W, dst_row_stride)) return rc;
  if (B == 0) return 0;
  return resize_launch<float, false>(src, dst, nullptr, g, B, 0, nullptr, nullptr, stream);
}

int crop_resize_cubic_u8_nhwc_launch(int dtype, const uint8_t* src, int B, int src_h, int src_w, int x1, int y1, int cw,
                                     int ch, uint8_t* dst, int H, int W, long dst_row_stride, void* act, int Cpad,
                                     const float mean255[3], const float std255[3], hipStream_t stream) {
  ResizeGeom g;
  if (int rc = resize_geometry(g, B, src_h, src_w, x1, y1, cw, ch, H, W, dst_row_stride)) return rc;
  D3F_CHECK(Cpad >= 3, "crop_resize_cubic: activation of %d channels", Cpad);
  if (B == 0) return 0;
  if (dtype == D3F_F32)
    return resize_launch<float, true>(src, dst, (float*)act, g, B, Cpad, mean255, std255, stream);
  return resize_launch<bf16_t, true>(src, dst, (bf16_t*)act, g, B, Cpad, mean255, std255, stream);
}

}  // namespace d3f
