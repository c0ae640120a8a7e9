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
//
// Staging and the two passes are device functions (resize_stage, resize_value): the paste kernel at the end of this file,
// the inverse of this operator, runs the same arithmetic on a patch instead of a crop.
//
// The multiband paste's first launch (multiband_diff_kernel, at the end) shares them too; its pyramid is multiband.hip.
//
// The antialiased form (d3f_crop_resize_cubic_aa_u8: Pillow's bicubic, whose window widens with the scale) has a kernel of
// its own behind the plain one.
//
// The rotated forms (the _rboxes_ operators: a box per frame, turned about its centre) are at the end of the file: kernels
// of their own around the same weights, 4 x 4 sum and epilogues.
#include <type_traits>

#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int RESIZE_TW = 32, RESIZE_TH = 8;
constexpr int RESIZE_LDS_BYTES = 32 * 1024;
constexpr int RESIZE_MAX_EXTENT = 16384;  // (2d + 1) * n_in stays below 2^31
constexpr int AA_MAX_RATIO = 32;          // the antialiased form: n_in <= 32 n_out per axis

struct ResizeGeom {
  int src_h, src_w, x1, y1, cw, ch, H, W;
  long dst_row_stride;
  int pitch;  // bytes of one staged patch row (a multiple of 4)
};

// the Keys weights (A = -0.75) of the taps s-1 .. s+2 at the fraction t = f - s
__device__ __forceinline__ void keys_weights(float t, float w[4]) {
  const float A = -0.75f;
  auto inner = [A](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };       // |x| <= 1
  auto outer = [A](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };  // 1 < |x| < 2
  w[0] = outer(t + 1.f);
  w[1] = inner(t);
  w[2] = inner(1.f - t);
  w[3] = outer(2.f - t);
}

// s = floor(f) and the four tap weights of output index d (n_in -> n_out)
__device__ __forceinline__ int cubic_taps(int d, int n_in, int n_out, float w[4]) {
  const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;
  int s = num / den, rem = num - s * den;
  if (rem < 0) {  // floor division
    rem += den;
    s -= 1;
  }
  keys_weights((float)rem / (float)den, w);
  return s;
}

__device__ __forceinline__ int floor_src(int d, int n_in, int n_out) {
  const int num = (2 * d + 1) * n_in - n_out, den = 2 * n_out;
  int s = num / den;
  if (num - s * den < 0) s -= 1;
  return s;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One resize n_h x n_w -> out_h x out_w of an image of 3-byte pixels: first pixel at img, rows src_pitch bytes apart.
// crop_resize_cubic_kernel reads the crop of a frame this way, paste_resize_cubic_kernel the whole patch.
struct ResizeSrc {
  const uint8_t* img;
  long src_pitch;
  int n_h, n_w, out_h, out_w;
  int pitch;  // bytes of one staged row (a multiple of 4)
};

// where a tile's staged part of the image sits in LDS: rows from ry0, columns from cx0, and the dword alignment of its
// rows (all zero when the taps are read from global memory)
struct ResizeTile {
  int ry0 = 0, cx0 = 0;
  unsigned align0 = 0, align_step = 0;
};

// stages columns [cx0, cx1] of rows [ry0, ry1] of the image (all inside it), with aligned dword loads; a dword is loaded
// whole only inside [lo, hi).  The caller synchronises the workgroup afterwards.
__device__ __forceinline__ ResizeTile resize_stage_rect(uint8_t* patch, const ResizeSrc& g, int cx0, int cx1, int ry0, int ry1,
                                                        const uint8_t* lo, const uint8_t* hi, int tid) {
  ResizeTile t;
  t.cx0 = cx0;
  t.ry0 = ry0;
  const int row_bytes = (cx1 - t.cx0 + 1) * 3, rows = ry1 - t.ry0 + 1, pitch_dw = g.pitch >> 2;
  // patch row r holds the aligned dwords that cover its bytes: byte k of the row sits at r * pitch + align_r + k
  const uint8_t* first = g.img + (long)t.ry0 * g.src_pitch + (long)t.cx0 * 3;
  t.align0 = (unsigned)(reinterpret_cast<uintptr_t>(first) & 3);
  t.align_step = (unsigned)(g.src_pitch & 3);
  for (int i = tid; i < rows * pitch_dw; i += RESIZE_TW * RESIZE_TH) {
    const int r = i / pitch_dw, k = i - r * pitch_dw;
    const unsigned al = (t.align0 + (unsigned)r * t.align_step) & 3;
    if (k * 4 >= (int)al + row_bytes) continue;
    const uint8_t* p = first + (long)r * g.src_pitch - al + k * 4;
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
  return t;
}

// stages what the output indices [ox_f, ox_l] x [oy_f, oy_l] read
__device__ __forceinline__ ResizeTile resize_stage(uint8_t* patch, const ResizeSrc& g, int ox_f, int ox_l, int oy_f,
                                                   int oy_l, const uint8_t* lo, const uint8_t* hi, int tid) {
  const int cx0 = max(floor_src(ox_f, g.n_w, g.out_w) - 1, 0), ry0 = max(floor_src(oy_f, g.n_h, g.out_h) - 1, 0);
  const int cx1 = min(floor_src(ox_l, g.n_w, g.out_w) + 2, g.n_w - 1);
  const int ry1 = min(floor_src(oy_l, g.n_h, g.out_h) + 2, g.n_h - 1);
  return resize_stage_rect(patch, g, cx0, cx1, ry0, ry1, lo, hi, tid);
}

// the 4 x 4 sum of the taps sx-1 .. sx+2, sy-1 .. sy+2 (indices clamped inside the image) with the weights wx, wy, in fp32:
// horizontal pass, then vertical pass
template <bool STAGED>
__device__ __forceinline__ void resize_sum(const uint8_t* patch, const ResizeSrc& g, const ResizeTile& t, int sx, int sy,
                                           const float wx[4], const float wy[4], float v[3]) {
  int col[4];
  for (int k = 0; k < 4; ++k) col[k] = (clampi(sx - 1 + k, 0, g.n_w - 1) - t.cx0) * 3;
  float hrow[4][3];
  for (int r = 0; r < 4; ++r) {
    const int cy = clampi(sy - 1 + r, 0, g.n_h - 1) - t.ry0;
    const uint8_t* row;
    if (STAGED)
      row = patch + (long)cy * g.pitch + ((t.align0 + (unsigned)cy * t.align_step) & 3);
    else
      row = g.img + (long)cy * g.src_pitch;
    for (int c = 0; c < 3; ++c) {  // horizontal pass
      float h = wx[0] * (float)row[col[0] + c];
      h = h + wx[1] * (float)row[col[1] + c];
      h = h + wx[2] * (float)row[col[2] + c];
      h = h + wx[3] * (float)row[col[3] + c];
      hrow[r][c] = h;
    }
  }
  for (int c = 0; c < 3; ++c) {  // vertical pass
    float a = wy[0] * hrow[0][c];
    a = a + wy[1] * hrow[1][c];
    a = a + wy[2] * hrow[2][c];
    a = a + wy[3] * hrow[3][c];
    v[c] = a;
  }
}

// the fp32 value of output pixel (ox, oy) before rounding
template <bool STAGED>
__device__ __forceinline__ void resize_value(const uint8_t* patch, const ResizeSrc& g, const ResizeTile& t, int ox, int oy,
                                             float v[3]) {
  float wx[4], wy[4];
  const int sx = cubic_taps(ox, g.n_w, g.out_w, wx), sy = cubic_taps(oy, g.n_h, g.out_h, wy);
  resize_sum<STAGED>(patch, g, t, sx, sy, wx, wy, v);
}

// the epilogue of the crop kernels: rintf and clamp of a pixel's fp32 value v -> its three bytes at o and, ACT, the
// normalised network input at a (u8bgr_to_nhwc_kernel on the rounded byte, operation for operation)
template <typename T, bool ACT>
__device__ __forceinline__ void resize_store(const float v[3], uint8_t* o, T* a, int Cpad, float m0, float m1, float m2,
                                             float s0, float s1, float s2) {
  uint8_t px[3];
  for (int c = 0; c < 3; ++c) {  // rintf, clamp
    const float r = rintf(v[c]);
    px[c] = (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
  }
  o[0] = px[0];
  o[1] = px[1];
  o[2] = px[2];
  if (ACT) {
    const float r = ((float)px[2] - m0) / s0, gg = ((float)px[1] - m1) / s1, bb = ((float)px[0] - m2) / s2;
    a[0] = from_f32<T>(r);
    a[1] = from_f32<T>(gg);
    a[2] = from_f32<T>(bb);
    for (int c = 3; c < Cpad; ++c) a[c] = from_f32<T>(0.f);
  }
}

// BOXES: frame b takes box b of the table; g.pitch (and STAGED) are then the launch's, sized for its largest patch
template <typename T, bool ACT, bool STAGED, bool BOXES>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void crop_resize_cubic_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, T* __restrict__ act, BoxedGeom<ResizeGeom, BOXES> geo,
    int Cpad, float m0, float m1, float m2, float s0, float s1, float s2) {
  extern __shared__ __attribute__((aligned(16))) uint8_t patch[];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * RESIZE_TW, oy0 = blockIdx.y * RESIZE_TH, b = blockIdx.z;
  const ResizeGeom g = frame_geom(geo, b);
  const long frame_bytes = (long)g.src_h * g.src_w * 3;
  const uint8_t* frame = src + b * frame_bytes;
  // the crop's first pixel; the tile stages rows and columns of the crop
  const ResizeSrc rs = {frame + ((long)g.y1 * g.src_w + g.x1) * 3, (long)g.src_w * 3, g.ch, g.cw, g.H, g.W, g.pitch};
  ResizeTile t;
  if (STAGED) {
    t = resize_stage(patch, rs, ox0, min(ox0 + RESIZE_TW, g.W) - 1, oy0, min(oy0 + RESIZE_TH, g.H) - 1, src,
                     src + (long)gridDim.z * frame_bytes, tid);
    __syncthreads();
  }
  const int ox = ox0 + (tid % RESIZE_TW), oy = oy0 + (tid / RESIZE_TW);
  if (ox >= g.W || oy >= g.H) return;
  float v[3];
  resize_value<STAGED>(patch, rs, t, ox, oy, v);
  resize_store<T, ACT>(v, dst + ((long)b * g.H + oy) * g.dst_row_stride + (long)ox * 3,
                       ACT ? act + (((long)b * g.H + oy) * g.W + ox) * Cpad : nullptr, Cpad, m0, m1, m2, s0, s1, s2);
}

// LDS bytes of the largest part of an n_h x n_w image a tile of a resize to out_h x out_w can need, and the pitch of its
// rows; 0 when that passes RESIZE_LDS_BYTES (the taps are then read from global memory)
// (the boxes form sizes one patch for a launch: the most rows and the widest pitch of any of its frames)
struct PatchExtent {
  long rows = 0, pitch = 0;
  void cover(const PatchExtent& e) {
    rows = rows > e.rows ? rows : e.rows;
    pitch = pitch > e.pitch ? pitch : e.pitch;
  }
  // LDS bytes and the rows' pitch, or 0 and 0 past RESIZE_LDS_BYTES
  long lds_bytes(int* pitch_out) const {
    const bool staged = rows * pitch <= RESIZE_LDS_BYTES;
    *pitch_out = staged ? (int)pitch : 0;
    return staged ? rows * pitch : 0;
  }
};
static PatchExtent resize_patch_extent(int n_h, int n_w, int out_h, int out_w) {
  // floor(a + n r) - floor(a) <= floor(n r) + 1 source steps over n output steps, plus the three taps around them, plus up
  // to 3 bytes of dword alignment in front
  const long cols = (long)(RESIZE_TW - 1) * n_w / out_w + 1 + 4, rows = (long)(RESIZE_TH - 1) * n_h / out_h + 1 + 4;
  return PatchExtent{rows, (cols * 3 + 3 + 3) / 4 * 4};
}

// ---- host: what the launches of every form share (the entry points are at the end of the file) ----
// the operator's name in a refusal: the call's form
static const char* crop_op(const CropCall& c) {
  if (c.form == FRAME_BOX_ROTATED) return "crop_resize_cubic_rboxes";
  if (c.form == FRAME_BOX_PER_FRAME) return c.antialias ? "crop_resize_cubic_aa_boxes" : "crop_resize_cubic_boxes";
  return c.antialias ? "crop_resize_cubic_aa" : "crop_resize_cubic";
}

// the crop kernels' mean and std arguments: null is 0 and 1
struct Norm255 {
  float m[3], s[3];
  Norm255(const float* mean255, const float* std255) {
    for (int i = 0; i < 3; ++i) {
      m[i] = mean255 ? mean255[i] : 0.f;
      s[i] = std255 ? std255[i] : 1.f;
    }
  }
};

static dim3 tile_grid(int w, int h, int frames) {
  return dim3((w + RESIZE_TW - 1) / RESIZE_TW, (h + RESIZE_TH - 1) / RESIZE_TH, frames);
}

// A kernel's STAGED instantiation with `lds` bytes of staged patch behind `fixed` bytes of LDS, or, lds == 0
// (PatchExtent::lds_bytes: the patch does not fit), the instantiation that reads its taps from global memory
template <typename... P, typename... A>
static int launch_staged(void (*staged)(P...), void (*unstaged)(P...), dim3 grid, long lds, size_t fixed, hipStream_t stream,
                         const A&... args) {
  const dim3 block(RESIZE_TW * RESIZE_TH);
  if (lds > 0)
    hipLaunchKernelGGL(staged, grid, block, fixed + (size_t)lds, stream, args...);
  else
    hipLaunchKernelGGL(unstaged, grid, block, fixed, stream, args...);
  D3F_HIP(hipGetLastError());
  return 0;
}

// The boxes one launch decides its LDS and its grid for: the table of a chunk's frames b0 .. b0 + n - 1, filled here from the
// call's boxes, or the call's single box
struct LaunchBoxes {
  FrameBox one;
  const FrameBox* box = &one;
  int n = 1;
  template <typename G, bool BOXES>
  LaunchBoxes(BoxedGeom<G, BOXES>& a, const int32_t* boxes, int b0, int frames, FrameBox single) : one(single) {
    if constexpr (BOXES) {
      fill_frame_boxes(a.boxes, boxes, b0, frames);
      box = a.boxes.box;
      n = frames;
    }
  }
  LaunchBoxes(const LaunchBoxes&) = delete;
};

// one launch of the plain crop: a single-box call, or a chunk of a per-frame call (c: its frames; its boxes from b0)
template <typename T, bool ACT, bool BOXES>
static int resize_launch_one(const CropCall& c, int b0, const Norm255& k, hipStream_t stream) {
  BoxedGeom<ResizeGeom, BOXES> a;
  ResizeGeom& g = a.g;
  g = ResizeGeom{c.src_h, c.src_w, c.x1, c.y1, c.cw, c.ch, c.H, c.W, c.dst_row_stride, 0};
  const LaunchBoxes bx(a, c.boxes, b0, c.B, FrameBox{c.x1, c.y1, c.cw, c.ch});
  PatchExtent e;
  for (int i = 0; i < bx.n; ++i) e.cover(resize_patch_extent(bx.box[i].ch, bx.box[i].cw, g.H, g.W));
  const long lds = e.lds_bytes(&g.pitch);
  return launch_staged(crop_resize_cubic_kernel<T, ACT, true, BOXES>, crop_resize_cubic_kernel<T, ACT, false, BOXES>,
                       tile_grid(g.W, g.H, c.B), lds, 0, stream, c.src, c.dst, (T*)c.act, a, c.Cpad, k.m[0], k.m[1], k.m[2],
                       k.s[0], k.s[1], k.s[2]);
}

// What the single-box operators refuse of a box, for every frame of a boxes call, before anything is launched; the message
// names the frame.  boxes: host memory [B][4] as x1, y1, cw, ch.  aa_H > 0: the antialiased form's ratio limit as well.
static int frame_boxes_check(const char* op, const int32_t* boxes, int B, int src_h, int src_w, int aa_H = 0, int aa_W = 0) {
  D3F_CHECK(boxes != nullptr || B <= 0, "%s: null boxes (host memory [B][4]: x1, y1, cw, ch per frame)", op);
  for (int b = 0; b < B; ++b) {
    const int x1 = boxes[4L * b], y1 = boxes[4L * b + 1], cw = boxes[4L * b + 2], ch = boxes[4L * b + 3];
    D3F_CHECK(cw > 0 && ch > 0, "%s: frame %d: non-positive box extent (%d x %d)", op, b, cw, ch);
    D3F_CHECK(x1 >= 0 && y1 >= 0 && (long)x1 + cw <= src_w && (long)y1 + ch <= src_h,
              "%s: frame %d: box (x1 %d, y1 %d, %d x %d) outside the %d x %d frame", op, b, x1, y1, cw, ch, src_w, src_h);
    D3F_CHECK(aa_H <= 0 || ((long)cw <= (long)AA_MAX_RATIO * aa_W && (long)ch <= (long)AA_MAX_RATIO * aa_H),
              "%s: frame %d: box %d x %d above %d times the output %d x %d on an axis", op, b, cw, ch, AA_MAX_RATIO, aa_W,
              aa_H);
  }
  return 0;
}

// ---- antialiased form: Pillow's bicubic (torch's interpolate(mode="bicubic", antialias=True)) ----
// include/d3f_hip.h: d3f_crop_resize_cubic_aa_u8 is the definition; tests/resize_aa_restatement.py restates it in float64.
// An axis that shrinks by r widens the Keys kernel (A = -0.5) by r: up to 4 r + 1 taps, 129 at the ratio limit of 32, and a
// tile's source footprint grows with r on both axes -- far beyond LDS at r = 16.  So nothing is staged whole.  One
// workgroup per 32 x 8 tile of output pixels:
//   * the normalised weights of the tile's 32 columns and 8 rows are computed once, as two tables in LDS (eight lanes per
//     output index: the taps t = lane, lane + 8, ... and their partial sum);
//   * the source rows the tile's 8 output rows read are streamed in chunks of AA_ROWS: the columns the tile reads of each
//     row are staged with aligned dword loads (as resize_stage does), the horizontal filter turns a staged row into 32
//     fp32 pixels of a row buffer in LDS (lane = one column of one row), and each lane -- now one output pixel -- adds the
//     chunk's rows that lie inside its window to its vertical sum.
// Loop bounds are the table's (first tap, count), which come from xmin / xmax alone: every index lies inside the crop.
constexpr int AA_ROWS = 8;        // source rows per chunk: one per 32 lanes of the horizontal filter
constexpr int AA_LDS_LIMIT = 64 * 1024;

struct AaGeom {
  int src_h, src_w, x1, y1, cw, ch, H, W;
  long dst_row_stride;
  int ntx, nty;  // floats per table row: at least the most taps of an output column / row (aa_max_taps), odd
  int pitch;     // bytes of one staged source row (a multiple of 4)
};

// the most taps an output index of an axis n_in -> n_out has: xmax - xmin <= floor(2 s) + 1, 2 s = 4 n_in / n_out or 4
static int aa_max_taps(int n_in, int n_out) { return (n_in >= n_out ? (int)(4L * n_in / n_out) : 4) + 1; }
// the most source columns RESIZE_TW consecutive output columns read: xmax(i + n) - xmin(i) <= floor(n n_in / n_out + 2 s) + 1
static int aa_max_cols(int n_in, int n_out) {
  const long S = n_in >= n_out ? 4L * n_in : 4L * n_out;
  const long cols = ((long)(RESIZE_TW - 1) * n_in + S) / n_out + 1;
  return (int)(cols < n_in ? cols : n_in);
}

__device__ __forceinline__ float keys_aa(float x) {  // x >= 0, A = -0.5
  const float A = -0.5f;
  if (x < 1.f) return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  if (x < 2.f) return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  return 0.f;
}

// The taps of output indices i0 .. i0 + n_idx - 1 (n_idx <= 32) of an axis n_in -> n_out: first tap lo[j], count cnt[j] and
// the normalised weights wt[j * nt + t], t < cnt[j].  Eight lanes per index: lane `sub` takes the taps t = sub, sub + 8, ...
// and their sum p_sub (in that order); the weights' sum is ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)); each weight is
// divided by it.  Called by all 256 lanes (two barriers inside); part: 256 floats of scratch.
__device__ __forceinline__ void aa_axis_table(float* wt, int* lo, int* cnt, float* part, int i0, int n_idx, int n_in,
                                              int n_out, int nt, int tid) {
  const int j = tid >> 3, sub = tid & 7;
  int count = 0;
  float p = 0.f;
  if (j < n_idx) {
    const bool down = n_in >= n_out;
    const int S = down ? 4 * n_in : 4 * n_out, D = down ? 2 * n_in : 2 * n_out;
    const int c2 = (2 * (i0 + j) + 1) * n_in, den = 2 * n_out;  // below 2^30 for extents up to RESIZE_MAX_EXTENT
    const int a = c2 - S + n_out;
    const int first = a > 0 ? a / den : 0;  // max(floor(a / den), 0)
    const int end = min((c2 + S + n_out) / den, n_in);
    count = min(end - first, nt);  // (end - first <= aa_max_taps <= nt)
    for (int t = sub; t < count; t += 8) {
      const int num = (2 * (first + t) + 1) * n_out - c2;  // |num| < 2^24: exact in fp32
      const float w = keys_aa(fabsf((float)num / (float)D));
      wt[j * nt + t] = w;
      p = p + w;
    }
    if (sub == 0) {
      lo[j] = first;
      cnt[j] = count;
    }
  }
  part[tid] = p;
  __syncthreads();
  if (j < n_idx) {
    const float* q = part + (j << 3);
    const float sum = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    for (int t = sub; t < count; t += 8) wt[j * nt + t] = wt[j * nt + t] / sum;
  }
  __syncthreads();
}

// BOXES: frame b takes box b of the table; g.ntx, g.nty and g.pitch are then the launch's, the most of any of its frames
// (aa_axis_table's count <= nt and row_bytes + 3 <= pitch hold for every frame; the three only place things in LDS)
template <typename T, bool ACT, bool BOXES>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void crop_resize_cubic_aa_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, T* __restrict__ act, BoxedGeom<AaGeom, BOXES> geo, int Cpad,
    float m0, float m1, float m2, float s0, float s1, float s2) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aa_lds[];
  const AaGeom g = frame_geom(geo, (int)blockIdx.z);
  // (aa_lds_bytes below is this layout)
  float* wx = reinterpret_cast<float*>(aa_lds);     // [RESIZE_TW][ntx]
  float* wy = wx + RESIZE_TW * g.ntx;               // [RESIZE_TH][nty]
  float* hbuf = wy + RESIZE_TH * g.nty;             // [AA_ROWS][RESIZE_TW][3]: the horizontal pass of a chunk's rows
  float* part = hbuf + AA_ROWS * RESIZE_TW * 3;     // [256]
  int* xlo = reinterpret_cast<int*>(part + RESIZE_TW * RESIZE_TH);
  int* xcnt = xlo + RESIZE_TW;
  int* ylo = xcnt + RESIZE_TW;
  int* ycnt = ylo + RESIZE_TH;
  uint8_t* rows = reinterpret_cast<uint8_t*>(ycnt + RESIZE_TH);  // [AA_ROWS][pitch]
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * RESIZE_TW, oy0 = blockIdx.y * RESIZE_TH, b = blockIdx.z;
  const int tile_w = min(RESIZE_TW, g.W - ox0), tile_h = min(RESIZE_TH, g.H - oy0);
  aa_axis_table(wx, xlo, xcnt, part, ox0, tile_w, g.cw, g.W, g.ntx, tid);
  aa_axis_table(wy, ylo, ycnt, part, oy0, tile_h, g.ch, g.H, g.nty, tid);
  // what the tile reads of the crop: columns [cx0, cx1), rows [ry0, ry1) (xmin and xmax do not decrease with the index)
  const int cx0 = xlo[0], cx1 = xlo[tile_w - 1] + xcnt[tile_w - 1];
  const int ry0 = ylo[0], ry1 = ylo[tile_h - 1] + ycnt[tile_h - 1];
  const int row_bytes = (cx1 - cx0) * 3, pitch_dw = g.pitch >> 2;  // row_bytes + 3 <= pitch (aa_max_cols)
  const long frame_bytes = (long)g.src_h * g.src_w * 3, src_pitch = (long)g.src_w * 3;
  const uint8_t* crop = src + b * frame_bytes + ((long)g.y1 * g.src_w + g.x1) * 3;
  const uint8_t* lo = src;
  const uint8_t* hi = src + (long)gridDim.z * frame_bytes;  // a dword is loaded whole only inside [lo, hi)
  const unsigned align_step = (unsigned)(src_pitch & 3);
  const int lx = tid % RESIZE_TW, ly = tid / RESIZE_TW;
  const bool live = lx < tile_w && ly < tile_h;  // as an output pixel
  const int my_lo = live ? ylo[ly] : 0, my_cnt = live ? ycnt[ly] : 0;
  const int my_x = lx < tile_w ? (xlo[lx] - cx0) * 3 : 0, my_nx = lx < tile_w ? xcnt[lx] : 0;
  const float* my_wx = wx + lx * g.ntx;
  const float* my_wy = wy + ly * g.nty;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int r0 = ry0; r0 < ry1; r0 += AA_ROWS) {  // (workgroup-uniform)
    const int nrows = min(AA_ROWS, ry1 - r0);
    // stage: byte k of chunk row r sits at rows[r * pitch + align_r + k], in the aligned dwords that cover the row's bytes
    const uint8_t* first = crop + (long)r0 * src_pitch + (long)cx0 * 3;
    const unsigned align0 = (unsigned)(reinterpret_cast<uintptr_t>(first) & 3);
    for (int i = tid; i < nrows * pitch_dw; i += RESIZE_TW * RESIZE_TH) {
      const int r = i / pitch_dw, k = i - r * pitch_dw;
      const unsigned al = (align0 + (unsigned)r * align_step) & 3;
      if (k * 4 >= (int)al + row_bytes) continue;
      const uint8_t* p = first + (long)r * src_pitch - al + k * 4;
      uint32_t v;
      if (p >= lo && p + 4 <= hi) {
        v = *reinterpret_cast<const uint32_t*>(p);
      } else {
        v = 0;
        for (int q = 0; q < 4; ++q)
          if (p + q >= lo && p + q < hi) v |= (uint32_t)p[q] << (8 * q);
      }
      *reinterpret_cast<uint32_t*>(rows + (long)r * g.pitch + k * 4) = v;
    }
    __syncthreads();
    // horizontal pass: lane = column lx of chunk row ly.  Four sums q_u over the taps t = u, u + 4, ... (in that order),
    // h = (q0 + q1) + (q2 + q3)
    if (ly < nrows && lx < tile_w) {
      const uint8_t* px = rows + (long)ly * g.pitch + ((align0 + (unsigned)ly * align_step) & 3) + my_x;
      float q[4][3] = {};
      int t = 0;
      for (; t + 4 <= my_nx; t += 4)
        for (int u = 0; u < 4; ++u) {
          const float w = my_wx[t + u];
          for (int c = 0; c < 3; ++c) q[u][c] = q[u][c] + w * (float)px[(t + u) * 3 + c];
        }
      for (int u = 0; u < 3; ++u)
        if (t + u < my_nx) {
          const float w = my_wx[t + u];
          for (int c = 0; c < 3; ++c) q[u][c] = q[u][c] + w * (float)px[(t + u) * 3 + c];
        }
      for (int c = 0; c < 3; ++c) hbuf[(ly * RESIZE_TW + lx) * 3 + c] = (q[0][c] + q[1][c]) + (q[2][c] + q[3][c]);
    }
    __syncthreads();
    // vertical pass: lane = output pixel (lx, ly).  The chunk's rows inside its window, in order, then onto the running sum
    float partial[3] = {0.f, 0.f, 0.f};
    for (int r = 0; r < nrows; ++r) {
      const int t = r0 + r - my_lo;
      if (t >= 0 && t < my_cnt) {
        const float w = my_wy[t];
        for (int c = 0; c < 3; ++c) partial[c] = partial[c] + w * hbuf[(r * RESIZE_TW + lx) * 3 + c];
      }
    }
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + partial[c];
    // (the next chunk's staging writes rows, read before the barrier above; its horizontal pass writes hbuf behind the
    // next barrier)
  }
  if (!live) return;
  const int ox = ox0 + lx, oy = oy0 + ly;
  resize_store<T, ACT>(acc, dst + ((long)b * g.H + oy) * g.dst_row_stride + (long)ox * 3,
                       ACT ? act + (((long)b * g.H + oy) * g.W + ox) * Cpad : nullptr, Cpad, m0, m1, m2, s0, s1, s2);
}

static size_t aa_lds_bytes(const AaGeom& g) {
  const size_t floats = (size_t)RESIZE_TW * g.ntx + (size_t)RESIZE_TH * g.nty + AA_ROWS * RESIZE_TW * 3 + RESIZE_TW * RESIZE_TH;
  return (floats + 2 * RESIZE_TW + 2 * RESIZE_TH) * 4 + (size_t)AA_ROWS * g.pitch;
}

// the table strides and the staged pitch of one box, and of a launch: the most of its boxes
static void aa_strides(AaGeom& g, int cw, int ch) {
  const int ntx = aa_max_taps(cw, g.W) | 1, nty = aa_max_taps(ch, g.H) | 1;
  const int pitch = (aa_max_cols(cw, g.W) * 3 + 3 + 3) / 4 * 4;  // up to 3 bytes of dword alignment in front
  g.ntx = g.ntx > ntx ? g.ntx : ntx;
  g.nty = g.nty > nty ? g.nty : nty;
  g.pitch = g.pitch > pitch ? g.pitch : pitch;
}

// one launch of the antialiased crop: a single-box call, or a chunk of a per-frame call (c: its frames; its boxes from b0).
// (The LDS of a launch -- its boxes' largest strides together -- stays below AA_LDS_LIMIT whatever the boxes: at the ratio
// limit on both axes it is 52 KB.)
template <typename T, bool ACT, bool BOXES>
static int aa_launch_one(const CropCall& c, int b0, const Norm255& k, hipStream_t stream) {
  BoxedGeom<AaGeom, BOXES> a;
  AaGeom& g = a.g;
  g = AaGeom{c.src_h, c.src_w, c.x1, c.y1, c.cw, c.ch, c.H, c.W, c.dst_row_stride, 0, 0, 0};
  const LaunchBoxes bx(a, c.boxes, b0, c.B, FrameBox{c.x1, c.y1, c.cw, c.ch});
  for (int i = 0; i < bx.n; ++i) aa_strides(g, bx.box[i].cw, bx.box[i].ch);
  D3F_CHECK(aa_lds_bytes(g) <= (size_t)AA_LDS_LIMIT, "%s: %zu bytes of LDS", crop_op(c), aa_lds_bytes(g));
  hipLaunchKernelGGL((crop_resize_cubic_aa_kernel<T, ACT, BOXES>), tile_grid(g.W, g.H, c.B), dim3(RESIZE_TW * RESIZE_TH),
                     aa_lds_bytes(g), stream, c.src, c.dst, (T*)c.act, a, c.Cpad, k.m[0], k.m[1], k.m[2], k.s[0], k.s[1],
                     k.s[2]);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ---- full-frame output: the inverse of crop_resize_cubic (the plain form) with a blend in the epilogue ----
// patch [B][H][W][3] (rows patch_row_stride bytes apart) is resized H x W -> ch x cw with resize_value and blended into the
// box (x1, y1, cw, ch) of frame [B][src_h][src_w][3]; everything else of out is the frame (include/d3f_hip.h:
// d3f_paste_resize_cubic_u8 is the definition; tests/paste_restatement.py restates it in float64).
// Tiles lie on the FRAME's 32 x 8 grid.  A tile that meets the box stages the part of the patch its box pixels read and
// runs one lane per pixel; a tile outside the box moves the frame's bytes as aligned dwords (a row of a tile is 96
// contiguous bytes).  out == frame: only the tiles that meet the box are launched (tx0, ty0: the first of them), and a
// lane reads no frame byte but the three it writes.
struct PasteGeom {
  int H, W;
  long patch_row_stride;
  int src_h, src_w, x1, y1, cw, ch, feather;
  int pitch;
  int tx0, ty0;
};
// the kernel's last argument: the geometry and, in the colour form only, the coefficients [B][3][2] (gain, offset) -- the
// plain form's arguments are the ones it had before there was a colour form
// BOXES: the table of the launch's boxes behind the geometry
template <bool COLOR, bool BOXES>
struct PasteArgs {
  BoxedGeom<PasteGeom, BOXES> geo;
};
template <bool BOXES>
struct PasteArgs<true, BOXES> {
  BoxedGeom<PasteGeom, BOXES> geo;
  const float* coef;
};

// the epilogue of the paste kernels: the clamped patch value v (COLOR: through frame b's gain and offset, clamped again)
// blended with weight a over the frame's three bytes at f -> the three bytes at o
template <bool COLOR, class Args>
__device__ __forceinline__ void paste_blend(const float v[3], float a, const uint8_t* f, uint8_t* o, const Args& args, int b) {
  const float na = 1.f - a;
  const float s[3] = {(float)f[0], (float)f[1], (float)f[2]};
  uint8_t px[3];
  for (int c = 0; c < 3; ++c) {
    float vc = fminf(fmaxf(v[c], 0.f), 255.f);
    if constexpr (COLOR) {
      const float scaled = args.coef[((long)b * 3 + c) * 2] * vc;
      vc = fminf(fmaxf(scaled + args.coef[((long)b * 3 + c) * 2 + 1], 0.f), 255.f);
    }
    const float pv = a * vc, ps = na * s[c];
    const float r = rintf(pv + ps);
    px[c] = (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
  }
  o[0] = px[0];
  o[1] = px[1];
  o[2] = px[2];
}

// COLOR (include/d3f_hip.h: d3f_paste_resize_cubic_color_u8): the clamped patch value goes through gain * v + offset of its
// frame and channel (product and sum rounded separately) and a second clamp before the blend
// BOXES: frame b takes box b of the table; g.pitch (and STAGED) are the launch's, sized for its largest staged part.  In
// place the grid is the largest tile count of any frame: a frame derives its own first tile here, and its workgroups past its
// own tile count return before they touch memory -- the tiles they would name belong to no box of THIS frame
template <bool STAGED, bool COLOR, bool BOXES>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void paste_resize_cubic_kernel(const uint8_t* __restrict__ patch,
                                                                                  const uint8_t* frame, uint8_t* out,
                                                                                  PasteArgs<COLOR, BOXES> args) {
  const int b = blockIdx.z;
  PasteGeom g = frame_geom(args.geo, b);
  const bool in_place = frame == out;
  if constexpr (BOXES) {
    if (in_place) {  // (workgroup-uniform)
      g.tx0 = g.x1 / RESIZE_TW;
      g.ty0 = g.y1 / RESIZE_TH;
      if ((int)blockIdx.x > (g.x1 + g.cw - 1) / RESIZE_TW - g.tx0 || (int)blockIdx.y > (g.y1 + g.ch - 1) / RESIZE_TH - g.ty0)
        return;
    }
  }
  extern __shared__ __attribute__((aligned(16))) uint8_t staged[];
  const int tid = threadIdx.x;
  const int ox0 = ((int)blockIdx.x + g.tx0) * RESIZE_TW, oy0 = ((int)blockIdx.y + g.ty0) * RESIZE_TH;
  const long frame_bytes = (long)g.src_h * g.src_w * 3, row_bytes = (long)g.src_w * 3;
  const uint8_t* f = frame + b * frame_bytes;
  uint8_t* o = out + b * frame_bytes;
  const int tile_w = min(RESIZE_TW, g.src_w - ox0), tile_h = min(RESIZE_TH, g.src_h - oy0);
  // the box pixels of this tile: columns [bx_f, bx_l] and rows [by_f, by_l] of the box
  const int bx_f = max(ox0, g.x1) - g.x1, bx_l = min(ox0 + tile_w, g.x1 + g.cw) - 1 - g.x1;
  const int by_f = max(oy0, g.y1) - g.y1, by_l = min(oy0 + tile_h, g.y1 + g.ch) - 1 - g.y1;
  const int lx = tid % RESIZE_TW, ly = tid / RESIZE_TW;
  if (bx_f > bx_l || by_f > by_l) {  // (workgroup-uniform) a tile outside the box: a copy
    if (in_place || ly >= tile_h) return;
    const long at = (long)(oy0 + ly) * row_bytes + (long)ox0 * 3;
    frame_tile_row_copy(f + at, o + at, tile_w, lx);
    return;
  }
  const uint8_t* img = patch + (long)b * g.H * g.patch_row_stride;
  const ResizeSrc rs = {img, g.patch_row_stride, g.H, g.W, g.ch, g.cw, g.pitch};
  ResizeTile t;
  if (STAGED) {
    // a dword is loaded whole only inside the bytes from the first patch's first pixel to the last one's last
    const uint8_t* hi = patch + ((long)gridDim.z * g.H - 1) * g.patch_row_stride + (long)g.W * 3;
    t = resize_stage(staged, rs, bx_f, bx_l, by_f, by_l, patch, hi, tid);
    __syncthreads();
  }
  if (lx >= tile_w || ly >= tile_h) return;
  const long at = (long)(oy0 + ly) * row_bytes + (long)(ox0 + lx) * 3;
  const int j = ox0 + lx - g.x1, i = oy0 + ly - g.y1;
  if (j < 0 || j >= g.cw || i < 0 || i >= g.ch) {  // a pixel of the tile outside the box
    if (!in_place) {
      const uint8_t s0 = f[at], s1 = f[at + 1], s2 = f[at + 2];
      o[at] = s0;
      o[at + 1] = s1;
      o[at + 2] = s2;
    }
    return;
  }
  float v[3];
  resize_value<STAGED>(staged, rs, t, j, i, v);
  // the separable ramp: 1 at distance >= feather from the box's edges, (d + 1) / (feather + 1) inside that
  const int dy = min(i, g.ch - 1 - i), dx = min(j, g.cw - 1 - j);
  const float ay = (float)min(dy + 1, g.feather + 1) / (float)(g.feather + 1);
  const float ax = (float)min(dx + 1, g.feather + 1) / (float)(g.feather + 1);
  paste_blend<COLOR>(v, ay * ax, f + at, o + at, args, b);
}

// color -> COLOR and the form -> BOXES as types, for the paste kernels and the multiband difference: fn(COLOR, BOXES)
template <class Fn>
static int paste_forms(const PasteCall& c, Fn fn) {
  using T = std::true_type;
  using F = std::false_type;
  if (c.form != FRAME_BOX_ONE) return c.color ? fn(T{}, T{}) : fn(F{}, T{});
  return c.color ? fn(T{}, F{}) : fn(F{}, F{});
}

// one launch of the paste, plain or colour: a single-box call, or a chunk of a per-frame call (c: its frames; its boxes from
// b0).  coef is read by the colour form only
template <bool COLOR, bool BOXES>
static int paste_launch_one(const PasteCall& c, int b0, hipStream_t stream) {
  PasteArgs<COLOR, BOXES> args;
  PasteGeom& g = args.geo.g;
  g = PasteGeom{c.H, c.W, c.patch_row_stride, c.src_h, c.src_w, c.x1, c.y1, c.cw, c.ch, c.feather, 0, 0, 0};
  if constexpr (COLOR) args.coef = c.coef;
  const LaunchBoxes bx(args.geo, c.boxes, b0, c.B, FrameBox{c.x1, c.y1, c.cw, c.ch});
  PatchExtent e;
  InPlaceTiles tiles{RESIZE_TW, RESIZE_TH};
  for (int i = 0; i < bx.n; ++i) {
    e.cover(resize_patch_extent(c.H, c.W, bx.box[i].ch, bx.box[i].cw));
    tiles.cover(bx.box[i]);
  }
  const long lds = e.lds_bytes(&g.pitch);
  dim3 grid = tile_grid(c.src_w, c.src_h, c.B);
  if (c.frame == c.out) {  // in place: the tiles that meet a box (BOXES: the kernel derives each frame's tx0, ty0)
    grid.x = tiles.nx;
    grid.y = tiles.ny;
    if constexpr (!BOXES) {
      g.tx0 = c.x1 / RESIZE_TW;
      g.ty0 = c.y1 / RESIZE_TH;
    }
  }
  return launch_staged(paste_resize_cubic_kernel<true, COLOR, BOXES>, paste_resize_cubic_kernel<false, COLOR, BOXES>, grid, lds,
                       0, stream, c.patch, c.frame, c.out, args);
}

// ---- multiband paste: the difference image (include/d3f_hip.h: d3f_paste_multiband_u8; the pyramid is multiband.hip) ----
// g_0 = (V - s) << 6 with V the byte the paste kernel above writes at feather 0 -- resize_stage, resize_value, the clamp, the
// colour form's two operations and rintf, the same device functions on the same operands -- and s the frame's byte.
// Tiles lie on the BOX's 32 x 8 grid, so that a tile's row of a plane starts on 64 bytes: a lane computes its pixel's three
// values into LDS, and 96 lanes then store the tile's three 8 x 32 planes as 16-byte vectors (a vector that crosses the
// box's right edge ends inside the row's padding; those lanes hold 0).
struct DiffGeom {
  int H, W;
  long patch_row_stride;
  int src_h, src_w, x1, y1, cw, ch;
  int pitch;   // bytes of one staged patch row
  int pitch0;  // int16 per row of g_0
  long slab_bytes;
};
constexpr int DIFF_TILE_BYTES = 3 * RESIZE_TH * RESIZE_TW * 2;

// BOXES: the grid is the largest box's; a frame's workgroups past its own box return at once
template <bool STAGED, bool COLOR, bool BOXES>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void multiband_diff_kernel(const uint8_t* __restrict__ patch,
                                                                              const uint8_t* __restrict__ frame,
                                                                              int16_t* __restrict__ g0,
                                                                              const float* __restrict__ coef,
                                                                              BoxedGeom<DiffGeom, BOXES> geo) {
  const int b = blockIdx.z;
  const DiffGeom g = frame_geom(geo, b);
  const int bx0 = blockIdx.x * RESIZE_TW, by0 = blockIdx.y * RESIZE_TH;
  if (bx0 >= g.cw || by0 >= g.ch) return;  // (workgroup-uniform)
  extern __shared__ __attribute__((aligned(16))) uint8_t diff_lds[];
  int16_t* dtile = reinterpret_cast<int16_t*>(diff_lds);  // [3][RESIZE_TH][RESIZE_TW]
  uint8_t* staged = diff_lds + DIFF_TILE_BYTES;
  const int tid = threadIdx.x;
  const int bx_l = min(bx0 + RESIZE_TW, g.cw) - 1, by_l = min(by0 + RESIZE_TH, g.ch) - 1;
  const uint8_t* img = patch + (long)b * g.H * g.patch_row_stride;
  const ResizeSrc rs = {img, g.patch_row_stride, g.H, g.W, g.ch, g.cw, g.pitch};
  ResizeTile t;
  if (STAGED) {
    const uint8_t* hi = patch + ((long)gridDim.z * g.H - 1) * g.patch_row_stride + (long)g.W * 3;
    t = resize_stage(staged, rs, bx0, bx_l, by0, by_l, patch, hi, tid);
    __syncthreads();
  }
  const int lx = tid % RESIZE_TW, ly = tid / RESIZE_TW;
  const int j = bx0 + lx, i = by0 + ly;
  int d[3] = {0, 0, 0};
  if (j < g.cw && i < g.ch) {
    float v[3];
    resize_value<STAGED>(staged, rs, t, j, i, v);
    const uint8_t* s = frame + (long)b * g.src_h * g.src_w * 3 + ((long)(g.y1 + i) * g.src_w + g.x1 + j) * 3;
    for (int c = 0; c < 3; ++c) {
      float vc = fminf(fmaxf(v[c], 0.f), 255.f);
      if constexpr (COLOR) {
        const float scaled = coef[((long)b * 3 + c) * 2] * vc;
        vc = fminf(fmaxf(scaled + coef[((long)b * 3 + c) * 2 + 1], 0.f), 255.f);
      }
      d[c] = ((int)rintf(vc) - (int)s[c]) * 64;
    }
  }
  for (int c = 0; c < 3; ++c) dtile[(c * RESIZE_TH + ly) * RESIZE_TW + lx] = (int16_t)d[c];
  __syncthreads();
  if (tid < 3 * RESIZE_TH * (RESIZE_TW / 8)) {
    const int c = tid / (RESIZE_TH * (RESIZE_TW / 8)), r = (tid / (RESIZE_TW / 8)) % RESIZE_TH, k = tid % (RESIZE_TW / 8);
    if (by0 + r < g.ch && bx0 + 8 * k < g.cw) {
      int16_t* plane = g0 + ((long)b * 3 + c) * (g.slab_bytes / 2);
      *reinterpret_cast<int4*>(plane + (long)(by0 + r) * g.pitch0 + bx0 + 8 * k) =
          *reinterpret_cast<const int4*>(dtile + (c * RESIZE_TH + r) * RESIZE_TW + 8 * k);
    }
  }
}

template <bool COLOR, bool BOXES>
static int diff_launch_one(const PasteCall& c, int b0, int16_t* g0, int pitch0, long slab_bytes, hipStream_t stream) {
  BoxedGeom<DiffGeom, BOXES> a;
  DiffGeom& g = a.g;
  g = DiffGeom{c.H, c.W, c.patch_row_stride, c.src_h, c.src_w, c.x1, c.y1, c.cw, c.ch, 0, pitch0, slab_bytes};
  const LaunchBoxes bx(a, c.boxes, b0, c.B, FrameBox{c.x1, c.y1, c.cw, c.ch});
  PatchExtent e;
  int cw_max = 1, ch_max = 1;
  for (int i = 0; i < bx.n; ++i) {
    e.cover(resize_patch_extent(c.H, c.W, bx.box[i].ch, bx.box[i].cw));
    cw_max = cw_max > bx.box[i].cw ? cw_max : bx.box[i].cw;
    ch_max = ch_max > bx.box[i].ch ? ch_max : bx.box[i].ch;
  }
  const long lds = e.lds_bytes(&g.pitch);
  return launch_staged(multiband_diff_kernel<true, COLOR, BOXES>, multiband_diff_kernel<false, COLOR, BOXES>,
                       tile_grid(cw_max, ch_max, c.B), lds, DIFF_TILE_BYTES, stream, c.patch, c.frame, g0, c.coef, a);
}

// (the caller, paste_multiband_u8_launch, has checked everything)
int multiband_diff_launch(const PasteCall& c, int b0, int16_t* g0, int pitch0, long slab_bytes, hipStream_t stream) {
  return paste_forms(c, [&](auto COLOR, auto BOXES) {
    return diff_launch_one<decltype(COLOR)::value, decltype(BOXES)::value>(c, b0, g0, pitch0, slab_bytes, stream);
  });
}

// ---- rotated boxes (include/d3f_hip.h: the _rboxes_ operators; DESIGN.md section 4 "Rotated crop") ----
// Frame b's box turned by its angle about its centre; the angle arrives as c16 = round(cos a * 65536), s16 = round(sin a *
// 65536), computed on the host.  Every coordinate is formed EXACTLY in 64-bit integers over one denominator and reduced once,
// by a floor division, to a fixed-point position with ROT_FRAC_BITS fractional bits: its integer part is s, its fraction
// t = (float)frac / 65536 is exact in fp32.  With extents up to RESIZE_MAX_EXTENT = 2^14 and |c16|, |s16| <= 65537:
//   crop:  num = (2 x1 + cw - 1) 2^16 W H + c16 cw (2 ox + 1 - W) H - s16 ch (2 oy + 1 - H) W over 2^17 W H; the first term is
//          below 2^15 2^16 2^28 = 2^59, the other two together below (|c16| + |s16|) 2^42 < 2^58.6: |num| < 2^60;
//   paste: n_j = (cw - 1) 2^16 + c16 dx2 + s16 dy2 over 2^17 with |dx2|, |dy2| < 2^16: |n_j| < 2^34; the patch position
//          (n_j + 2^16) W - 2^16 cw over 2^17 cw stays below 2^49.
// From s and t on it is the arithmetic of the plain forms: keys_weights, resize_sum, resize_store / paste_blend.  A tile
// stages the axis-aligned bounding box of its footprint (the map is affine: the extremes sit at the tile's four corners),
// clipped to the image; the crop's image is the whole FRAME, so its taps clamp to the frame and not to the box.
constexpr int ROT_FRAC_BITS = 16;
constexpr long ROT_ONE = 1L << ROT_FRAC_BITS;

struct RotBox {
  int x1, y1, cw, ch, c16, s16;
};

// floor(a / b), b > 0, exactly.  On the device the quotient is first taken in fp64: the conversion of a and the division
// are each off by 2^-53 of the quotient, which stays below 2^48 here (the crop's positions below 2^33, the paste's patch
// positions below 2^48), so its floor is off by at most one; the exact 64-bit remainder then corrects it.  The same integer
// as the host's division, without the 64-bit integer division's long expansion -- a lane needs up to ten of them
__host__ __device__ inline long floor_div64(long a, long b) {  // b > 0
#if defined(__HIP_DEVICE_COMPILE__)
  long q = (long)floor((double)a / (double)b);
  const long r = a - q * b;
  if (r < 0) q -= 1;
  if (r >= b) q += 1;
  return q;
#else
  long q = a / b;
  if (a - q * b < 0) q -= 1;
  return q;
#endif
}
__host__ __device__ inline long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the fixed-point frame position of output pixel (ox, oy) of an H x W crop of the rotated box
__host__ __device__ inline void rot_crop_pos(const RotBox& r, int H, int W, int ox, int oy, long& px, long& py) {
  const long nu = (long)r.cw * (2 * ox + 1 - W), nv = (long)r.ch * (2 * oy + 1 - H);
  const long base = ROT_ONE * W * H;
  const long numx = (2L * r.x1 + r.cw - 1) * base + (long)r.c16 * nu * H - (long)r.s16 * nv * W;
  const long numy = (2L * r.y1 + r.ch - 1) * base + (long)r.s16 * nu * H + (long)r.c16 * nv * W;
  const long den = 2L * W * H;  // (num / (2^17 W H)) 2^16
  px = floor_div64(numx, den);
  py = floor_div64(numy, den);
}

// the numerators over 2^17 of the box-local position (j', i') of frame pixel (x, y)
__host__ __device__ inline void rot_local(const RotBox& r, int x, int y, long& nj, long& ni) {
  const long dx2 = 2L * x - 2L * r.x1 - r.cw + 1, dy2 = 2L * y - 2L * r.y1 - r.ch + 1;
  nj = (r.cw - 1) * ROT_ONE + r.c16 * dx2 + r.s16 * dy2;
  ni = (r.ch - 1) * ROT_ONE - r.s16 * dx2 + r.c16 * dy2;
}
// -0.5 <= position < extent - 0.5
__host__ __device__ inline bool rot_inside(long n, int extent) { return n >= -ROT_ONE && n < (2L * extent - 1) * ROT_ONE; }
// the fixed-point position in a patch of n_out samples of the local position n / 2^17 on an axis of `extent` pixels:
// (j' + 0.5) n_out / extent - 0.5
__host__ __device__ inline long rot_patch_pos(long n, int extent, int n_out) {
  return floor_div64((n + ROT_ONE) * n_out - ROT_ONE * extent, 2L * extent);
}
// the ramp of one axis on the continuous distance: min(d' + 1, feather + 1) / (feather + 1), d' = min(j', extent - 1 - j')
// in fixed point (two integers converted to fp32, one division)
__host__ __device__ inline float rot_ramp(long n, int extent, int feather) {
  const long fx = n >> 1;  // floor, ROT_FRAC_BITS fractional bits
  const long other = (extent - 1) * ROT_ONE - fx;
  const long d = fx < other ? fx : other;
  const long full = (feather + 1) * ROT_ONE;
  return (float)(d + ROT_ONE < full ? d + ROT_ONE : full) / (float)full;
}
// the frame pixels [bx0, bx1] x [by0, by1] that hold the rotated rectangle (a pixel more on every side: c16, s16 are a
// rotation to 2^-15 only), clipped to the frame; the box's centre lies inside the frame, so none is empty
__host__ __device__ inline void rot_bbox(const RotBox& r, int src_h, int src_w, int& bx0, int& bx1, int& by0, int& by1) {
  const long ac = r.c16 < 0 ? -(long)r.c16 : r.c16, as = r.s16 < 0 ? -(long)r.s16 : r.s16;
  const long ax = (2L * r.x1 + r.cw - 1) * ROT_ONE, ay = (2L * r.y1 + r.ch - 1) * ROT_ONE;
  const long hx = ac * r.cw + as * r.ch, hy = as * r.cw + ac * r.ch;  // over 2^17, as ax and ay
  bx0 = (int)clampl(((ax - hx) >> 17) - 1, 0, src_w - 1);
  bx1 = (int)clampl(((ax + hx) >> 17) + 2, 0, src_w - 1);
  by0 = (int)clampl(((ay - hy) >> 17) - 1, 0, src_h - 1);
  by1 = (int)clampl(((ay + hy) >> 17) + 2, 0, src_h - 1);
}

__device__ __forceinline__ RotBox rot_box(const FrameRBoxes& t, int b) {
  const FrameBox bx = t.box[b];
  const FrameRot r = t.rot[b];
  return RotBox{bx.x1, bx.y1, bx.cw, bx.ch, r.c16, r.s16};
}

// stages the bounding box of the positions pos(x, y) of x in [x_f, x_l], y in [y_f, y_l] with their taps, clipped to the
// image -- and to the launch's LDS (rows_max rows of g.pitch bytes: the host's bound holds it; the clip keeps a wrong bound
// from writing past the allocation)
template <class Pos>
__device__ __forceinline__ ResizeTile rot_stage(uint8_t* patch, const ResizeSrc& g, int rows_max, Pos pos, int x_f, int x_l,
                                                int y_f, int y_l, const uint8_t* lo, const uint8_t* hi, int tid) {
  long lox, hix, loy, hiy;
  pos(x_f, y_f, lox, loy);
  hix = lox;
  hiy = loy;
  for (int k = 1; k < 4; ++k) {
    long px, py;
    pos(k & 1 ? x_l : x_f, k & 2 ? y_l : y_f, px, py);
    lox = px < lox ? px : lox;
    hix = px > hix ? px : hix;
    loy = py < loy ? py : loy;
    hiy = py > hiy ? py : hiy;
  }
  const int cx0 = (int)clampl((lox >> ROT_FRAC_BITS) - 1, 0, g.n_w - 1), ry0 = (int)clampl((loy >> ROT_FRAC_BITS) - 1, 0, g.n_h - 1);
  int cx1 = (int)clampl((hix >> ROT_FRAC_BITS) + 2, 0, g.n_w - 1), ry1 = (int)clampl((hiy >> ROT_FRAC_BITS) + 2, 0, g.n_h - 1);
  cx1 = min(cx1, cx0 + (g.pitch - 3) / 3 - 1);
  ry1 = min(ry1, ry0 + rows_max - 1);
  return resize_stage_rect(patch, g, cx0, cx1, ry0, ry1, lo, hi, tid);
}

// the value at a fixed-point position of the image
template <bool STAGED>
__device__ __forceinline__ void rot_value(const uint8_t* patch, const ResizeSrc& g, const ResizeTile& t, long px, long py,
                                          float v[3]) {
  float wx[4], wy[4];
  keys_weights((float)(int)(px & (ROT_ONE - 1)) / (float)ROT_ONE, wx);
  keys_weights((float)(int)(py & (ROT_ONE - 1)) / (float)ROT_ONE, wy);
  resize_sum<STAGED>(patch, g, t, (int)(px >> ROT_FRAC_BITS), (int)(py >> ROT_FRAC_BITS), wx, wy, v);
}

struct RotCropGeom {
  int src_h, src_w, H, W;
  long dst_row_stride;
  int pitch, rows_max;  // the launch's staged rows: their pitch in bytes and their count
};
struct RotCropArgs {
  RotCropGeom g;
  FrameRBoxes t;
};

template <typename T, bool ACT, bool STAGED>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void crop_resize_cubic_rot_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, T* __restrict__ act, RotCropArgs a, int Cpad, float m0,
    float m1, float m2, float s0, float s1, float s2) {
  extern __shared__ __attribute__((aligned(16))) uint8_t patch[];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * RESIZE_TW, oy0 = blockIdx.y * RESIZE_TH, b = blockIdx.z;
  const RotCropGeom& g = a.g;
  const RotBox r = rot_box(a.t, b);
  const long frame_bytes = (long)g.src_h * g.src_w * 3;
  // the image is the whole frame: a tap index clamps to the frame
  const ResizeSrc rs = {src + b * frame_bytes, (long)g.src_w * 3, g.src_h, g.src_w, g.H, g.W, g.pitch};
  auto pos = [&](int ox, int oy, long& px, long& py) { rot_crop_pos(r, g.H, g.W, ox, oy, px, py); };
  ResizeTile t;
  if (STAGED) {
    t = rot_stage(patch, rs, g.rows_max, pos, ox0, min(ox0 + RESIZE_TW, g.W) - 1, oy0, min(oy0 + RESIZE_TH, g.H) - 1, src,
                  src + (long)gridDim.z * frame_bytes, tid);
    __syncthreads();
  }
  const int ox = ox0 + (tid % RESIZE_TW), oy = oy0 + (tid / RESIZE_TW);
  if (ox >= g.W || oy >= g.H) return;
  long px, py;
  pos(ox, oy, px, py);
  float v[3];
  rot_value<STAGED>(patch, rs, t, px, py, v);
  resize_store<T, ACT>(v, dst + ((long)b * g.H + oy) * g.dst_row_stride + (long)ox * 3,
                       ACT ? act + (((long)b * g.H + oy) * g.W + ox) * Cpad : nullptr, Cpad, m0, m1, m2, s0, s1, s2);
}

// what a tile may stage of an n_h x n_w image when its footprint spans xext x yext samples (floors): floor(a + e) - floor(a)
// <= floor(e) + 1 steps, the three taps around them and one sample for the count; the pitch as resize_patch_extent's
static PatchExtent rot_patch_extent(long xext, long yext, int n_h, int n_w) {
  long cols = xext + 5, rows = yext + 5;
  cols = cols < n_w ? cols : n_w;
  rows = rows < n_h ? rows : n_h;
  return PatchExtent{rows, (cols * 3 + 3 + 3) / 4 * 4};
}
static long labs64(long v) { return v < 0 ? -v : v; }

static void fill_frame_rboxes(FrameRBoxes& t, const int32_t* boxes, const int32_t* rot, int b0, int n) {
  t = FrameRBoxes{};
  for (int i = 0; i < n; ++i) {
    const int32_t* bx = boxes + 4L * (b0 + i);
    t.box[i] = FrameBox{bx[0], bx[1], bx[2], bx[3]};
    t.rot[i] = FrameRot{rot[2L * (b0 + i)], rot[2L * (b0 + i) + 1]};
  }
}

// one launch of the rotated crop: a chunk of at most FRAME_BOXES_MAX frames (c: its frames; its boxes and rotations from b0)
template <typename T, bool ACT>
static int rot_crop_launch_one(const CropCall& c, int b0, const Norm255& k, hipStream_t stream) {
  RotCropArgs a;
  RotCropGeom& g = a.g;
  g = RotCropGeom{c.src_h, c.src_w, c.H, c.W, c.dst_row_stride, 0, 0};
  fill_frame_rboxes(a.t, c.boxes, c.rot, b0, c.B);
  PatchExtent e;
  for (int i = 0; i < c.B; ++i) {
    // a tile's footprint: (RESIZE_TW - 1) cw / W along the crop's columns and (RESIZE_TH - 1) ch / H along its rows, turned
    const long ac = labs64(a.t.rot[i].c16), as = labs64(a.t.rot[i].s16);
    const long du = (long)(RESIZE_TW - 1) * a.t.box[i].cw * g.H, dv = (long)(RESIZE_TH - 1) * a.t.box[i].ch * g.W;
    const long den = ROT_ONE * g.W * g.H;
    e.cover(rot_patch_extent((ac * du + as * dv) / den, (as * du + ac * dv) / den, g.src_h, g.src_w));
  }
  const long lds = e.lds_bytes(&g.pitch);
  g.rows_max = (int)e.rows;
  return launch_staged(crop_resize_cubic_rot_kernel<T, ACT, true>, crop_resize_cubic_rot_kernel<T, ACT, false>,
                       tile_grid(g.W, g.H, c.B), lds, 0, stream, c.src, c.dst, (T*)c.act, a, c.Cpad, k.m[0], k.m[1], k.m[2],
                       k.s[0], k.s[1], k.s[2]);
}

// every frame's rotation: null, or no rotation (a table that would scale)
static int frame_rot_check(const char* op, const int32_t* rot, int B) {
  D3F_CHECK(rot != nullptr, "%s: null rot (host memory [B][2]: c16, s16 per frame)", op);
  for (int b = 0; b < B; ++b) {
    const long c = rot[2L * b], s = rot[2L * b + 1];
    const bool small = labs64(c) <= 2 * ROT_ONE && labs64(s) <= 2 * ROT_ONE;
    D3F_CHECK(small && labs64(c * c + s * s - (1L << 32)) <= (1L << 17),
              "%s: frame %d: rot (c16 %ld, s16 %ld) is no rotation: c16^2 + s16^2 lies further than 2^17 from 2^32 (such a "
              "table would scale)", op, b, c, s);
  }
  return 0;
}

// the paste of a rotated box: tiles on the FRAME's 32 x 8 grid, as the plain form's.  A tile that misses the rectangle's
// bounding box is a copy (out == frame: not launched); inside it a pixel belongs to the box when its centre lies in the
// rotated rectangle, and every other pixel is the frame's
struct RotPasteGeom {
  int H, W;
  long patch_row_stride;
  int src_h, src_w, feather;
  int pitch, rows_max;
};
template <bool COLOR>
struct RotPasteArgs {
  RotPasteGeom g;
  FrameRBoxes t;
};
template <>
struct RotPasteArgs<true> {
  RotPasteGeom g;
  FrameRBoxes t;
  const float* coef;
};

template <bool STAGED, bool COLOR>
__global__ __launch_bounds__(RESIZE_TW * RESIZE_TH) void paste_resize_cubic_rot_kernel(const uint8_t* __restrict__ patch,
                                                                                      const uint8_t* frame, uint8_t* out,
                                                                                      RotPasteArgs<COLOR> args) {
  const int b = blockIdx.z;
  const RotPasteGeom& g = args.g;
  const RotBox r = rot_box(args.t, b);
  const bool in_place = frame == out;
  int bx0, bx1, by0, by1;
  rot_bbox(r, g.src_h, g.src_w, bx0, bx1, by0, by1);
  int tx0 = 0, ty0 = 0;
  if (in_place) {  // (workgroup-uniform) the launch's grid is the most tiles any frame's bounding box meets
    tx0 = bx0 / RESIZE_TW;
    ty0 = by0 / RESIZE_TH;
    if ((int)blockIdx.x > bx1 / RESIZE_TW - tx0 || (int)blockIdx.y > by1 / RESIZE_TH - ty0) return;
  }
  extern __shared__ __attribute__((aligned(16))) uint8_t staged[];
  const int tid = threadIdx.x;
  const int ox0 = ((int)blockIdx.x + tx0) * RESIZE_TW, oy0 = ((int)blockIdx.y + ty0) * RESIZE_TH;
  const long frame_bytes = (long)g.src_h * g.src_w * 3, row_bytes = (long)g.src_w * 3;
  const uint8_t* f = frame + b * frame_bytes;
  uint8_t* o = out + b * frame_bytes;
  const int tile_w = min(RESIZE_TW, g.src_w - ox0), tile_h = min(RESIZE_TH, g.src_h - oy0);
  const int lx = tid % RESIZE_TW, ly = tid / RESIZE_TW;
  if (ox0 > bx1 || ox0 + tile_w - 1 < bx0 || oy0 > by1 || oy0 + tile_h - 1 < by0) {  // (workgroup-uniform) a copy
    if (in_place || ly >= tile_h) return;
    const long at = (long)(oy0 + ly) * row_bytes + (long)ox0 * 3;
    frame_tile_row_copy(f + at, o + at, tile_w, lx);
    return;
  }
  const uint8_t* img = patch + (long)b * g.H * g.patch_row_stride;
  const ResizeSrc rs = {img, g.patch_row_stride, g.H, g.W, r.ch, r.cw, g.pitch};
  // the patch position of frame pixel (x, y): taps clamp inside the patch
  auto pos = [&](int x, int y, long& px, long& py) {
    long nj, ni;
    rot_local(r, x, y, nj, ni);
    px = rot_patch_pos(nj, r.cw, g.W);
    py = rot_patch_pos(ni, r.ch, g.H);
  };
  ResizeTile t;
  if (STAGED) {
    const uint8_t* hi = patch + ((long)gridDim.z * g.H - 1) * g.patch_row_stride + (long)g.W * 3;
    t = rot_stage(staged, rs, g.rows_max, pos, ox0, ox0 + tile_w - 1, oy0, oy0 + tile_h - 1, patch, hi, tid);
    __syncthreads();
  }
  if (lx >= tile_w || ly >= tile_h) return;
  const long at = (long)(oy0 + ly) * row_bytes + (long)(ox0 + lx) * 3;
  long nj, ni;
  rot_local(r, ox0 + lx, oy0 + ly, nj, ni);
  if (!rot_inside(nj, r.cw) || !rot_inside(ni, r.ch)) {  // a pixel of the tile outside the rectangle
    if (!in_place) {
      const uint8_t q0 = f[at], q1 = f[at + 1], q2 = f[at + 2];
      o[at] = q0;
      o[at + 1] = q1;
      o[at + 2] = q2;
    }
    return;
  }
  float v[3];
  rot_value<STAGED>(staged, rs, t, rot_patch_pos(nj, r.cw, g.W), rot_patch_pos(ni, r.ch, g.H), v);
  const float ay = rot_ramp(ni, r.ch, g.feather), ax = rot_ramp(nj, r.cw, g.feather);
  paste_blend<COLOR>(v, ay * ax, f + at, o + at, args, b);
}

// one launch of the rotated paste: a chunk of at most FRAME_BOXES_MAX frames (c: its frames; its boxes and rotations from b0)
template <bool COLOR>
static int rot_paste_launch_one(const PasteCall& c, int b0, hipStream_t stream) {
  RotPasteArgs<COLOR> args;
  RotPasteGeom& g = args.g;
  g = RotPasteGeom{c.H, c.W, c.patch_row_stride, c.src_h, c.src_w, c.feather, 0, 0};
  if constexpr (COLOR) args.coef = c.coef;
  fill_frame_rboxes(args.t, c.boxes, c.rot, b0, c.B);
  PatchExtent e;
  InPlaceTiles tiles{RESIZE_TW, RESIZE_TH};  // in place: the most tiles any frame's bounding box meets
  for (int i = 0; i < c.B; ++i) {
    const FrameBox& bx = args.t.box[i];
    // a tile's footprint in the box: 31 and 7 frame pixels, turned; in the patch: times W / cw and H / ch
    const long ac = labs64(args.t.rot[i].c16), as = labs64(args.t.rot[i].s16);
    const long xext = (ac * (RESIZE_TW - 1) + as * (RESIZE_TH - 1)) * g.W / (ROT_ONE * bx.cw);
    const long yext = (as * (RESIZE_TW - 1) + ac * (RESIZE_TH - 1)) * g.H / (ROT_ONE * bx.ch);
    e.cover(rot_patch_extent(xext, yext, g.H, g.W));
    int bx0, bx1, by0, by1;
    rot_bbox(RotBox{bx.x1, bx.y1, bx.cw, bx.ch, args.t.rot[i].c16, args.t.rot[i].s16}, g.src_h, g.src_w, bx0, bx1, by0, by1);
    tiles.cover(bx0, bx1, by0, by1);
  }
  const long lds = e.lds_bytes(&g.pitch);
  g.rows_max = (int)e.rows;
  dim3 grid = tile_grid(g.src_w, g.src_h, c.B);
  if (c.frame == c.out) {  // (the kernel derives each frame's first tile)
    grid.x = tiles.nx;
    grid.y = tiles.ny;
  }
  return launch_staged(paste_resize_cubic_rot_kernel<true, COLOR>, paste_resize_cubic_rot_kernel<false, COLOR>, grid, lds, 0,
                       stream, c.patch, c.frame, c.out, args);
}

// ---- the entry points: one check and one launch sequence for every form of the crop, and of the paste ----
// A per-frame form is checked as the single-box call with a box every frame has (so that everything that is not the box is
// refused in the single-box operator's words), then every frame's box, then every frame's rotation.
int crop_resize_check(const CropCall& c) {
  const bool one = c.form == FRAME_BOX_ONE;
  const char* op = crop_op(c);
  const int x1 = one ? c.x1 : 0, y1 = one ? c.y1 : 0, cw = one ? c.cw : 1, ch = one ? c.ch : 1;
  D3F_CHECK(c.B >= 0 && c.src_h > 0 && c.src_w > 0 && cw > 0 && ch > 0 && c.H > 0 && c.W > 0,
            "crop_resize_cubic: non-positive size (B %d, frame %dx%d, crop %dx%d, output %dx%d)", c.B, c.src_h, c.src_w, ch, cw,
            c.H, c.W);
  D3F_CHECK(x1 >= 0 && y1 >= 0 && (long)x1 + cw <= c.src_w && (long)y1 + ch <= c.src_h,
            "crop_resize_cubic: crop box (x1 %d, y1 %d, %d x %d) outside the %d x %d frame", x1, y1, cw, ch, c.src_w, c.src_h);
  D3F_CHECK(c.src_h <= RESIZE_MAX_EXTENT && c.src_w <= RESIZE_MAX_EXTENT && c.H <= RESIZE_MAX_EXTENT && c.W <= RESIZE_MAX_EXTENT,
            "crop_resize_cubic: extents up to %d (32-bit source coordinates)", RESIZE_MAX_EXTENT);
  D3F_CHECK(c.B <= 65535, "crop_resize_cubic: at most 65535 frames per call (B %d)", c.B);
  D3F_CHECK(c.dst_row_stride >= 3L * c.W, "crop_resize_cubic: output row stride %ld below 3 * W = %ld bytes", c.dst_row_stride,
            3L * c.W);
  if (c.antialias && one) {
    D3F_CHECK((long)cw <= (long)AA_MAX_RATIO * c.W && (long)ch <= (long)AA_MAX_RATIO * c.H,
              "crop_resize_cubic_aa: crop %d x %d above %d times the output %d x %d on an axis (at most %d taps per axis)", cw,
              ch, AA_MAX_RATIO, c.W, c.H, 4 * AA_MAX_RATIO + 1);
    AaGeom g = {};
    g.H = c.H;
    g.W = c.W;
    aa_strides(g, cw, ch);
    D3F_CHECK(aa_lds_bytes(g) <= (size_t)AA_LDS_LIMIT, "crop_resize_cubic_aa: %zu bytes of LDS", aa_lds_bytes(g));
  }
  if (!one)
    if (int rc = frame_boxes_check(op, c.boxes, c.B, c.src_h, c.src_w, c.antialias ? c.H : 0, c.antialias ? c.W : 0)) return rc;
  if (c.form == FRAME_BOX_ROTATED) {
    if (int rc = frame_rot_check(op, c.rot, c.B)) return rc;
    D3F_CHECK(!c.antialias, "%s: the rotated crop has no antialiased form", op);
  }
  D3F_CHECK(!c.act || c.Cpad >= 3, "%s: activation of %d channels", op, c.Cpad);
  return 0;
}

int crop_resize_launch(const CropCall& c, hipStream_t stream) {
  if (int rc = crop_resize_check(c)) return rc;
  const bool one = c.form == FRAME_BOX_ONE;
  const Norm255 k(c.mean255, c.std255);
  const long frame_bytes = (long)c.src_h * c.src_w * 3, out_bytes = (long)c.H * c.dst_row_stride;
  // dtype -> T and act -> ACT as types, then the form's launch for every chunk
  auto go = [&](auto* type, auto ACT) {
    using T = std::remove_pointer_t<decltype(type)>;
    constexpr bool A = decltype(ACT)::value;
    int (*launch_one)(const CropCall&, int, const Norm255&, hipStream_t) =
        c.form == FRAME_BOX_ROTATED ? rot_crop_launch_one<T, A>
        : c.antialias               ? (one ? aa_launch_one<T, A, false> : aa_launch_one<T, A, true>)
                                    : (one ? resize_launch_one<T, A, false> : resize_launch_one<T, A, true>);
    return for_frame_chunks(
        c.B, one ? c.B : FRAME_BOXES_MAX,
        [&](int b0, int n, const uint8_t* src, uint8_t* dst, T* act) {
          CropCall chunk = c;
          chunk.B = n;
          chunk.src = src;
          chunk.dst = dst;
          chunk.act = act;
          return launch_one(chunk, b0, k, stream);
        },
        FramePtr<const uint8_t>{c.src, frame_bytes}, FramePtr<uint8_t>{c.dst, out_bytes},
        FramePtr<T>{(T*)c.act, (long)c.H * c.W * c.Cpad});
  };
  if (!c.act) return go((float*)nullptr, std::false_type{});
  if (c.dtype == D3F_F32) return go((float*)nullptr, std::true_type{});
  return go((bf16_t*)nullptr, std::true_type{});
}

static const char* paste_op(const PasteCall& c) {
  if (c.form == FRAME_BOX_ROTATED) return c.color ? "paste_resize_cubic_color_rboxes" : "paste_resize_cubic_rboxes";
  if (c.form == FRAME_BOX_PER_FRAME) return c.color ? "paste_resize_cubic_color_boxes" : "paste_resize_cubic_boxes";
  return c.color ? "paste_resize_cubic_color" : "paste_resize_cubic";
}

int paste_resize_check(const PasteCall& c) {
  const bool one = c.form == FRAME_BOX_ONE;
  const char* op = paste_op(c);
  const int x1 = one ? c.x1 : 0, y1 = one ? c.y1 : 0, cw = one ? c.cw : 1, ch = one ? c.ch : 1;
  D3F_CHECK(c.B >= 0 && c.B <= 65535, "paste_resize_cubic: B %d outside 0..65535 frames per call", c.B);
  D3F_CHECK(c.src_h > 0 && c.src_w > 0 && cw > 0 && ch > 0 && c.H > 0 && c.W > 0,
            "paste_resize_cubic: non-positive size (frame %dx%d, box %dx%d, patch %dx%d)", c.src_h, c.src_w, ch, cw, c.H, c.W);
  D3F_CHECK(x1 >= 0 && y1 >= 0 && (long)x1 + cw <= c.src_w && (long)y1 + ch <= c.src_h,
            "paste_resize_cubic: box (x1 %d, y1 %d, %d x %d) outside the %d x %d frame", x1, y1, cw, ch, c.src_w, c.src_h);
  D3F_CHECK(c.src_h <= RESIZE_MAX_EXTENT && c.src_w <= RESIZE_MAX_EXTENT && c.H <= RESIZE_MAX_EXTENT && c.W <= RESIZE_MAX_EXTENT,
            "paste_resize_cubic: extents up to %d (32-bit source coordinates)", RESIZE_MAX_EXTENT);
  D3F_CHECK(c.feather >= 0 && c.feather <= RESIZE_MAX_EXTENT, "paste_resize_cubic: feather %d outside 0..%d", c.feather,
            RESIZE_MAX_EXTENT);
  D3F_CHECK(c.patch_row_stride >= 3L * c.W, "paste_resize_cubic: patch row stride %ld below 3 * W = %ld bytes",
            c.patch_row_stride, 3L * c.W);
  const long bytes = (long)c.B * c.src_h * c.src_w * 3;
  D3F_CHECK(c.frame == c.out || c.out + bytes <= c.frame || c.frame + bytes <= c.out,
            "paste_resize_cubic: frame and out overlap in part (out == frame runs in place)");
  // other workgroups write out while a tile stages its part of the patch: the patches' bytes must lie outside out
  const long patch_bytes = c.B > 0 ? ((long)c.B * c.H - 1) * c.patch_row_stride + 3L * c.W : 0;
  D3F_CHECK(patch_bytes == 0 || c.patch + patch_bytes <= c.out || c.out + bytes <= c.patch,
            "paste_resize_cubic: patch overlaps out");
  if (c.color) {
    D3F_CHECK(c.coef != nullptr, "paste_resize_cubic_color: null coef");
    // a tile reads its frame's coefficients while other tiles write out
    const long coef_bytes = (long)c.B * 6 * sizeof(float);
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(c.coef);
    D3F_CHECK(cb + coef_bytes <= c.out || c.out + bytes <= cb, "paste_resize_cubic_color: coef overlaps out");
  }
  if (!one)
    if (int rc = frame_boxes_check(op, c.boxes, c.B, c.src_h, c.src_w)) return rc;
  if (c.form == FRAME_BOX_ROTATED) return frame_rot_check(op, c.rot, c.B);
  return 0;
}

int paste_resize_launch(const PasteCall& c, hipStream_t stream) {
  if (int rc = paste_resize_check(c)) return rc;
  const bool one = c.form == FRAME_BOX_ONE;
  const long frame_bytes = (long)c.src_h * c.src_w * 3, patch_bytes = (long)c.H * c.patch_row_stride;
  return paste_forms(c, [&](auto COLOR, auto BOXES) {
    constexpr bool C = decltype(COLOR)::value, BX = decltype(BOXES)::value;
    int (*launch_one)(const PasteCall&, int, hipStream_t) =
        c.form == FRAME_BOX_ROTATED ? rot_paste_launch_one<C> : paste_launch_one<C, BX>;
    return for_frame_chunks(
        c.B, one ? c.B : FRAME_BOXES_MAX,
        [&](int b0, int n, const uint8_t* patch, const uint8_t* frame, uint8_t* out, const float* coef) {
          return launch_one(paste_chunk(c, n, patch, frame, out, coef), b0, stream);
        },
        FramePtr<const uint8_t>{c.patch, patch_bytes}, FramePtr<const uint8_t>{c.frame, frame_bytes},
        FramePtr<uint8_t>{c.out, frame_bytes}, FramePtr<const float>{C ? c.coef : nullptr, 6});
  });
}


}  // namespace d3f
