// Training image grids (d3f/train_deep_fake/lit_module.py:235-249, d3f/train_denoiser/lit_module.py:157-171,
// d3f/balance_training_images/lit_module.py:197-211): torchvision.utils.make_grid(batch[:images], nrow, padding,
// pad_value), the whole grid scaled (* scale + shift, clamp to 0..1) and TensorBoard's uint8 conversion (* 255,
// truncated) -- up to 8 fp32 NCHW batches of one shape in, 8 finished uint8 HWC grid images out, one launch.
//
// Definition (the acceptance contract; tests/image_grid_restatement.py restates it with torch ops):
//   * xmaps = min(nrow, images), ymaps = ceil(images / xmaps); a cell is (H + padding) x (W + padding); the grid is
//     (ymaps * (H + padding) + padding) x (xmaps * (W + padding) + padding); image k sits at row
//     (k / xmaps) * (H + padding) + padding, column (k % xmaps) * (W + padding) + padding; every other pixel -- borders and
//     the blank cells of a ragged last row -- is pad_value; images == 1 is the bare image (no border); C == 1 is
//     replicated to three channels;
//   * byte = (uint8_t)(clamp(v * scale + shift, 0, 1) * 255.0f): fp32, the product and the sum rounded separately
//     (-ffp-contract=off), NaN -> 0, truncation.  The padding takes the same route (pad 0 at scale = shift = 0.5: 127).
//
// Form: pure streaming, no reuse, no LDS.  One lane makes four consecutive pixels of one output row = 12 bytes.  The
// groups of a row start where its bytes are dword aligned (3 s = -row_start mod 4 has the solution s = row_start mod 4
// pixels), so that every whole group is three aligned dword stores whatever GW * 3 is; the at most three pixels in front
// of the first whole group and behind the last are stored byte by byte.  A group that lies inside one image row reads one
// 16-byte vector per colour plane (planes are only 4-byte aligned in general: H * W is not a multiple of 4); a group that
// touches a cell edge takes its pixels one at a time.
#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int GRID_MAX_BATCHES = 8;
constexpr int GRID_MAX_PADDING = 64;
constexpr int GRID_MAX_EXTENT = 16384;
constexpr int GRID_THREADS = 256;

struct GridParams {
  const float* batch[GRID_MAX_BATCHES];
  int n, C, H, W, images, xmaps, pad;  // pad: 0 when images == 1
  int cellH, cellW, GH, GW;
  int groups;  // lanes per output row: ceil((GW + 3) / 4), the leading partial group included
  int total;   // n * GH * groups
  float pad_value, scale, shift;
  unsigned div_groups_mul, div_groups_shr, div_gh_mul, div_gh_shr, div_cellh_mul, div_cellh_shr, div_cellw_mul,
      div_cellw_shr;
};

typedef float grid_f4 __attribute__((ext_vector_type(4), aligned(4)));  // a 16-byte load from a 4-byte aligned address

__device__ __forceinline__ uint32_t grid_byte(float v, float scale, float shift) {
  float t = v * scale;
  t = t + shift;
  t = fminf(fmaxf(t, 0.f), 1.f);  // NaN -> 0
  return (uint32_t)(uint8_t)(t * 255.0f);
}

__global__ __launch_bounds__(GRID_THREADS) void image_grid_u8_kernel(GridParams g, uint8_t* __restrict__ out) {
  const int idx = blockIdx.x * GRID_THREADS + threadIdx.x;
  if (idx >= g.total) return;
  const int row = fast_div(idx, g.div_groups_mul, g.div_groups_shr), i = idx - row * g.groups;
  const int t = fast_div(row, g.div_gh_mul, g.div_gh_shr), gy = row - t * g.GH;
  uint8_t* orow = out + (long)row * g.GW * 3;
  const int lead = (int)(reinterpret_cast<uintptr_t>(orow) & 3);  // pixels in front of the first whole group: r + 3 r = 4 r
  const int p0 = 4 * i - ((4 - lead) & 3);
  if (p0 >= g.GW) return;
  const uint32_t padb = grid_byte(g.pad_value, g.scale, g.shift);

  // the row of the grid: an image row iy of cell row cy, or padding
  const int yy = gy - g.pad;
  int cy = 0, iy = 0;
  bool img_row = yy >= 0;
  if (img_row) {
    cy = fast_div(yy, g.div_cellh_mul, g.div_cellh_shr);
    iy = yy - cy * g.cellH;
    img_row = iy < g.H;
  }
  const float* __restrict__ src = g.batch[t];
  const long plane = (long)g.H * g.W, cstep = g.C == 1 ? 0 : plane;

  uint32_t px[4][3];
  bool whole = false;
  if (img_row && p0 >= g.pad && p0 + 4 <= g.GW) {
    const int xx = p0 - g.pad, cx = fast_div(xx, g.div_cellw_mul, g.div_cellw_shr), ix = xx - cx * g.cellW;
    const int k = cy * g.xmaps + cx;
    if (ix + 4 <= g.W && k < g.images) {  // four pixels of one image row: one 16-byte load per plane
      whole = true;
      const float* p = src + (long)k * g.C * plane + (long)iy * g.W + ix;
      for (int c = 0; c < 3; ++c) {
        const grid_f4 v = *reinterpret_cast<const grid_f4*>(p + c * cstep);
        px[0][c] = grid_byte(v.x, g.scale, g.shift);
        px[1][c] = grid_byte(v.y, g.scale, g.shift);
        px[2][c] = grid_byte(v.z, g.scale, g.shift);
        px[3][c] = grid_byte(v.w, g.scale, g.shift);
      }
    }
  }
  if (!whole) {  // a cell edge, padding, or the ends of the row: pixel by pixel
    for (int j = 0; j < 4; ++j) {
      px[j][0] = px[j][1] = px[j][2] = padb;
      const int xx = p0 + j - g.pad;
      if (!img_row || xx < 0 || p0 + j >= g.GW) continue;
      const int cx = fast_div(xx, g.div_cellw_mul, g.div_cellw_shr), ix = xx - cx * g.cellW;
      const int k = cy * g.xmaps + cx;
      if (ix >= g.W || cx >= g.xmaps || k >= g.images) continue;
      const float* p = src + (long)k * g.C * plane + (long)iy * g.W + ix;
      for (int c = 0; c < 3; ++c) px[j][c] = grid_byte(p[c * cstep], g.scale, g.shift);
    }
  }
  if (p0 >= 0 && p0 + 4 <= g.GW) {  // a whole group: 12 bytes from a dword-aligned address
    uint32_t* o = reinterpret_cast<uint32_t*>(orow + (long)p0 * 3);
    o[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
    o[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
    o[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
  } else {
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + j;
      if (p < 0 || p >= g.GW) continue;
      uint8_t* o = orow + (long)p * 3;
      o[0] = (uint8_t)px[j][0];
      o[1] = (uint8_t)px[j][1];
      o[2] = (uint8_t)px[j][2];
    }
  }
}

// layout of the grid: xmaps, the padding in effect and {GH, GW} (all refusals that do not need the batch)
static int grid_layout(int images, int nrow, int padding, int H, int W, int& xmaps, int& pad, long& GH, long& GW) {
  D3F_CHECK(images >= 1, "image_grid: %d images (at least 1)", images);
  D3F_CHECK(nrow >= 1, "image_grid: nrow %d (at least 1)", nrow);
  D3F_CHECK(padding >= 0 && padding <= GRID_MAX_PADDING, "image_grid: padding %d outside 0..%d", padding, GRID_MAX_PADDING);
  D3F_CHECK(H >= 1 && W >= 1 && H <= GRID_MAX_EXTENT && W <= GRID_MAX_EXTENT,
            "image_grid: image extent %d x %d outside 1..%d", H, W, GRID_MAX_EXTENT);
  xmaps = nrow < images ? nrow : images;
  const long ymaps = ((long)images + xmaps - 1) / xmaps;
  pad = images == 1 ? 0 : padding;  // make_grid returns a single image as it is
  GH = ymaps * (H + pad) + pad;
  GW = (long)xmaps * (W + pad) + pad;
  D3F_CHECK(GH * GW * 3 < (1L << 31), "image_grid: a grid of %ld x %ld pixels is 2^31 bytes or more", GH, GW);
  return 0;
}

int image_grid_shape(int images, int nrow, int padding, int H, int W, int32_t dims[2]) {
  int xmaps, pad;
  long GH, GW;
  if (int rc = grid_layout(images, nrow, padding, H, W, xmaps, pad, GH, GW)) return rc;
  dims[0] = (int32_t)GH;
  dims[1] = (int32_t)GW;
  return 0;
}

int image_grid_u8_launch(const float* const* batches, int n, int B, int C, int H, int W, int images, int nrow, int padding,
                         float pad_value, float scale, float shift, uint8_t* out, hipStream_t stream) {
  D3F_CHECK(n >= 1 && n <= GRID_MAX_BATCHES, "image_grid_u8: %d batches outside 1..%d", n, GRID_MAX_BATCHES);
  D3F_CHECK(B >= 1 && images >= 1 && images <= B, "image_grid_u8: %d images outside 1..B = %d", images, B);
  D3F_CHECK(C == 1 || C == 3, "image_grid_u8: %d channels (1 or 3)", C);
  GridParams g{};
  long GH, GW;
  if (int rc = grid_layout(images, nrow, padding, H, W, g.xmaps, g.pad, GH, GW)) return rc;
  D3F_CHECK(n * GH * GW * 3 < (1L << 31), "image_grid_u8: an output of %d x %ld x %ld x 3 is 2^31 bytes or more", n, GH, GW);
  for (int i = 0; i < n; ++i) {
    D3F_CHECK(batches[i] != nullptr, "image_grid_u8: batch %d is null", i);
    g.batch[i] = batches[i];
  }
  g.n = n, g.C = C, g.H = H, g.W = W, g.images = images;
  g.cellH = H + g.pad, g.cellW = W + g.pad, g.GH = (int)GH, g.GW = (int)GW;
  g.groups = (g.GW + 3 + 3) / 4;
  g.total = n * g.GH * g.groups;  // < n * GH * (GW * 3) < 2^31
  g.pad_value = pad_value, g.scale = scale, g.shift = shift;
  fast_div_setup((unsigned)g.groups, &g.div_groups_mul, &g.div_groups_shr);
  fast_div_setup((unsigned)g.GH, &g.div_gh_mul, &g.div_gh_shr);
  fast_div_setup((unsigned)g.cellH, &g.div_cellh_mul, &g.div_cellh_shr);
  fast_div_setup((unsigned)g.cellW, &g.div_cellw_mul, &g.div_cellw_shr);
  hipLaunchKernelGGL(image_grid_u8_kernel, dim3(cdiv(g.total, GRID_THREADS)), dim3(GRID_THREADS), 0, stream, g, out);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
