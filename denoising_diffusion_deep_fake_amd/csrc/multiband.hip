// Multiband paste (Burt & Adelson) of the full-frame output: include/d3f_hip.h: d3f_paste_multiband_u8 is the definition,
// tests/multiband_restatement.py restates it in numpy integers, DESIGN.md section 4 "Multiband paste" explains it.
//
// The pyramid is built on the DIFFERENCE image D = V - s (V: the plain paste's byte at feather 0, s: the frame's byte), per
// frame and byte-in-pixel, in integers: g_0 = D << 6 in int16, REDUCE with the 5 x 5 binomial kernel, EXPAND with its
// polyphase halves, every Laplacian band faded by the separable ramp of ITS level, the bands collapsed in int32.  2N + 1
// launches for N levels:
//   * multiband_diff_kernel (resize.hip, where the paste's arithmetic lives): g_0;
//   * multiband_reduce_kernel, N times: g_{l+1} from g_l;
//   * multiband_collapse_kernel, N - 1 times, l = N - 1 .. 1: R_l = EXPAND(R_{l+1}) + m_l(g_l - EXPAND(g_{l+1})), both EXPANDs
//     from one staged coarse tile; R_N = m_N(g_N) is formed while g_N is staged (TOP), so no launch writes it;
//   * multiband_final_kernel: level 0 of the collapse, (R_0 + 32) >> 6 added to the frame's byte, and the tiles outside the
//     box copied as the plain paste copies them.
// The planes are planar -- one slab per frame and byte-in-pixel (pointwise.h: MultibandPlan) -- so that every pyramid
// kernel is a one-channel 2-D filter whose rows start on 16 bytes: gridDim.z = frames * 3, 64 x 16 output tiles, a lane
// takes four adjacent columns and moves them as one vector (8 bytes of int16, 16 of int32); the input tile with its halo
// is staged in LDS with 16-byte loads.  Indices are clamped where a tile is STAGED; the filters then read LDS unclamped.
// A vector may reach past a row's last sample into the row's padding: what is read there is never used (a clamped index
// never points at it), what is written there is never read.
#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int MB_TW = 64, MB_TH = 16, MB_THREADS = 256;  // the pyramid kernels' output tile; MB_THREADS lanes x 4 columns
constexpr int MB_FRAMES_MAX = 16384;                     // per launch of the single-box form: gridDim.z = 3 * frames

struct MbGeom {
  int src_h, src_w, x1, y1, cw, ch;
  int tx0, ty0;  // the final kernel in place: the first frame tile that meets the box
};

// extent of level l of an axis of n samples: l times (n + 1) / 2
__host__ __device__ __forceinline__ int mb_dim(int n, int l) { return (n + (1 << l) - 1) >> l; }
__device__ __forceinline__ int mb_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// n_y(i) of the definition: the ramp's numerator at sample i of an axis of n samples
__device__ __forceinline__ int mb_band_n(int i, int n, int F) { return min(min(i, n - 1 - i) + 1, F + 1); }
// m(x) = floor((2 x M + den) / (2 den)), 0 < M <= den = (F + 1)^2, |x| <= 32640
__device__ __forceinline__ int mb_mask(int x, int M, int den) {
  if (M == den) return x;  // the interior: almost every sample
  if (den <= 16384) {      // (workgroup-uniform) |2 x M| + den < 2^31
    const int num = 2 * x * M + den, d2 = 2 * den;
    int q = num / d2;
    if (num - q * d2 < 0) q -= 1;  // floor division
    return q;
  }
  const long num = 2L * x * M + den, d2 = 2L * den;
  long q = num / d2;
  if (num - q * d2 < 0) q -= 1;
  return (int)q;
}
// EXPAND's weights of output index y over the coarse samples (y >> 1) - 1, (y >> 1), (y >> 1) + 1
__device__ __forceinline__ void mb_expand_w(int y, int w[3]) {
  const bool odd = y & 1;
  w[0] = odd ? 0 : 1;
  w[1] = odd ? 4 : 6;
  w[2] = odd ? 4 : 1;
}

__device__ __forceinline__ int16_t* mb_g(char* ws, const MultibandPlan& p, int z, int l) {
  return reinterpret_cast<int16_t*>(ws + (long)z * p.slab_bytes + p.g_off[l]);
}
__device__ __forceinline__ int* mb_r(char* ws, const MultibandPlan& p, int z, int l) {
  return reinterpret_cast<int*>(ws + (long)z * p.slab_bytes + p.r_off[l]);
}

// ---- REDUCE: g_{l+1}[i][j] = (sum_{a,b} w_a w_b g_l[clamp(2i + a)][clamp(2j + b)] + 128) >> 8, w = 1 4 6 4 1 ----
// The tile's input: rows 2 oy0 - 2 .. 2 oy0 + 2 MB_TH (clamped into the level when staged), columns from xa = 2 ox0 - 8 (a
// vector boundary) to 2 ox0 + 2 MB_TW.  Horizontal pass into int32 in LDS (|sum| <= 16 * 32640), vertical pass from there:
// nothing is rounded between the two.
constexpr int RED_ROWS = 2 * MB_TH + 3, RED_VECS = (2 * MB_TW + 8 + 3 + 7) / 8, RED_PITCH = RED_VECS * 8;

// BOXES: frame z / 3 takes its own box; the grid is the largest box's and a frame's workgroups past its own level return
template <bool BOXES>
__global__ __launch_bounds__(MB_THREADS) void multiband_reduce_kernel(char* __restrict__ ws, MultibandPlan p,
                                                                      BoxedGeom<MbGeom, BOXES> geo, int l) {
  __shared__ __attribute__((aligned(16))) int16_t tile[RED_ROWS * RED_PITCH];
  __shared__ __attribute__((aligned(16))) int hbuf[RED_ROWS * MB_TW];
  const int z = blockIdx.z, tid = threadIdx.x;
  const MbGeom g = frame_geom(geo, z / 3);
  const int w = mb_dim(g.cw, l), h = mb_dim(g.ch, l), wo = mb_dim(g.cw, l + 1), ho = mb_dim(g.ch, l + 1);
  const int ox0 = blockIdx.x * MB_TW, oy0 = blockIdx.y * MB_TH;
  if (ox0 >= wo || oy0 >= ho) return;  // (workgroup-uniform)
  const int16_t* in = mb_g(ws, p, z, l);
  const int pin = p.pitch[l], xa = 2 * ox0 - 8;
  for (int i = tid; i < RED_ROWS * RED_VECS; i += MB_THREADS) {
    const int r = i / RED_VECS, k = i - r * RED_VECS;
    const int x = xa + 8 * k, y = mb_clamp(2 * oy0 - 2 + r, h - 1);
    if (x < 0 || x >= pin) continue;  // no sample of the level in this vector
    *reinterpret_cast<int4*>(tile + r * RED_PITCH + 8 * k) = *reinterpret_cast<const int4*>(in + (long)y * pin + x);
  }
  __syncthreads();
  for (int i = tid; i < RED_ROWS * MB_TW; i += MB_THREADS) {
    const int r = i / MB_TW, c = i - r * MB_TW;
    const int16_t* row = tile + r * RED_PITCH - xa;
    const int x = 2 * (ox0 + c);
    // (a column past the level's last output reads clamped samples and is not stored)
    hbuf[i] = (int)row[mb_clamp(x - 2, w - 1)] + 4 * (int)row[mb_clamp(x - 1, w - 1)] + 6 * (int)row[mb_clamp(x, w - 1)] +
              4 * (int)row[mb_clamp(x + 1, w - 1)] + (int)row[mb_clamp(x + 2, w - 1)];
  }
  __syncthreads();
  const int ty = tid / (MB_TW / 4), tx = (tid % (MB_TW / 4)) * 4;
  const int oy = oy0 + ty, ox = ox0 + tx;
  if (oy >= ho || ox >= wo) return;
  const int* col = hbuf + 2 * ty * MB_TW + tx;  // row 2 ty of the tile is input row 2 oy - 2
  int4 s = *reinterpret_cast<const int4*>(col);
  const int4 s1 = *reinterpret_cast<const int4*>(col + MB_TW), s2 = *reinterpret_cast<const int4*>(col + 2 * MB_TW);
  const int4 s3 = *reinterpret_cast<const int4*>(col + 3 * MB_TW), s4 = *reinterpret_cast<const int4*>(col + 4 * MB_TW);
  s.x = (s.x + 4 * s1.x + 6 * s2.x + 4 * s3.x + s4.x + 128) >> 8;
  s.y = (s.y + 4 * s1.y + 6 * s2.y + 4 * s3.y + s4.y + 128) >> 8;
  s.z = (s.z + 4 * s1.z + 6 * s2.z + 4 * s3.z + s4.z + 128) >> 8;
  s.w = (s.w + 4 * s1.w + 6 * s2.w + 4 * s3.w + s4.w + 128) >> 8;
  short4 o;
  o.x = (short)s.x;
  o.y = (short)s.y;
  o.z = (short)s.z;
  o.w = (short)s.w;
  *reinterpret_cast<short4*>(mb_g(ws, p, z, l + 1) + (long)oy * p.pitch[l + 1] + ox) = o;
}

// ---- the coarse tile of a collapse step ----
// What EXPAND to the fine samples rows [fy0, fy0 + fh), columns [fx0, fx0 + fw) (fy0, fx0 even) reads of level lc:
// rows fy0 / 2 - 1 .. and columns fx0 / 2 - 1 .., `rows` x `cols` of them, clamped into the level here.  cg gets g_lc, cr
// gets R_lc -- or, TOP, m_lc(g_lc): the collapse's start at the coarsest level.
template <bool TOP>
__device__ __forceinline__ void mb_stage_coarse(int* cg, int* cr, int rows, int cols, int stride, const int16_t* gc,
                                                const int* rc, int pitch, int hc, int wc, int ky0, int kx0, int F, int tid,
                                                int nthreads) {
  const int den = (F + 1) * (F + 1);
  for (int i = tid; i < rows * cols; i += nthreads) {
    const int r = i / cols, c = i - r * cols;
    const int y = mb_clamp(ky0 + r, hc - 1), x = mb_clamp(kx0 + c, wc - 1);
    const int v = gc[(long)y * pitch + x];
    cg[r * stride + c] = v;
    cr[r * stride + c] = TOP ? mb_mask(v, mb_band_n(y, hc, F) * mb_band_n(x, wc, F), den) : rc[(long)y * pitch + x];
  }
}

// EXPAND of both coarse planes at fine sample (y, x): t points at the staged sample of coarse (y >> 1, x >> 1)
__device__ __forceinline__ void mb_expand2(const int* tg, const int* tr, int stride, const int wy[3], const int wx[3],
                                           int* eg, int* er) {
  int sg = 0, sr = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const int wgt = wy[a] * wx[b], at = (a - 1) * stride + (b - 1);
      sg += wgt * tg[at];
      sr += wgt * tr[at];
    }
  *eg = (sg + 32) >> 6;
  *er = (sr + 32) >> 6;
}

// ---- collapse, levels N - 1 .. 1: R_l = EXPAND(R_{l+1}) + m_l(g_l - EXPAND(g_{l+1})) ----
constexpr int COL_ROWS = MB_TH / 2 + 2, COL_COLS = MB_TW / 2 + 2;

template <bool TOP, bool BOXES>
__global__ __launch_bounds__(MB_THREADS) void multiband_collapse_kernel(char* __restrict__ ws, MultibandPlan p,
                                                                        BoxedGeom<MbGeom, BOXES> geo, int l) {
  __shared__ int cg[COL_ROWS * COL_COLS], cr[COL_ROWS * COL_COLS];
  const int z = blockIdx.z, tid = threadIdx.x;
  const MbGeom g = frame_geom(geo, z / 3);
  const int w = mb_dim(g.cw, l), h = mb_dim(g.ch, l), wc = mb_dim(g.cw, l + 1), hc = mb_dim(g.ch, l + 1);
  const int ox0 = blockIdx.x * MB_TW, oy0 = blockIdx.y * MB_TH;
  if (ox0 >= w || oy0 >= h) return;  // (workgroup-uniform)
  mb_stage_coarse<TOP>(cg, cr, COL_ROWS, COL_COLS, COL_COLS, mb_g(ws, p, z, l + 1), TOP ? nullptr : mb_r(ws, p, z, l + 1),
                       p.pitch[l + 1], hc, wc, oy0 / 2 - 1, ox0 / 2 - 1, p.F, tid, MB_THREADS);
  __syncthreads();
  const int ty = tid / (MB_TW / 4), tx = (tid % (MB_TW / 4)) * 4;
  const int y = oy0 + ty, x4 = ox0 + tx;
  if (y >= h || x4 >= w) return;
  const long at = (long)y * p.pitch[l] + x4;
  const short4 fine = *reinterpret_cast<const short4*>(mb_g(ws, p, z, l) + at);
  const int fv[4] = {fine.x, fine.y, fine.z, fine.w};
  const int den = (p.F + 1) * (p.F + 1), ny = mb_band_n(y, h, p.F);
  int wy[3], out[4];
  mb_expand_w(y, wy);
  for (int j = 0; j < 4; ++j) {
    const int x = x4 + j;
    if (x >= w) {  // the row's padding
      out[j] = 0;
      continue;
    }
    int wx[3], eg, er;
    mb_expand_w(x, wx);
    const int at_c = ((y >> 1) - (oy0 >> 1) + 1) * COL_COLS + (x >> 1) - (ox0 >> 1) + 1;
    mb_expand2(cg + at_c, cr + at_c, COL_COLS, wy, wx, &eg, &er);
    out[j] = er + mb_mask(fv[j] - eg, ny * mb_band_n(x, w, p.F), den);
  }
  *reinterpret_cast<int4*>(mb_r(ws, p, z, l) + at) = make_int4(out[0], out[1], out[2], out[3]);
}

// ---- the last launch: level 0 of the collapse, onto the frame ----
// Tiles lie on the FRAME's 32 x 8 grid, a lane per pixel, as in paste_resize_cubic_kernel: a tile outside the box is copied,
// out == frame launches only the tiles that meet the box, and a lane reads no frame byte but the three it writes.  A tile
// that meets the box stages, per byte-in-pixel, its samples of g_0 (whole vectors from the vector boundary at or before its
// first column) and the coarse tile of level 1.
constexpr int FIN_TW = 32, FIN_TH = 8;
constexpr int FIN_PITCH = FIN_TW + 8, FIN_VECS = FIN_PITCH / 8;
constexpr int FIN_CROWS = FIN_TH / 2 + 3, FIN_CCOLS = FIN_TW / 2 + 3;

template <bool TOP, bool BOXES>
__global__ __launch_bounds__(FIN_TW * FIN_TH) void multiband_final_kernel(const uint8_t* frame, uint8_t* out,
                                                                          char* __restrict__ ws, MultibandPlan p,
                                                                          BoxedGeom<MbGeom, BOXES> geo) {
  __shared__ __attribute__((aligned(16))) int16_t fine[3 * FIN_TH * FIN_PITCH];
  __shared__ int cg[3 * FIN_CROWS * FIN_CCOLS], cr[3 * FIN_CROWS * FIN_CCOLS];
  const int b = blockIdx.z, tid = threadIdx.x;
  MbGeom g = frame_geom(geo, b);
  const bool in_place = frame == out;
  if constexpr (BOXES) {
    if (in_place) {  // (workgroup-uniform) the grid is the most tiles any frame's box meets
      g.tx0 = g.x1 / FIN_TW;
      g.ty0 = g.y1 / FIN_TH;
      if ((int)blockIdx.x > (g.x1 + g.cw - 1) / FIN_TW - g.tx0 || (int)blockIdx.y > (g.y1 + g.ch - 1) / FIN_TH - g.ty0) return;
    }
  }
  const int ox0 = ((int)blockIdx.x + g.tx0) * FIN_TW, oy0 = ((int)blockIdx.y + g.ty0) * FIN_TH;
  const long frame_bytes = (long)g.src_h * g.src_w * 3, row_bytes = (long)g.src_w * 3;
  const uint8_t* f = frame + b * frame_bytes;
  uint8_t* o = out + b * frame_bytes;
  const int tile_w = min(FIN_TW, g.src_w - ox0), tile_h = min(FIN_TH, g.src_h - oy0);
  // the box pixels of this tile: columns [bx_f, bx_l] and rows [by_f, by_l] of the box
  const int bx_f = max(ox0, g.x1) - g.x1, bx_l = min(ox0 + tile_w, g.x1 + g.cw) - 1 - g.x1;
  const int by_f = max(oy0, g.y1) - g.y1, by_l = min(oy0 + tile_h, g.y1 + g.ch) - 1 - g.y1;
  const int lx = tid % FIN_TW, ly = tid / FIN_TW;
  if (bx_f > bx_l || by_f > by_l) {  // (workgroup-uniform) a tile outside the box: a copy
    if (in_place || ly >= tile_h) return;
    const long at = (long)(oy0 + ly) * row_bytes + (long)ox0 * 3;
    frame_tile_row_copy(f + at, o + at, tile_w, lx);
    return;
  }
  const int xa = bx_f & ~7, w1 = mb_dim(g.cw, 1), h1 = mb_dim(g.ch, 1);
  for (int i = tid; i < 3 * FIN_TH * FIN_VECS; i += FIN_TW * FIN_TH) {
    const int c = i / (FIN_TH * FIN_VECS), r = (i / FIN_VECS) % FIN_TH, k = i % FIN_VECS;
    const int y = by_f + r, x = xa + 8 * k;
    if (y > by_l || x > bx_l) continue;
    *reinterpret_cast<int4*>(fine + (c * FIN_TH + r) * FIN_PITCH + 8 * k) =
        *reinterpret_cast<const int4*>(mb_g(ws, p, b * 3 + c, 0) + (long)y * p.pitch[0] + x);
  }
  for (int c = 0; c < 3; ++c)
    mb_stage_coarse<TOP>(cg + c * FIN_CROWS * FIN_CCOLS, cr + c * FIN_CROWS * FIN_CCOLS, FIN_CROWS, FIN_CCOLS, FIN_CCOLS,
                         mb_g(ws, p, b * 3 + c, 1), TOP ? nullptr : mb_r(ws, p, b * 3 + c, 1), p.pitch[1], h1, w1,
                         (by_f >> 1) - 1, (bx_f >> 1) - 1, p.F, tid, FIN_TW * FIN_TH);
  __syncthreads();
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
  const int den = (p.F + 1) * (p.F + 1), M = mb_band_n(i, g.ch, p.F) * mb_band_n(j, g.cw, p.F);
  int wy[3], wx[3];
  mb_expand_w(i, wy);
  mb_expand_w(j, wx);
  const int at_c = ((i >> 1) - (by_f >> 1) + 1) * FIN_CCOLS + (j >> 1) - (bx_f >> 1) + 1;
  const int s[3] = {f[at], f[at + 1], f[at + 2]};
  uint8_t px[3];
  for (int c = 0; c < 3; ++c) {
    int eg, er;
    mb_expand2(cg + c * FIN_CROWS * FIN_CCOLS + at_c, cr + c * FIN_CROWS * FIN_CCOLS + at_c, FIN_CCOLS, wy, wx, &eg, &er);
    const int lap = (int)fine[(c * FIN_TH + i - by_f) * FIN_PITCH + j - xa] - eg;
    const int v = s[c] + ((er + mb_mask(lap, M, den) + 32) >> 6);
    px[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
  o[at] = px[0];
  o[at + 1] = px[1];
  o[at + 2] = px[2];
}

// ---- host ----
static void mb_plan(MultibandPlan& p, int cw_max, int ch_max, int levels, int feather) {
  p = MultibandPlan{};
  p.levels = levels;
  p.F = (feather + (1 << levels) - 1) >> levels;
  long off = 0;
  for (int l = 0; l <= levels; ++l) {
    p.pitch[l] = (mb_dim(cw_max, l) + 7) & ~7;
    p.g_off[l] = off;
    off += (long)mb_dim(ch_max, l) * p.pitch[l] * 2;  // (a multiple of 16)
  }
  for (int l = 1; l < levels; ++l) {
    p.r_off[l] = off;
    off += (long)mb_dim(ch_max, l) * p.pitch[l] * 4;
  }
  p.slab_bytes = off;
}

static int mb_levels_check(int levels) {
  D3F_CHECK(levels >= 1 && levels <= MULTIBAND_MAX_LEVELS, "paste_multiband: levels %d outside 1..%d", levels,
            MULTIBAND_MAX_LEVELS);
  return 0;
}

long paste_multiband_workspace_bytes(int B, int cw_max, int ch_max, int levels) {
  if (mb_levels_check(levels)) return -1;
  if (B < 0 || B > 65535 || cw_max <= 0 || ch_max <= 0 || cw_max > 16384 || ch_max > 16384) {
    return set_error(-1, "paste_multiband_workspace_bytes: B %d outside 0..65535 or a box extent (%d x %d) outside 1..16384", B,
                     cw_max, ch_max);
  }
  MultibandPlan p;
  mb_plan(p, cw_max, ch_max, levels, 0);
  return (long)B * 3 * p.slab_bytes;
}

static bool mb_overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const char* p = reinterpret_cast<const char*>(a);
  const char* q = reinterpret_cast<const char*>(b);
  return a_bytes > 0 && b_bytes > 0 && p < q + b_bytes && q < p + a_bytes;
}

int paste_multiband_check(const PasteCall& c, int levels, const void* workspace, long workspace_bytes) {
  if (int rc = mb_levels_check(levels)) return rc;
  D3F_CHECK(c.form != FRAME_BOX_ROTATED, "paste_multiband: the multiband paste has no rotated form");
  // the plain paste's refusals: sizes, the box(es), strides, feather, overlaps
  if (int rc = paste_resize_check(c)) return rc;
  const int32_t* boxes = c.form == FRAME_BOX_PER_FRAME ? c.boxes : nullptr;
  if (boxes) {
    for (int b = 0; b < c.B; ++b) {
      const int bw = boxes[4L * b + 2], bh = boxes[4L * b + 3];
      D3F_CHECK((bw < bh ? bw : bh) >= (1 << levels), "paste_multiband: frame %d: box %d x %d below %d on a side (%d levels)", b,
                bw, bh, 1 << levels, levels);
    }
  } else {
    D3F_CHECK((c.cw < c.ch ? c.cw : c.ch) >= (1 << levels), "paste_multiband: box %d x %d below %d on a side (%d levels)", c.cw,
              c.ch, 1 << levels, levels);
  }
  if (c.B == 0) return 0;
  int cw_max, ch_max;
  frame_boxes_max_extent(boxes, c.B, c.cw, c.ch, &cw_max, &ch_max);
  const long need = paste_multiband_workspace_bytes(c.B, cw_max, ch_max, levels);
  D3F_CHECK(workspace != nullptr, "paste_multiband: null workspace");
  D3F_CHECK((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "paste_multiband: the workspace must start on 16 bytes");
  D3F_CHECK(workspace_bytes >= need,
            "paste_multiband: workspace of %ld bytes, %ld needed (d3f_paste_multiband_workspace_bytes(%d, %d, %d, %d))",
            workspace_bytes, need, c.B, cw_max, ch_max, levels);
  const long bytes = (long)c.B * c.src_h * c.src_w * 3, patch_bytes = ((long)c.B * c.H - 1) * c.patch_row_stride + 3L * c.W;
  D3F_CHECK(!mb_overlap(workspace, need, c.out, bytes) && !mb_overlap(workspace, need, c.frame, bytes) &&
                !mb_overlap(workspace, need, c.patch, patch_bytes) &&
                !(c.color && mb_overlap(workspace, need, c.coef, (long)c.B * 6 * sizeof(float))),
            "paste_multiband: the workspace overlaps patch, frame, out or coef");
  return 0;
}

// the sequence for a chunk of a call (c: its frames, paste_chunk; its boxes from b0; ws: its slabs)
template <bool BOXES>
static int mb_launch_frames(const MultibandPlan& p, const PasteCall& c, int b0, char* ws, hipStream_t stream) {
  if (int rc = multiband_diff_launch(c, b0, reinterpret_cast<int16_t*>(ws + p.g_off[0]), p.pitch[0], p.slab_bytes, stream))
    return rc;
  const int n = c.B;
  BoxedGeom<MbGeom, BOXES> a;
  a.g = MbGeom{c.src_h, c.src_w, c.x1, c.y1, c.cw, c.ch, 0, 0};
  int cw_max, ch_max;
  frame_boxes_max_extent(BOXES ? c.boxes + 4L * b0 : nullptr, n, c.cw, c.ch, &cw_max, &ch_max);
  InPlaceTiles tiles{FIN_TW, FIN_TH};
  if constexpr (BOXES) {
    fill_frame_boxes(a.boxes, c.boxes, b0, n);
    for (int i = 0; i < n; ++i) tiles.cover(a.boxes.box[i]);
  } else {
    tiles.cover(FrameBox{c.x1, c.y1, c.cw, c.ch});
  }
  dim3 fin((c.src_w + FIN_TW - 1) / FIN_TW, (c.src_h + FIN_TH - 1) / FIN_TH, n);
  if (c.frame == c.out) {  // in place: the tiles that meet a box (BOXES: the kernel derives each frame's first tile)
    fin.x = tiles.nx;
    fin.y = tiles.ny;
    if constexpr (!BOXES) {
      a.g.tx0 = c.x1 / FIN_TW;
      a.g.ty0 = c.y1 / FIN_TH;
    }
  }
  const int N = p.levels;
  auto tiles_of = [&](int l) {
    return dim3((mb_dim(cw_max, l) + MB_TW - 1) / MB_TW, (mb_dim(ch_max, l) + MB_TH - 1) / MB_TH, 3 * n);
  };
  for (int l = 0; l < N; ++l)
    hipLaunchKernelGGL((multiband_reduce_kernel<BOXES>), tiles_of(l + 1), dim3(MB_THREADS), 0, stream, ws, p, a, l);
  for (int l = N - 1; l >= 1; --l) {
    if (l == N - 1)
      hipLaunchKernelGGL((multiband_collapse_kernel<true, BOXES>), tiles_of(l), dim3(MB_THREADS), 0, stream, ws, p, a, l);
    else
      hipLaunchKernelGGL((multiband_collapse_kernel<false, BOXES>), tiles_of(l), dim3(MB_THREADS), 0, stream, ws, p, a, l);
  }
  if (N == 1)
    hipLaunchKernelGGL((multiband_final_kernel<true, BOXES>), fin, dim3(FIN_TW * FIN_TH), 0, stream, c.frame, c.out, ws, p, a);
  else
    hipLaunchKernelGGL((multiband_final_kernel<false, BOXES>), fin, dim3(FIN_TW * FIN_TH), 0, stream, c.frame, c.out, ws, p, a);
  D3F_HIP(hipGetLastError());
  return 0;
}

int paste_multiband_u8_launch(const PasteCall& c, int levels, void* workspace, long workspace_bytes, hipStream_t stream) {
  if (int rc = paste_multiband_check(c, levels, workspace, workspace_bytes)) return rc;
  if (c.B == 0) return 0;
  const bool boxes = c.form == FRAME_BOX_PER_FRAME;
  int cw_max, ch_max;
  frame_boxes_max_extent(boxes ? c.boxes : nullptr, c.B, c.cw, c.ch, &cw_max, &ch_max);
  MultibandPlan p;
  mb_plan(p, cw_max, ch_max, levels, c.feather);
  const long frame_bytes = (long)c.src_h * c.src_w * 3, patch_bytes = (long)c.H * c.patch_row_stride;
  return for_frame_chunks(
      c.B, boxes ? FRAME_BOXES_MAX : MB_FRAMES_MAX,
      [&](int b0, int n, const uint8_t* patch, const uint8_t* frame, uint8_t* out, const float* coef, char* ws) {
        const PasteCall k = paste_chunk(c, n, patch, frame, out, coef);
        return boxes ? mb_launch_frames<true>(p, k, b0, ws, stream) : mb_launch_frames<false>(p, k, b0, ws, stream);
      },
      FramePtr<const uint8_t>{c.patch, patch_bytes}, FramePtr<const uint8_t>{c.frame, frame_bytes},
      FramePtr<uint8_t>{c.out, frame_bytes}, FramePtr<const float>{c.color ? c.coef : nullptr, 6},
      FramePtr<char>{reinterpret_cast<char*>(workspace), 3 * p.slab_bytes});
}

}  // namespace d3f
