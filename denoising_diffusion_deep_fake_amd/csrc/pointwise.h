// HBM-bound kernels of the U-Net hot path (pointwise.hip, batchnorm.hip, loss.hip, optim.hip).
#pragma once
#include <string>

#include "common.h"
#include "philox.h"

namespace d3f {

constexpr int PACK_MAX_LAYERS = 64;  // layers per kernel-argument table

// ---- BatchNorm (K5/K7, batchnorm.hip) ----------------------------------------------------
// A layer's coefficient block: BN_COEF_ROWS rows of C floats, mean invstd scale shift (the forward folds the affine
// transform into y*scale + shift) and k[3] (the backward's k0 k1 k2).  The conv kernels' fused BatchNorm backward reads
// it as well (ConvParams::bn_coef).
enum BnCoefRow { BN_MEAN, BN_INVSTD, BN_SCALE, BN_SHIFT, BN_K, BN_COEF_ROWS = BN_K + 3 };
inline float* bn_coef(float* block, int C, BnCoefRow row) { return block + (long)row * C; }
inline const float* bn_coef(const float* block, int C, BnCoefRow row) { return block + (long)row * C; }

// eval mode: scale / shift from the running statistics, every BatchNorm of a network in one launch: the scale and shift
// rows of each coefficient block
struct BnEvalEntry {
  uint32_t g_off, b_off, rm_off, rv_off;  // floats into params / bnstats
  uint32_t coef_off16;                     // the coefficient block: 16-byte units into the workspace
  int32_t C;
};
struct BnEvalTable {
  int n;
  BnEvalEntry e[PACK_MAX_LAYERS];
};
int bn_eval_coeff_all_launch(const float* params, const float* bnstats, void* ws, const BnEvalTable& t,
                             hipStream_t stream);

// Train mode.  Forward: the conv epilogue's per-tile (sum, sum of squares) rows -> mean / invstd (saved for backward),
// folded scale / shift and the running statistics (momentum, unbiased variance, like torch.nn.BatchNorm2d), then
// a = act(y*scale + shift + residual).  Backward: partial sums of dz = dA*[mask] and dz*xhat -> dgamma, dbeta and
// k -> dy = k0*(dz - k1 - xhat*k2), dz -> the residual's gradient.
enum BnResidual { BN_RES_NONE, BN_RES_TENSOR, BN_RES_LAYER };  // + an activation, or + another layer's y*scale + shift
enum BnMask { BN_MASK_NONE, BN_MASK_FROM_Y, BN_MASK_FROM_A };    // the backward's ReLU mask: y*scale+shift > 0, a > 0
struct BnLayer {
  // ---- description ----
  std::string name;          // module path (error messages)
  int C = 0, Cpad = 0;       // channels; the forward statistics rows' stride (the conv's CoutPad)
  long rows = 0;             // rows (pixels) per network
  int dtype = D3F_F32;       // storage dtype
  int plan_nets = 1;         // networks whose workgroups the fused passes count (ConvLayer::plan_nets)
  bool apply = true, relu = true;  // apply false: a downsample branch, only finalized (its consumer applies it)
  BnResidual res = BN_RES_NONE;
  BnMask mask = BN_MASK_NONE;
  int fwd_rows = 0;          // forward partial rows: the conv's fwd.stat_rows, or wino_rows for a Winograd layer
  int fused_rows = 0;        // > 0: backward partial rows already written by the producing data gradient
  bool allow_fused = false;  // the finalize may fold into the streaming pass (the engine, not the C API)
  // ---- plan (bn_layer_plan) ----
  bool fwd_fused = false, bwd_fused = false;  // finalize folded into the streaming pass (fp32 / bf16, C % 32, few rows)
  int reduce_blocks = 0;     // bn_bwd_reduce's workgroups = its partial rows
  int bwd_rows = 0;          // the backward's partial rows: fused_rows, or reduce_blocks
  long rows_per_block = 0;   // the fused passes' rows per workgroup
  size_t stat_floats = 0;    // scratch: forward statistics rows, fwd_rows x Cpad x 2
  size_t part_floats = 0;    // scratch: backward partial sums (as many rows as the reduce writes, at least)
};
void bn_layer_plan(BnLayer& L);
// Buffers of one call, net 0's (ns: two networks in one launch, common.h NetSplit).
struct BnBufs {
  float* stats = nullptr;     // forward: the statistics rows; backward: the partial sums
  const float *gamma = nullptr, *beta = nullptr;
  float *running_mean = nullptr, *running_var = nullptr;  // updated by the forward pass (null: not tracked)
  float* coef = nullptr;      // the layer's coefficient block
  float* k = nullptr;         // the backward's k rows when not the block's own (the C API's workspace)
  const void* y = nullptr;    // raw conv output
  void* a = nullptr;          // forward: written; backward: the ReLU mask of BN_MASK_FROM_A
  const void* res = nullptr;  // residual: the activation (BN_RES_TENSOR) or the other layer's y (BN_RES_LAYER)
  const float* res_coef = nullptr;  // BN_RES_LAYER: the other layer's coefficient block
  const void* dA = nullptr;   // backward: gradient w.r.t. a
  void* dy = nullptr;         // backward: gradient w.r.t. y
  void* dres = nullptr;       // backward, optional: dz for the residual branch, added to it with dres_acc
  int dres_acc = 0;
  float *dgamma = nullptr, *dbeta = nullptr;
};
// synchronised statistics across data-parallel ranks: fn sum-all-reduces `count` floats in place, ordered on `stream`
struct BnSync {
  int (*fn)(void* ctx, float* data, int64_t count, void* stream);
  void* ctx;
  int world;
};
// The planned form, or with sync: the split form over the all-reduced sums (count = rows x world; dgamma / dbeta stay
// the LOCAL sums, summed over ranks with the other gradients).
int bn_layer_forward(const BnLayer& L, const BnBufs& b, const BnSync* sync, hipStream_t stream,
                     const NetSplit* ns = nullptr);
int bn_layer_backward(const BnLayer& L, const BnBufs& b, const BnSync* sync, hipStream_t stream,
                      const NetSplit* ns = nullptr);
// the split forward's two steps on their own: statistics over `count` rows -> coefficients (+ running statistics), and
// the streaming pass
int bn_layer_finalize(const BnLayer& L, const BnBufs& b, long count, hipStream_t stream, const NetSplit* ns = nullptr);
int bn_layer_apply(const BnLayer& L, const BnBufs& b, hipStream_t stream, const NetSplit* ns = nullptr);

// ---- pooling / resampling / layout (K6, K8 backward, boundary) ---------------------------
int maxpool3x3s2_fwd_launch(int dtype, const void* in, void* out, uint8_t* idx, int B, int H, int W,
                            int C, hipStream_t stream, const NetSplit* ns = nullptr);
int maxpool3x3s2_bwd_launch(int dtype, const void* dout, const uint8_t* idx, void* din, int accumulate,
                            int B, int H, int W, int C, hipStream_t stream, const NetSplit* ns = nullptr);
// dlow[b,y,x,c] = sum of the 2x2 block of dfull  (backward of nearest x2 up-sampling)
int sum2x2_launch(int dtype, const void* dfull, void* dlow, int B, int Hl, int Wl, int C,
                  hipStream_t stream, const NetSplit* ns = nullptr);
// NCHW fp32 [B][C][H][W] -> NHWC T [B][H][W][Cpad] (pad channels zero) and back
int nchw_to_nhwc_launch(int dtype, const float* in, void* out, int B, int C, int H, int W, int Cpad,
                        hipStream_t stream, const NetSplit* ns = nullptr);
int nhwc_to_nchw_launch(int dtype, const void* in, float* out, int B, int C, int H, int W, int Cpad,
                        hipStream_t stream);

// K16: uint8 BGR frames <-> normalised activations (mean255 = mean*255, std255 = std*255, RGB order)
int u8bgr_to_nhwc_launch(int dtype, const uint8_t* in, void* out, long npix, int Cpad, const float mean255[3],
                         const float std255[3], hipStream_t stream);
// out: rows of W pixels, out_row_stride bytes apart (3 * W: packed frames; 6 * W: the right half of a real|fake pair)
int nchw_to_u8bgr_launch(const float* in, uint8_t* out, int B, int H, int W, long out_row_stride, const float mean255[3],
                         const float std255[3], hipStream_t stream);

// script_tools frame path (resize.hip).  Crop: box (x1, y1, cw, ch) of uint8 BGR frames [B][src_h][src_w][3] -> bicubic
// (cv2.INTER_CUBIC in float arithmetic) -> [B][H][W][3] with rows dst_row_stride bytes apart, optionally with the K16
// normalisation of the rounded bytes, [B][H][W][Cpad] in RGB order, as u8bgr_to_nhwc_launch would write it.  The antialiased
// form is Pillow's bicubic (the window widens with the scale; include/d3f_hip.h: d3f_crop_resize_cubic_aa_u8): it refuses
// what the plain form refuses and a crop above 32 times the output on an axis.
// Paste, the full-frame output: patch [B][H][W][3], rows patch_row_stride bytes apart, resized to the box of frame
// [B][src_h][src_w][3] with the same arithmetic and blended in over a ramp of `feather` pixels; the rest of out is the
// frame.  out == frame runs in place.  The colour form (include/d3f_hip.h: d3f_paste_resize_cubic_color_u8): the clamped
// patch value times coef[b][c][0] plus coef[b][c][1], clamped again, in front of the blend; coef [B][3][2] fp32 in device
// memory.  The same kernel with one more template parameter; refuses what the plain form refuses and a coef that overlaps out.
// Both in three forms of the box -- one for the call, one per frame, one per frame and turned: CropCall and PasteCall below.
// A box per frame (include/d3f_hip.h: the _boxes_ operators): crop and paste with (x1, y1, cw, ch) replaced by boxes,
// HOST memory [B][4] as x1, y1, cw, ch, read before the call returns.  The boxes travel by value in the kernels' arguments,
// FRAME_BOXES_MAX per launch; a longer call is several launches, in order.  Frame b is byte for byte the single-box call on
// frame b with box b.  Refused before anything is launched: null boxes with B > 0, and for any frame what the single-box
// function refuses of a box (the message names the frame)
constexpr int FRAME_BOXES_MAX = 64;
// The boxes of a launch travel BY VALUE in the kernel's arguments: a table of at most FRAME_BOXES_MAX of them (1 KB), filled
// on the host from host memory after every box has been checked.  No device buffer, no copy, no lifetime, and no device-side
// read of a box nobody has checked.  A workgroup of frame blockIdx.z reads its own 16-byte entry -- a uniform index into the
// kernel-argument segment, so one scalar load, and the box stays in SGPRs as the single box of the other form does -- and
// from there on runs the code of the single-box kernel: the same device functions on the same operands, hence the same
// bytes.  What a launch decides once (the staged pitch and STAGED, the antialiased form's table strides, the in-place
// paste's grid) is the maximum over its boxes; each of these says where something sits in LDS or which workgroups exist,
// none enters a value.  More than FRAME_BOXES_MAX frames are several launches, in order.
struct alignas(16) FrameBox {
  int x1, y1, cw, ch;
};
struct FrameBoxes {
  FrameBox box[FRAME_BOXES_MAX];
};
// a kernel's geometry argument: G alone (the single-box form: the arguments it always had), or G and the table
template <typename G, bool BOXES>
struct BoxedGeom {
  G g;
};
template <typename G>
struct BoxedGeom<G, true> {
  G g;
  FrameBoxes boxes;
};
// the geometry of frame b (= blockIdx.z of the launch): a.g, with frame b's own box in the boxes form
template <typename G, bool BOXES>
__device__ __forceinline__ G frame_geom(const BoxedGeom<G, BOXES>& a, int b) {
  G g = a.g;
  if constexpr (BOXES) {
    const FrameBox bx = a.boxes.box[b];
    g.x1 = bx.x1;
    g.y1 = bx.y1;
    g.cw = bx.cw;
    g.ch = bx.ch;
  }
  return g;
}
// the table of a launch over frames b0 .. b0 + n - 1 of a call's boxes [B][4] (host memory, checked by the caller)
inline void fill_frame_boxes(FrameBoxes& t, const int32_t* boxes, int b0, int n) {
  t = FrameBoxes{};
  for (int i = 0; i < n; ++i) {
    const int32_t* bx = boxes + 4L * (b0 + i);
    t.box[i] = FrameBox{bx[0], bx[1], bx[2], bx[3]};
  }
}
// One row of a 32-pixel-wide frame tile outside the box, frame -> out (the paste kernels: a tile lies on the frame's 32 x 8
// grid): tile_w * 3 contiguous bytes from p to q.  Lane lx (0..31) of the row takes the aligned dword lx: whole where it
// lies inside the row's bytes, else its bytes that do.
__device__ __forceinline__ void frame_tile_row_copy(const uint8_t* p, uint8_t* q, int tile_w, int lx) {
  const int n = tile_w * 3;
  const int al = (int)(reinterpret_cast<uintptr_t>(p) & 3);
  if (al == (int)(reinterpret_cast<uintptr_t>(q) & 3)) {
    const int k = lx * 4 - al;  // offset of the dword's first byte from p
    if (k >= 0 && k + 4 <= n) {
      *reinterpret_cast<uint32_t*>(q + k) = *reinterpret_cast<const uint32_t*>(p + k);
    } else {
      for (int j = 0; j < 4; ++j)
        if (k + j >= 0 && k + j < n) q[k + j] = p[k + j];
    }
  } else if (lx < tile_w) {  // frame and out a different number of bytes past a dword: bytes
    q[lx * 3 + 0] = p[lx * 3 + 0];
    q[lx * 3 + 1] = p[lx * 3 + 1];
    q[lx * 3 + 2] = p[lx * 3 + 2];
  }
}

// Rotated boxes (include/d3f_hip.h: the _rboxes_ operators; DESIGN.md section 4 "Rotated crop"): the boxes form with one
// more table, rot: HOST memory [B][2] as c16 = round(cos a * 65536), s16 = round(sin a * 65536) of frame b's angle.  A
// launch's table holds box and rotation per frame (1.5 KB by value, FRAME_BOXES_MAX frames); the kernels are forms of their
// own (a sample's 4 x 4 neighbourhood sits per pixel, not per row and column), the 4 x 4 sum and the epilogues are shared.
// Refused before anything is launched: what the boxes form refuses, a null rot, and for any frame a rot whose
// c16^2 + s16^2 lies further than 2^17 from 2^32 (the message names the frame)
struct alignas(8) FrameRot {
  int c16, s16;
};
struct FrameRBoxes {
  FrameBox box[FRAME_BOXES_MAX];
  FrameRot rot[FRAME_BOXES_MAX];
};

// Which box a frame takes.  A field of its own in the two descriptors: "a box per frame, and no table" is a refusal of the
// _boxes_ and _rboxes_ operators (null boxes with B > 0; a null rot with any B) that the tables' pointers alone cannot tell
// from the single-box call.
enum FrameBoxForm {
  FRAME_BOX_ONE,        // (x1, y1, cw, ch) for every frame; boxes and rot are ignored
  FRAME_BOX_PER_FRAME,  // boxes: HOST memory [B][4] as x1, y1, cw, ch, read before the call returns; the four are ignored
  FRAME_BOX_ROTATED,    // boxes and rot (HOST memory [B][2])
};
inline FrameBoxForm frame_box_form(const int32_t* boxes, const int32_t* rot) {
  return rot ? FRAME_BOX_ROTATED : boxes ? FRAME_BOX_PER_FRAME : FRAME_BOX_ONE;
}
// One crop call and one paste call, in every form.  In the two per-frame forms frame b is byte for byte the single-box call on
// frame b with box b; a call of more than FRAME_BOXES_MAX frames is several launches, in order.  _check is everything the
// launch refuses, on the host (for a caller that must refuse before it starts a capture); the operator's name in a message
// is the form's (crop_resize_cubic_aa_boxes: frame 2: ...).  B == 0 launches nothing.
struct CropCall {
  const uint8_t* src = nullptr;
  int B = 0, src_h = 0, src_w = 0;
  FrameBoxForm form = FRAME_BOX_ONE;
  int x1 = 0, y1 = 0, cw = 0, ch = 0;
  const int32_t* boxes = nullptr;
  const int32_t* rot = nullptr;
  bool antialias = false;  // (not with FRAME_BOX_ROTATED)
  uint8_t* dst = nullptr;
  int H = 0, W = 0;
  long dst_row_stride = 0;
  // the fused network input; act null: bytes only, and the four below are ignored
  void* act = nullptr;
  int dtype = D3F_F32, Cpad = 0;
  const float* mean255 = nullptr;  // null: 0
  const float* std255 = nullptr;   // null: 1
};
struct PasteCall {
  const uint8_t* patch = nullptr;
  int B = 0, H = 0, W = 0;
  long patch_row_stride = 0;
  const uint8_t* frame = nullptr;
  int src_h = 0, src_w = 0;
  FrameBoxForm form = FRAME_BOX_ONE;
  int x1 = 0, y1 = 0, cw = 0, ch = 0;
  const int32_t* boxes = nullptr;
  const int32_t* rot = nullptr;
  int feather = 0;
  uint8_t* out = nullptr;
  bool color = false;  // the colour form; a field of its own: the colour form with a null coef is refused
  const float* coef = nullptr;
};
int crop_resize_check(const CropCall& c);
int crop_resize_launch(const CropCall& c, hipStream_t stream);
int paste_resize_check(const PasteCall& c);
int paste_resize_launch(const PasteCall& c, hipStream_t stream);

// A pointer of a call that advances with the frame: its first frame's address (null stays null) and its elements per frame.
template <typename T>
struct FramePtr {
  T* p;
  long per_frame;
};
// Cuts a call of B frames into chunks of at most `step`, in order: fn(b0, n, pointers advanced to frame b0...) for each; the
// first non-zero answer ends the walk.  Every launch sequence of a per-frame form goes through here (step FRAME_BOXES_MAX),
// and the single-box forms with their one launch (step B).
template <class Fn, typename... T>
int for_frame_chunks(int B, int step, Fn fn, FramePtr<T>... ptr) {
  for (int b0 = 0; b0 < B; b0 += step) {
    const int n = B - b0 < step ? B - b0 : step;
    if (int rc = fn(b0, n, (ptr.p ? ptr.p + b0 * ptr.per_frame : nullptr)...)) return rc;
  }
  return 0;
}
// frames b0 .. b0 + n - 1 of a paste call as a call of their own (boxes and rot stay the call's: index them from b0)
inline PasteCall paste_chunk(const PasteCall& c, int n, const uint8_t* patch, const uint8_t* frame, uint8_t* out,
                             const float* coef) {
  PasteCall k = c;
  k.B = n;
  k.patch = patch;
  k.frame = frame;
  k.out = out;
  k.coef = coef;
  return k;
}
// the largest box extents of a call's boxes [B][4] (checked by the caller); boxes null: the single box cw x ch
inline void frame_boxes_max_extent(const int32_t* boxes, int B, int cw, int ch, int* cw_max, int* ch_max) {
  *cw_max = cw;
  *ch_max = ch;
  if (!boxes) return;
  *cw_max = *ch_max = 1;
  for (int b = 0; b < B; ++b) {
    *cw_max = *cw_max > boxes[4L * b + 2] ? *cw_max : boxes[4L * b + 2];
    *ch_max = *ch_max > boxes[4L * b + 3] ? *ch_max : boxes[4L * b + 3];
  }
}
// In place (out == frame) a paste launches only the tiles of the frame's tw x th grid that a box meets; with a box per frame
// the grid is the most any frame needs, and the kernel derives each frame's first tile.  cover: a box's pixels
// [px0, px1] x [py0, py1]
struct InPlaceTiles {
  int tw, th;
  unsigned nx = 1, ny = 1;
  void cover(int px0, int px1, int py0, int py1) {
    const unsigned x = px1 / tw - px0 / tw + 1, y = py1 / th - py0 / th + 1;
    nx = nx > x ? nx : x;
    ny = ny > y ? ny : y;
  }
  void cover(const FrameBox& b) { cover(b.x1, b.x1 + b.cw - 1, b.y1, b.y1 + b.ch - 1); }
};

// Multiband paste (multiband.hip; include/d3f_hip.h: d3f_paste_multiband_u8 is the definition): the paste's byte at
// feather 0 minus the frame's byte, as a Laplacian pyramid of `levels` levels in int16 planes of a caller's workspace, each
// band faded over its own ramp, collapsed and added to the frame.
// The workspace of a call: per frame and byte-in-pixel one slab of planes -- g_0 .. g_N (int16) and R_1 .. R_{N-1} (int32) --
// laid out for the call's LARGEST box, every row `pitch[l]` elements long (a multiple of 8, so that rows start on 16 bytes)
// and every plane on a 16-byte boundary.  A frame with a smaller box uses the top-left part of its planes.
constexpr int MULTIBAND_MAX_LEVELS = 6;
struct MultibandPlan {
  int levels, F;                            // F: the ramp's width in samples of every level, ceil(feather / 2^levels)
  int pitch[MULTIBAND_MAX_LEVELS + 1];      // elements per row of the planes of level l
  long g_off[MULTIBAND_MAX_LEVELS + 1];     // bytes from a slab's start to g_l
  long r_off[MULTIBAND_MAX_LEVELS + 1];     // ... and to R_l (levels 1 .. N - 1)
  long slab_bytes;                          // of one frame and byte-in-pixel
};
// the bytes of a workspace for B frames whose boxes are at most cw_max x ch_max; < 0 with the error set for levels outside
// 1..MULTIBAND_MAX_LEVELS, B < 0 or a non-positive extent
long paste_multiband_workspace_bytes(int B, int cw_max, int ch_max, int levels);
// c: the paste call, in the single-box or the per-frame form, plain or colour (no rotated form).  _check: everything the
// launch refuses, for a caller that must refuse before it starts a capture
int paste_multiband_check(const PasteCall& c, int levels, const void* workspace, long workspace_bytes);
int paste_multiband_u8_launch(const PasteCall& c, int levels, void* workspace, long workspace_bytes, hipStream_t stream);
// the first launch of the sequence (resize.hip, next to the paste kernel whose arithmetic it shares): g_0 = (V - s) << 6 of
// a chunk's frames into their slabs (frame b's first plane at g0 + b * 3 * slab_bytes, byte-in-pixel c's slab_bytes further
// on each).  c: the chunk (paste_chunk), at most FRAME_BOXES_MAX frames in the per-frame form; its boxes from b0
int multiband_diff_launch(const PasteCall& c, int b0, int16_t* g0, int pitch0, long slab_bytes, hipStream_t stream);

// colour match (color.hip; include/d3f_hip.h: d3f_channel_sums_u8, d3f_color_match_coef).  Sums: per frame and byte-in-pixel
// S = sum p, Q = sum p^2 as uint64 [B][3][2], exact; at most COLOR_MAX_PIXELS pixels per frame, so that n Q and S^2 stay
// below 2^60.  channel_sums_u8_launch overwrites sums (a zeroing launch, then one 64-bit atomic add per workgroup and
// quantity).  channel_sums_pair_slabs_launch takes two image sets img_delta bytes apart (the halves of a pair buffer) in ONE
// launch and resets nothing: every workgroup stores its sums as a row of slabs [2][B][*parts_out][3][2], and
// color_match_coef_launch adds `parts` rows per frame in order (parts == 1: plain sums) before it forms gain and offset.
constexpr long COLOR_MAX_PIXELS = 1L << 22;
constexpr int COLOR_SUMS_MAX_PARTS = 64;  // workgroups per image, the rows of a slab
int channel_sums_check(int B, int H, int W, long row_stride);
int channel_sums_u8_launch(const uint8_t* img, int B, int H, int W, long row_stride, uint64_t* sums, hipStream_t stream);
int channel_sums_pair_slabs_launch(const uint8_t* img, long img_delta, int B, int H, int W, long row_stride, uint64_t* slabs,
                                   int* parts_out, hipStream_t stream);
int color_match_coef_launch(const uint64_t* sums_from, const uint64_t* sums_to, int parts, int B, long n, float* coef,
                            hipStream_t stream);

// temporal filter (temporal.hip, color.hip; include/d3f_hip.h: d3f_temporal_filter_u8, d3f_color_coef_smooth).  Both
// launch functions enqueue their kernel and, behind it, a launch that sets state_valid to 1 (the kernels read the flag and
// never write it): temporal_flag_set_launch for the smoothing; for the filter the launch that also copies the call's last
// real frame into state_real, which the filter kernel's workgroups read across tile borders.  temporal_filter_check is the host-side refusal of temporal_filter_u8_launch (real and fake may be
// the two halves of a pair buffer: one stride, the rows interleaved).  color_coef_smooth_launch reads S of `sums_to`
// [B][parts][3][2], adding `parts` rows per frame as color_match_coef_launch does.
int temporal_flag_set_launch(int* flag, int value, hipStream_t stream);
int temporal_filter_check(const uint8_t* real, const uint8_t* fake, int B, int H, int W, long real_stride, long fake_stride,
                          const float* state_fake, const uint8_t* state_real, const int* state_valid, float strength,
                          int threshold);
int temporal_filter_u8_launch(const uint8_t* real, uint8_t* fake, int B, int H, int W, long real_stride, long fake_stride,
                              float* state_fake, uint8_t* state_real, int* state_valid, float strength, int threshold,
                              hipStream_t stream);
int color_coef_smooth_launch(float* coef, const uint64_t* sums_to, int parts, int B, long n, float strength, float* state_coef,
                             uint64_t* state_sum, int* state_valid, hipStream_t stream);

// template tracker (track.hip; include/d3f_hip.h: d3f_gray_decimate_u8 .. d3f_track_template_u8).  Every range is refused on
// the host before a launch; the two checks are what track_template_u8_launch asks before it enqueues either kernel.  T is
// packed (th rows of tw bytes) in a buffer of 64 * 64 bytes, pos int32[2], out int32 [B][4].
int gray_decimate_check(int B, int h, int w, int s);
int gray_decimate_u8_launch(const uint8_t* frames, int B, int h, int w, int s, uint8_t* out, hipStream_t stream);
int track_seed_u8_launch(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, uint8_t* templ, int* pos,
                         bool with_level, hipStream_t stream);  // with_level: pos is int32[3], pos[2] = max(tw, th)
int track_search_check(int B, int gh, int gw, int tw, int th, int search, int adapt, int lost, const int* pos,
                       const int* out);
int track_search_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                           uint8_t* templ, int* pos, int* out, hipStream_t stream);
int track_template_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt,
                             int lost, uint8_t* templ, int* pos, uint8_t* gray_ws, int* out, hipStream_t stream);
// the scale search (d3f_track_search_scale_u8): templ stays at the seed's tw0 x th0, pos int32[3] = x, y, level, out int32 [B][8]
int track_search_scale_check(int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost, int levels, int penalty,
                             const int* pos, const int* out);
int track_search_scale_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                                 int levels, int penalty, uint8_t* templ, int* pos, int* out, hipStream_t stream);
int track_template_scale_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                                   int lost, int levels, int penalty, uint8_t* templ, int* pos, uint8_t* gray_ws, int* out,
                                   hipStream_t stream);
// the rotation search (d3f_track_search_rot_u8): templ is the upright tw0 x th0 template, pos int32[3] = x, y, angle index,
// out int32 [B][8]; table is HOST memory, (c16, s16) of the angle indices -amax..amax, checked and then passed by value
int track_seed_rot_u8_launch(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, int a0, int c16, int s16,
                             uint8_t* templ, int* pos, hipStream_t stream);
int track_search_rot_check(int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost, int steps, int penalty,
                           int amax, const int* table, const int* pos, const int* out);
int track_search_rot_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                               int steps, int penalty, int amax, const int* table, uint8_t* templ, int* pos, int* out,
                               hipStream_t stream);
int track_template_rot_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                                 int lost, int steps, int penalty, int amax, const int* table, uint8_t* templ, int* pos,
                                 uint8_t* gray_ws, int* out, hipStream_t stream);
// re-acquisition (d3f_track_global_u8, d3f_track_search_reacq_u8): key_templ is packed as templ is and never written, keys
// uint64 [B] = cost << 32 | y << 16 | x of the key template's best position in each frame
int track_global_check(int B, int gh, int gw, int tw, int th, const void* keys);
int track_global_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw, int th, const uint8_t* key_templ,
                           unsigned long long* keys, hipStream_t stream);
int track_search_reacq_check(int B, int gh, int gw, int tw, int th, int search, int adapt, int lost, int relost,
                             const uint8_t* templ, const uint8_t* key_templ, const int* pos, const void* keys, const int* out);
int track_search_reacq_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                                 int relost, uint8_t* templ, const uint8_t* key_templ, int* pos,
                                 const unsigned long long* keys, int* out, hipStream_t stream);
int track_template_reacq_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt,
                                   int lost, int relost, uint8_t* templ, const uint8_t* key_templ, int* pos, uint8_t* gray_ws,
                                   unsigned long long* keys_ws, int* out, hipStream_t stream);

// training image grids (image_grid.hip): make_grid + scale + clamp + uint8 of up to 8 fp32 NCHW batches in one launch;
// `batches` is a host array of n device pointers, out [n][GH][GW][3] with {GH, GW} from image_grid_shape
int image_grid_shape(int images, int nrow, int padding, int H, int W, int32_t dims[2]);
int image_grid_u8_launch(const float* const* batches, int n, int B, int C, int H, int W, int images, int nrow, int padding,
                         float pad_value, float scale, float shift, uint8_t* out, hipStream_t stream);

// input pipeline: uint8 RGB [B][H][W][3] -> NCHW fp32, ((float)u8 / 255 - mean[c]) / std[c]
int u8rgb_to_nchw_launch(const uint8_t* in, float* out, int B, long HW, const float mean[3], const float stdv[3],
                         hipStream_t stream);
// that expression -- the order of fp32 operations of albumentations.Normalize(max_pixel_value=255): ONE definition for
// u8rgb_to_nchw_kernel and for the device dataset's kernel (dataset.hip), so that both give the same bits
struct U8Normalise {
  float m0, m1, m2, s0, s1, s2;
  __device__ __forceinline__ float operator()(uint8_t v, int c) const {
    return ((float)v / 255.0f - (c == 0 ? m0 : c == 1 ? m1 : m2)) / (c == 0 ? s0 : c == 1 ? s1 : s2);
  }
};

// K17: affine_grid + grid_sample(bilinear, zeros, align_corners=False) on NCHW fp32, theta [B][2][3]
int affine_warp_launch(const float* in, const float* theta, float* out, int B, int C, int H, int W,
                       hipStream_t stream);
// The texel sources of the sampling: texel (channel c, offset y * W + x) of ONE image, either fp32 channel planes HW apart
// or a uint8 HWC image of the device dataset's pool normalised on the fly (32-bit offsets: an image is below 2^31 bytes).
struct PlaneTexels {
  const float* __restrict__ img;
  long HW;
  __device__ __forceinline__ float operator()(int c, long off) const { return img[(long)c * HW + off]; }
};
struct PoolTexels {
  const uint8_t* __restrict__ img;
  U8Normalise norm;
  __device__ __forceinline__ float operator()(int c, long off) const { return norm(img[(int)off * 3 + c], c); }
};
// one output pixel of an image, every channel: the sampling every warp kernel shares (affine_warp_kernel,
// affine_warp_rng_kernel, pool_batch_kernel).  theta t[6] maps normalised output coordinates to normalised input
// coordinates; a tap outside the frame is 0; dst_image: the image's C output planes.
template <class Texels>
__device__ __forceinline__ void affine_warp_pixel(const Texels& src, float* __restrict__ dst_image, const float* t, int pix,
                                                  int C, int H, int W) {
  const long HW = (long)H * W;
  const int y = pix / W, x = pix - y * W;
  const float xn = (2.0f * x + 1.0f) / W - 1.0f, yn = (2.0f * y + 1.0f) / H - 1.0f;
  const float xs = t[0] * xn + t[1] * yn + t[2], ys = t[3] * xn + t[4] * yn + t[5];
  const float fx = ((xs + 1.0f) * W - 1.0f) * 0.5f, fy = ((ys + 1.0f) * H - 1.0f) * 0.5f;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float wx1 = fx - x0f, wy1 = fy - y0f, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  const bool vx0 = (unsigned)x0 < (unsigned)W, vx1 = (unsigned)(x0 + 1) < (unsigned)W;
  const bool vy0 = (unsigned)y0 < (unsigned)H, vy1 = (unsigned)(y0 + 1) < (unsigned)H;
  float* dst = dst_image + pix;
  for (int c = 0; c < C; ++c) {
    const float v00 = (vx0 && vy0) ? src(c, (long)y0 * W + x0) : 0.f;
    const float v01 = (vx1 && vy0) ? src(c, (long)y0 * W + x0 + 1) : 0.f;
    const float v10 = (vx0 && vy1) ? src(c, (long)(y0 + 1) * W + x0) : 0.f;
    const float v11 = (vx1 && vy1) ? src(c, (long)(y0 + 1) * W + x0 + 1) : 0.f;
    dst[(long)c * HW] = v00 * (wx0 * wy0) + v01 * (wx1 * wy0) + v10 * (wx0 * wy1) + v11 * (wx1 * wy1);
  }
}
// K17 with theta drawn inside (philox.h): the ranges of RandomAffine (kind 0) / ShiftScaleRotate (kind 1) as the kernels
// take them -- python-side double constants rounded to fp32 once, like a python scalar meeting a float tensor
struct AffineRngParams {
  int kind;
  float angle_unit;          // kind 0: radians(degrees); kind 1: rotate_limit (degrees)
  float deg2rad;             // pi / 180
  float scale_lo, scale_span;  // kind 0: scale_lo, scale_hi - scale_lo; kind 1: -, scale_limit
  float shift_x, shift_y;    // kind 0: translate_x, translate_y; kind 1: shift_limit twice
  float p;                   // probability that an image is warped at all
  float h_over_w, w_over_h;
};
int affine_rng_params(int kind, const float params[5], int H, int W, AffineRngParams& q);
int affine_warp_rng_launch(const float* in, float* out, uint64_t seed, uint64_t offset, const AffineRngParams& q, int B,
                           int C, int H, int W, hipStream_t stream);
int affine_theta_draw_launch(uint64_t seed, uint64_t offset, const AffineRngParams& q, float* theta, uint8_t* apply, int B,
                             hipStream_t stream);
// the draws + theta of K17 (philox.h: the draw layout), shared by affine_warp_rng_kernel, affine_theta_draw_kernel and
// pool_batch_kernel.
// The python draws + theta of RandomAffine.forward (d3f/train_denoiser/lit_module.py:55-65) and of ShiftScaleRotate
// (d3f/train_deep_fake/lit_module.py:99-111) -- two to three dozen tiny launches per step -- as arithmetic on five
// uniforms per image: u0..u3 = block 0xFFFFFFFE of image b, u4 = word 0 of block 0xFFFFFFFD.
//   kind 0, RandomAffine:     ang = (2 u0 - 1) radians(degrees), sc = u1 (scale_hi - scale_lo) + scale_lo,
//                             tx = (2 u2 - 1) translate_x 2, ty = (2 u3 - 1) translate_y 2, always applied;
//                             theta = [[cos/sc, -sin/sc, tx], [sin/sc, cos/sc, ty]]
//   kind 1, ShiftScaleRotate: angle = (2 u0 - 1) rotate_limit, scale = 1 + (2 u1 - 1) scale_limit, dx = (2 u2 - 1) shift_limit,
//                             dy = (2 u3 - 1) shift_limit, apply = u4 < p; theta as ShiftScaleRotate.theta
// Returns whether the image is warped; the python expressions' order of fp32 operations (no contraction).
__device__ __forceinline__ bool affine_theta_rng(uint64_t seed, uint64_t offset, int b, const AffineRngParams& q,
                                                 float t[6]) {
  const Philox4 p = rng_block(seed, offset, (uint32_t)b, RNG_G_AUG);
  const float s0 = rng_uniform24(p.x[0]) * 2.0f - 1.0f, u1 = rng_uniform24(p.x[1]);
  const float s2 = rng_uniform24(p.x[2]) * 2.0f - 1.0f, s3 = rng_uniform24(p.x[3]) * 2.0f - 1.0f;
  float sn, cs;
  if (q.kind == 0) {
    const float sc = u1 * q.scale_span + q.scale_lo;
    sincosf(s0 * q.angle_unit, &sn, &cs);
    cs = cs / sc;
    sn = sn / sc;
    t[0] = cs, t[1] = -sn, t[2] = s2 * q.shift_x * 2.0f;
    t[3] = sn, t[4] = cs, t[5] = s3 * q.shift_y * 2.0f;
    return true;
  }
  const float angle = s0 * q.angle_unit, scale = 1.0f + (u1 * 2.0f - 1.0f) * q.scale_span;
  const float dx = s2 * q.shift_x, dy = s3 * q.shift_y;
  sincosf(angle * q.deg2rad, &sn, &cs);
  cs = cs / scale;
  sn = sn / scale;
  const float a11 = cs, a12 = -sn * q.h_over_w, a21 = sn * q.w_over_h, a22 = cs;
  t[0] = a11, t[1] = a12, t[2] = -2.0f * (a11 * dx + a12 * dy);
  t[3] = a21, t[4] = a22, t[5] = -2.0f * (a21 * dx + a22 * dy);
  return rng_uniform24(rng_block(seed, offset, (uint32_t)b, RNG_G_APPLY).x[0]) < q.p;
}

// Device dataset (dataset.hip): a training batch out [B][3][H][W] f32 assembled from a resident pool [N][H][W][3] uint8
// RGB in one launch -- gather by index [B] (int64, device), the normalisation of u8rgb_to_nchw_launch, then nothing
// (theta == apply == nullptr, q == nullptr), the sampling of affine_warp_launch with theta [B][2][3] where apply [B] is set
// (apply == nullptr: everywhere), or what affine_warp_rng_launch does (q != nullptr).  An index outside [0, N): the image
// is all NaN and nothing is read for it.
int pool_batch_launch(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                      const float mean[3], const float stdv[3], const float* theta, const uint8_t* apply, uint64_t seed,
                      uint64_t offset, const AffineRngParams* q, hipStream_t stream);
// Balanced sampling: pool_batch_launch's rng form (q == nullptr: no augmentation) with the index of image b drawn inside the
// launch and written to index_out [B], and the draws alone.  The table, in device memory: members [M] int64, the listed
// images sorted by (class, index); class_start [Kn + 1] int64, offsets into members of the Kn non-empty classes.
int pool_batch_balanced_launch(const uint8_t* pool, int64_t N, const int64_t* members, const int64_t* class_start, int Kn,
                               float* out, int64_t* index_out, int B, int H, int W, const float mean[3],
                               const float stdv[3], uint64_t seed, uint64_t offset, const AffineRngParams* q,
                               hipStream_t stream);
int balanced_index_draw_launch(const int64_t* members, const int64_t* class_start, int Kn, uint64_t seed, uint64_t offset,
                               int64_t* index_out, int B, hipStream_t stream);
// the draw (philox.h: words 1 and 2 of block 0xFFFFFFFD): a class among the Kn non-empty ones, then one of its members,
// each by multiply-high -- integers only, so a host restatement is exact.  A class_start that does not ascend (the host
// builds it; the kernel cannot know M) gives -1, which pool_batch_kernel answers with a NaN image.
__device__ __forceinline__ int64_t balanced_index_rng(uint64_t seed, uint64_t offset, int b,
                                                      const int64_t* __restrict__ members,
                                                      const int64_t* __restrict__ class_start, int Kn) {
  const Philox4 p = rng_block(seed, offset, (uint32_t)b, RNG_G_APPLY);
  const uint32_t j = (uint32_t)(((uint64_t)p.x[1] * (uint32_t)Kn) >> 32);
  const int64_t start = class_start[j], cnt = class_start[j + 1] - start;
  if (cnt <= 0 || cnt >= ((int64_t)1 << 31)) return -1;
  const int64_t m = (int64_t)(((uint64_t)p.x[2] * (uint64_t)cnt) >> 32);
  return members[start + m];
}

// ---- weights -------------------------------------------------------------------------------
// conv(cat(upsample2x(x), skip)) with the up-sampling folded into pre-summed weights (pointwise.hip): per-class
// forward matrices wfc [4][CoutPad][4*C0 + 9*C1], the 4x4 stride-2 data-gradient matrix wd4 [C0Rows][16*CoutD]
// (gradient w.r.t. the low-resolution source) and the skip tensor's 3x3 data-gradient matrix wds [C1Rows][9*CoutD]
int pack_up_launch(int dtype, const float* w, int Cout, int C0, int C1, void* wfc, int CoutPad, void* wd4,
                   int C0Rows, void* wds, int C1Rows, hipStream_t stream);

// PyTorch [Cout][CinReal][KH][KW] fp32 -> forward layout [CoutPad][Kpad] (k = tap*Cin + c) and / or data-gradient layout
// [CinRows][KpadD] (k = flipped tap*CoutD + co), T = dtype: every layer of a network in one launch (engine), or one layout
// of one layer (C API).  The table is passed by value as a kernel argument; conv_pack_entry (conv_plan.hip) fills entries.
constexpr int PACK_NT = 32;        // filters per tile
constexpr int PACK_LDS_ROW = 288;  // floats per filter in a tile: CT channels x taps  (32 x 9)
struct PackEntry {
  uint32_t w_off;               // floats into the flat parameter buffer
  uint32_t wf_off16, wd_off16;  // 16-byte units into the workspace
  uint32_t block0;              // first block of this layer; blocks are (filter tile, channel tile)
  uint16_t Cout, CinReal, Cin, taps, CoutPad, Kpad, CinRows, CoutD, KpadD, has_d, CT, ctiles;
  uint16_t conv_stride;         // 2: data-gradient taps stored parity class by class (dgrad_tap_slot_to_flipped)
  uint16_t has_f;               // write the forward layout (has_d: the data-gradient layout)
  uint16_t taps_shr, ct_log2;   // index arithmetic without divisions: q / taps = umulhi(q, taps_mul) >> taps_shr
  uint32_t taps_mul;            // (fast_div_setup, common.h; 0 = one tap), CT = 1 << ct_log2
};
struct PackTable {
  int n;
  PackEntry e[PACK_MAX_LAYERS];
};
static_assert(sizeof(PackEntry) == 52, "PackTable travels as a kernel argument: keep its entries small");
int pack_all_launch(int dtype, const float* params, void* ws, const PackTable& t, int blocks,
                    hipStream_t stream);

// ---- noise blend (K12), loss (K13), Adam (K14), EMA (K15) --------------------------------
int noise_blend_launch(const float* x, const float* noise, const float* y_uniform, float lam,
                       float* out, float* r_out, int B, long per_image, hipStream_t stream);
int noise_blend_fixed_launch(const float* x, const float* noise, const float* r, float* out, int B, long per_image,
                             hipStream_t stream);
// the same with the draws made inside the kernel, and the draws alone (philox.h: the layout)
int noise_blend_rng_launch(const float* x, uint64_t seed, uint64_t offset, float lam, float* out, float* r_out, int B,
                           long per_image, hipStream_t stream);
int noise_blend_fixed_rng_launch(const float* x, uint64_t seed, uint64_t offset, const float* r, float* out, int B,
                                 long per_image, hipStream_t stream);
// noise_blend_fixed_rng with the counter's image word read from index[b] (loss.hip)
int noise_blend_fixed_index_rng_launch(const float* x, uint64_t seed, uint64_t offset, const float* r,
                                       const int64_t* index, float* out, int B, long per_image, hipStream_t stream);
int noise_draw_launch(uint64_t seed, uint64_t offset, float* noise, float* y, int B, long per_image,
                      hipStream_t stream);
// per-image mse / ssim / psnr / loss of a prediction, forward only, scattered into metrics [4][N] (quality.hip)
size_t quality_per_image_workspace_bytes(int B, int H, int W);
int quality_per_image_scatter_launch(const float* pred, const float* target, float in_min, float in_max,
                                     const int64_t* index_or_null, float* metrics, int N, void* workspace, int B, int H,
                                     int W, hipStream_t stream);
size_t l1_per_image_workspace_bytes(int B);
int l1_per_image_launch(const float* pred, const float* target, float* out, void* workspace, int B, long per_image,
                        hipStream_t stream);
// its two stages, shared with the scattered form (difficulty.hip): L1_PARTS float64 partial sums per image, added in index
// order and divided once -- ONE expression for both last stages, so that both give the same bits
constexpr int L1_PARTS = 64;
int l1_partials_launch(const float* pred, const float* target, double* partial /*[B][L1_PARTS]*/, int B, long per_image,
                       hipStream_t stream);
__device__ __forceinline__ float l1_image_mean(const double* __restrict__ partial, int b, long per_image) {
  double s = 0.0;
  for (int i = 0; i < L1_PARTS; ++i) s += partial[(long)b * L1_PARTS + i];
  return (float)(s / (double)per_image);
}
// balance_training_images' scoring epoch on the device (difficulty.hip; include/d3f_hip.h states the contracts)
int l1_per_image_scatter_launch(const float* pred, const float* target, const int64_t* index, float* scores, int N,
                                void* workspace, int B, long per_image, hipStream_t stream);
size_t difficulty_classes_workspace_bytes(int N);
int difficulty_classes_launch(const float* scores, int N, int number_of_classes, int64_t* classes, int32_t* counts,
                              float* minmax, void* workspace, hipStream_t stream);
size_t difficulty_histogram_workspace_bytes(int N);
int difficulty_histogram_u8_launch(const int64_t* classes, int N, int bins, int32_t* bin_counts, double* range,
                                   uint8_t* chart, int H, int W, void* workspace, hipStream_t stream);
size_t loss_workspace_floats(int B, int H, int W);
int mse_ssim_loss_launch(const float* pred, const float* target, float in_min, float in_max,
                         float* loss_out /*[3]: loss, mse, ssim*/, float* grad_pred, float* workspace,
                         int B, int H, int W, hipStream_t stream);
int adam_step_launch(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                     float beta2, float eps, int step, float grad_scale, hipStream_t stream);
void adam_coefficients(float lr, float beta1, float beta2, float eps, int step, float grad_scale, float coef[8]);
int adam_step_dev_launch(float* p, const float* g, float* m, float* v, long n, const float* coef_dev,
                         hipStream_t stream);
int ema_lerp_launch(float* ema, const float* online, long n, float weight, hipStream_t stream);

}  // namespace d3f
