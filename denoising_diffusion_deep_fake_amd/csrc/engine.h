// Whole-network engine for Unet(resnet18|resnet34): a static plan of the layer graph
// (units = conv [+ BatchNorm + ReLU + residual]), the workspace layout and the forward /
// backward launch sequences.  No device memory is allocated here: the caller (PyTorch)
// owns params, grads, BN statistics and one workspace buffer; the engine only enqueues
// kernels on the caller's stream.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "pointwise.h"

namespace d3f {

struct TensorD {
  size_t off = 0;  // bytes into the workspace
  int H = 0, W = 0, C = 0;
  long elems(int B) const { return (long)B * H * W * C; }
};

struct ParamInfo {
  std::string name;
  int shape[4];
  int ndim;
  long offset;  // floats into the flat parameter (and gradient) buffer
  long numel;
};

struct BnInfo {
  std::string prefix;  // module path, e.g. "encoder.layer1.0.bn1"
  int C;
  long rm_off, rv_off;  // floats into the flat BN-statistics buffer
};

// one convolution layer of the network: its plan (common.h, ConvLayer: description, geometry, launches, packed sizes)
// plus its place in the network -- tensors, parameters, BatchNorm, workspace regions
struct Unit : ConvLayer {
  std::string conv_name;
  int in0 = -1, in1 = -1, y = -1, a = -1;
  bool bn = true, bias = false;
  BnLayer norm;  // bn: its BatchNorm (pointwise.h: description and plan, ReLU and residual included)
  int res_tensor = -1, res_unit = -1;
  long w_off = -1, bias_off = -1, g_off = -1, b_off = -1, rm_off = -1, rv_off = -1;
  size_t wf_off = 0, wd_off = 0;  // packed weights (bytes into workspace)
  size_t coef_off = 0;  // bytes: the BatchNorm's coefficient block (pointwise.h, bn_coef)
  int segment = 0;      // backward bucket this unit belongs to
  size_t dy_off = 0;    // this unit's own dY buffer (kept until its weight-gradient group has run)
  // decoder conv(cat(upsample2x(in0), in1)) with the up-sampling folded into pre-summed weights (pointwise.hip,
  // pack_up_kernel): per-class forward matrices, the 4x4 stride-2 data gradient w.r.t. in0 (written at in0's own
  // resolution: no full-resolution scratch, no 2x2 sum) and the skip tensor's 3x3 data gradient as its own launch
  size_t wfc_off = 0, wd4_off = 0, wds_off = 0;
  size_t wu_off = 0;     // Winograd F(2x2, 3x3) filters (conv_winograd.hip) of a layer whose forward runs as Winograd
  size_t wslab_off = 0;  // this unit's own weight-gradient slab region
};

enum BwdKind { BW_HEAD, BW_UNIT, BW_SUM2X2, BW_POOL };
struct BwdOp {
  BwdKind kind;
  int unit = -1;
  // BW_UNIT
  int dA = -1;          // gradient tensor wrt the unit's output activation (grad id)
  // BatchNorm-backward reduce fusion: this op's data gradient is the ONLY writer of the next unit op's dA and
  // that unit recomputes its ReLU mask from y -> its reduction rides in this dgrad's epilogue
  int fuse_for_unit = -1;   // producer side: unit whose (dbeta, dgamma) partial sums this dgrad also emits
  int fused_rows = 0;       // consumer side: > 0 = partial rows already written by the producer (skip the reduce)
  bool mask = true;     // apply the ReLU mask of unit.a
  int dres = -1;        // grad tensor receiving dz (identity / downsample path) or -1
  bool dres_acc = false;
  int dst0 = -1, dst1 = -1;  // dgrad destinations (grad ids); dst0 may be the full-res scratch
  bool acc0 = false, acc1 = false;
  bool dst0_is_full_scratch = false;
  // BW_SUM2X2: src = full-res scratch (C channels at 2H x 2W) -> dst0
  int C = 0, Hl = 0, Wl = 0;
  // BW_POOL: dA (pooled grad) -> dst0 (acc0)
  int segment = 0;
};

// Two networks in one engine (common.h, NetSplit): the caller-owned buffers of the second network as byte offsets from
// the first one's (parameters, running statistics, gradients, NCHW input, NCHW prediction, NCHW output gradient).  The
// workspace of a pair is ONE buffer of UnetEngine::workspace_bytes: two copies of the single-network layout,
// net_ws_stride bytes apart.
struct NetIO {
  long params = 0, bnstats = 0, grads = 0, x = 0, out = 0, dout = 0;
};

class UnetEngine {
 public:
  ~UnetEngine();
  // nets: 1, or 2 = train_deep_fake's denoise-mode pair (model_a / model_b, d3f/train_deep_fake/lit_module.py:142-181) as
  // ONE set of launches; plan_nets (>= nets): the tile / split / patch-kernel choices count the workgroups of plan_nets
  // networks -- a single engine built with plan_nets = 2 runs exactly the kernels of the pair, net by net
  int build(const char* encoder, int in_channels, int classes, int B, int H, int W, int dtype, int nets = 1,
            int plan_nets = 1);

  int pack_weights(const float* params, void* ws, hipStream_t s, const NetIO* io = nullptr) const;
  int forward(const float* params, float* bnstats, const float* x, float* out, void* ws, int training,
              hipStream_t s, const NetIO* io = nullptr) const;
  // join != 0: every gradient of the segments is final on `s` when the call returns.  join == 0 (data-parallel
  // callers): nothing makes `s` wait -- the segments' gradients are final on side_stream() once everything this call
  // enqueued there has run (the side stream also waits for the caller's stream at the end of each segment, so an
  // event recorded on it covers the BatchNorm / bias gradients written on the caller's stream too); backward_join()
  // later makes a stream wait for all of it.
  int backward(const float* params, const float* dout, float* grads, void* ws, int seg_begin,
               int seg_end, hipStream_t s, int join = 1, const NetIO* io = nullptr) const;
  int backward_join(hipStream_t s) const;
  hipStream_t side_stream() const;  // creates the engine's streams on first use; nullptr in D3F_SERIAL_BACKWARD mode
  // eval-mode forward on uint8 BGR frames with the K16 pre/post kernels fused in (in_channels = classes = 3);
  // use_graph: the launch sequence is captured once per set of pointers into a hipGraph and replayed
  int predict_u8(const float* params, float* bnstats, const uint8_t* bgr_in, uint8_t* bgr_out,
                 const float mean[3], const float stdv[3], void* ws, int use_graph, hipStream_t s) const;
  // One call of the frame path: the frame loop of d3f/script_tools/put_video_through_fake_model.py:111-119, 64-68 on raw
  // frames.  Crop box (x1, y1, cw, ch) of uint8 BGR frames [B][src_h][src_w][3] -> resize to the plan's H x W (resize.hip;
  // set_frame_resample), written both as the left half of pair_out [B][H][2W][3] and, normalised, as the network input ->
  // eval-mode forward -> the fake frame into the right half -> [temporal filter on the two halves (set_frame_temporal)].
  // full_out null is d3f_unet_predict_frames_u8 and ends there.  Otherwise (d3f_unet_predict_frames_full_u8) the fake half
  // is resized back to the box and blended into raw_in over `feather` pixels -> full_out [B][src_h][src_w][3]: one paste
  // launch, or with set_frame_color_match sums -> coefficients -> [their smoothing] -> the paste in its colour form.
  // With set_frame_blend(FRAME_BLEND_MULTIBAND) the paste is the multiband sequence instead (multiband.hip), in either form.
  // full_out == raw_in pastes in place, eager only: a replay would read frames it has overwritten.
  struct FrameCall {
    const uint8_t* raw_in;
    int src_h, src_w, x1, y1, cw, ch;
    uint8_t* pair_out;
    uint8_t* full_out;  // null: the pair entry, which ignores feather and the colour mode
    int feather;
    // HOST memory [B][4] (x1, y1, cw, ch of frame b), read before the call returns: a box per frame in place of the one
    // above (d3f_unet_predict_frames_boxes_u8 / _full_boxes_u8).  The crop and the paste launches then run in their boxes
    // forms (resize.hip); everything between them works on the pair buffer and is the same.  null: one box, as ever
    const int32_t* boxes;
    // HOST memory [B][2] (c16, s16 of frame b's angle) next to boxes: the boxes turned about their centres
    // (d3f_unet_predict_frames_rboxes_u8 / _full_rboxes_u8); the crop and the paste then run in their rotated forms.
    // null: as today
    const int32_t* rot;
  };
  // use_graph: captured once per set of pointers, constants, frame size, crop box and settings; a slot per entry.  Refused
  // with boxes: a captured launch bakes its kernel arguments in, the boxes among them, and a key on their values would
  // re-capture on every call of a moving box
  int predict_frames(const FrameCall& c, const float* params, float* bnstats, const float mean[3], const float stdv[3],
                     void* ws, int use_graph, hipStream_t s) const;
  // eval-mode forward (f32 NCHW in / out) replayed from a hipGraph captured once per set of pointers -- the
  // "hipGraph-captured denoise step" of BASELINE.json configs[4]; bit-identical to forward(training = 0)
  int forward_graph(const float* params, float* bnstats, const float* x, float* out, void* ws, hipStream_t s) const;
  // One whole training step of the noisy -> clean objective (d3f/train_denoiser/lit_module.py:107-126 + Lightning's
  // backward / optimizer step) as ONE call: pack -> noise blend -> forward -> (MSE + 1 - SSIM) / 2 -> backward -> Adam.
  // use_graph: the ~330 launches over the engine's streams are captured once per set of pointers and replayed with one
  // hipGraphLaunch on the caller's stream (the small configurations are bound by the host's launch loop, not the GPU).
  struct StepArgs {
    float* params; float* bnstats; float* grads; float* exp_avg; float* exp_avg_sq;
    const float* image; const float* noise; const float* y_uniform;
    float* noisy; float* pred; float* gpred; float* loss_out; float* loss_ws;
    const float* adam_coef;  // device: adam_coefficients()
    float lam, lo, hi;
  };
  int train_step(const StepArgs& a, void* ws, int use_graph, hipStream_t s) const;
  // Optional synchronised BatchNorm statistics across data-parallel ranks (SURVEY.md 8e "optional SyncBN": makes
  // N x bs numerically one process with batch N*bs).  fn sum-all-reduces `count` floats of the workspace in place,
  // ordered on `stream`; it is called once per BatchNorm layer in the forward pass (the per-tile (sum, sum of squares)
  // partials) and once in the backward pass (the (sum dz, sum dz*xhat) partials); the finalize kernels then divide by
  // rows * world.  dgamma / dbeta stay LOCAL sums (the gradient all-reduce adds them up like every other gradient).
  typedef int (*AllReduceFn)(void* ctx, float* data, int64_t count, void* stream);
  bool bn_sync_installed() const { return bn_sync_.fn != nullptr; }
  void set_bn_sync(AllReduceFn fn, void* ctx, int world) { bn_sync_ = BnSync{fn, ctx, world > 0 ? world : 1}; }
  // The activation behind the segmentation head (head_act.h: HeadAct; smp's Activation).  Identity: the head's convolution
  // writes the caller's `out`, exactly the launches of a network without the feature.  Otherwise it writes z into the
  // workspace (head_nchw_off), one more launch writes out = act(z), and the backward pass's head turns (z, dout) into dz,
  // overwriting z: ONE backward pass (its segment 0) per training forward; a second one is refused.
  // A pair's two networks share the setting.  A change drops the captured graphs, as a pointer change does.
  int set_head_activation(int act);
  int head_activation() const { return head_act_; }
  // The settings of predict_frames.  Each default gives exactly the launches of an engine without the setting; a
  // change drops the two captured frame graphs; device memory a setting needs is the engine's own, allocated at its first
  // switch away from the default and freed with the engine.
  // How the crop is resized to the network's size (D3F_RESAMPLE_*): the plain bicubic or the antialiased one
  // (crop_resize_cubic_aa, resize.hip).  The paste is not touched.
  enum { FRAME_RESAMPLE_CUBIC = 0, FRAME_RESAMPLE_CUBIC_AA = 1 };
  int set_frame_resample(int mode);
  int frame_resample() const { return frame_.resample; }
  // Whether the full entry matches the fake's colour to the resized real crop before the paste (D3F_COLOR_*).  MEANSTD: the
  // sums of both halves of pair_out in one launch (color.hip: a partial row per workgroup), the rows' fixed-order sum and
  // the coefficients in a second one, and the paste in its colour form.  H * W above COLOR_MAX_PIXELS is refused here.
  enum { FRAME_COLOR_NONE = 0, FRAME_COLOR_MEANSTD = 1 };
  int set_frame_color_match(int mode);
  int frame_color_match() const { return frame_.color; }
  // The temporal filter (include/d3f_hip.h: d3f_unet_set_frame_temporal); strength 0 is off.  On: the filter launch on the
  // two halves of pair_out with its state-and-flag launch, and with MEANSTD the coefficients' smoothing.  A change of either
  // value also makes the next frame a first frame: the setter has no stream, so the reset is enqueued by the next frame
  // call, on its stream, in front of its launches.
  int set_frame_temporal(float strength, int threshold);
  float frame_temporal_strength() const { return frame_.strength; }
  int frame_temporal_threshold() const { return frame_.threshold; }
  int frame_temporal_reset(hipStream_t s) const;
  // How the full entry blends the fake into the frame (D3F_BLEND_*).  FEATHER: the one paste launch.  MULTIBAND: the
  // launches of paste_multiband_u8_launch (multiband.hip) in its place, with `levels` pyramid levels; the pyramid workspace
  // is the engine's, grown at the start of a full call that needs more -- before anything is enqueued or captured, never
  // shrunk -- and a growth drops the full entry's graph.  FEATHER ignores and keeps `levels`.
  enum { FRAME_BLEND_FEATHER = 0, FRAME_BLEND_MULTIBAND = 1 };
  int set_frame_blend(int mode, int levels);
  int frame_blend() const { return frame_.blend; }
  int frame_blend_levels() const { return frame_.blend_levels; }
  int export_tensor(const char* name, const void* ws, float* out_nchw, hipStream_t s) const;
  int export_shape(const char* name, int32_t dims[3]) const;

  std::vector<ParamInfo> params;
  std::vector<BnInfo> bns;
  long param_floats = 0, bnstat_floats = 0;
  size_t workspace_bytes = 0;
  int num_segments = 4;
  long seg_grad_begin[8] = {0}, seg_grad_end[8] = {0};
  int B = 0, H = 0, W = 0, dtype = 0, in_channels = 3, classes = 3;
  int nets = 1, plan_nets = 1;     // B = images PER network
  size_t net_ws_stride = 0;        // bytes between the two networks' workspace copies (0 for a single network)
  int cdtype = 0;  // contraction dtype handed to the conv kernels (dtype = storage dtype; differs for D3F_F32X3)
  double fwd_flops = 0, bwd_flops = 0;  // algorithmic conv FLOPs (2*MAC) per call
  std::vector<Unit> units;

 private:
  int esize() const { return dtype == D3F_F32 ? 4 : 2; }
  int wsize() const { return cdtype == D3F_F32X3 ? 6 : esize(); }  // bytes per packed weight (x3: three bf16 planes)
  int ve() const { return dtype == D3F_F32 ? 4 : 8; }
  const TensorD* find_export(const char* name) const;
  int new_tensor(int H_, int W_, int C_);
  int new_grad(int tensor_id);
  size_t alloc(size_t bytes);
  int add_unit(const std::string& conv_name, const std::string& bn_name, int in0, int in1, int up0,
               int Cout, int k, int stride, int pad, bool bn, bool bias, bool relu, bool apply,
               int segment);

  std::vector<TensorD> tensors;   // activations
  std::vector<TensorD> gtensors;  // activation gradients
  std::vector<int> grad_of;       // tensor id -> grad id or -1
  std::vector<bool> grad_init;    // plan-time: has a writer been emitted yet
  std::vector<BwdOp> bwd_ops;
  std::vector<int> fwd_order_;    // unit ids in execution order, -1 = max-pool
  // backward concurrency: weight gradients run on a side stream next to the data-gradient / BN chain.  Every unit
  // keeps its own dY (585 MB at bs 16, 256x256: nothing next to 288 GB), so the side stream never holds the main
  // chain back.
  mutable hipStream_t side_ = nullptr;
  mutable std::vector<hipEvent_t> ev_dy_;  // one per weight-gradient launch of a backward pass
  mutable hipEvent_t ev_join_ = nullptr;
  mutable hipEvent_t ev_seg_ = nullptr;   // "caller's stream has left the segment" (join == 0 calls)
  mutable bool side_dirty_ = false;       // work was put on the side stream that no stream has joined yet
  // weight packing off the critical path: the layouts of encoder.conv1 / layer1 / layer2 (5 % of the parameters) are
  // packed on the caller's stream, the rest on the side stream while those layers already run; the forward pass
  // waits for it in front of the first later layer
  int ensure_streams() const;
  mutable hipEvent_t ev_pack_in_ = nullptr, ev_pack_done_ = nullptr, ev_pack_mid_ = nullptr;
  mutable bool pack_pending_ = false, pack_mid_pending_ = false;
  // Weight packing in three parts: encoder.conv1 on the caller's stream (the forward needs it at once), layer1-2 and
  // then everything else on the side stream, each behind its own event.
  int first_mid_unit_ = -1;   // first unit (index into `units`) of the second part (encoder.layer1)
  int first_late_unit_ = -1;  // first unit of the third part (encoder.layer3)
  // predict_u8 graph: private capture/launch stream + the pointers and constants the captured graph bakes in
  // apply_act false: `out` receives z, whatever the activation (the uint8 entries apply it in their last kernel)
  int forward_body(const float* params, float* bnstats, float* out, char* ws, int training, hipStream_t s,
                   const NetSplit* ns = nullptr, bool apply_act = true) const;
  // the uint8 entries' last kernel: head output (head_nchw_off) -> [activation ->] de-normalised BGR bytes
  int head_to_u8bgr(const char* ws, uint8_t* out, long out_row_stride, const float mean255[3], const float std255[3],
                    hipStream_t s) const;
  void drop_graphs() const;
  void drop_frame_graphs() const;  // the two slots of predict_frames: they bake its settings' launches in
  // what a launch of this engine hands to the kernels: null for a single network
  bool make_split(const NetIO* io, long in_delta, NetSplit* ns) const;
  int predict_u8_launches(const float* params, float* bnstats, const uint8_t* bgr_in, uint8_t* bgr_out,
                          const float mean255[3], const float std255[3], char* ws, hipStream_t s) const;
  // captured graphs: one slot per entry point; a slot is re-captured when what it baked in changes -- the pointers, the
  // constants and (predict_frames) the raw frame size and crop box, the full entry's full_out, feather and colour match
  // mode, blend mode and levels, and the temporal filter setting (strength bits, threshold)
  struct GraphKey {
    const void* ptr[6];
    float cst[6];
    int geo[12];
  };
  struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    GraphKey key = {};
    void destroy();
  };
  template <typename F>
  int graph_replay(GraphSlot& slot, const GraphKey& key, hipStream_t s, F&& launches) const;
  int wait_for_packed_weights(hipStream_t s) const;
  mutable hipStream_t gstream_ = nullptr;
  mutable GraphSlot g_predict_, g_eval_, g_frames_, g_frames_full_;
  BnSync bn_sync_{nullptr, nullptr, 1};
  const BnSync* bn_sync() const { return bn_sync_.fn != nullptr ? &bn_sync_ : nullptr; }
  int train_step_launches(const StepArgs& a, void* ws, hipStream_t s) const;
  mutable hipGraphExec_t g_step_ = nullptr;
  mutable StepArgs g_step_key_{};
  mutable const void* g_step_ws_ = nullptr;
  mutable hipEvent_t ev_gin_ = nullptr, ev_gout_ = nullptr;
  int head_act_ = 0;          // HEAD_ACT_IDENTITY
  // device memory of a frame setting: allocated once, when the setting first needs it, and freed with the engine
  template <typename T>
  struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // (a setter that got one buffer and failed on the next leaves a state its next call completes)
    hipError_t ensure(size_t bytes) { return p ? hipSuccess : hipMalloc(reinterpret_cast<void**>(&p), bytes); }
  };
  // what predict_frames takes from the handle: the settings and their device memory
  struct FrameOptions {
    int resample = FRAME_RESAMPLE_CUBIC;
    int color = FRAME_COLOR_NONE;
    float strength = 0.f;  // of the temporal filter; 0: off
    int threshold = 8;     // D3F_TEMPORAL_THRESHOLD
    mutable bool reset_pending = false;  // a changed temporal setting: the next (const) frame call zeroes the flags on its stream
    // colour match: the partial sums of a call, [2][B][parts][3][2] (the real half's, then the fake's; parts <=
    // COLOR_SUMS_MAX_PARTS comes from the sums launch, and the buffer has room for the most), and the coefficients [B][3][2]
    DevBuf<uint64_t> color_slabs;
    DevBuf<float> color_coef;
    // temporal: the filter's state (fake [H][W][3] fp32, real [H][W][3] bytes), the smoothing's (coef [3][2] fp32, sum [3]
    // uint64) and the two valid flags (the filter's, then the smoothing's)
    DevBuf<float> state_fake;
    DevBuf<uint8_t> state_real;
    DevBuf<float> state_coef;
    DevBuf<uint64_t> state_sum;
    DevBuf<int> valid;
    // blend: the mode, the multiband form's levels and its pyramid workspace (grown by a const frame call, before it
    // enqueues anything)
    int blend = FRAME_BLEND_FEATHER;
    int blend_levels = 1;
    mutable DevBuf<char> blend_ws;
    mutable long blend_ws_bytes = 0;
  };
  FrameOptions frame_;
  // the pair buffer [B][H][2W][3]: where the fake half starts in a row, and the bytes from row to row
  long pair_fake_off() const { return 3L * W; }
  long pair_stride() const { return 2 * pair_fake_off(); }
  // NCHW fp32 head output: predict_u8's, and z of an activated head, which the head of the backward pass turns into dz IN
  // PLACE (the bias gradient's channel sum reads that): the workspace is the one of a plan without activations
  size_t head_nchw_off = 0;
  mutable bool head_z_live_ = false;  // the slot holds the z of a training forward that no backward pass has consumed
  size_t ws_top = 0;
  int t_x = -1, t_pool = -1, head = -1, conv1 = -1;
  size_t pool_idx_off = 0, stats_off = 0, bnpart_off = 0, dz_off = 0, dfull_off = 0,
         bsum_off = 0, splitk_off = 0;
  size_t stats_bytes = 0, bnpart_bytes = 0, dy_bytes = 0, dz_bytes = 0, dfull_bytes = 0, splitk_bytes = 0;
};

int channel_sum_nchw_launch(const float* x, int B, int C, long HW, float* partial, float* out,
                            hipStream_t stream, const NetSplit* ns = nullptr);

}  // namespace d3f
