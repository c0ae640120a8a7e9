// extern "C" surface of libd3f_hip.so: see include/d3f_hip.h for the contract.
#include "../../include/d3f_hip.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "engine.h"
#include "head_act.h"
#include "philox.h"

namespace d3f {
static thread_local char g_err[1024] = "";
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace d3f

// ---- HIP-event profiling of the contraction kernels ------------------------------------------
namespace d3f {
struct ProfRec {
  hipEvent_t a, b;
  int cls;
  double flops;
};
static std::vector<ProfRec> g_prof;  // pre-created event pairs
static size_t g_prof_used = 0;
static bool g_prof_on = false;
static int g_prof_mask = 7;  // bit per class
bool prof_enabled(int cls) { return g_prof_on && ((g_prof_mask >> cls) & 1) && g_prof_used < g_prof.size(); }
void prof_begin(int cls, double flops, hipStream_t s) {
  ProfRec& r = g_prof[g_prof_used];
  r.cls = cls;
  r.flops = flops;
  (void)hipEventRecord(r.a, s);
}
void prof_end(hipStream_t s) {
  (void)hipEventRecord(g_prof[g_prof_used].b, s);
  ++g_prof_used;
}
}  // namespace d3f

using namespace d3f;

struct d3f_unet {
  UnetEngine e;
};

// storage dtype of a compute dtype (D3F_F32X3 keeps fp32 tensors)
static inline int sdt(int dtype) { return dtype == D3F_F32X3 ? D3F_F32 : dtype; }

// describe -> plan: the layer a descriptor describes (conv_plan.hip), with the launches `what` asks for
enum { PLAN_FWD = 1, PLAN_DGRAD = 2, PLAN_WGRAD = 4, PLAN_SPLITK = 8, PLAN_SUM2 = 16 };
static int plan(ConvLayer& L, int dtype, const d3f_conv_desc* d, int what) {
  D3F_CHECK(d != nullptr, "conv: null descriptor");
  L.B = d->B; L.Hv = d->H; L.Wv = d->W; L.C0 = d->C0; L.C1 = d->C1; L.up0 = d->upsample0 ? 1 : 0;
  L.CinReal = d->CinReal; L.Cout = d->Cout; L.KH = d->KH; L.KW = d->KW; L.stride = d->stride; L.pad = d->pad;
  L.dtype = dtype;
  L.need_fwd = what & PLAN_FWD;
  L.need_dgrad = what & PLAN_DGRAD;
  L.need_wgrad = what & PLAN_WGRAD;
  L.allow_splitk = what & PLAN_SPLITK;
  // want_sum2: the caller takes dx0 of an up-sampled single source at the source's LOW resolution where a launch can sum
  // the 2x2 blocks itself (d3f_conv_desc::upsample0 == 2, or the availability query d3f_conv_upsample_summed)
  L.want_sum2 = what & PLAN_SUM2;
  return conv_layer_plan(L);
}

extern "C" {

int d3f_version(void) { return 100; }

int d3f_profile_enable(int max_launches) {
  if (max_launches <= 0) {
    g_prof_on = false;
    return 0;
  }
  while ((int)g_prof.size() < max_launches) {
    ProfRec r;
    D3F_HIP(hipEventCreate(&r.a));
    D3F_HIP(hipEventCreate(&r.b));
    r.cls = 0;
    r.flops = 0;
    g_prof.push_back(r);
  }
  g_prof_used = 0;
  g_prof_on = true;
  return 0;
}
int d3f_profile_classes(int mask) {
  g_prof_mask = mask & 7;
  return 0;
}

int d3f_profile_collect(double ms[3], int64_t launches[3], double flops[3]) {
  D3F_CHECK(ms && launches && flops, "profile_collect: null argument");
  for (int k = 0; k < 3; ++k) { ms[k] = 0; launches[k] = 0; flops[k] = 0; }
  for (size_t i = 0; i < g_prof_used; ++i) {
    ProfRec& r = g_prof[i];
    D3F_HIP(hipEventSynchronize(r.b));
    float t = 0.f;
    D3F_HIP(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.cls] += (double)t;
    launches[r.cls] += 1;
    flops[r.cls] += r.flops;
  }
  const int dropped = (g_prof_on && g_prof_used >= g_prof.size()) ? 1 : 0;
  g_prof_used = 0;
  return dropped ? set_error(1, "profile buffer filled up: some launches were not timed") : 0;
}
const char* d3f_last_error(void) { return g_err; }

// ---- whole network ------------------------------------------------------------------------
int d3f_unet_create(const char* encoder_name, int in_channels, int classes, int B, int H, int W,
                    int dtype, d3f_unet_t* out) {
  return d3f_unet_create_nets(encoder_name, in_channels, classes, B, H, W, dtype, 1, 1, out);
}
int d3f_unet_create_nets(const char* encoder_name, int in_channels, int classes, int B, int H, int W, int dtype,
                         int nets, int plan_nets, d3f_unet_t* out) {
  D3F_CHECK(out != nullptr && encoder_name != nullptr, "unet_create_nets: null argument");
  d3f_unet* h = new (std::nothrow) d3f_unet();
  D3F_CHECK(h != nullptr, "unet_create_nets: out of host memory");
  const int rc = h->e.build(encoder_name, in_channels, classes, B, H, W, dtype, nets, plan_nets);
  if (rc != 0) {
    delete h;
    return rc;
  }
  *out = h;
  return 0;
}
// the single-network entry points on a pair handle (d3f_unet_create_nets(..., nets = 2, ...)): refused before anything is
// enqueued; `instead` says what a pair runs in its place
static int single_net(d3f_unet_t h, const char* fn, const char* instead) {
  D3F_CHECK(h->e.nets == 1, "%s: a pair handle %s", fn, instead);
  return 0;
}
int d3f_unet_destroy(d3f_unet_t h) {
  delete h;
  return 0;
}
int d3f_unet_nets(d3f_unet_t h) { return h ? h->e.nets : -1; }
size_t d3f_unet_net_workspace_stride(d3f_unet_t h) { return h ? h->e.net_ws_stride : 0; }

// the second network's buffers as byte offsets from the first one's (engine.h, NetIO)
static inline long byte_delta(const void* b, const void* a) {
  return (long)(reinterpret_cast<const char*>(b) - reinterpret_cast<const char*>(a));
}
int d3f_unet_pair_pack_weights(d3f_unet_t h, const float* const params[2], void* workspace, void* stream) {
  D3F_CHECK(h && params && params[0] && params[1] && workspace, "pair_pack_weights: null argument");
  D3F_CHECK(h->e.nets == 2, "pair_pack_weights: the handle is not a pair (d3f_unet_create_nets(..., nets = 2, ...))");
  NetIO io;
  io.params = byte_delta(params[1], params[0]);
  return h->e.pack_weights(params[0], workspace, (hipStream_t)stream, &io);
}
int d3f_unet_pair_forward(d3f_unet_t h, const float* const params[2], float* const bnstats[2], const float* const x[2],
                          float* const out[2], void* workspace, void* stream) {
  D3F_CHECK(h && params && bnstats && x && out && workspace, "pair_forward: null argument");
  D3F_CHECK(h->e.nets == 2, "pair_forward: the handle is not a pair (d3f_unet_create_nets(..., nets = 2, ...))");
  for (int n = 0; n < 2; ++n)
    D3F_CHECK(params[n] && bnstats[n] && x[n] && out[n], "pair_forward: null buffer of network %d", n);
  D3F_CHECK(params[0] != params[1] && bnstats[0] != bnstats[1] && out[0] != out[1],
            "pair_forward: the two networks must own distinct parameters, statistics and outputs");
  NetIO io;
  io.params = byte_delta(params[1], params[0]);
  io.bnstats = byte_delta(bnstats[1], bnstats[0]);
  io.x = byte_delta(x[1], x[0]);
  io.out = byte_delta(out[1], out[0]);
  return h->e.forward(params[0], bnstats[0], x[0], out[0], workspace, 1, (hipStream_t)stream, &io);
}
int d3f_unet_pair_backward(d3f_unet_t h, const float* const params[2], const float* const grad_out[2],
                           float* const grads[2], void* workspace, int seg_begin, int seg_end, int join, void* stream) {
  D3F_CHECK(h && params && grad_out && grads && workspace, "pair_backward: null argument");
  D3F_CHECK(h->e.nets == 2, "pair_backward: the handle is not a pair (d3f_unet_create_nets(..., nets = 2, ...))");
  for (int n = 0; n < 2; ++n)
    D3F_CHECK(params[n] && grad_out[n] && grads[n], "pair_backward: null buffer of network %d", n);
  D3F_CHECK(grads[0] != grads[1], "pair_backward: the two networks must own distinct gradient buffers");
  D3F_CHECK(seg_begin >= 0 && seg_end <= h->e.num_segments && seg_begin <= seg_end,
            "pair_backward: segments [%d,%d)", seg_begin, seg_end);
  NetIO io;
  io.params = byte_delta(params[1], params[0]);
  io.grads = byte_delta(grads[1], grads[0]);
  io.dout = byte_delta(grad_out[1], grad_out[0]);
  return h->e.backward(params[0], grad_out[0], grads[0], workspace, seg_begin, seg_end, (hipStream_t)stream, join ? 1 : 0,
                       &io);
}
static_assert(D3F_ACT_IDENTITY == HEAD_ACT_IDENTITY && D3F_ACT_SIGMOID == HEAD_ACT_SIGMOID && D3F_ACT_TANH == HEAD_ACT_TANH &&
                  D3F_ACT_SOFTMAX == HEAD_ACT_SOFTMAX && D3F_ACT_LOGSOFTMAX == HEAD_ACT_LOGSOFTMAX &&
                  D3F_ACT_CLAMP == HEAD_ACT_CLAMP && HEAD_ACT_COUNT == 6,
              "d3f_hip.h states the activation codes");
int d3f_unet_set_head_activation(d3f_unet_t h, int act) {
  D3F_CHECK(h, "unet_set_head_activation: null handle");
  return h->e.set_head_activation(act);
}
int d3f_unet_head_activation(d3f_unet_t h) { return h ? h->e.head_activation() : -1; }
// the frame settings' entries: a non-null handle of a single network
static int frame_handle(d3f_unet_t h, const char* fn) {
  D3F_CHECK(h, "%s: null handle", fn);
  return single_net(h, fn, "has no frame entries (run each network alone)");
}
int d3f_unet_set_frame_resample(d3f_unet_t h, int mode) {
  if (int rc = frame_handle(h, "unet_set_frame_resample")) return rc;
  return h->e.set_frame_resample(mode);
}
int d3f_unet_frame_resample(d3f_unet_t h) { return h ? h->e.frame_resample() : -1; }
static_assert(D3F_COLOR_NONE == UnetEngine::FRAME_COLOR_NONE && D3F_COLOR_MEANSTD == UnetEngine::FRAME_COLOR_MEANSTD,
              "d3f_hip.h states the colour match modes");
int d3f_unet_set_frame_color_match(d3f_unet_t h, int mode) {
  if (int rc = frame_handle(h, "unet_set_frame_color_match")) return rc;
  return h->e.set_frame_color_match(mode);
}
int d3f_unet_frame_color_match(d3f_unet_t h) { return h ? h->e.frame_color_match() : -1; }
int d3f_unet_set_frame_temporal(d3f_unet_t h, float strength, int threshold) {
  if (int rc = frame_handle(h, "unet_set_frame_temporal")) return rc;
  return h->e.set_frame_temporal(strength, threshold);
}
int d3f_unet_frame_temporal(d3f_unet_t h, float* strength, int* threshold) {
  D3F_CHECK(h, "unet_frame_temporal: null handle");
  if (strength) *strength = h->e.frame_temporal_strength();
  if (threshold) *threshold = h->e.frame_temporal_threshold();
  return 0;
}
int d3f_unet_frame_temporal_reset(d3f_unet_t h, void* stream) {
  if (int rc = frame_handle(h, "unet_frame_temporal_reset")) return rc;
  return h->e.frame_temporal_reset((hipStream_t)stream);
}
static_assert(D3F_BLEND_FEATHER == UnetEngine::FRAME_BLEND_FEATHER && D3F_BLEND_MULTIBAND == UnetEngine::FRAME_BLEND_MULTIBAND &&
                  D3F_MULTIBAND_MAX_LEVELS == MULTIBAND_MAX_LEVELS,
              "d3f_hip.h states the blend modes and the most levels");
int d3f_unet_set_frame_blend(d3f_unet_t h, int mode, int levels) {
  if (int rc = frame_handle(h, "unet_set_frame_blend")) return rc;
  return h->e.set_frame_blend(mode, levels);
}
int d3f_unet_frame_blend(d3f_unet_t h, int* levels) {
  if (!h) return -1;
  if (levels) *levels = h->e.frame_blend_levels();
  return h->e.frame_blend();
}
int d3f_unet_num_params(d3f_unet_t h) { return h ? (int)h->e.params.size() : -1; }
int d3f_unet_param_info(d3f_unet_t h, int i, char* name, int name_cap, int32_t shape[4], int* ndim,
                        int64_t* offset) {
  D3F_CHECK(h && i >= 0 && i < (int)h->e.params.size(), "param_info: index %d", i);
  const ParamInfo& p = h->e.params[i];
  if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", p.name.c_str());
  for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
  *ndim = p.ndim;
  *offset = p.offset;
  return 0;
}
int64_t d3f_unet_param_floats(d3f_unet_t h) { return h ? h->e.param_floats : -1; }
int d3f_unet_num_bn(d3f_unet_t h) { return h ? (int)h->e.bns.size() : -1; }
int d3f_unet_bn_info(d3f_unet_t h, int i, char* prefix, int prefix_cap, int* C, int64_t* rm_offset,
                     int64_t* rv_offset) {
  D3F_CHECK(h && i >= 0 && i < (int)h->e.bns.size(), "bn_info: index %d", i);
  const BnInfo& b = h->e.bns[i];
  if (prefix && prefix_cap > 0) snprintf(prefix, (size_t)prefix_cap, "%s", b.prefix.c_str());
  *C = b.C;
  *rm_offset = b.rm_off;
  *rv_offset = b.rv_off;
  return 0;
}
int64_t d3f_unet_bnstat_floats(d3f_unet_t h) { return h ? h->e.bnstat_floats : -1; }
size_t d3f_unet_workspace_bytes(d3f_unet_t h) { return h ? h->e.workspace_bytes : 0; }
double d3f_unet_forward_flops(d3f_unet_t h) { return h ? h->e.fwd_flops : 0.0; }
double d3f_unet_backward_flops(d3f_unet_t h) { return h ? h->e.bwd_flops : 0.0; }

int d3f_unet_pack_weights(d3f_unet_t h, const float* params, void* workspace, void* stream) {
  D3F_CHECK(h && params && workspace, "pack_weights: null argument");
  if (int rc = single_net(h, "pack_weights", "takes d3f_unet_pair_pack_weights")) return rc;
  return h->e.pack_weights(params, workspace, (hipStream_t)stream);
}
int d3f_unet_forward(d3f_unet_t h, const float* params, float* bnstats, const float* x, float* out,
                     void* workspace, int training, void* stream) {
  D3F_CHECK(h && params && bnstats && x && out && workspace, "unet_forward: null argument");
  if (int rc = single_net(h, "unet_forward", "takes d3f_unet_pair_forward")) return rc;
  return h->e.forward(params, bnstats, x, out, workspace, training, (hipStream_t)stream);
}
int d3f_unet_forward_graph(d3f_unet_t h, const float* params, float* bnstats, const float* x, float* out,
                           void* workspace, void* stream) {
  D3F_CHECK(h && params && bnstats && x && out && workspace, "unet_forward_graph: null argument");
  if (int rc = single_net(h, "unet_forward_graph", "has no eval-mode forward (run each network alone)")) return rc;
  return h->e.forward_graph(params, bnstats, x, out, workspace, (hipStream_t)stream);
}
int d3f_unet_predict_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* bgr_in, uint8_t* bgr_out,
                        const float mean[3], const float std[3], void* workspace, int use_graph, void* stream) {
  D3F_CHECK(h && params && bnstats && bgr_in && bgr_out && mean && std && workspace, "predict_u8: null argument");
  if (int rc = single_net(h, "predict_u8", "has no eval-mode forward (run each network alone)")) return rc;
  return h->e.predict_u8(params, bnstats, bgr_in, bgr_out, mean, std, workspace, use_graph, (hipStream_t)stream);
}

// the six frame entries: what an entry requires of its arguments, then the engine's one path.  who: the entry's name
enum { FRAMES_FULL = 1, FRAMES_BOXES = 2, FRAMES_ROT = 4 };
static int predict_frames_entry(const char* who, int needs, d3f_unet_t h, const float* params, float* bnstats,
                                const UnetEngine::FrameCall& c, const float* mean, const float* std, void* workspace,
                                int use_graph, void* stream) {
  D3F_CHECK(h && params && bnstats && c.raw_in && c.pair_out && (c.full_out || !(needs & FRAMES_FULL)) && mean && std && workspace,
            "%s: null argument", who);
  D3F_CHECK(c.boxes || !(needs & FRAMES_BOXES), "%s: null boxes (host memory [B][4]: x1, y1, cw, ch per frame)", who);
  D3F_CHECK(c.rot || !(needs & FRAMES_ROT), "%s: null rot (host memory [B][2]: c16, s16 per frame)", who);
  if (int rc = single_net(h, who, "has no eval-mode forward (run each network alone)")) return rc;
  return h->e.predict_frames(c, params, bnstats, mean, std, workspace, use_graph, (hipStream_t)stream);
}

int d3f_unet_predict_frames_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                               int src_w, int x1, int y1, int cw, int ch, uint8_t* pair_out, const float mean[3],
                               const float std[3], void* workspace, int use_graph, void* stream) {
  const UnetEngine::FrameCall c = {raw_in, src_h, src_w, x1, y1, cw, ch, pair_out, nullptr, 0, nullptr, nullptr};
  return predict_frames_entry("predict_frames_u8", 0, h, params, bnstats, c, mean, std, workspace, use_graph, stream);
}

int d3f_unet_predict_frames_full_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                                    int src_w, int x1, int y1, int cw, int ch, int feather, uint8_t* pair_out,
                                    uint8_t* full_out, const float mean[3], const float std[3], void* workspace,
                                    int use_graph, void* stream) {
  const UnetEngine::FrameCall c = {raw_in, src_h, src_w, x1, y1, cw, ch, pair_out, full_out, feather, nullptr, nullptr};
  return predict_frames_entry("predict_frames_full_u8", FRAMES_FULL, h, params, bnstats, c, mean, std, workspace, use_graph,
                              stream);
}

int d3f_unet_predict_frames_boxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                                     int src_w, const int32_t* boxes, uint8_t* pair_out, const float mean[3],
                                     const float std[3], void* workspace, int use_graph, void* stream) {
  const UnetEngine::FrameCall c = {raw_in, src_h, src_w, 0, 0, 0, 0, pair_out, nullptr, 0, boxes, nullptr};
  return predict_frames_entry("predict_frames_boxes_u8", FRAMES_BOXES, h, params, bnstats, c, mean, std, workspace, use_graph,
                              stream);
}

int d3f_unet_predict_frames_full_boxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in,
                                          int src_h, int src_w, const int32_t* boxes, int feather, uint8_t* pair_out,
                                          uint8_t* full_out, const float mean[3], const float std[3], void* workspace,
                                          int use_graph, void* stream) {
  const UnetEngine::FrameCall c = {raw_in, src_h, src_w, 0, 0, 0, 0, pair_out, full_out, feather, boxes, nullptr};
  return predict_frames_entry("predict_frames_full_boxes_u8", FRAMES_FULL | FRAMES_BOXES, h, params, bnstats, c, mean, std,
                              workspace, use_graph, stream);
}

int d3f_unet_predict_frames_rboxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                                      int src_w, const int32_t* boxes, const int32_t* rot, uint8_t* pair_out,
                                      const float mean[3], const float std[3], void* workspace, int use_graph, void* stream) {
  const UnetEngine::FrameCall c = {raw_in, src_h, src_w, 0, 0, 0, 0, pair_out, nullptr, 0, boxes, rot};
  return predict_frames_entry("predict_frames_rboxes_u8", FRAMES_BOXES | FRAMES_ROT, h, params, bnstats, c, mean, std, workspace,
                              use_graph, stream);
}

int d3f_unet_predict_frames_full_rboxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in,
                                           int src_h, int src_w, const int32_t* boxes, const int32_t* rot, int feather,
                                           uint8_t* pair_out, uint8_t* full_out, const float mean[3], const float std[3],
                                           void* workspace, int use_graph, void* stream) {
  const UnetEngine::FrameCall c = {raw_in, src_h, src_w, 0, 0, 0, 0, pair_out, full_out, feather, boxes, rot};
  return predict_frames_entry("predict_frames_full_rboxes_u8", FRAMES_FULL | FRAMES_BOXES | FRAMES_ROT, h, params, bnstats, c,
                              mean, std, workspace, use_graph, stream);
}

int d3f_unet_num_segments(d3f_unet_t h) { return h ? h->e.num_segments : -1; }
int d3f_unet_plan_counts(d3f_unet_t h, int32_t fwd[16], int32_t dgrad[16], int32_t wgrad[16]) {
  D3F_CHECK(h && fwd && dgrad && wgrad, "unet_plan_counts: null argument");
  for (int i = 0; i < 16; ++i) fwd[i] = dgrad[i] = wgrad[i] = 0;
  auto slot = [](int id) { return id < 0 ? 0 : id > 14 ? 14 : id; };
  for (const Unit& u : h->e.units) {
    ++fwd[u.wino ? 15 : slot(u.fwd.patch)];
    if (u.need_dgrad) {
      if (u.upfold) {
        ++dgrad[slot(u.dgrad_lo.patch)];
        if (u.C1 > 0) ++dgrad[slot(u.dgrad.patch)];
      } else {
        ++dgrad[slot(u.dgrad.patch)];
      }
    }
    for (int i = 0; i < u.wl.nparts; ++i) ++wgrad[slot(u.wl.part[i].patch)];
  }
  return 0;
}
int d3f_unet_segment_range(d3f_unet_t h, int segment, int64_t* begin, int64_t* end) {
  D3F_CHECK(h && segment >= 0 && segment < h->e.num_segments, "segment_range: segment %d", segment);
  *begin = h->e.seg_grad_begin[segment];
  *end = h->e.seg_grad_end[segment];
  return 0;
}
int d3f_unet_backward(d3f_unet_t h, const float* params, const float* grad_out, float* grads,
                      void* workspace, int seg_begin, int seg_end, void* stream) {
  D3F_CHECK(h && params && grad_out && grads && workspace, "unet_backward: null argument");
  if (int rc = single_net(h, "unet_backward", "takes d3f_unet_pair_backward")) return rc;
  D3F_CHECK(seg_begin >= 0 && seg_end <= h->e.num_segments && seg_begin <= seg_end,
            "unet_backward: segments [%d,%d)", seg_begin, seg_end);
  return h->e.backward(params, grad_out, grads, workspace, seg_begin, seg_end, (hipStream_t)stream);
}
int d3f_unet_backward_nojoin(d3f_unet_t h, const float* params, const float* grad_out, float* grads,
                             void* workspace, int seg_begin, int seg_end, void* stream) {
  D3F_CHECK(h && params && grad_out && grads && workspace, "unet_backward_nojoin: null argument");
  if (int rc = single_net(h, "unet_backward_nojoin", "takes d3f_unet_pair_backward(join = 0)")) return rc;
  D3F_CHECK(seg_begin >= 0 && seg_end <= h->e.num_segments && seg_begin <= seg_end,
            "unet_backward_nojoin: segments [%d,%d)", seg_begin, seg_end);
  return h->e.backward(params, grad_out, grads, workspace, seg_begin, seg_end, (hipStream_t)stream, 0);
}
int d3f_unet_side_stream(d3f_unet_t h, void** stream_out) {
  D3F_CHECK(h && stream_out, "unet_side_stream: null argument");
  *stream_out = (void*)h->e.side_stream();
  return 0;
}
int d3f_unet_backward_join(d3f_unet_t h, void* stream) {
  D3F_CHECK(h, "unet_backward_join: null handle");
  return h->e.backward_join((hipStream_t)stream);
}
int d3f_adam_coefficients(float lr, float beta1, float beta2, float eps, int step, float grad_scale, float coef[8]) {
  D3F_CHECK(coef && step >= 1, "adam_coefficients: step counts from 1");
  adam_coefficients(lr, beta1, beta2, eps, step, grad_scale, coef);
  return 0;
}
int d3f_unet_train_step(d3f_unet_t h, const d3f_step_buffers* b, float lam, float input_min, float input_max,
                        void* workspace, int use_graph, void* stream) {
  D3F_CHECK(h && b && workspace, "unet_train_step: null argument");
  if (int rc = single_net(h, "unet_train_step", "has no captured step (d3f_unet_pair_forward / _backward, then per network)"))
    return rc;
  D3F_CHECK(b->params && b->bnstats && b->grads && b->exp_avg && b->exp_avg_sq && b->image && b->noise && b->y_uniform &&
                b->noisy && b->pred && b->grad_pred && b->loss_out && b->loss_workspace && b->adam_coef,
            "unet_train_step: null buffer");
  D3F_CHECK(!h->e.bn_sync_installed(),
            "unet_train_step: synchronised BatchNorm statistics call back into the host inside the pass; the captured "
            "step is the single-GPU form (use forward / backward)");
  UnetEngine::StepArgs a;
  std::memset(&a, 0, sizeof(a));  // (the struct is compared bytewise as the graph's key)
  a.params = b->params; a.bnstats = b->bnstats; a.grads = b->grads; a.exp_avg = b->exp_avg; a.exp_avg_sq = b->exp_avg_sq;
  a.image = b->image; a.noise = b->noise; a.y_uniform = b->y_uniform;
  a.noisy = b->noisy; a.pred = b->pred; a.gpred = b->grad_pred; a.loss_out = b->loss_out;
  a.loss_ws = reinterpret_cast<float*>(b->loss_workspace);
  a.adam_coef = b->adam_coef;
  a.lam = lam; a.lo = input_min; a.hi = input_max;
  return h->e.train_step(a, workspace, use_graph, (hipStream_t)stream);
}
int d3f_unet_set_bn_sync(d3f_unet_t h, d3f_allreduce_fn fn, void* ctx, int world_size) {
  D3F_CHECK(h && (fn == nullptr || world_size >= 1), "unet_set_bn_sync: arguments");
  if (fn != nullptr) {  // (removing a callback is always allowed)
    if (int rc = single_net(h, "unet_set_bn_sync", "keeps per-GPU BatchNorm statistics")) return rc;
  }
  h->e.set_bn_sync(fn, ctx, world_size);
  return 0;
}
int d3f_unet_export(d3f_unet_t h, const char* name, const void* workspace, float* out_nchw, void* stream) {
  D3F_CHECK(h && name && workspace && out_nchw, "unet_export: null argument");
  return h->e.export_tensor(name, workspace, out_nchw, (hipStream_t)stream);
}
int d3f_unet_export_shape(d3f_unet_t h, const char* name, int32_t dims[3]) {
  D3F_CHECK(h && name && dims, "unet_export_shape: null argument");
  return h->e.export_shape(name, dims);
}

// ---- single operators ----------------------------------------------------------------------
size_t d3f_conv_packed_bytes(int dtype, const d3f_conv_desc* d, int which) {
  ConvLayer L;
  if (plan(L, dtype, d, 0) != 0) return 0;
  if (L.upfold) return which == 0 ? L.wfc : L.wd4 + L.wds;  // data gradient: [wd4 (low-resolution source) | wds (skip)]
  return which == 0 ? L.wf : L.wd;
}
int d3f_conv_pack_weights(int dtype, const d3f_conv_desc* d, const float* w, void* w_fwd, void* w_dgrad,
                          void* stream) {
  ConvLayer L;
  if (int rc = plan(L, dtype, d, 0)) return rc;
  if (L.upfold) {
    D3F_CHECK(w_fwd != nullptr && d->CinReal == d->C0 + d->C1, "conv_pack_weights: up-sample folded layer");
    char* wds = w_dgrad && d->C1 > 0 ? reinterpret_cast<char*>(w_dgrad) + L.wd4 : nullptr;
    return pack_up_launch(dtype, w, d->Cout, d->C0, d->C1, w_fwd, L.CoutPad, w_dgrad, L.C0Rows, wds, L.C1Rows,
                          (hipStream_t)stream);
  }
  // the network's packing kernel, one launch per layout given (each its own buffer); every table entry is filled and
  // range-checked before the first launch
  void* const dst[2] = {w_fwd, w_dgrad};
  PackTable t[2];
  int blocks[2] = {0, 0};
  for (int k = 0; k < 2; ++k) {
    t[k].n = dst[k] != nullptr ? 1 : 0;
    if (t[k].n && (blocks[k] = conv_pack_entry(L, 0, 0, 0, k == 0, k == 1, 0, t[k].e[0])) < 0) return blocks[k];
  }
  for (int k = 0; k < 2; ++k)
    if (int rc = pack_all_launch(dtype, w, dst[k], t[k], blocks[k], (hipStream_t)stream)) return rc;
  return 0;
}
int d3f_conv_upsample_folded(int dtype, const d3f_conv_desc* d) {
  ConvLayer L;
  return (d != nullptr && plan(L, dtype, d, 0) == 0 && L.upfold) ? 1 : 0;
}
int d3f_conv_upsample_summed(int dtype, const d3f_conv_desc* d) {
  ConvLayer L, D;  // (a folded layer plans no data-gradient launch for the question)
  if (d == nullptr || !d->upsample0 || plan(L, dtype, d, 0) != 0 || L.upfold) return 0;
  return (plan(D, dtype, d, PLAN_DGRAD | PLAN_SUM2) == 0 && D.dgrad.sum2) ? 1 : 0;
}
size_t d3f_conv_workspace_bytes(int dtype, const d3f_conv_desc* d, int which) {
  ConvLayer L;
  const int what = which == 0 ? PLAN_FWD : PLAN_DGRAD | (d != nullptr && d->upsample0 == 2 ? PLAN_SUM2 : 0);
  return plan(L, dtype, d, what | PLAN_SPLITK) != 0 ? 0 : L.splitk_floats * sizeof(float);
}
size_t d3f_conv_stats_floats(int dtype, const d3f_conv_desc* d, int with_workspace, int* tiles) {
  ConvLayer L;
  if (plan(L, dtype, d, PLAN_FWD | (with_workspace ? PLAN_SPLITK : 0)) != 0) return 0;
  if (tiles) *tiles = L.fwd.stat_rows;
  return (size_t)L.fwd.stat_rows * L.CoutPad * 2;
}
int d3f_conv_forward(int dtype, const d3f_conv_desc* d, const void* src0, const void* src1,
                     const void* w_fwd, void* y, float* stats, void* workspace, void* stream) {
  ConvLayer L;
  if (int rc = plan(L, dtype, d, PLAN_FWD | (workspace ? PLAN_SPLITK : 0))) return rc;
  if (d->B == 0) return 0;  // empty batch: nothing to compute (an empty tensor has a null data pointer)
  D3F_CHECK(src0 && w_fwd && y && (d->C1 == 0 || src1), "conv_forward: null argument");
  ConvFwdBufs b;
  b.src0 = src0; b.src1 = src1; b.w = w_fwd; b.out = y; b.stats = stats;
  b.slabs = reinterpret_cast<float*>(workspace);
  return conv_layer_forward(L, b, false, (hipStream_t)stream);
}
// ---- Winograd F(2x2, 3x3) form of a stride-1 3x3 fp32 layer on its own (conv_winograd.hip) ----
// (the layer planned as fp32 with its Winograd sizes filled, i.e. the kernel fits it)
static int wino_plan(ConvLayer& L, const d3f_conv_desc* d) {
  if (int rc = plan(L, D3F_F32, d, PLAN_FWD)) return rc;
  D3F_CHECK(L.wu != 0,
            "conv_winograd: needs 3x3 / stride 1 / pad 1, one source, H and W multiples of 16, channels a multiple of 16, "
            "filters a multiple of 64 (got %dx%d k%d s%d p%d C0=%d C1=%d up=%d Cout=%d)",
            d->H, d->W, d->KH, d->stride, d->pad, d->C0, d->C1, d->upsample0, d->Cout);
  return 0;
}
int d3f_conv_winograd_applies(int dtype, const d3f_conv_desc* d) {
  ConvLayer L;
  return (d != nullptr && plan(L, dtype, d, PLAN_FWD) == 0 && L.wino) ? 1 : 0;
}
size_t d3f_conv_winograd_filter_bytes(const d3f_conv_desc* d) {
  ConvLayer L;
  return (d == nullptr || plan(L, D3F_F32, d, PLAN_FWD) != 0) ? 0 : L.wu;
}
size_t d3f_conv_winograd_stats_floats(const d3f_conv_desc* d, int* tiles) {
  ConvLayer L;
  if (d == nullptr || plan(L, D3F_F32, d, PLAN_FWD) != 0 || L.wu == 0) return 0;
  if (tiles) *tiles = L.wino_rows;
  return (size_t)L.wino_rows * L.CoutPad * 2;
}
int d3f_conv_winograd_pack(const d3f_conv_desc* d, const float* w, void* u, void* stream) {
  ConvLayer L;
  if (int rc = wino_plan(L, d)) return rc;
  D3F_CHECK(w && u && d->CinReal == d->C0, "conv_winograd_pack: null argument or padded input channels");
  return conv_winograd_pack_launch(w, reinterpret_cast<float*>(u), d->Cout, d->C0, (hipStream_t)stream);
}
int d3f_conv_winograd_forward(const d3f_conv_desc* d, const void* src0, const void* u, void* y, float* stats,
                              const float* scale, const float* shift, const void* residual, int relu, void* stream) {
  ConvLayer L;
  if (int rc = wino_plan(L, d)) return rc;
  if (d->B == 0) return 0;
  D3F_CHECK(src0 && u && y && ((scale == nullptr) == (shift == nullptr)), "conv_winograd_forward: null argument");
  D3F_CHECK(scale != nullptr || (residual == nullptr && relu == 0),
            "conv_winograd_forward: residual / ReLU belong to the eval epilogue (scale and shift)");
  ConvFwdBufs b;
  b.src0 = src0; b.w = u; b.out = y;
  if (scale != nullptr) {
    b.scale = scale; b.shift = shift; b.res = residual; b.relu = relu ? 1 : 0;
  } else {
    b.stats = stats;
  }
  return conv_layer_forward(L, b, true, (hipStream_t)stream);
}
int d3f_conv_backward_data(int dtype, const d3f_conv_desc* d, const void* dy, const void* w_dgrad,
                           void* dx0, void* dx1, int acc0, int acc1, void* workspace, void* stream) {
  ConvLayer L;
  const int sum2 = d != nullptr && d->upsample0 == 2 ? PLAN_SUM2 : 0;
  if (int rc = plan(L, dtype, d, PLAN_DGRAD | sum2 | (workspace ? PLAN_SPLITK : 0))) return rc;
  if (d->B == 0) return 0;
  D3F_CHECK(dy && w_dgrad && dx0 && (d->C1 == 0 || dx1), "conv_backward_data: null argument");
  // an up-folded layer: dx0 = gradient of the LOW-resolution source [B][H/2][W/2][C0], w_dgrad = [wd4 | wds]
  ConvDgradBufs b;
  b.dy = dy; b.w = w_dgrad; b.dx0 = dx0; b.dx1 = dx1; b.acc0 = acc0; b.acc1 = acc1;
  b.w_skip = L.upfold ? reinterpret_cast<const char*>(w_dgrad) + L.wd4 : nullptr;
  b.slabs = reinterpret_cast<float*>(workspace);
  return conv_layer_dgrad(L, b, (hipStream_t)stream);
}
size_t d3f_conv_backward_weight_workspace_bytes(int dtype, const d3f_conv_desc* d) {
  ConvLayer L;
  return plan(L, dtype, d, PLAN_WGRAD) != 0 ? 0 : L.wslab_bytes;
}
int d3f_conv_backward_weight(int dtype, const d3f_conv_desc* d, const void* dy, const void* src0,
                             const void* src1, void* workspace, float* dw, void* stream) {
  ConvLayer L;
  if (int rc = plan(L, dtype, d, PLAN_WGRAD)) return rc;
  if (d->B == 0) {  // empty batch: the gradient is zero
    D3F_CHECK(dw, "conv_backward_weight: null argument");
    D3F_HIP(hipMemsetAsync(dw, 0, (size_t)d->Cout * d->CinReal * d->KH * d->KW * sizeof(float), (hipStream_t)stream));
    return 0;
  }
  D3F_CHECK(dy && src0 && workspace && dw && (d->C1 == 0 || src1), "conv_backward_weight: null argument");
  // the passes the engine runs for this layer (class form behind an up-sampling where it applies), then its slab reduce
  return wgrad_layer_launch(L.wl, dy, src0, src1, reinterpret_cast<float*>(workspace), dw, d->Cout, d->CinReal, dtype,
                            (hipStream_t)stream);
}

// ---- plan introspection: the planned layer's own fields, copied out ----
static void conv_launch_out(const ConvParams& p, int dtype, d3f_conv_launch_plan* o) {
  const bool igemm = p.patch == 0, smallc = igemm && conv_igemm_small_c(p, dtype);
  o->planned = 1;
  o->patch = p.patch; o->tile_bm = p.tile_bm; o->tile_bn = p.tile_bn; o->tiles_m = p.tiles_m; o->tiles_n = p.tiles_n;
  o->splitk = p.splitk; o->par = p.par; o->nz = p.nz;
  o->small_c = smallc ? 1 : 0;
  o->fast_addr = igemm && conv_igemm_fast_addr(p, smallc) ? 1 : 0;
  o->sum2 = p.sum2; o->stat_rows = p.stat_rows;
}
static void conv_layer_out(const ConvLayer& L, d3f_conv_plan* o) {
  o->upfold = L.upfold; o->parity = L.parity;
}
static void conv_fwd_out(const ConvLayer& L, d3f_conv_plan* o) {
  o->wino = L.wino; o->wino_rows = L.wino_rows;
  conv_launch_out(L.fwd, L.dtype, &o->fwd);
}
static void conv_dgrad_out(const ConvLayer& L, d3f_conv_plan* o) {
  if (L.upfold) conv_launch_out(L.dgrad_lo, L.dtype, &o->dgrad_lo);
  if (!L.upfold || L.C1 > 0) conv_launch_out(L.dgrad, L.dtype, &o->dgrad);
}
static void conv_wgrad_out(const ConvLayer& L, d3f_conv_plan* o) {
  o->wgrad_parts = L.wl.nparts;
  for (int i = 0; i < L.wl.nparts; ++i) {
    const WgradParams& w = L.wl.part[i];
    d3f_conv_wgrad_plan& q = o->wgrad[i];
    q.part = w.part; q.cls = w.cls; q.patch = w.patch; q.splits = w.splits; q.chunks_per_split = w.chunks_per_split;
    q.tile = wgrad_tile_edge(w); q.tiles = wgrad_tiles(w);
  }
}
int d3f_conv_layer_plan(int dtype, const d3f_conv_desc* d, int with_workspace, d3f_conv_plan* out) {
  D3F_CHECK(out != nullptr, "conv_layer_plan: null argument");
  std::memset(out, 0, sizeof(*out));
  ConvLayer G, F, D, W;  // geometry, then the layer as d3f_conv_forward / _backward_data / _backward_weight plan it
  if (int rc = plan(G, dtype, d, 0)) return rc;
  conv_layer_out(G, out);
  const int sk = with_workspace ? PLAN_SPLITK : 0;
  if (plan(F, dtype, d, PLAN_FWD | sk) == 0) conv_fwd_out(F, out);
  if (plan(D, dtype, d, PLAN_DGRAD | (d->upsample0 == 2 ? PLAN_SUM2 : 0) | sk) == 0) conv_dgrad_out(D, out);
  if (plan(W, dtype, d, PLAN_WGRAD) == 0) conv_wgrad_out(W, out);
  return 0;
}
int d3f_unet_num_conv_layers(d3f_unet_t h) { return h ? (int)h->e.units.size() : -1; }
int d3f_unet_conv_layer(d3f_unet_t h, int i, d3f_conv_desc* d, d3f_conv_plan* plan) {
  D3F_CHECK(h && d && plan && i >= 0 && i < (int)h->e.units.size(), "unet_conv_layer: index %d", i);
  const Unit& u = h->e.units[i];
  d->B = u.B; d->H = u.Hv; d->W = u.Wv; d->C0 = u.C0; d->C1 = u.C1;
  d->upsample0 = u.up0 ? (u.want_sum2 ? 2 : 1) : 0;
  d->Cout = u.Cout; d->KH = u.KH; d->KW = u.KW; d->stride = u.stride; d->pad = u.pad; d->CinReal = u.CinReal;
  std::memset(plan, 0, sizeof(*plan));
  conv_layer_out(u, plan);
  if (u.need_fwd) conv_fwd_out(u, plan);
  if (u.need_dgrad) conv_dgrad_out(u, plan);
  if (u.need_wgrad) conv_wgrad_out(u, plan);
  return 0;
}

// describe -> plan: a BatchNorm layer of the single-operator entry points (the split form)
static BnLayer bn_layer(int dtype, int C, int64_t rows, int fwd_rows = 0) {
  BnLayer L;
  L.C = C; L.Cpad = (int)round_up(C, 16); L.rows = (long)rows; L.dtype = sdt(dtype); L.fwd_rows = fwd_rows;
  L.allow_fused = false;
  bn_layer_plan(L);
  return L;
}
int d3f_bn_finalize(const float* stats, int tiles, int C, int64_t count, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, float* coef, void* stream) {
  D3F_CHECK(stats && gamma && beta && coef && C > 0 && tiles > 0 && count > 0, "bn_finalize: argument");
  const BnLayer L = bn_layer(D3F_F32, C, count, tiles);
  BnBufs b;
  b.stats = const_cast<float*>(stats);  // (read only)
  b.gamma = gamma; b.beta = beta; b.running_mean = running_mean; b.running_var = running_var; b.coef = coef;
  return bn_layer_finalize(L, b, (long)count, (hipStream_t)stream);
}
int d3f_bn_apply(int dtype, const void* y, const float* coef, int C, int64_t rows, const void* residual,
                 int relu, void* out, void* stream) {
  D3F_CHECK(y && coef && out, "bn_apply: null argument");
  BnLayer L = bn_layer(dtype, C, rows);
  L.relu = relu != 0;
  L.res = residual ? BN_RES_TENSOR : BN_RES_NONE;
  BnBufs b;
  b.coef = const_cast<float*>(coef);  // (the forward's scale / shift rows: read only)
  b.y = y; b.res = residual; b.a = out;
  return bn_layer_apply(L, b, (hipStream_t)stream);
}
size_t d3f_bn_backward_workspace_bytes(int dtype, int C, int64_t rows) {
  return ((size_t)bn_layer(dtype, C, rows).reduce_blocks * C * 2 + 3 * (size_t)C) * sizeof(float) + 256;
}
int d3f_bn_backward(int dtype, const void* dA, const void* a_or_null, const void* y, const float* coef,
                    const float* gamma, int C, int64_t rows, void* dy, void* dres, float* dgamma,
                    float* dbeta, void* workspace, void* stream) {
  D3F_CHECK(dA && y && coef && gamma && dy && dgamma && dbeta && workspace, "bn_backward: null argument");
  BnLayer L = bn_layer(dtype, C, rows);
  L.mask = a_or_null ? BN_MASK_FROM_A : BN_MASK_NONE;
  BnBufs b;
  b.stats = reinterpret_cast<float*>(workspace);  // the partial sums, then k (this workspace holds it: coef has 4 rows)
  b.k = b.stats + (size_t)round_up((long)L.reduce_blocks * C * 2, 4);
  b.coef = const_cast<float*>(coef);  // (mean / invstd rows: read only)
  b.gamma = gamma; b.y = y; b.a = const_cast<void*>(a_or_null);
  b.dA = dA; b.dy = dy; b.dres = dres; b.dgamma = dgamma; b.dbeta = dbeta;
  return bn_layer_backward(L, b, nullptr, (hipStream_t)stream);
}

// describe -> plan: the layer a d3f_bn_desc describes, as the engine would hold it
static_assert(D3F_BN_COEF_ROWS == BN_COEF_ROWS, "d3f_hip.h states the coefficient block's rows");
static int bn_plan(BnLayer& L, const d3f_bn_desc* d) {
  D3F_CHECK(d != nullptr, "bn_layer: null descriptor");
  D3F_CHECK(d->dtype == D3F_F32 || d->dtype == D3F_BF16 || d->dtype == D3F_F32X3, "bn_layer: dtype %d", d->dtype);
  D3F_CHECK(d->C > 0 && d->Cpad >= d->C && d->rows >= 0, "bn_layer: C=%d Cpad=%d rows=%lld", d->C, d->Cpad,
            (long long)d->rows);
  D3F_CHECK(d->res >= BN_RES_NONE && d->res <= BN_RES_LAYER && d->mask >= BN_MASK_NONE && d->mask <= BN_MASK_FROM_A,
            "bn_layer: res=%d mask=%d", d->res, d->mask);
  D3F_CHECK(d->fwd_rows >= 0 && d->fused_rows >= 0, "bn_layer: fwd_rows=%d fused_rows=%d", d->fwd_rows, d->fused_rows);
  D3F_CHECK(d->plan_nets == 1 || d->plan_nets == 2, "bn_layer: plan_nets=%d", d->plan_nets);
  L.name = "bn_layer";
  L.C = d->C; L.Cpad = d->Cpad; L.rows = (long)d->rows; L.dtype = sdt(d->dtype); L.plan_nets = d->plan_nets;
  L.apply = d->apply != 0; L.relu = d->relu != 0;
  L.res = (BnResidual)d->res; L.mask = (BnMask)d->mask;
  L.fwd_rows = d->fwd_rows; L.fused_rows = d->fused_rows; L.allow_fused = d->allow_fused != 0;
  bn_layer_plan(L);
  return 0;
}
static void bn_plan_out(const BnLayer& L, d3f_bn_plan* p) {
  p->fwd_fused = L.fwd_fused; p->bwd_fused = L.bwd_fused; p->reduce_blocks = L.reduce_blocks; p->bwd_rows = L.bwd_rows;
  p->rows_per_block = L.rows_per_block; p->stat_floats = L.stat_floats; p->part_floats = L.part_floats;
}
// the streaming kernels of the split form take whole 16-byte vectors per thread and a row pattern that repeats within a
// workgroup; bn_bwd_reduce one row per group of C / ve threads
static bool bn_split_channels_ok(const BnLayer& L) {
  const int ve = L.dtype == D3F_F32 ? 4 : 8;
  return L.C % ve == 0 && (256 * ve) % L.C == 0;
}
int d3f_bn_layer_plan(const d3f_bn_desc* d, d3f_bn_plan* plan) {
  D3F_CHECK(plan != nullptr, "bn_layer_plan: null argument");
  BnLayer L;
  if (int rc = bn_plan(L, d)) return rc;
  bn_plan_out(L, plan);
  return 0;
}
int d3f_bn_layer_forward(const d3f_bn_desc* d, float* stats, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* coef, const void* y, const void* res, const float* res_coef, void* a,
                         void* stream) {
  BnLayer L;
  if (int rc = bn_plan(L, d)) return rc;
  if (L.rows == 0) return 0;
  D3F_CHECK(L.fwd_rows >= 1, "bn_layer_forward: the forward pass reads fwd_rows >= 1 partial rows (fwd_rows=%d)", L.fwd_rows);
  D3F_CHECK(stats && gamma && beta && coef && y, "bn_layer_forward: null argument");
  D3F_CHECK((running_mean == nullptr) == (running_var == nullptr), "bn_layer_forward: one running statistic without the other");
  if (L.apply) {
    D3F_CHECK(a != nullptr, "bn_layer_forward: apply needs the output tensor");
    D3F_CHECK(L.res == BN_RES_NONE || res != nullptr, "bn_layer_forward: res=%d needs the residual tensor", (int)L.res);
    D3F_CHECK(L.res != BN_RES_LAYER || res_coef != nullptr, "bn_layer_forward: res=2 needs res_coef, the other layer's coefficient block");
  }
  if (L.fwd_fused)  // (16-byte loads of the statistics rows)
    D3F_CHECK(L.Cpad % 2 == 0, "bn_layer_forward: the fused form needs an even Cpad (Cpad=%d)", L.Cpad);
  else if (L.apply)
    D3F_CHECK(bn_split_channels_ok(L), "bn_layer_forward: the split form needs C to divide %d (C=%d)",
              256 * (L.dtype == D3F_F32 ? 4 : 8), L.C);
  BnBufs b;
  b.stats = stats; b.gamma = gamma; b.beta = beta; b.running_mean = running_mean; b.running_var = running_var;
  b.coef = coef; b.y = y; b.a = a; b.res = res; b.res_coef = res_coef;
  return bn_layer_forward(L, b, nullptr, (hipStream_t)stream);
}
int d3f_bn_layer_backward(const d3f_bn_desc* d, float* partial, const float* gamma, float* coef, const void* y,
                          const void* a, const void* dA, void* dy, void* dres, int dres_acc, float* dgamma, float* dbeta,
                          void* stream) {
  BnLayer L;
  if (int rc = bn_plan(L, d)) return rc;
  if (L.rows == 0) return 0;
  D3F_CHECK(partial != nullptr, "bn_layer_backward: null partial rows (fused_rows=%d: %s)", L.fused_rows,
            L.fused_rows > 0 ? "the caller's sums" : "scratch of part_floats floats");
  D3F_CHECK(gamma && coef && y && dA && dy, "bn_layer_backward: null argument");
  D3F_CHECK(L.mask != BN_MASK_FROM_A || a != nullptr, "bn_layer_backward: mask=2 needs the activation a");
  D3F_CHECK((dgamma == nullptr) == (dbeta == nullptr), "bn_layer_backward: dgamma without dbeta or the reverse");
  if (L.fused_rows == 0 || !L.bwd_fused)
    D3F_CHECK(bn_split_channels_ok(L), "bn_layer_backward: the split kernels need C to divide %d (C=%d)",
              256 * (L.dtype == D3F_F32 ? 4 : 8), L.C);
  BnBufs b;
  b.stats = partial; b.gamma = gamma; b.coef = coef; b.y = y;
  b.a = const_cast<void*>(a);  // (the ReLU mask: read only)
  b.dA = dA; b.dy = dy; b.dres = dres; b.dres_acc = dres != nullptr && dres_acc ? 1 : 0;
  b.dgamma = dgamma; b.dbeta = dbeta;
  return bn_layer_backward(L, b, nullptr, (hipStream_t)stream);
}
int d3f_unet_bn_layer(d3f_unet_t h, int i, d3f_bn_desc* d, d3f_bn_plan* plan) {
  D3F_CHECK(h && d && plan && i >= 0 && i < (int)h->e.bns.size(), "bn_layer: index %d", i);
  int k = -1;
  for (const Unit& u : h->e.units) {  // (bns lists the units with a BatchNorm, in order)
    if (!u.bn || ++k != i) continue;
    const BnLayer& L = u.norm;
    d->dtype = L.dtype; d->C = L.C; d->Cpad = L.Cpad; d->rows = L.rows; d->apply = L.apply; d->relu = L.relu;
    d->res = L.res; d->mask = L.mask; d->fwd_rows = L.fwd_rows; d->fused_rows = L.fused_rows;
    d->allow_fused = L.allow_fused; d->plan_nets = L.plan_nets;
    bn_plan_out(L, plan);
    return 0;
  }
  return set_error(-1, "bn_layer: index %d", i);
}

int d3f_head_activation_forward(int act, const float* z, float* a, int B, int C, int H, int W, void* stream) {
  if (int rc = head_act_check(act, C, C)) return rc;
  D3F_CHECK(z && a, "head_activation_forward: null argument");
  return head_act_forward_launch(act, z, a, B, C, H, W, (hipStream_t)stream);
}
int d3f_head_activation_backward(int act, int dtype, const float* z, const float* g, float* dz_nchw, void* dy_nhwc,
                                 int B, int C, int H, int W, int Cpad, void* stream) {
  if (int rc = head_act_check(act, C, Cpad)) return rc;
  D3F_CHECK(z && g && dz_nchw && dy_nhwc, "head_activation_backward: null argument");
  return head_act_backward_launch(act, sdt(dtype), z, g, dz_nchw, dy_nhwc, B, C, H, W, Cpad, (hipStream_t)stream);
}

int d3f_maxpool3x3s2_forward(int dtype, const void* in, void* out, uint8_t* idx, int B, int H, int W,
                             int C, void* stream) {
  D3F_CHECK(in && out && idx, "maxpool: null argument");
  return maxpool3x3s2_fwd_launch(sdt(dtype), in, out, idx, B, H, W, C, (hipStream_t)stream);
}
int d3f_maxpool3x3s2_backward(int dtype, const void* dout, const uint8_t* idx, void* din, int accumulate,
                              int B, int H, int W, int C, void* stream) {
  D3F_CHECK(dout && idx && din, "maxpool: null argument");
  return maxpool3x3s2_bwd_launch(sdt(dtype), dout, idx, din, accumulate, B, H, W, C, (hipStream_t)stream);
}
int d3f_upsample2x_backward(int dtype, const void* dfull, void* dlow, int B, int Hlow, int Wlow, int C,
                            void* stream) {
  D3F_CHECK(dfull && dlow, "upsample2x_backward: null argument");
  return sum2x2_launch(sdt(dtype), dfull, dlow, B, Hlow, Wlow, C, (hipStream_t)stream);
}
int d3f_u8rgb_normalise(const uint8_t* in_hwc, float* out_nchw, int B, int H, int W, const float mean[3],
                        const float std[3], void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(in_hwc && out_nchw && mean && std, "u8rgb_normalise: null argument");
  D3F_CHECK(B > 0 && H > 0 && W > 0, "u8rgb_normalise: bad shape");
  D3F_CHECK(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "u8rgb_normalise: zero std");
  return u8rgb_to_nchw_launch(in_hwc, out_nchw, B, (long)H * W, mean, std, (hipStream_t)stream);
}

// The frame path's crop and paste operators: each keeps its own null-argument check, then fills the call's descriptor
// (pointwise.h: CropCall, PasteCall) and takes the one entry point.  The paste operators' common arguments:
static PasteCall paste_call(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes, const uint8_t* frame,
                            int src_h, int src_w, FrameBoxForm form, int feather, uint8_t* out) {
  return {.patch = patch, .B = B, .H = H, .W = W, .patch_row_stride = (long)patch_row_stride_bytes, .frame = frame,
          .src_h = src_h, .src_w = src_w, .form = form, .feather = feather, .out = out};
}
static void set_box(PasteCall& c, int x1, int y1, int cw, int ch) { c.x1 = x1, c.y1 = y1, c.cw = cw, c.ch = ch; }
static void set_color(PasteCall& c, const float* coef) { c.color = true, c.coef = coef; }

int d3f_crop_resize_cubic_u8(const uint8_t* src, int B, int src_h, int src_w, int x1, int y1, int cw, int ch, uint8_t* dst,
                             int H, int W, int64_t dst_row_stride_bytes, void* stream) {
  D3F_CHECK(src && dst, "crop_resize_cubic_u8: null argument");
  return crop_resize_launch({.src = src, .B = B, .src_h = src_h, .src_w = src_w, .x1 = x1, .y1 = y1, .cw = cw, .ch = ch,
                             .dst = dst, .H = H, .W = W, .dst_row_stride = (long)dst_row_stride_bytes},
                            (hipStream_t)stream);
}

int d3f_crop_resize_cubic_aa_u8(const uint8_t* src, int B, int src_h, int src_w, int x1, int y1, int cw, int ch,
                                uint8_t* dst, int H, int W, int64_t dst_row_stride_bytes, void* stream) {
  D3F_CHECK(src && dst, "crop_resize_cubic_aa_u8: null argument");
  return crop_resize_launch({.src = src, .B = B, .src_h = src_h, .src_w = src_w, .x1 = x1, .y1 = y1, .cw = cw, .ch = ch,
                             .antialias = true, .dst = dst, .H = H, .W = W, .dst_row_stride = (long)dst_row_stride_bytes},
                            (hipStream_t)stream);
}

int d3f_paste_resize_cubic_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                              const uint8_t* frame, int src_h, int src_w, int x1, int y1, int cw, int ch, int feather,
                              uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out, "paste_resize_cubic_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_ONE, feather, out);
  set_box(c, x1, y1, cw, ch);
  return paste_resize_launch(c, (hipStream_t)stream);
}


int d3f_channel_sums_u8(const uint8_t* img, int B, int H, int W, int64_t row_stride_bytes, uint64_t* sums, void* stream) {
  D3F_CHECK(img && sums, "channel_sums_u8: null argument");
  return channel_sums_u8_launch(img, B, H, W, (long)row_stride_bytes, sums, (hipStream_t)stream);
}

int d3f_color_match_coef(const uint64_t* sums_from, const uint64_t* sums_to, int B, int64_t n, float* coef, void* stream) {
  D3F_CHECK(sums_from && sums_to && coef, "color_match_coef: null argument");
  return color_match_coef_launch(sums_from, sums_to, 1, B, (long)n, coef, (hipStream_t)stream);
}

int d3f_paste_resize_cubic_color_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                    const uint8_t* frame, int src_h, int src_w, int x1, int y1, int cw, int ch, int feather,
                                    const float* coef, uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out && coef, "paste_resize_cubic_color_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_ONE, feather, out);
  set_box(c, x1, y1, cw, ch);
  set_color(c, coef);
  return paste_resize_launch(c, (hipStream_t)stream);
}

static_assert(D3F_FRAME_BOXES_MAX == FRAME_BOXES_MAX, "d3f_hip.h states the boxes of a launch");
int d3f_crop_resize_cubic_boxes_u8(const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes, uint8_t* dst, int H,
                                   int W, int64_t dst_row_stride_bytes, void* stream) {
  D3F_CHECK(src && dst, "crop_resize_cubic_boxes_u8: null argument");
  return crop_resize_launch({.src = src, .B = B, .src_h = src_h, .src_w = src_w, .form = FRAME_BOX_PER_FRAME, .boxes = boxes,
                             .dst = dst, .H = H, .W = W, .dst_row_stride = (long)dst_row_stride_bytes},
                            (hipStream_t)stream);
}

int d3f_crop_resize_cubic_aa_boxes_u8(const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes, uint8_t* dst,
                                      int H, int W, int64_t dst_row_stride_bytes, void* stream) {
  D3F_CHECK(src && dst, "crop_resize_cubic_aa_boxes_u8: null argument");
  return crop_resize_launch({.src = src, .B = B, .src_h = src_h, .src_w = src_w, .form = FRAME_BOX_PER_FRAME, .boxes = boxes,
                             .antialias = true, .dst = dst, .H = H, .W = W, .dst_row_stride = (long)dst_row_stride_bytes},
                            (hipStream_t)stream);
}

int d3f_paste_resize_cubic_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                    const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather,
                                    uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out, "paste_resize_cubic_boxes_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_PER_FRAME, feather, out);
  c.boxes = boxes;
  return paste_resize_launch(c, (hipStream_t)stream);
}

int d3f_paste_resize_cubic_color_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                          const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather,
                                          const float* coef, uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out && coef, "paste_resize_cubic_color_boxes_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_PER_FRAME, feather, out);
  c.boxes = boxes;
  set_color(c, coef);
  return paste_resize_launch(c, (hipStream_t)stream);
}

int d3f_crop_resize_cubic_rboxes_u8(const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes, const int32_t* rot,
                                    uint8_t* dst, int H, int W, int64_t dst_row_stride_bytes, void* stream) {
  D3F_CHECK(src && dst, "crop_resize_cubic_rboxes_u8: null argument");
  return crop_resize_launch({.src = src, .B = B, .src_h = src_h, .src_w = src_w, .form = FRAME_BOX_ROTATED, .boxes = boxes,
                             .rot = rot, .dst = dst, .H = H, .W = W, .dst_row_stride = (long)dst_row_stride_bytes},
                            (hipStream_t)stream);
}

int d3f_crop_resize_cubic_rboxes_u8_nhwc(int dtype, const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes,
                                         const int32_t* rot, uint8_t* dst, int H, int W, int64_t dst_row_stride_bytes,
                                         void* act, int Cpad, const float mean[3], const float std[3], void* stream) {
  D3F_CHECK(src && dst && act && mean && std, "crop_resize_cubic_rboxes_u8_nhwc: null argument");
  D3F_CHECK(dtype == D3F_F32 || dtype == D3F_BF16, "crop_resize_cubic_rboxes_u8_nhwc: dtype %d is neither D3F_F32 nor D3F_BF16",
            dtype);
  // (mean * 255, std * 255 in fp32, as the frame entries scale them)
  const float m[3] = {mean[0] * 255.0f, mean[1] * 255.0f, mean[2] * 255.0f};
  const float sd[3] = {std[0] * 255.0f, std[1] * 255.0f, std[2] * 255.0f};
  return crop_resize_launch({.src = src, .B = B, .src_h = src_h, .src_w = src_w, .form = FRAME_BOX_ROTATED, .boxes = boxes,
                             .rot = rot, .dst = dst, .H = H, .W = W, .dst_row_stride = (long)dst_row_stride_bytes, .act = act,
                             .dtype = dtype, .Cpad = Cpad, .mean255 = m, .std255 = sd},
                            (hipStream_t)stream);
}

int d3f_paste_resize_cubic_rboxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                     const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, const int32_t* rot,
                                     int feather, uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out, "paste_resize_cubic_rboxes_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_ROTATED, feather, out);
  c.boxes = boxes, c.rot = rot;
  return paste_resize_launch(c, (hipStream_t)stream);
}

int d3f_paste_resize_cubic_color_rboxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                           const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, const int32_t* rot,
                                           int feather, const float* coef, uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out && coef, "paste_resize_cubic_color_rboxes_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_ROTATED, feather, out);
  c.boxes = boxes, c.rot = rot;
  set_color(c, coef);
  return paste_resize_launch(c, (hipStream_t)stream);
}


int64_t d3f_paste_multiband_workspace_bytes(int B, int cw_max, int ch_max, int levels) {
  return paste_multiband_workspace_bytes(B, cw_max, ch_max, levels);
}

int d3f_paste_multiband_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes, const uint8_t* frame,
                           int src_h, int src_w, int x1, int y1, int cw, int ch, int feather, int levels, void* workspace,
                           int64_t workspace_bytes, uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out, "paste_multiband_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_ONE, feather, out);
  set_box(c, x1, y1, cw, ch);
  return paste_multiband_u8_launch(c, levels, workspace, (long)workspace_bytes, (hipStream_t)stream);
}

int d3f_paste_multiband_color_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                 const uint8_t* frame, int src_h, int src_w, int x1, int y1, int cw, int ch, int feather,
                                 int levels, const float* coef, void* workspace, int64_t workspace_bytes, uint8_t* out,
                                 void* stream) {
  D3F_CHECK(patch && frame && out && coef, "paste_multiband_color_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_ONE, feather, out);
  set_box(c, x1, y1, cw, ch);
  set_color(c, coef);
  return paste_multiband_u8_launch(c, levels, workspace, (long)workspace_bytes, (hipStream_t)stream);
}

int d3f_paste_multiband_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                 const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather, int levels,
                                 void* workspace, int64_t workspace_bytes, uint8_t* out, void* stream) {
  D3F_CHECK(patch && frame && out && boxes, "paste_multiband_boxes_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_PER_FRAME, feather, out);
  c.boxes = boxes;
  return paste_multiband_u8_launch(c, levels, workspace, (long)workspace_bytes, (hipStream_t)stream);
}

int d3f_paste_multiband_color_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                       const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather,
                                       int levels, const float* coef, void* workspace, int64_t workspace_bytes, uint8_t* out,
                                       void* stream) {
  D3F_CHECK(patch && frame && out && coef && boxes, "paste_multiband_color_boxes_u8: null argument");
  PasteCall c = paste_call(patch, B, H, W, patch_row_stride_bytes, frame, src_h, src_w, FRAME_BOX_PER_FRAME, feather, out);
  c.boxes = boxes;
  set_color(c, coef);
  return paste_multiband_u8_launch(c, levels, workspace, (long)workspace_bytes, (hipStream_t)stream);
}


int d3f_temporal_filter_u8(const uint8_t* real, int64_t real_row_stride_bytes, uint8_t* fake, int64_t fake_row_stride_bytes,
                           int B, int H, int W, float* state_fake, uint8_t* state_real, int32_t* state_valid, float strength,
                           int threshold, void* stream) {
  D3F_CHECK(real && fake && state_fake && state_real && state_valid, "temporal_filter_u8: null argument");
  return temporal_filter_u8_launch(real, fake, B, H, W, (long)real_row_stride_bytes, (long)fake_row_stride_bytes, state_fake,
                                   state_real, state_valid, strength, threshold, (hipStream_t)stream);
}

int d3f_color_coef_smooth(float* coef, const uint64_t* sums_to, int B, int64_t n, float strength, float* state_coef,
                          uint64_t* state_sum, int32_t* state_valid, void* stream) {
  D3F_CHECK(coef && sums_to && state_coef && state_sum && state_valid, "color_coef_smooth: null argument");
  return color_coef_smooth_launch(coef, sums_to, 1, B, (long)n, strength, state_coef, state_sum, state_valid,
                                  (hipStream_t)stream);
}

int d3f_temporal_flag_set(int32_t* flag, int value, void* stream) {
  return temporal_flag_set_launch(flag, value, (hipStream_t)stream);
}

int d3f_gray_decimate_u8(const uint8_t* frames, int B, int h, int w, int s, uint8_t* out, void* stream) {
  D3F_CHECK(frames && out, "gray_decimate_u8: null argument");
  return gray_decimate_u8_launch(frames, B, h, w, s, out, (hipStream_t)stream);
}

int d3f_track_seed_u8(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, uint8_t* templ, int32_t* pos,
                      void* stream) {
  D3F_CHECK(frame && templ && pos, "track_seed_u8: null argument");
  return track_seed_u8_launch(frame, h, w, s, tx, ty, tw, th, templ, pos, false, (hipStream_t)stream);
}

int d3f_track_seed_scale_u8(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, uint8_t* templ,
                            int32_t* pos, void* stream) {
  D3F_CHECK(frame && templ && pos, "track_seed_scale_u8: null argument");
  return track_seed_u8_launch(frame, h, w, s, tx, ty, tw, th, templ, pos, true, (hipStream_t)stream);
}

int d3f_track_search_scale_u8(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                              int levels, int penalty, uint8_t* templ, int32_t* pos, int32_t* out, void* stream) {
  D3F_CHECK(gray && templ && pos && out, "track_search_scale_u8: null argument");
  return track_search_scale_u8_launch(gray, B, gh, gw, tw0, th0, search, adapt, lost, levels, penalty, templ, pos, out,
                                      (hipStream_t)stream);
}

int d3f_track_template_scale_u8(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                                int lost, int levels, int penalty, uint8_t* templ, int32_t* pos, uint8_t* gray_ws,
                                int32_t* out, void* stream) {
  D3F_CHECK(frames && templ && pos && gray_ws && out, "track_template_scale_u8: null argument");
  return track_template_scale_u8_launch(frames, B, h, w, s, tw0, th0, search, adapt, lost, levels, penalty, templ, pos, gray_ws,
                                        out, (hipStream_t)stream);
}

int d3f_track_seed_rot_u8(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, int a0, int c16, int s16,
                          uint8_t* templ, int32_t* pos, void* stream) {
  D3F_CHECK(frame && templ && pos, "track_seed_rot_u8: null argument");
  return track_seed_rot_u8_launch(frame, h, w, s, tx, ty, tw, th, a0, c16, s16, templ, pos, (hipStream_t)stream);
}

int d3f_track_search_rot_u8(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                            int steps, int penalty, int amax, const int32_t* table, uint8_t* templ, int32_t* pos, int32_t* out,
                            void* stream) {
  D3F_CHECK(gray && templ && pos && out, "track_search_rot_u8: null argument");
  return track_search_rot_u8_launch(gray, B, gh, gw, tw0, th0, search, adapt, lost, steps, penalty, amax, table, templ, pos, out,
                                    (hipStream_t)stream);
}

int d3f_track_template_rot_u8(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                              int lost, int steps, int penalty, int amax, const int32_t* table, uint8_t* templ, int32_t* pos,
                              uint8_t* gray_ws, int32_t* out, void* stream) {
  D3F_CHECK(frames && templ && pos && gray_ws && out, "track_template_rot_u8: null argument");
  return track_template_rot_u8_launch(frames, B, h, w, s, tw0, th0, search, adapt, lost, steps, penalty, amax, table, templ, pos,
                                      gray_ws, out, (hipStream_t)stream);
}

int d3f_track_search_u8(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                        uint8_t* templ, int32_t* pos, int32_t* out, void* stream) {
  D3F_CHECK(gray && templ && pos && out, "track_search_u8: null argument");
  return track_search_u8_launch(gray, B, gh, gw, tw, th, search, adapt, lost, templ, pos, out, (hipStream_t)stream);
}

int d3f_track_template_u8(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt, int lost,
                          uint8_t* templ, int32_t* pos, uint8_t* gray_ws, int32_t* out, void* stream) {
  D3F_CHECK(frames && templ && pos && gray_ws && out, "track_template_u8: null argument");
  return track_template_u8_launch(frames, B, h, w, s, tw, th, search, adapt, lost, templ, pos, gray_ws, out,
                                  (hipStream_t)stream);
}

int d3f_track_global_u8(const uint8_t* gray, int B, int gh, int gw, int tw, int th, const uint8_t* key_templ, uint64_t* keys,
                        void* stream) {
  D3F_CHECK(gray && key_templ && keys, "track_global_u8: null argument");
  return track_global_u8_launch(gray, B, gh, gw, tw, th, key_templ, reinterpret_cast<unsigned long long*>(keys),
                                (hipStream_t)stream);
}

int d3f_track_search_reacq_u8(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                              int relost, uint8_t* templ, const uint8_t* key_templ, int32_t* pos, const uint64_t* keys,
                              int32_t* out, void* stream) {
  D3F_CHECK(gray && templ && key_templ && pos && keys && out, "track_search_reacq_u8: null argument");
  return track_search_reacq_u8_launch(gray, B, gh, gw, tw, th, search, adapt, lost, relost, templ, key_templ, pos,
                                      reinterpret_cast<const unsigned long long*>(keys), out, (hipStream_t)stream);
}

int d3f_track_template_reacq_u8(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt,
                                int lost, int relost, uint8_t* templ, const uint8_t* key_templ, int32_t* pos, uint8_t* gray_ws,
                                uint64_t* keys_ws, int32_t* out, void* stream) {
  D3F_CHECK(frames && templ && key_templ && pos && gray_ws && keys_ws && out, "track_template_reacq_u8: null argument");
  return track_template_reacq_u8_launch(frames, B, h, w, s, tw, th, search, adapt, lost, relost, templ, key_templ, pos, gray_ws,
                                        reinterpret_cast<unsigned long long*>(keys_ws), out, (hipStream_t)stream);
}

int d3f_image_grid_shape(int images, int nrow, int padding, int H, int W, int32_t dims[2]) {
  D3F_CHECK(dims != nullptr, "image_grid_shape: null argument");
  return image_grid_shape(images, nrow, padding, H, W, dims);
}

int d3f_image_grid_u8(const float* const* batches, int n, int B, int C, int H, int W, int images, int nrow, int padding,
                      float pad_value, float scale, float shift, uint8_t* out, void* stream) {
  D3F_CHECK(batches && out, "image_grid_u8: null argument");
  return image_grid_u8_launch(batches, n, B, C, H, W, images, nrow, padding, pad_value, scale, shift, out,
                              (hipStream_t)stream);
}

int d3f_affine_warp(const float* in, const float* theta, float* out, int B, int C, int H, int W, void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(in && theta && out && in != out, "affine_warp: null or aliased argument");
  D3F_CHECK(B >= 0 && C > 0 && H > 0 && W > 0, "affine_warp: bad shape");
  return affine_warp_launch(in, theta, out, B, C, H, W, (hipStream_t)stream);
}

int d3f_affine_warp_rng(const float* in, float* out, uint64_t seed, uint64_t offset, int kind, const float params[5],
                        int B, int C, int H, int W, void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(in && out && params && in != out, "affine_warp_rng: null or aliased argument");
  D3F_CHECK(B >= 0 && C > 0 && H > 0 && W > 0, "affine_warp_rng: bad shape");
  AffineRngParams q;
  if (int rc = affine_rng_params(kind, params, H, W, q)) return rc;
  return affine_warp_rng_launch(in, out, seed, offset, q, B, C, H, W, (hipStream_t)stream);
}
int d3f_affine_theta_draw(uint64_t seed, uint64_t offset, int kind, const float params[5], float* theta, uint8_t* apply,
                          int B, int H, int W, void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(params && theta && apply, "affine_theta_draw: null argument");
  D3F_CHECK(B >= 0, "affine_theta_draw: bad shape");
  AffineRngParams q;
  if (int rc = affine_rng_params(kind, params, H, W, q)) return rc;
  return affine_theta_draw_launch(seed, offset, q, theta, apply, B, (hipStream_t)stream);
}

// the argument checks both device-dataset entries share; `who` names the entry in the message (B == 0: an empty batch has
// no index and no output to point at)
static int pool_batch_check(const char* who, const uint8_t* pool, int64_t N, const int64_t* index, const float* out, int B,
                            int H, int W, const float mean[3], const float std[3]) {
  D3F_CHECK(pool != nullptr, "%s: pool is null", who);
  D3F_CHECK(index != nullptr || B == 0, "%s: index is null", who);
  D3F_CHECK(out != nullptr || B == 0, "%s: out is null", who);
  D3F_CHECK(mean != nullptr, "%s: mean is null", who);
  D3F_CHECK(std != nullptr, "%s: std is null", who);
  D3F_CHECK(N >= 1, "%s: N %lld < 1", who, (long long)N);
  D3F_CHECK(B >= 0, "%s: B %d < 0", who, B);
  D3F_CHECK(H >= 1 && W >= 1, "%s: H %d, W %d below 1", who, H, W);
  D3F_CHECK(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "%s: zero std", who);
  D3F_CHECK((long)H * W * 3 < (1L << 31), "%s: an image of %ld bytes (H x W x 3 must stay below 2^31)", who,
            (long)H * W * 3);
  return 0;
}
int d3f_pool_batch(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                   const float mean[3], const float std[3], const float* theta, const uint8_t* apply, void* stream) {
  if (int rc = pool_batch_check("pool_batch", pool, N, index, out, B, H, W, mean, std)) return rc;
  D3F_CHECK(theta != nullptr || apply == nullptr, "pool_batch: apply without theta");
  return pool_batch_launch(pool, N, index, out, B, H, W, mean, std, theta, apply, 0, 0, nullptr, (hipStream_t)stream);
}
int d3f_pool_batch_rng(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                       const float mean[3], const float std[3], uint64_t seed, uint64_t offset, int kind,
                       const float params[5], void* stream) {
  if (int rc = pool_batch_check("pool_batch_rng", pool, N, index, out, B, H, W, mean, std)) return rc;
  D3F_CHECK(params != nullptr, "pool_batch_rng: params is null");
  AffineRngParams q;
  if (int rc = affine_rng_params(kind, params, H, W, q)) return rc;
  return pool_batch_launch(pool, N, index, out, B, H, W, mean, std, nullptr, nullptr, seed, offset, &q,
                           (hipStream_t)stream);
}

int d3f_pool_batch_balanced_rng(const uint8_t* pool, int64_t N, const int64_t* members, const int64_t* class_start, int Kn,
                                float* out, int64_t* index_out, int B, int H, int W, const float mean[3],
                                const float std[3], uint64_t seed, uint64_t offset, int kind, const float params[5],
                                void* stream) {
  const char* who = "pool_batch_balanced_rng";
  D3F_CHECK(members != nullptr, "%s: members is null", who);
  D3F_CHECK(class_start != nullptr, "%s: class_start is null", who);
  D3F_CHECK(index_out != nullptr || B == 0, "%s: index_out is null", who);
  D3F_CHECK(Kn >= 1, "%s: Kn %d < 1 (no class with an image)", who, Kn);
  D3F_CHECK(B <= 65535, "%s: B %d above 65535 images per launch", who, B);
  if (int rc = pool_batch_check(who, pool, N, index_out, out, B, H, W, mean, std)) return rc;
  AffineRngParams q;
  if (kind != D3F_AUGMENT_NONE) {
    D3F_CHECK(params != nullptr, "%s: params is null", who);
    if (int rc = affine_rng_params(kind, params, H, W, q)) return rc;
  }
  return pool_batch_balanced_launch(pool, N, members, class_start, Kn, out, index_out, B, H, W, mean, std, seed, offset,
                                    kind != D3F_AUGMENT_NONE ? &q : nullptr, (hipStream_t)stream);
}
int d3f_balanced_index_draw(const int64_t* members, const int64_t* class_start, int Kn, uint64_t seed, uint64_t offset,
                            int64_t* index_out, int B, void* stream) {
  const char* who = "balanced_index_draw";
  D3F_CHECK(members != nullptr, "%s: members is null", who);
  D3F_CHECK(class_start != nullptr, "%s: class_start is null", who);
  D3F_CHECK(index_out != nullptr || B == 0, "%s: index_out is null", who);
  D3F_CHECK(Kn >= 1, "%s: Kn %d < 1 (no class with an image)", who, Kn);
  D3F_CHECK(B >= 0, "%s: B %d < 0", who, B);
  D3F_CHECK(B <= 65535, "%s: B %d above 65535 images per launch", who, B);
  return balanced_index_draw_launch(members, class_start, Kn, seed, offset, index_out, B, (hipStream_t)stream);
}

int d3f_nchw_to_nhwc(int dtype, const float* in, void* out, int B, int C, int H, int W, int Cpad, void* stream) {
  D3F_CHECK(in && out && Cpad >= C, "nchw_to_nhwc: argument");
  return nchw_to_nhwc_launch(sdt(dtype), in, out, B, C, H, W, Cpad, (hipStream_t)stream);
}
int d3f_nhwc_to_nchw(int dtype, const void* in, float* out, int B, int C, int H, int W, int Cpad, void* stream) {
  D3F_CHECK(in && out && Cpad >= C, "nhwc_to_nchw: argument");
  return nhwc_to_nchw_launch(sdt(dtype), in, out, B, C, H, W, Cpad, (hipStream_t)stream);
}

// ---- training-step arithmetic ---------------------------------------------------------------
int d3f_noise_blend(const float* x, const float* noise, const float* y_uniform, float lam, float* out,
                    float* r_out_or_null, int B, int64_t per_image, void* stream) {
  if (B == 0 || per_image == 0) return 0;
  D3F_CHECK(x && noise && y_uniform && out, "noise_blend: null argument");
  return noise_blend_launch(x, noise, y_uniform, lam, out, r_out_or_null, B, (long)per_image,
                            (hipStream_t)stream);
}
int d3f_noise_blend_fixed(const float* x, const float* noise, const float* r, float* out, int B, int64_t per_image,
                          void* stream) {
  if (B == 0 || per_image == 0) return 0;
  D3F_CHECK(x && noise && r && out, "noise_blend_fixed: null argument");
  return noise_blend_fixed_launch(x, noise, r, out, B, (long)per_image, (hipStream_t)stream);
}
int d3f_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  D3F_CHECK(counter && key && out, "philox4x32_10: null argument");
  const Philox4 p = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = p.x[i];
  return 0;
}
int d3f_noise_blend_rng(const float* x, uint64_t seed, uint64_t offset, float lam, float* out, float* r_out_or_null,
                        int B, int64_t per_image, void* stream) {
  if (B == 0 || per_image == 0) return 0;
  D3F_CHECK(x && out && x != out, "noise_blend_rng: null or aliased argument");
  D3F_CHECK(B > 0 && per_image > 0, "noise_blend_rng: bad shape");
  return noise_blend_rng_launch(x, seed, offset, lam, out, r_out_or_null, B, (long)per_image, (hipStream_t)stream);
}
int d3f_noise_blend_fixed_rng(const float* x, uint64_t seed, uint64_t offset, const float* r, float* out, int B,
                              int64_t per_image, void* stream) {
  if (B == 0 || per_image == 0) return 0;
  D3F_CHECK(x && r && out && x != out, "noise_blend_fixed_rng: null or aliased argument");
  D3F_CHECK(B > 0 && per_image > 0, "noise_blend_fixed_rng: bad shape");
  return noise_blend_fixed_rng_launch(x, seed, offset, r, out, B, (long)per_image, (hipStream_t)stream);
}
int d3f_noise_blend_fixed_index_rng(const float* x, uint64_t seed, uint64_t offset, const float* r, const int64_t* index,
                                    float* out, int B, int64_t per_image, void* stream) {
  if (B == 0 || per_image == 0) return 0;
  D3F_CHECK(x && r && index && out && x != out, "noise_blend_fixed_index_rng: null or aliased argument");
  D3F_CHECK(B > 0 && per_image > 0, "noise_blend_fixed_index_rng: bad shape");
  return noise_blend_fixed_index_rng_launch(x, seed, offset, r, index, out, B, (long)per_image, (hipStream_t)stream);
}
int d3f_noise_draw(uint64_t seed, uint64_t offset, float* noise_or_null, float* y_or_null, int B, int64_t per_image,
                   void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(B > 0 && per_image >= 0, "noise_draw: bad shape");
  return noise_draw_launch(seed, offset, noise_or_null, y_or_null, B, (long)per_image, (hipStream_t)stream);
}
size_t d3f_l1_per_image_workspace_bytes(int B) { return l1_per_image_workspace_bytes(B); }
int d3f_l1_per_image(const float* prediction, const float* target, float* out, void* workspace, int B,
                     int64_t per_image, void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(prediction && target && out && workspace, "l1_per_image: null argument");
  return l1_per_image_launch(prediction, target, out, workspace, B, (long)per_image, (hipStream_t)stream);
}
int d3f_l1_per_image_scatter(const float* prediction, const float* target, const int64_t* index, float* scores, int N,
                             void* workspace, int B, int64_t per_image, void* stream) {
  if (B == 0) return 0;
  D3F_CHECK(prediction && target && index && scores && workspace, "l1_per_image_scatter: null argument");
  D3F_CHECK(B > 0 && N >= 0 && per_image > 0, "l1_per_image_scatter: bad shape");
  return l1_per_image_scatter_launch(prediction, target, index, scores, N, workspace, B, (long)per_image,
                                     (hipStream_t)stream);
}
size_t d3f_quality_per_image_workspace_bytes(int B, int H, int W) { return quality_per_image_workspace_bytes(B, H, W); }
int d3f_quality_per_image_scatter(const float* prediction, const float* target, float input_min, float input_max,
                                  const int64_t* index_or_null, float* metrics, int N, void* workspace, int B, int H, int W,
                                  void* stream) {
  // every refusal is the host's, made before a device call (quality_per_image_scatter_launch states the shape ones)
  D3F_CHECK(prediction && target && metrics && workspace, "quality_per_image_scatter: null argument");
  return quality_per_image_scatter_launch(prediction, target, input_min, input_max, index_or_null, metrics, N, workspace,
                                          B, H, W, (hipStream_t)stream);
}
size_t d3f_difficulty_classes_workspace_bytes(int N) { return difficulty_classes_workspace_bytes(N); }
int d3f_difficulty_classes(const float* scores, int N, int number_of_classes, int64_t* classes, int32_t* counts,
                           float* minmax, void* workspace, void* stream) {
  D3F_CHECK(counts && minmax, "difficulty_classes: null argument");
  D3F_CHECK(N <= 0 || (scores && classes && workspace), "difficulty_classes: null argument");
  return difficulty_classes_launch(scores, N, number_of_classes, classes, counts, minmax, workspace, (hipStream_t)stream);
}
size_t d3f_difficulty_histogram_u8_workspace_bytes(int N) { return difficulty_histogram_workspace_bytes(N); }
int d3f_difficulty_histogram_u8(const int64_t* classes, int N, int bins, int32_t* bin_counts, double* range, uint8_t* chart,
                                int H, int W, void* workspace, void* stream) {
  D3F_CHECK(bin_counts && range && chart && workspace, "difficulty_histogram_u8: null argument");
  D3F_CHECK(N <= 0 || classes, "difficulty_histogram_u8: null argument");
  return difficulty_histogram_u8_launch(classes, N, bins, bin_counts, range, chart, H, W, workspace, (hipStream_t)stream);
}
size_t d3f_mse_ssim_loss_workspace_bytes(int B, int H, int W) {
  return loss_workspace_floats(B, H, W) * sizeof(float);
}
int d3f_mse_ssim_loss(const float* pred, const float* target, float input_min, float input_max,
                      float* loss_out, float* grad_pred, void* workspace, int B, int H, int W, void* stream) {
  D3F_CHECK(pred && target && loss_out && grad_pred && workspace, "mse_ssim_loss: null argument");
  return mse_ssim_loss_launch(pred, target, input_min, input_max, loss_out, grad_pred,
                              reinterpret_cast<float*>(workspace), B, H, W, (hipStream_t)stream);
}
int d3f_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream) {
  D3F_CHECK(params && grads && exp_avg && exp_avg_sq, "adam_step: null argument");
  return adam_step_launch(params, grads, exp_avg, exp_avg_sq, (long)n, lr, beta1, beta2, eps, step,
                          grad_scale, (hipStream_t)stream);
}
int d3f_ema_lerp(float* ema, const float* online, int64_t n, float weight, void* stream) {
  D3F_CHECK(ema && online, "ema_lerp: null argument");
  return ema_lerp_launch(ema, online, (long)n, weight, (hipStream_t)stream);
}

}  // extern "C"
