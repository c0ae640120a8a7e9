// One convolution layer planned once (host only): the geometry, the kernel-form decisions, the launch descriptions and the
// packed sizes that the whole-network engine (engine.hip) and the single-operator C API (c_api.hip) both read.  Which
// dtype each rule sees is decided here and nowhere else: the layouts, the folding and the parity rule follow the storage
// dtype, the contraction plans and Winograd the compute dtype (D3F_F32X3 keeps fp32 storage).
#include "common.h"

#include <algorithm>

namespace d3f {

// L: a fresh description (every plan field at its default)
int conv_layer_plan(ConvLayer& L) {
  D3F_CHECK(L.dtype == D3F_F32 || L.dtype == D3F_BF16 || L.dtype == D3F_F32X3, "conv: dtype %d", L.dtype);
  L.sdtype = L.dtype == D3F_F32X3 ? D3F_F32 : L.dtype;
  const int ve = L.sdtype == D3F_F32 ? 4 : 8, bke = L.sdtype == D3F_F32 ? 32 : 64;
  const size_t wsz = L.dtype == D3F_F32X3 ? 6 : L.sdtype == D3F_F32 ? 4 : 2;  // bytes per packed weight (x3: three bf16 planes)
  D3F_CHECK(L.B >= 0 && L.Hv > 0 && L.Wv > 0 && L.C0 > 0 && L.C1 >= 0 && L.Cout > 0, "conv: extent");
  D3F_CHECK(L.C0 % ve == 0 && L.C1 % ve == 0, "conv: channels must be multiples of %d", ve);
  D3F_CHECK(L.KH == L.KW && L.KH >= 1 && L.KH <= 7, "conv: kernel %dx%d", L.KH, L.KW);
  D3F_CHECK(L.stride == 1 || L.stride == 2, "conv: stride %d", L.stride);
  D3F_CHECK(!L.up0 || (L.Hv % 2 == 0 && L.Wv % 2 == 0), "conv: up-sampled extent must be even");
  D3F_CHECK(L.CinReal > 0 && L.CinReal <= L.C0 + L.C1, "conv: CinReal");

  // ---- geometry and packed sizes ----
  const int B = L.B, K = L.KH;
  L.Cin = L.C0 + L.C1;
  L.Ho = (L.Hv + 2 * L.pad - K) / L.stride + 1;
  L.Wo = (L.Wv + 2 * L.pad - K) / L.stride + 1;
  L.CoutPad = (int)round_up(L.Cout, 16);
  L.Kpad = (int)round_up((long)K * K * L.Cin, bke);
  L.CoutD = (int)round_up(L.Cout, ve);
  L.KpadD = (int)round_up((long)K * K * L.CoutD, bke);
  L.CinRows = (int)round_up(L.Cin, 16);
  L.C0Rows = (int)round_up(L.C0, 16);
  L.C1Rows = (int)round_up(L.C1, 16);
  L.macs = (double)B * L.Ho * L.Wo * L.Cout * K * K * L.CinReal;
  // conv(cat(upsample2x(src0), src1)) with the up-sampling folded into pre-summed weights (ConvParams::par == 3 forward,
  // 4x4 stride-2 data gradient): needs whole k-tiles per tap in both sources
  static const bool no_upfold = prof_knob("D3F_NO_UPFOLD") != nullptr;  // debugging knob: gather through the up-sampling
  L.upfold = !no_upfold && L.up0 && K == 3 && L.stride == 1 && L.pad == 1 && L.C0 % bke == 0 && L.C1 % bke == 0;
  // the data gradient as output-parity classes (ConvParams::par 1 / 2); the weight packers store the flipped taps class
  // by class exactly when it does
  L.parity = L.stride == 2 && L.C1 == 0 && L.CoutD % bke == 0 && ((K == 3 && L.pad == 1) || (K == 1 && L.pad == 0));
  L.wf = (size_t)L.CoutPad * L.Kpad * wsz;
  L.wd = (size_t)L.CinRows * L.KpadD * wsz;
  if (L.upfold) {  // four per-class forward matrices; data gradient: wd4 (low-resolution source) | wds (skip tensor)
    L.wfc = (size_t)4 * L.CoutPad * (4 * L.C0 + 9 * L.C1) * wsz;
    L.wd4 = (size_t)L.C0Rows * 16 * L.CoutD * wsz;
    L.wds = (size_t)L.C1Rows * L.KpadD * wsz;
  }
  auto plan = [&](ConvParams& p, double flops) {
    p.plan_nets = L.plan_nets;
    p.flops = flops;
    const int rc = conv_igemm_plan(p, L.dtype, L.allow_splitk);
    L.splitk_floats = std::max(L.splitk_floats, conv_splitk_floats(p));
    return rc;
  };

  // ---- forward ----
  if (L.need_fwd) {
    ConvParams& f = L.fwd;
    f.B = B; f.Hv = L.Hv; f.Wv = L.Wv; f.C0 = L.C0; f.C1 = L.C1; f.cin_real = L.CinReal;
    f.H0s = L.Hv >> L.up0; f.W0s = L.Wv >> L.up0; f.shift0 = L.up0;
    f.Ho = L.Ho; f.Wo = L.Wo; f.Cout = L.Cout; f.CoutPad = L.CoutPad; f.Kpad = L.Kpad;
    f.KH = f.KW = K; f.stride = L.stride; f.pad = L.pad;
    f.M = B * L.Ho * L.Wo;
    f.mode = L.head ? CONV_HEAD_NCHW : CONV_RAW_STATS;
    if (L.upfold) {  // rows = one output-parity class; src0 described at its own (low) resolution
      f.par = 3;
      f.shift0 = 0;
      f.Ho = f.H0s; f.Wo = f.W0s;
      f.M = B * f.H0s * f.W0s;
      f.Kpad = 4 * L.C0 + 9 * L.C1;
    }
    if (int rc = plan(f, 2.0 * L.macs)) return rc;
    L.wino = conv_winograd_applies(f, L.dtype);
    const bool fits = conv_winograd_fits(f, L.dtype);
    L.wino_rows = fits ? conv_winograd_stat_rows(f) : 0;
    L.wu = fits ? conv_winograd_filter_floats(f) * sizeof(float) : 0;
  }

  // ---- weight gradient: the passes of conv_wgrad.hip (class form behind an up-sampling where it applies) ----
  if (L.need_wgrad) {
    WgradParams g{};
    g.B = B; g.Hv = L.Hv; g.Wv = L.Wv; g.C0 = L.C0; g.C1 = L.C1;
    g.H0s = L.Hv >> L.up0; g.W0s = L.Wv >> L.up0; g.shift0 = L.up0;
    g.Ho = L.Ho; g.Wo = L.Wo; g.Cout = L.CoutD;
    g.KH = g.KW = K; g.stride = L.stride; g.pad = L.pad; g.M = B * L.Ho * L.Wo;
    g.cin_real = L.CinReal;
    g.flops = 2.0 * L.macs;
    g.plan_nets = L.plan_nets;
    if (int rc = wgrad_layer_plan(L.wl, g, L.sdtype)) return rc;
    L.wslab_bytes = wgrad_layer_partial_floats(L.wl) * sizeof(float);
  }

  // ---- data gradient ----
  if (!L.need_dgrad) return 0;
  D3F_CHECK(L.stride == 2 ? (L.Ho * 2 == L.Hv && L.Wo * 2 == L.Wv) : (L.Ho == L.Hv && L.Wo == L.Wv),
            "conv_backward_data: needs a 'same' (stride 1) or exactly halving (stride 2) conv");
  ConvParams dy{};  // every data-gradient launch reads dY [B][Ho][Wo][CoutD]
  dy.B = B; dy.C0 = L.CoutD;
  dy.mode = CONV_DGRAD;
  ConvParams& d = L.dgrad;
  if (L.upfold) {
    // (1) the low-resolution source: 4x4 stride-2 pad-1 convolution over dY with pre-summed weights, written at [B][H/2][W/2]
    ConvParams& l = L.dgrad_lo;
    l = dy;
    l.Hv = l.H0s = L.Hv; l.Wv = l.W0s = L.Wv;
    l.Ho = L.Hv / 2; l.Wo = L.Wv / 2;
    l.Cout = l.out_c0 = L.C0; l.CoutPad = L.C0Rows; l.Kpad = 16 * L.CoutD;
    l.KH = l.KW = 4; l.stride = 2; l.pad = 1;
    l.M = B * l.Ho * l.Wo;
    if (int rc = plan(l, 2.0 * L.macs * L.C0 / L.Cin)) return rc;
    // (2) the skip tensor: an ordinary 3x3 data gradient with C1 outputs
    if (L.C1 == 0) return 0;
    d = dy;
    d.Hv = d.H0s = d.Ho = L.Hv; d.Wv = d.W0s = d.Wo = L.Wv;
    d.Cout = d.out_c0 = L.C1; d.CoutPad = L.C1Rows; d.Kpad = L.KpadD;
    d.KH = d.KW = 3; d.stride = 1; d.pad = 1;
    d.M = B * L.Hv * L.Wv;
    return plan(d, 2.0 * L.macs * L.C1 / L.Cin);
  }
  d = dy;
  d.Cout = L.Cin; d.CoutPad = L.CinRows; d.Kpad = L.KpadD;
  d.out_c0 = L.C1 > 0 ? L.C0 : L.Cin;
  if (L.parity) {
    // stride 2: four plain sub-convolutions over dY, one per output-parity class (conv_igemm.hip)
    d.par = K == 3 ? 1 : 2;
    d.Hv = d.Ho = d.H0s = L.Ho; d.Wv = d.Wo = d.W0s = L.Wo;
    d.KH = d.KW = K == 3 ? 2 : 1; d.stride = 1; d.pad = 0;
    d.M = B * L.Ho * L.Wo;
  } else {
    const int s2 = L.stride == 2 ? 1 : 0;
    d.Hv = L.Hv; d.Wv = L.Wv;  // extent of the (zero-inserted) dY == extent of dX
    d.H0s = L.Ho; d.W0s = L.Wo; d.shift0 = s2; d.zi = s2;
    d.Ho = L.Hv; d.Wo = L.Wv;
    d.KH = d.KW = K; d.stride = 1; d.pad = K - 1 - L.pad;
    d.M = B * L.Hv * L.Wv;
    // a source read through the up-sampling without folded weights: ask for the gradient at the source's own resolution,
    // 2x2 blocks summed in the epilogue; the plan keeps the request only where a patch kernel takes the launch
    // (conv_patch.hip), otherwise full-resolution output that the caller sums itself
    d.sum2 = (L.want_sum2 && L.up0 && L.C1 == 0) ? 1 : 0;
  }
  return plan(d, 2.0 * L.macs);
}

}  // namespace d3f
