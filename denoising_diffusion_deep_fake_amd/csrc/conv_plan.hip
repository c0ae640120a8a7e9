// One convolution layer planned once (host only): the geometry, the kernel-form decisions, the launch descriptions and the
// packed sizes that the whole-network engine (engine.hip) and the single-operator C API (c_api.hip) both read -- and the
// launches of the planned layer, which both issue through this file too.  Which dtype each rule sees is decided here and
// nowhere else: the layouts, the folding and the parity rule follow the storage dtype, the contraction plans and Winograd
// the compute dtype (D3F_F32X3 keeps fp32 storage).
#include "pointwise.h"

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

// two networks in one launch: every pointer of net 1 lies net_ws further on (the head's exceptions: conv_layer_forward)
static void net_conv(ConvParams& p, const NetSplit* ns) {
  if (ns != nullptr) {
    p.nets = ns->nets;
    p.net_ws = p.net_out0 = p.net_scale = ns->ws;
  }
}

int conv_layer_forward(const ConvLayer& L, const ConvFwdBufs& b, bool wino, hipStream_t s, const NetSplit* ns) {
  ConvParams p = L.fwd;
  p.src0 = b.src0; p.src1 = b.src1; p.w = b.w; p.out0 = b.out;
  net_conv(p, ns);
  if (L.head) {
    p.mode = CONV_HEAD_NCHW;
    p.scale = b.bias;
    if (ns != nullptr) {  // the prediction and the bias live outside the workspace
      p.net_out0 = ns->out;
      p.net_scale = ns->par;
    }
    return conv_igemm_launch(p, L.dtype, s);
  }
  p.partial = p.splitk > 1 ? b.slabs : nullptr;
  if (b.scale != nullptr) {
    p.mode = CONV_EVAL_FUSED;
    p.scale = b.scale; p.shift = b.shift; p.res = b.res; p.relu = b.relu;
  } else {
    p.mode = CONV_RAW_STATS;
    p.stats = b.stats;
    if (wino) p.stat_rows = L.wino_rows;  // one statistics row per workgroup
  }
  return wino ? conv_winograd_launch(p, s) : conv_igemm_launch(p, L.dtype, s);
}

int conv_layer_dgrad(const ConvLayer& L, const ConvDgradBufs& b, hipStream_t s, const NetSplit* ns) {
  // the launch that writes dx0 (it alone carries the fused reduction)
  ConvParams p = L.upfold ? L.dgrad_lo : L.dgrad;
  p.src0 = b.dy; p.w = b.w; p.out0 = b.dx0; p.acc0 = b.acc0;
  if (!L.upfold) {
    p.out1 = b.dx1;
    p.acc1 = b.acc1;
  }
  p.partial = p.splitk > 1 ? b.slabs : nullptr;
  p.bn_y = b.bn_y; p.bn_coef = b.bn_coef; p.bn_partial = b.bn_partial; p.bn_a = b.bn_a;
  net_conv(p, ns);
  if (p.par == 2 && !p.acc0) {  // 1x1 stride 2: only even pixels receive a gradient; the others are zero
    const NetSplit nv = net_split_or_single(ns);
    for (int n = 0; n < nv.nets; ++n)
      D3F_HIP(hipMemsetAsync(reinterpret_cast<char*>(b.dx0) + (size_t)n * nv.ws, 0,
                             (size_t)4 * p.M * p.Cout * (L.sdtype == D3F_F32 ? 4 : 2), s));
  }
  if (int rc = conv_igemm_launch(p, L.dtype, s)) return rc;
  if (!L.upfold || L.C1 == 0) return 0;
  // an up-folded layer's skip tensor: an ordinary 3x3 data gradient of its own
  ConvParams k = L.dgrad;
  k.src0 = b.dy; k.w = b.w_skip; k.out0 = b.dx1; k.acc0 = b.acc1;
  k.partial = k.splitk > 1 ? b.slabs : nullptr;
  net_conv(k, ns);
  return conv_igemm_launch(k, L.dtype, s);
}

int conv_pack_entry(const ConvLayer& L, long w_off, size_t wf_off, size_t wd_off, bool fwd, bool dgrad, uint32_t block0,
                    PackEntry& e) {
  const int taps = L.KH * L.KW;
  const long nf = fwd ? (long)L.CoutPad * L.Kpad : 0, nd = dgrad ? (long)L.CinRows * L.KpadD : 0;
  D3F_CHECK((!fwd || L.Kpad >= taps * L.Cin) && (!dgrad || L.KpadD >= taps * L.CoutD), "pack_weights: padded K too small");
  // 16-bit extents, 32-bit element indices (pack_all_kernel)
  const int extent = std::max({L.Cout, L.CinReal, L.Cin, L.CoutPad, L.Kpad, L.CinRows, L.CoutD, L.KpadD});
  D3F_CHECK(extent < 65536 && nf + nd < 0x7fffffffL,
            "pack_weights: the layer exceeds the packing table (extents below 65536, fewer than 2^31 packed elements): "
            "extent %d, %ld elements", extent, nf + nd);
  D3F_CHECK(w_off >= 0 && w_off <= 0xffffffffL && wf_off % 16 == 0 && wd_off % 16 == 0 && (wf_off >> 4) < 0xffffffffull &&
                (wd_off >> 4) < 0xffffffffull,
            "pack_weights: layer out of table range");
  D3F_CHECK(taps <= PACK_LDS_ROW, "pack_weights: %d taps exceed the tile", taps);
  int CT = 32;
  while (CT * taps > PACK_LDS_ROW) CT >>= 1;
  const int crows = std::max(fwd ? L.Cin : 0, dgrad ? L.CinRows : 0);
  const int nrows = std::max(fwd ? L.CoutPad : 0, dgrad ? L.CoutD : 0);
  unsigned mul, shr;
  fast_div_setup((unsigned)taps, &mul, &shr);
  e = PackEntry{};
  e.w_off = (uint32_t)w_off;
  e.wf_off16 = (uint32_t)(wf_off >> 4);
  e.wd_off16 = (uint32_t)(wd_off >> 4);
  e.block0 = block0;
  e.Cout = (uint16_t)L.Cout; e.CinReal = (uint16_t)L.CinReal; e.Cin = (uint16_t)L.Cin;
  e.taps = (uint16_t)taps; e.CoutPad = (uint16_t)L.CoutPad; e.Kpad = (uint16_t)L.Kpad;
  e.CinRows = (uint16_t)L.CinRows; e.CoutD = (uint16_t)L.CoutD; e.KpadD = (uint16_t)L.KpadD;
  e.has_f = fwd ? 1 : 0;
  e.has_d = dgrad ? 1 : 0;
  e.conv_stride = (dgrad && L.parity) ? 2 : 1;
  e.CT = (uint16_t)CT;
  e.ctiles = (uint16_t)((crows + CT - 1) / CT);
  e.taps_mul = mul;
  e.taps_shr = (uint16_t)shr;
  e.ct_log2 = (uint16_t)__builtin_ctz((unsigned)CT);
  return e.ctiles * ((nrows + PACK_NT - 1) / PACK_NT);
}

}  // namespace d3f
