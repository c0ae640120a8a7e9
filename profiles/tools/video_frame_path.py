"""The frame path of script_tools at the authors' size, 1080x1920 BGR frames -> 448x448 (HIP events, device resident).

  resize       : d3f_crop_resize_cubic_u8 alone (centre crop 1080x1080 -> 448x448), B = 1 and B = 8; and its
                 global-tap form at 2160x3840 -> 64x64
  frames       : Unet.predict_frames_u8 (resize + forward + real|fake pair), B = 1 eager / hipGraph, B = 8 eager
  yardstick    : Unet.predict_u8 on frames that are ALREADY 448x448 (what the parent commit offers), same B and mode
  paste        : d3f_paste_resize_cubic_u8 alone (448x448 -> the 1080x1080 centre box of the 1080x1920 frame, default
                 feather 67), out of place (the whole frame is written) and in place (only the box's tiles), B = 1 and 8
  full         : Unet.predict_frames_full_u8 (frames + paste), B = 1 eager / hipGraph, B = 8 eager; the added time per
                 frame against predict_frames_u8 in the same run, next to the byte-bound estimate of the paste

  --antialias  : instead of the above, d3f_crop_resize_cubic_aa_u8 next to d3f_crop_resize_cubic_u8 on the same inputs and
                 Unet.predict_u8 (the eval forward of the same call) at the same size: 1080x1920 -> 448x448 and 256x256,
                 2160x3840 -> 256x256, B = 1 and B = 8; with the byte bound (crop read once, output written once)

  --color      : instead of the above, the colour match of the full-frame output: Unet.predict_frames_full_u8 with
                 color_match=None and "meanstd" (two networks, so that neither handle's mode ever changes and no graph is
                 re-captured inside a timed block), eager and hipGraph, next to the operators the mode adds -- the sums of
                 both halves of the pair (two d3f_channel_sums_u8 calls: each a zeroing launch and the sums kernel, where the
                 fused call takes both halves in one launch and zeroes nothing), d3f_color_match_coef, and the paste in its
                 plain and colour forms: 1080x1920 -> 448x448 and 256x256, B = 1 and B = 8; with the byte bound of the sums
                 (2 * H * W * 3 bytes read per frame).  On a library without the colour entries (an older build named
                 through D3F_LIB), or with --off-only, only the color_match=None forms run: the parent's figures for the
                 same launches, and this library's in the same sequence of allocations and captures (the hipGraph figures
                 depend on that sequence: profiles/README.md "Colour match")

  --temporal   : instead of the above, the temporal filter of the two frame entries: Unet.predict_frames_u8 and
                 Unet.predict_frames_full_u8 with color_match="meanstd", each with temporal=None and temporal=0.75 (two
                 networks, so that neither handle's setting ever changes inside a timed block), eager and hipGraph, next to
                 the filter operator alone on the halves of the pair: 1080x1920 -> 448x448 and 256x256, B = 1 and B = 8; with
                 the filter's byte bound (H * W * 3 bytes read twice and written once per frame, plus 15 bytes per pixel of
                 state read and written once per call).  The same raw frames every call, so the gate is fully open (k = s
                 everywhere): the kernel's work does not depend on the data.  With --off-only, or on a library without the
                 entries (an older build named through D3F_LIB), only the temporal=None forms run: the parent's figures for
                 the same launches, in the same sequence of allocations and captures

  --boxes      : instead of the above, the tracked crop: the per-frame-box forms with ALL boxes equal to the centre box next
                 to the single-box forms on the same inputs -- the crop alone (plain; out=), the paste alone (out of place,
                 default feather) and the whole Unet.predict_frames_full_u8 call, eager; and the single-box call's hipGraph
                 replay at B = 1, which a tracked call gives up: 1080x1920 -> 448x448 and 256x256, B = 1 and B = 8.  On a
                 library without the boxes entries (the parent's build named through D3F_LIB), or with --off-only, only the
                 single-box forms run: the same sequence of calls on both sides of an A/B of the unchanged path

  --blend      : instead of the above, the multiband paste of the full-frame output: Unet.predict_frames_full_u8 with blend=None
                 and blend="multiband" (two networks, so that neither handle's mode ever changes inside a timed block), eager,
                 next to Unet.predict_u8 (the forward pass the paste follows) and the two paste operators alone, out of place:
                 1080x1920 -> 448x448 and 256x256, centre box, default feather and levels, B = 1 and B = 8; with the byte
                 bound of the multiband launches -- patch and box read by the first launch, the frame read and written by the
                 last, every int16 plane g_l written once and read twice (REDUCE, and the collapse of its level; g_N once),
                 every int32 plane R_l (l = 1 .. N - 1) written once and read once

  --rotate     : instead of the above, the rotated crop and paste: the _rboxes_ forms at 0.01 and at 20 degrees next to the
                 _boxes_ forms on the same boxes (every box the centre box) in the same run -- the crop alone (out=) and the paste
                 alone (out of place, default feather): 1080x1920 -> 448x448 and 256x256, B = 1 and B = 8; with the LDS bytes a
                 workgroup's tile may stage in each form (the launch's bound: rows times pitch), which is what the rotated
                 forms pay for first.  With --off-only only the _boxes_ forms run

Back-to-back enqueues on one stream, ITERS iterations after WARMUP, the forms alternating in ROUNDS rounds; the figure is
the median round's time per call (and per frame).  Host work of the reference's loop (cv2.resize on one CPU thread, the
concatenate, two PCIe trips) is not part of any figure here.  One JSON line at the end.
    python profiles/tools/video_frame_path.py [--precision f32|bf16] [--iters N] [--antialias | --color [--off-only] | --temporal [--off-only] | --boxes [--off-only] | --blend | --rotate [--off-only]]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from denoising_diffusion_deep_fake_amd import Unet, _lib, ops

RAW, SIZE = (1080, 1920), (448, 448)
MEAN, STD = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def compare(forms, warmup, iters, rounds):
    """forms: {name: callable}; returns {name: (median, min, max)} in us per call, the forms alternating"""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def antialias_section(net, args, g):
    """the antialiased resize against the plain one and the eval forward, per frame; one JSON line"""
    result = {"precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds,
              "antialias_us_per_frame": {}}
    for raw_hw, side in (((1080, 1920), 448), ((1080, 1920), 256), ((2160, 3840), 256)):
        size = (side, side)
        box = ops.center_crop_box(raw_hw[0], raw_hw[1], side, side)
        need = box[2] * box[3] * 3 + side * side * 3  # bytes per frame: the crop read once, the output written once
        for B in (1, 8):
            raw = torch.randint(0, 256, (B,) + raw_hw + (3,), generator=g, dtype=torch.uint8).cuda()
            small = ops.crop_resize_cubic_u8(raw, size, antialias=True)
            resized, fake = torch.empty_like(small), torch.empty_like(small)
            forms = {
                "plain": lambda: ops.crop_resize_cubic_u8(raw, size, out=resized),
                "antialias": lambda: ops.crop_resize_cubic_u8(raw, size, out=resized, antialias=True),
                "predict_u8": lambda: net.predict_u8(small, MEAN, STD, graph=False, out=fake),
            }
            t = {name: med / B for name, (med, _, _) in compare(forms, args.warmup, args.iters, args.rounds).items()}
            bound = need / 6.3e12 * 1e6  # at 6.3 TB/s achievable HBM
            key = f"{raw_hw[0]}x{raw_hw[1]}_to_{side}_B{B}"
            print(f"{key:28s} plain {t['plain']:8.2f}  antialias {t['antialias']:8.2f}  predict_u8 {t['predict_u8']:9.1f} us per "
                  f"frame; {need} bytes per frame, byte bound {bound:.2f} us, antialias at {t['antialias'] / bound:.1f} times it")
            result["antialias_us_per_frame"][key] = {"plain": round(t["plain"], 2), "antialias": round(t["antialias"], 2),
                                                     "predict_u8": round(t["predict_u8"], 1), "bytes": need,
                                                     "byte_bound_us": round(bound, 2)}
            del raw
    print(json.dumps(result))


def color_section(args, g):
    """the colour match mode against the same call without it, and the operators it adds, per frame; one JSON line"""
    has_color = hasattr(_lib.lib(), "d3f_unet_set_frame_color_match") and not args.off_only
    result = {"precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds,
              "has_color": has_color, "color_us_per_frame": {}}
    torch.manual_seed(0)
    net_off = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    net_on = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    for side in (448, 256):
        size = (side, side)
        box = ops.center_crop_box(RAW[0], RAW[1], side, side)
        feather = ops.default_feather(box[2], box[3])
        need = 2 * side * side * 3  # bytes the sums read per frame: both halves of the pair once
        bound = need / 6.3e12 * 1e6  # at 6.3 TB/s achievable HBM
        for B in (1, 8):
            raw = torch.randint(0, 256, (B,) + RAW + (3,), generator=g, dtype=torch.uint8).cuda()
            pair = net_off.predict_frames_u8(raw, size, MEAN, STD, graph=False).clone()
            bufs = {k: (torch.empty_like(raw), torch.empty_like(pair)) for k in ("oe", "og", "me", "mg")}
            full = torch.empty_like(raw)

            def call(net, key, graph, mode):
                return lambda: net.predict_frames_full_u8(raw, size, MEAN, STD, graph=graph, out=bufs[key][0],
                                                          pair_out=bufs[key][1], color_match=mode)
            forms = {"off_eager": call(net_off, "oe", False, None), "off_graph": call(net_off, "og", True, None),
                     "paste": lambda: ops.paste_resize_cubic_u8(pair[:, :, side:], raw, box, feather, out=full)}
            if has_color:
                s_to = ops.channel_sums_u8(pair[:, :, :side])
                s_from = ops.channel_sums_u8(pair[:, :, side:])
                coef = ops.color_match_coef(s_from, s_to, side * side)

                def both_sums():
                    ops.channel_sums_u8(pair[:, :, :side], out=s_to)
                    ops.channel_sums_u8(pair[:, :, side:], out=s_from)
                forms.update({
                    "meanstd_eager": call(net_on, "me", False, "meanstd"), "meanstd_graph": call(net_on, "mg", True, "meanstd"),
                    "sums_both_halves_ops": both_sums,
                    "coef_op": lambda: ops.color_match_coef(s_from, s_to, side * side),
                    "paste_color": lambda: ops.paste_resize_cubic_u8(pair[:, :, side:], raw, box, feather, out=full, color=coef),
                })
            t = compare(forms, args.warmup, args.iters, args.rounds)
            key = f"{RAW[0]}x{RAW[1]}_to_{side}_B{B}"
            row = {}
            for name, (med, lo, hi) in t.items():
                print(f"{key:24s} {name:22s} {med / B:9.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f})")
                row[name] = [round(med / B, 2), round(lo / B, 2), round(hi / B, 2)]
            if has_color:
                row["added_eager"] = round((t["meanstd_eager"][0] - t["off_eager"][0]) / B, 2)
                row["added_graph"] = round((t["meanstd_graph"][0] - t["off_graph"][0]) / B, 2)
                row["sums_bytes"], row["sums_byte_bound_us"] = need, round(bound, 3)
                print(f"{key:24s} colour match adds {row['added_eager']:.2f} (eager) / {row['added_graph']:.2f} (hipGraph) us per "
                      f"frame; the sums read {need} bytes per frame, byte bound {bound:.3f} us")
            result["color_us_per_frame"][key] = row
            del raw, bufs, full
    print(json.dumps(result))


def temporal_section(args, g):
    """the temporal filter mode against the same calls without it, and the filter operator alone, per frame; one JSON line"""
    has_temporal = hasattr(_lib.lib(), "d3f_unet_set_frame_temporal") and not args.off_only
    result = {"precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds,
              "has_temporal": has_temporal, "temporal_us_per_frame": {}}
    torch.manual_seed(0)
    net_off = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    net_on = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    for side in (448, 256):
        size = (side, side)
        for B in (1, 8):
            # bytes the filter must move per frame: real read, fake read and written, and the state once per call
            need = 3 * side * side * 3 + 2 * 15 * side * side // B
            bound = need / 6.3e12 * 1e6  # at 6.3 TB/s achievable HBM
            raw = torch.randint(0, 256, (B,) + RAW + (3,), generator=g, dtype=torch.uint8).cuda()
            pair = net_off.predict_frames_u8(raw, size, MEAN, STD, graph=False).clone()
            names = ("fe", "fg", "ue", "ug", "tfe", "tfg", "tue", "tug")
            bufs = {k: (torch.empty_like(raw), torch.empty_like(pair)) for k in names}

            def frames(net, key, graph, **kw):
                return lambda: net.predict_frames_u8(raw, size, MEAN, STD, graph=graph, out=bufs[key][1], **kw)

            def full(net, key, graph, **kw):
                return lambda: net.predict_frames_full_u8(raw, size, MEAN, STD, graph=graph, out=bufs[key][0],
                                                          pair_out=bufs[key][1], color_match="meanstd", **kw)
            forms = {"frames_off_eager": frames(net_off, "fe", False), "frames_off_graph": frames(net_off, "fg", True),
                     "full_off_eager": full(net_off, "ue", False), "full_off_graph": full(net_off, "ug", True)}
            if has_temporal:
                state = ops.TemporalState(side, side)
                forms.update({
                    "frames_on_eager": frames(net_on, "tfe", False, temporal=0.75),
                    "frames_on_graph": frames(net_on, "tfg", True, temporal=0.75),
                    "full_on_eager": full(net_on, "tue", False, temporal=0.75),
                    "full_on_graph": full(net_on, "tug", True, temporal=0.75),
                    "filter_op": lambda: ops.temporal_filter_u8(pair[:, :, :side], pair[:, :, side:], state),
                })
            t = compare(forms, args.warmup, args.iters, args.rounds)
            key = f"{RAW[0]}x{RAW[1]}_to_{side}_B{B}"
            row = {}
            for name, (med, lo, hi) in t.items():
                print(f"{key:24s} {name:18s} {med / B:9.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f})")
                row[name] = [round(med / B, 2), round(lo / B, 2), round(hi / B, 2)]
            if has_temporal:
                for what in ("frames", "full"):
                    for mode in ("eager", "graph"):
                        row[f"{what}_added_{mode}"] = round((t[f"{what}_on_{mode}"][0] - t[f"{what}_off_{mode}"][0]) / B, 2)
                row["filter_bytes"], row["filter_byte_bound_us"] = need, round(bound, 3)
                row["filter_op_times_bound"] = round(t["filter_op"][0] / B / bound, 1)
                print(f"{key:24s} the mode adds {row['frames_added_eager']:.2f} / {row['frames_added_graph']:.2f} us per frame to "
                      f"predict_frames_u8 (eager / hipGraph), {row['full_added_eager']:.2f} / {row['full_added_graph']:.2f} to "
                      f"predict_frames_full_u8 with colour match; the filter moves {need} bytes per frame, byte bound "
                      f"{bound:.3f} us, the operator (kernel and state launch) at {row['filter_op_times_bound']:.1f} times it")
            result["temporal_us_per_frame"][key] = row
            del raw, bufs
    print(json.dumps(result))


def boxes_section(args, g):
    """the per-frame-box forms (every box the centre box) against the single-box forms, per frame; one JSON line"""
    has_boxes = hasattr(_lib.lib(), "d3f_unet_predict_frames_full_boxes_u8") and not args.off_only
    result = {"precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds,
              "has_boxes": has_boxes, "boxes_us_per_frame": {}}
    torch.manual_seed(0)
    net = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    for side in (448, 256):
        size = (side, side)
        box = ops.center_crop_box(RAW[0], RAW[1], side, side)
        feather = ops.default_feather(box[2], box[3])
        for B in (1, 8):
            raw = torch.randint(0, 256, (B,) + RAW + (3,), generator=g, dtype=torch.uint8).cuda()
            small = ops.crop_resize_cubic_u8(raw, size)
            resized = torch.empty_like(small)
            bufs = {k: (torch.empty_like(raw), torch.empty((B, side, 2 * side, 3), dtype=torch.uint8, device="cuda"))
                    for k in ("e", "g", "b")}
            full = torch.empty_like(raw)
            many = [box] * B
            forms = {
                "crop_box": lambda: ops.crop_resize_cubic_u8(raw, size, box=box, out=resized),
                "paste_box": lambda: ops.paste_resize_cubic_u8(small, raw, box, feather, out=full),
                "full_box_eager": lambda: net.predict_frames_full_u8(raw, size, MEAN, STD, feather=feather, graph=False,
                                                                     out=bufs["e"][0], pair_out=bufs["e"][1]),
            }
            if B == 1:
                forms["full_box_graph"] = lambda: net.predict_frames_full_u8(raw, size, MEAN, STD, feather=feather, graph=True,
                                                                             out=bufs["g"][0], pair_out=bufs["g"][1])
            if has_boxes:
                forms.update({
                    "crop_boxes": lambda: ops.crop_resize_cubic_u8(raw, size, boxes=many, out=resized),
                    "paste_boxes": lambda: ops.paste_resize_cubic_u8(small, raw, boxes=many, feather=feather, out=full),
                    "full_boxes_eager": lambda: net.predict_frames_full_u8(raw, size, MEAN, STD, feather=feather, boxes=many,
                                                                           out=bufs["b"][0], pair_out=bufs["b"][1]),
                })
            t = compare(forms, args.warmup, args.iters, args.rounds)
            key = f"{RAW[0]}x{RAW[1]}_to_{side}_B{B}"
            row = {}
            for name, (med, lo, hi) in t.items():
                print(f"{key:24s} {name:18s} {med / B:9.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f})")
                row[name] = [round(med / B, 2), round(lo / B, 2), round(hi / B, 2)]
            result["boxes_us_per_frame"][key] = row
            del raw, bufs, full
    print(json.dumps(result))


def multiband_bytes(H, W, h, w, cw, ch, levels):
    """bytes per frame the multiband launches must move (see --blend above)"""
    plane = [3 * -(-ch // (1 << l)) * -(-cw // (1 << l)) for l in range(levels + 1)]
    total = H * W * 3 + cw * ch * 3 + 2 * h * w * 3             # patch and box in; frame in, frame out
    total += sum(2 * p for p in plane)                            # every g_l written
    total += sum(2 * 2 * p for p in plane[:-1]) + 2 * plane[-1]   # g_l read by REDUCE and by its collapse; g_N once
    total += sum(2 * 4 * p for p in plane[1:-1])                  # R_l written and read
    return total


def blend_section(args, g):
    """the multiband paste against the plain one inside the whole call and alone, per frame; one JSON line"""
    result = {"precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds,
              "blend_us_per_frame": {}}
    torch.manual_seed(0)
    net_off = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    net_on = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    for side in (448, 256):
        size = (side, side)
        box = ops.center_crop_box(RAW[0], RAW[1], side, side)
        feather = ops.default_feather(box[2], box[3])
        levels = ops.multiband_levels(feather)
        need = multiband_bytes(side, side, RAW[0], RAW[1], box[2], box[3], levels)
        bound = need / 6.3e12 * 1e6  # at 6.3 TB/s achievable HBM
        plain_bound = 2 * RAW[0] * RAW[1] * 3 / 6.3e12 * 1e6
        for B in (1, 8):
            raw = torch.randint(0, 256, (B,) + RAW + (3,), generator=g, dtype=torch.uint8).cuda()
            pair = net_off.predict_frames_u8(raw, size, MEAN, STD, graph=False).clone()
            small = pair[:, :, :side].contiguous()
            fake = torch.empty_like(small)
            bufs = {k: (torch.empty_like(raw), torch.empty_like(pair)) for k in ("off", "on")}
            full = torch.empty_like(raw)
            forms = {
                "full_feather_eager": lambda: net_off.predict_frames_full_u8(raw, size, MEAN, STD, graph=False, out=bufs["off"][0],
                                                                             pair_out=bufs["off"][1]),
                "full_multiband_eager": lambda: net_on.predict_frames_full_u8(raw, size, MEAN, STD, graph=False,
                                                                              out=bufs["on"][0], pair_out=bufs["on"][1],
                                                                              blend="multiband"),
                "predict_u8": lambda: net_off.predict_u8(small, MEAN, STD, graph=False, out=fake),
                "paste_op": lambda: ops.paste_resize_cubic_u8(pair[:, :, side:], raw, box, feather, out=full),
                "multiband_op": lambda: ops.paste_multiband_u8(pair[:, :, side:], raw, box, feather, levels, out=full),
            }
            t = compare(forms, args.warmup, args.iters, args.rounds)
            key = f"{RAW[0]}x{RAW[1]}_to_{side}_B{B}"
            row = {}
            for name, (med, lo, hi) in t.items():
                print(f"{key:24s} {name:22s} {med / B:9.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f})")
                row[name] = [round(med / B, 2), round(lo / B, 2), round(hi / B, 2)]
            row["added_eager"] = round((t["full_multiband_eager"][0] - t["full_feather_eager"][0]) / B, 2)
            row["added_share_of_predict_u8"] = round(row["added_eager"] / (t["predict_u8"][0] / B), 4)
            row["feather"], row["levels"], row["launches"] = feather, levels, 2 * levels + 1
            row["multiband_bytes"], row["multiband_byte_bound_us"] = need, round(bound, 2)
            row["multiband_op_times_bound"] = round(t["multiband_op"][0] / B / bound, 1)
            row["paste_op_times_bound"] = round(t["paste_op"][0] / B / plain_bound, 1)
            print(f"{key:24s} multiband (feather {feather}, {levels} levels, {2 * levels + 1} launches) adds {row['added_eager']:.2f} "
                  f"us per frame to the call, {100 * row['added_share_of_predict_u8']:.1f} % of predict_u8; its launches move "
                  f"{need} bytes per frame, byte bound {bound:.2f} us, the operator at {row['multiband_op_times_bound']:.1f} "
                  f"times it (the plain paste at {row['paste_op_times_bound']:.1f} times its own)")
            result["blend_us_per_frame"][key] = row
            del raw, bufs, full
    print(json.dumps(result))


def staged_bytes(n_h, n_w, out_h, out_w, angle=None, clip=None):
    """the LDS bytes a tile of a resize n_h x n_w -> out_h x out_w may stage (csrc/resize.hip: resize_patch_extent; with an
    angle rot_patch_extent on the turned footprint, clipped to the image clip = (h, w)), 0 past 32 KB (taps from global memory)"""
    du, dv = 31 * n_w * out_h, 7 * n_h * out_w
    if angle is None:
        cols, rows = 31 * n_w // out_w + 5, 7 * n_h // out_h + 5
    else:
        c16, s16 = (abs(v) for v in ops.box_rotation(angle))
        den = 65536 * out_w * out_h
        cols, rows = min((c16 * du + s16 * dv) // den + 5, clip[1]), min((s16 * du + c16 * dv) // den + 5, clip[0])
    total = rows * ((cols * 3 + 6) // 4 * 4)
    return total if total <= 32 * 1024 else 0


def rotate_section(args, g):
    """the rotated crop and paste against the boxes forms on the same boxes, per frame; one JSON line"""
    has_rot = hasattr(_lib.lib(), "d3f_crop_resize_cubic_rboxes_u8") and not args.off_only
    result = {"precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds,
              "has_rot": has_rot, "rotate_us_per_frame": {}}
    for side in (448, 256):
        size = (side, side)
        box = ops.center_crop_box(RAW[0], RAW[1], side, side)
        feather = ops.default_feather(box[2], box[3])
        for B in (1, 8):
            raw = torch.randint(0, 256, (B,) + RAW + (3,), generator=g, dtype=torch.uint8).cuda()
            small = ops.crop_resize_cubic_u8(raw, size)
            resized, full = torch.empty_like(small), torch.empty_like(raw)
            many = [box] * B
            forms = {"crop_boxes": lambda: ops.crop_resize_cubic_u8(raw, size, boxes=many, out=resized),
                     "paste_boxes": lambda: ops.paste_resize_cubic_u8(small, raw, boxes=many, feather=feather, out=full)}
            if has_rot:
                for angle in (0.01, 20.0):
                    turn = [angle] * B
                    forms[f"crop_rboxes_{angle}"] = lambda turn=turn: ops.crop_resize_cubic_u8(raw, size, boxes=many, angles=turn,
                                                                                             out=resized)
                    forms[f"paste_rboxes_{angle}"] = lambda turn=turn: ops.paste_resize_cubic_u8(small, raw, boxes=many, angles=turn,
                                                                                               feather=feather, out=full)
            t = compare(forms, args.warmup, args.iters, args.rounds)
            key = f"{RAW[0]}x{RAW[1]}_to_{side}_B{B}"
            row = {}
            for name, (med, lo, hi) in t.items():
                print(f"{key:24s} {name:20s} {med / B:9.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f})")
                row[name] = [round(med / B, 2), round(lo / B, 2), round(hi / B, 2)]
            row["crop_staged_bytes"] = {"boxes": staged_bytes(box[3], box[2], side, side)}
            row["paste_staged_bytes"] = {"boxes": staged_bytes(side, side, box[3], box[2])}
            if has_rot:
                for angle in (0.01, 20.0):
                    row["crop_staged_bytes"][str(angle)] = staged_bytes(box[3], box[2], side, side, angle, RAW)
                    row["paste_staged_bytes"][str(angle)] = staged_bytes(side, side, box[3], box[2], angle, size)
                    for what in ("crop", "paste"):
                        row[f"{what}_ratio_{angle}"] = round(t[f"{what}_rboxes_{angle}"][0] / t[f"{what}_boxes"][0], 3)
                print(f"{key:24s} rotated / boxes: crop {row['crop_ratio_0.01']:.2f} (0.01 deg) {row['crop_ratio_20.0']:.2f} (20 deg), "
                      f"paste {row['paste_ratio_0.01']:.2f} {row['paste_ratio_20.0']:.2f}; staged bytes per tile: crop "
                      f"{row['crop_staged_bytes']}, paste {row['paste_staged_bytes']}")
            result["rotate_us_per_frame"][key] = row
            del raw, full
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--antialias", action="store_true", help="measure the antialiased resize instead (see above)")
    ap.add_argument("--color", action="store_true", help="measure the colour match of the full-frame output instead (see above)")
    ap.add_argument("--temporal", action="store_true", help="measure the temporal filter of the frame entries instead (see above)")
    ap.add_argument("--boxes", action="store_true", help="measure the per-frame-box forms against the single-box ones instead (see above)")
    ap.add_argument("--blend", action="store_true", help="measure the multiband paste of the full-frame output instead (see above)")
    ap.add_argument("--rotate", action="store_true", help="measure the rotated crop and paste against the boxes forms instead (see above)")
    ap.add_argument("--off-only", action="store_true",
                    help="--color / --temporal / --boxes: only the forms without the mode, as on a library without its entries -- the same "
                         "sequence of allocations and captures on both sides of an A/B of the unchanged path")
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}")
    if args.color:
        return color_section(args, torch.Generator().manual_seed(1))
    if args.temporal:
        return temporal_section(args, torch.Generator().manual_seed(1))
    if args.boxes:
        return boxes_section(args, torch.Generator().manual_seed(1))
    if args.blend:
        return blend_section(args, torch.Generator().manual_seed(1))
    if args.rotate:
        return rotate_section(args, torch.Generator().manual_seed(1))
    torch.manual_seed(0)
    net = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    g = torch.Generator().manual_seed(1)
    if args.antialias:
        return antialias_section(net, args, g)
    result = {"raw": list(RAW), "size": list(SIZE), "precision": args.precision, "digest": _lib.built_digest(),
              "iters": args.iters, "rounds": args.rounds, "us_per_call": {}}
    for B in (1, 8):
        raw = torch.randint(0, 256, (B,) + RAW + (3,), generator=g, dtype=torch.uint8).cuda()
        small = ops.crop_resize_cubic_u8(raw, SIZE)
        resized = torch.empty_like(small)
        pair = torch.empty((B, SIZE[0], 2 * SIZE[1], 3), dtype=torch.uint8, device="cuda")
        fake = torch.empty_like(small)
        full, work = torch.empty_like(raw), raw.clone()
        box = ops.center_crop_box(RAW[0], RAW[1], SIZE[1], SIZE[0])
        feather = ops.default_feather(box[2], box[3])
        pair2 = torch.empty_like(pair)
        forms = {
            f"paste_B{B}": lambda: ops.paste_resize_cubic_u8(small, raw, box, feather, out=full),
            f"paste_in_place_B{B}": lambda: ops.paste_resize_cubic_u8(small, work, box, feather, out=work),
            f"full_eager_B{B}": lambda: net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=False, out=full, pair_out=pair2),
            f"resize_B{B}": lambda: ops.crop_resize_cubic_u8(raw, SIZE, out=resized),
            f"frames_eager_B{B}": lambda: net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False, out=pair),
            f"predict_u8_eager_B{B}": lambda: net.predict_u8(small, MEAN, STD, graph=False, out=fake),
        }
        if B == 1:
            forms[f"frames_graph_B{B}"] = lambda: net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=True, out=pair)
            forms[f"predict_u8_graph_B{B}"] = lambda: net.predict_u8(small, MEAN, STD, graph=True, out=fake)
            forms[f"full_graph_B{B}"] = lambda: net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=True, out=full,
                                                                          pair_out=pair2)
        for name, (med, lo, hi) in compare(forms, args.warmup, args.iters, args.rounds).items():
            print(f"{name:24s} {med:9.1f} us per call (min {lo:.1f}, max {hi:.1f})   {med / B:9.1f} us per frame")
            result["us_per_call"][name] = round(med, 1)
    # the kernel's other form: a crop so much larger than the output that a tile's patch exceeds the LDS budget (taps from
    # global memory) -- 2160x3840 -> 64x64, a shrink of 33.75
    big = torch.randint(0, 256, (1, 2160, 3840, 3), generator=g, dtype=torch.uint8).cuda()
    thumb = torch.empty((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
    forms = {"resize_global_taps_2160x3840_to_64x64_B1": lambda: ops.crop_resize_cubic_u8(big, (64, 64), out=thumb)}
    for name, (med, lo, hi) in compare(forms, args.warmup, args.iters, args.rounds).items():
        print(f"{name:24s} {med:9.1f} us per call (min {lo:.1f}, max {hi:.1f})")
        result["us_per_call"][name] = round(med, 1)
    u = result["us_per_call"]
    result["resize_share_of_predict_u8_B1"] = round(u["resize_B1"] / u["predict_u8_eager_B1"], 4)
    result["resize_share_of_predict_u8_B8"] = round(u["resize_B8"] / u["predict_u8_eager_B8"], 4)
    # bytes the resize must move per frame: the crop once, the output once
    need = 1080 * 1080 * 3 + SIZE[0] * SIZE[1] * 3
    result["resize_GBps_B8"] = round(8 * need / (u["resize_B8"] * 1e-6) / 1e9, 1)
    # full-frame output: what the paste adds per frame to predict_frames_u8 of the same run, and the least the paste could
    # take -- the frame read once and written once (12.4 MB; the 0.6 MB patch is not counted) at 6.3 TB/s achievable HBM
    frame_bytes = 2 * RAW[0] * RAW[1] * 3
    result["paste_bytes_per_frame"] = frame_bytes
    result["paste_byte_bound_us_per_frame"] = round(frame_bytes / 6.3e12 * 1e6, 2)
    result["paste_GBps_B8"] = round(8 * frame_bytes / (u["paste_B8"] * 1e-6) / 1e9, 1)
    result["full_added_us_per_frame"] = {
        "eager_B1": round(u["full_eager_B1"] - u["frames_eager_B1"], 1),
        "graph_B1": round(u["full_graph_B1"] - u["frames_graph_B1"], 1),
        "eager_B8": round((u["full_eager_B8"] - u["frames_eager_B8"]) / 8, 1),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
