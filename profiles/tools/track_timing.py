"""The template tracker at the authors' size, 1080x1920 BGR frames (HIP events, device resident).

  decimate : d3f_gray_decimate_u8 alone, stride 4 and 8, B = 1 and B = 8, next to its byte bound: every frame byte read
             once and the reduced image written once, 3 h w + gh gw bytes per frame at 6.3 TB/s achievable HBM
  search   : d3f_track_search_u8 alone on a reduced image of 270 x 480, a 48 x 48 template, search 16 (1089 candidates a
             frame), B = 1 and B = 8: one workgroup, the frames in order inside the kernel; beside it, in the same rounds,
             d3f_track_search_scale_u8 at the same shape with levels = 1 (three levels a frame) and levels = 0, and
             d3f_track_search_rot_u8 with steps = 1 (three angles a frame, on the disc) and steps = 0; and the
             re-acquisition's two parts, d3f_track_global_u8 alone (the key template at all 433 x 223 = 96 559 positions of
             every frame, two launches; next to its operation bound) and d3f_track_search_reacq_u8 alone (the serial kernel
             in its re-acquiring form, on the keys of that search)
  tool     : ops.track_template_u8 (decimate + search, what track_face_box runs per batch once the frames are on the
             device) and ops.track_template_reacq_u8 (decimate + whole-frame search + serial search, what it runs with
             --reacquire) for a 190 x 190 face (stride 4, a 47 x 47 template), B = 1 and B = 8, next to
             Unet.predict_frames_full_u8 on the same frames (448 x 448, eager): the share the tracking pass is of the render

Back-to-back enqueues on one stream, ITERS iterations after WARMUP, the forms alternating in ROUNDS rounds; the figure is
the median round's time per call, given per frame.  Random frames, the same every call: the template finds itself in its
key frame and nothing in the others, and neither kernel's work depends on the data.  One JSON line at the end.
    python profiles/tools/track_timing.py [--precision f32|bf16] [--iters N]
"""
import argparse
import ctypes
import json
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from denoising_diffusion_deep_fake_amd import Unet, _lib, ops
from video_frame_path import MEAN, RAW, STD, compare

HBM = 6.3e12  # bytes per second, the achievable rate profiles/README.md uses for every byte bound
# the whole-frame search's operation bound: one v_qsad_pk_u16_u8 is 16 absolute differences (four candidates x four bytes) of a
# lane, 1024 of a wave; a wave's vector instruction issues in 4 cycles on one of a CU's four SIMDs, 256 CUs at 2.4 GHz
QSAD_ABSDIFF_PER_S = 1024 / 4 * 4 * 256 * 2.4e9
FACE = (860, 440, 190, 190)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}")
    g = torch.Generator().manual_seed(1)
    h, w = RAW
    result = {"raw": list(RAW), "precision": args.precision, "digest": _lib.built_digest(), "iters": args.iters,
              "rounds": args.rounds, "decimate_us_per_frame": {}, "search_us_per_frame": {}, "search_scale_us_per_frame": {},
              "search_scale_levels0_us_per_frame": {}, "search_rot_us_per_frame": {}, "search_rot_steps0_us_per_frame": {},
              "global_us_per_frame": {}, "search_reacq_us_per_frame": {}, "tool_us_per_frame": {}}
    torch.manual_seed(0)
    net = Unet("resnet34", None, 3, 3, None, compute_dtype=args.precision).cuda().eval()
    lib = _lib.lib()
    for B in (1, 8):
        raw = torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8).cuda()
        # the reduced image alone
        grey = {s: torch.empty((B, h // s, w // s), dtype=torch.uint8, device="cuda") for s in (4, 8)}
        forms = {f"s{s}": (lambda s=s: ops.gray_decimate_u8(raw, s, out=grey[s])) for s in (4, 8)}
        for name, (med, lo, hi) in compare(forms, args.warmup, args.iters, args.rounds).items():
            s = int(name[1:])
            need = 3 * h * w + (h // s) * (w // s)
            bound = need / HBM * 1e6
            print(f"decimate {name} B{B}: {med / B:8.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f}); {need} bytes per "
                  f"frame, byte bound {bound:.2f} us, at {med / B / bound:.1f} times it, {need * B / (med * 1e-6) / 1e9:.0f} GB/s")
            result["decimate_us_per_frame"][f"{name}_B{B}"] = {"us": round(med / B, 2), "min": round(lo / B, 2),
                                                              "max": round(hi / B, 2), "bytes": need,
                                                              "byte_bound_us": round(bound, 2)}
        # the search alone: a 48 x 48 template cut from frame 0's reduced image, search 16
        ops.gray_decimate_u8(raw, 4, out=grey[4])
        gh, gw = h // 4, w // 4
        templ = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
        templ[:48 * 48] = grey[4][0, 100:148, 200:248].reshape(-1)
        pos = torch.tensor([200, 100], dtype=torch.int32, device="cuda")
        rows = torch.empty((B, 4), dtype=torch.int32, device="cuda")

        def search():
            _lib.check(lib.d3f_track_search_u8(_lib.ptr(grey[4]), B, gh, gw, 48, 48, ops.TRACK_SEARCH, ops.TRACK_ADAPT,
                                               ops.TRACK_LOST, _lib.ptr(templ), _lib.ptr(pos), _lib.ptr(rows),
                                               _lib.stream_ptr()))
        # the scale search on the same image and template, next to it in the same rounds: levels = 1 (three levels: 3267
        # candidates and four resamples a frame) and levels = 0 (the plain search's candidates through the new kernel)
        # (a state each: the level that levels = 1 ends at must not become the size that levels = 0 is timed at)
        state_scale = {levels: (templ.clone(), torch.tensor([200, 100, 48], dtype=torch.int32, device="cuda"))
                       for levels in (0, 1)}
        rows_scale = {levels: torch.empty((B, 8), dtype=torch.int32, device="cuda") for levels in (0, 1)}

        def search_scale(levels):
            _lib.check(lib.d3f_track_search_scale_u8(_lib.ptr(grey[4]), B, gh, gw, 48, 48, ops.TRACK_SEARCH, ops.TRACK_ADAPT,
                                                     ops.TRACK_LOST, levels, ops.TRACK_SCALE_PENALTY,
                                                     _lib.ptr(state_scale[levels][0]), _lib.ptr(state_scale[levels][1]),
                                                     _lib.ptr(rows_scale[levels]), _lib.stream_ptr()))
        # the rotation search likewise: steps = 1 (three angles: 3267 candidates on the disc and four turns of the template a
        # frame) and steps = 0, a state each
        table = [v for pair in ops.track_rot_table() for v in pair]
        amax, table = len(table) // 4, (ctypes.c_int32 * len(table))(*table)
        state_rot = {steps: (templ.clone(), torch.tensor([200, 100, 0], dtype=torch.int32, device="cuda")) for steps in (0, 1)}
        rows_rot = {steps: torch.empty((B, 8), dtype=torch.int32, device="cuda") for steps in (0, 1)}

        def search_rot(steps):
            _lib.check(lib.d3f_track_search_rot_u8(_lib.ptr(grey[4]), B, gh, gw, 48, 48, ops.TRACK_SEARCH, ops.TRACK_ADAPT,
                                                   ops.TRACK_LOST, steps, ops.TRACK_ROT_PENALTY, amax, table,
                                                   _lib.ptr(state_rot[steps][0]), _lib.ptr(state_rot[steps][1]),
                                                   _lib.ptr(rows_rot[steps]), _lib.stream_ptr()))
        # the re-acquisition's parts on the same image: the key template (the same bytes) at every position of every frame,
        # and the serial search that reads its keys (random frames: frame 0 is found by the window, the others are lost by
        # both searches, so the template is never replaced -- 2304 bytes once a re-acquired frame, against the search itself)
        key_templ, keys = templ.clone(), torch.empty((B,), dtype=torch.int64, device="cuda")
        state_reacq = (templ.clone(), pos.clone())
        rows_reacq = torch.empty((B, 4), dtype=torch.int32, device="cuda")

        def global_search():
            _lib.check(lib.d3f_track_global_u8(_lib.ptr(grey[4]), B, gh, gw, 48, 48, _lib.ptr(key_templ), _lib.ptr(keys),
                                               _lib.stream_ptr()))

        def search_reacq():
            _lib.check(lib.d3f_track_search_reacq_u8(_lib.ptr(grey[4]), B, gh, gw, 48, 48, ops.TRACK_SEARCH, ops.TRACK_ADAPT,
                                                     ops.TRACK_LOST, ops.TRACK_RELOST, _lib.ptr(state_reacq[0]),
                                                     _lib.ptr(key_templ), _lib.ptr(state_reacq[1]), _lib.ptr(keys),
                                                     _lib.ptr(rows_reacq), _lib.stream_ptr()))
        global_search()
        forms = {"search": search, "search_scale": lambda: search_scale(1), "search_scale_levels0": lambda: search_scale(0),
                 "search_rot": lambda: search_rot(1), "search_rot_steps0": lambda: search_rot(0), "global": global_search,
                 "search_reacq": search_reacq}
        t = compare(forms, args.warmup, args.iters, args.rounds)
        med, lo, hi = t["search"]
        print(f"search 48x48 R16 B{B}: {med / B:8.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f}); rows {rows[0].tolist()}")
        result["search_us_per_frame"][f"B{B}"] = {"us": round(med / B, 2), "min": round(lo / B, 2), "max": round(hi / B, 2)}
        for name, levels in (("search_scale", 1), ("search_scale_levels0", 0)):
            m, lo, hi = t[name]
            print(f"{name} 48x48 R16 B{B}: {m / B:8.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f}), {m / med:.2f} times "
                  f"the plain search; rows {rows_scale[levels][0].tolist()}")
            result[f"{name}_us_per_frame"][f"B{B}"] = {"us": round(m / B, 2), "min": round(lo / B, 2), "max": round(hi / B, 2),
                                                       "times_plain": round(m / med, 3)}
        for name, steps in (("search_rot", 1), ("search_rot_steps0", 0)):
            m, lo, hi = t[name]
            print(f"{name} 48x48 R16 B{B}: {m / B:8.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f}), {m / med:.2f} times "
                  f"the plain search; rows {rows_rot[steps][0].tolist()}")
            result[f"{name}_us_per_frame"][f"B{B}"] = {"us": round(m / B, 2), "min": round(lo / B, 2), "max": round(hi / B, 2),
                                                       "times_plain": round(m / med, 3)}
        m, lo, hi = t["global"]
        candidates = (gw - 48 + 1) * (gh - 48 + 1)
        bound = candidates * 48 * 48 / QSAD_ABSDIFF_PER_S * 1e6
        print(f"global 48x48 B{B}: {m / B:8.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f}), two launches; {candidates} "
              f"candidates of 2304 samples, operation bound {bound:.2f} us, at {m / B / bound:.1f} times it, {m / med:.2f} times "
              f"the plain search; keys {[(k >> 32, k & 0xffff, (k >> 16) & 0xffff) for k in keys.tolist()][:2]}")
        result["global_us_per_frame"][f"B{B}"] = {"us": round(m / B, 2), "min": round(lo / B, 2), "max": round(hi / B, 2),
                                                   "candidates": candidates, "operation_bound_us": round(bound, 3),
                                                   "times_plain": round(m / med, 3)}
        m, lo, hi = t["search_reacq"]
        print(f"search_reacq 48x48 R16 B{B}: {m / B:8.2f} us per frame (min {lo / B:.2f}, max {hi / B:.2f}), {m / med:.2f} times "
              f"the plain search; rows {rows_reacq[0].tolist()}")
        result["search_reacq_us_per_frame"][f"B{B}"] = {"us": round(m / B, 2), "min": round(lo / B, 2), "max": round(hi / B, 2),
                                                         "times_plain": round(m / med, 3)}
        # the tool's device call against the render of the same frames
        state = ops.TrackState()
        geometry = ops.track_seed(state, raw[0], FACE)
        state_reacq = ops.TrackState()
        ops.track_seed(state_reacq, raw[0], FACE, reacquire=True)
        full, pair = torch.empty_like(raw), torch.empty((B, 448, 896, 3), dtype=torch.uint8, device="cuda")
        forms = {
            "track_template_u8": lambda: ops.track_template_u8(raw, state),
            "track_template_reacq_u8": lambda: ops.track_template_reacq_u8(raw, state_reacq),
            "predict_frames_full_u8": lambda: net.predict_frames_full_u8(raw, (448, 448), MEAN, STD, graph=False, out=full,
                                                                         pair_out=pair),
        }
        t = {name: v[0] / B for name, v in compare(forms, args.warmup, args.iters, args.rounds).items()}
        share = t["track_template_u8"] / t["predict_frames_full_u8"]
        print(f"tool B{B}: track_template_u8 {t['track_template_u8']:8.2f}, predict_frames_full_u8 "
              f"{t['predict_frames_full_u8']:9.1f} us per frame: the tracking pass is {100 * share:.1f} % of the render "
              f"(geometry {geometry}, last row {ops.track_template_u8(raw, state)[-1].tolist()})")
        print(f"tool B{B}: track_template_reacq_u8 {t['track_template_reacq_u8']:8.2f} us per frame, "
              f"{t['track_template_reacq_u8'] / t['track_template_u8']:.2f} times track_template_u8 (last row "
              f"{ops.track_template_reacq_u8(raw, state_reacq)[-1].tolist()})")
        result["tool_us_per_frame"][f"B{B}"] = {"track_template_u8": round(t["track_template_u8"], 2),
                                               "track_template_reacq_u8": round(t["track_template_reacq_u8"], 2),
                                               "predict_frames_full_u8": round(t["predict_frames_full_u8"], 1),
                                               "share": round(share, 4), "stride": geometry[0]}
        del raw, full, pair
    print(json.dumps(result))


if __name__ == "__main__":
    main()
