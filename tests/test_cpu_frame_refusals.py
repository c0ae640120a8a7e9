"""CPU: every refusal of the frame path's crop, paste and multiband operators, as the WHOLE text of d3f_last_error(), against
strings recorded once (tests/golden/frame_refusals.json).  The substring asserts of test_cpu_frame_boxes.py,
test_cpu_frame_rotation.py, test_cpu_paste.py and test_cpu_multiband.py say that a call is refused and roughly why; this
file pins the full message -- the operator's name in it, the numbers, the frame it names -- and, for calls with two faults,
which of the two messages wins.

No device: every pointer is a fake address that is never dereferenced, because every call here is either refused on the host
or has B = 0 (recorded as null: returns 0, launches nothing).  A case that would pass the host checks must not be added."""
import ctypes as C
import json
from pathlib import Path

import pytest

from denoising_diffusion_deep_fake_amd import _lib

GOLDEN = Path(__file__).parent / "golden" / "frame_refusals.json"

# 3 frames of 90 x 160 at D, the output at E, 64 x 64 patches at P, coefficients at COEF, a workspace at WS
D, E, P, COEF, WS = 0x100000, 0x900000, 0x500000, 0x700000, 0xA00000
GOOD = [(35, 0, 90, 90), (0, 0, 160, 90), (70, 10, 33, 47)]
ROT = [(65536, 0), (0, 65536), (46341, 46341)]
BOX_OUT = (71, 0, 90, 90)     # 71 + 90 > 160
BOX_EMPTY = (35, 0, 0, 90)
NO_ROT = (65536, 65536)       # c16^2 + s16^2 = 2^33


def _table(rows):
    if rows is None:
        return None
    return (C.c_int32 * (len(rows[0]) * len(rows)))(*[v for row in rows for v in row])


def _swap(rows, at, row):
    rows = list(rows)
    rows[at] = row
    return rows


def _crop(lib, op, B=3, src_h=90, src_w=160, box=GOOD[0], boxes=GOOD, rot=ROT, H=64, W=64, stride=None, Cpad=4):
    stride = 3 * W if stride is None else stride
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    if op in ("crop", "crop_aa"):
        fn = lib.d3f_crop_resize_cubic_u8 if op == "crop" else lib.d3f_crop_resize_cubic_aa_u8
        return fn(D, B, src_h, src_w, *box, E, H, W, stride, None)
    if op in ("crop_boxes", "crop_aa_boxes"):
        fn = lib.d3f_crop_resize_cubic_boxes_u8 if op == "crop_boxes" else lib.d3f_crop_resize_cubic_aa_boxes_u8
        return fn(D, B, src_h, src_w, _table(boxes), E, H, W, stride, None)
    if op == "crop_rboxes":
        return lib.d3f_crop_resize_cubic_rboxes_u8(D, B, src_h, src_w, _table(boxes), _table(rot), E, H, W, stride, None)
    assert op == "crop_rboxes_nhwc"
    return lib.d3f_crop_resize_cubic_rboxes_u8_nhwc(_lib.F32, D, B, src_h, src_w, _table(boxes), _table(rot), E, H, W, stride,
                                                    WS, Cpad, ms, ms, None)


CROP_ONE, CROP_BOXES, CROP_ROT = ("crop", "crop_aa"), ("crop_boxes", "crop_aa_boxes"), ("crop_rboxes", "crop_rboxes_nhwc")


def _crop_cases():
    cases = {}
    for op in CROP_ONE + CROP_BOXES + CROP_ROT:
        c = {
            "no_frames": dict(B=0),
            "negative_B": dict(B=-1),
            "zero_H": dict(H=0),
            "zero_frame": dict(src_w=0),
            "extent": dict(src_w=20000),
            "extent_out": dict(W=16385),
            "too_many_frames": dict(B=70000),
            "stride": dict(stride=100),
            "extent_and_stride": dict(src_w=20000, stride=100),
            "frames_and_stride": dict(B=70000, stride=100),
        }
        if op in CROP_ONE:
            c.update({
                "box_outside": dict(box=BOX_OUT),
                "box_negative": dict(box=(-1, 0, 90, 90)),
                "box_empty": dict(box=BOX_EMPTY),
                "box_outside_and_stride": dict(box=BOX_OUT, stride=100),
            })
        else:
            c.update({
                "null_boxes": dict(boxes=None),
                "null_boxes_no_frames": dict(boxes=None, B=0) if op in CROP_BOXES else dict(boxes=None, rot=None, B=0),
                "null_boxes_and_stride": dict(boxes=None, stride=100),
                "frame1_empty": dict(boxes=_swap(GOOD, 1, BOX_EMPTY)),
                "frame2_outside": dict(boxes=_swap(GOOD, 2, BOX_OUT)),
                "frame0_negative": dict(boxes=_swap(GOOD, 0, (0, -1, 90, 90))),
                "frame1_outside_frame2_empty": dict(boxes=[GOOD[0], BOX_OUT, BOX_EMPTY]),
                "frame2_outside_and_stride": dict(boxes=_swap(GOOD, 2, BOX_OUT), stride=100),
            })
        if op == "crop_aa":
            c["ratio"] = dict(box=(0, 0, 160, 90), W=4)
            c["ratio_rows"] = dict(box=(0, 0, 160, 90), H=2)
            c["ratio_and_stride"] = dict(box=(0, 0, 160, 90), W=4, stride=3)
        if op == "crop_aa_boxes":
            c["frame2_ratio"] = dict(boxes=[GOOD[0], GOOD[2], (0, 0, 160, 90)], W=4)
            c["frame0_ratio_frame1_outside"] = dict(boxes=[(0, 0, 160, 90), BOX_OUT, GOOD[2]], W=4)
        if op in CROP_ROT:
            c.update({
                "null_rot": dict(rot=None),
                "null_rot_no_frames": dict(rot=None, B=0),
                "null_boxes_null_rot": dict(boxes=None, rot=None),
                "frame1_no_rotation": dict(rot=_swap(ROT, 1, NO_ROT)),
                "frame2_zero_rotation": dict(rot=_swap(ROT, 2, (0, 0))),
                "frame0_huge_rotation": dict(rot=_swap(ROT, 0, (1 << 30, 0))),
                "frame1_outside_frame0_no_rotation": dict(boxes=_swap(GOOD, 1, BOX_OUT), rot=_swap(ROT, 0, NO_ROT)),
                "null_rot_and_frame2_empty": dict(rot=None, boxes=_swap(GOOD, 2, BOX_EMPTY)),
            })
        if op == "crop_rboxes_nhwc":
            c["channels"] = dict(Cpad=2)
            c["channels_and_no_rotation"] = dict(Cpad=2, rot=_swap(ROT, 0, NO_ROT))
            c["channels_and_stride"] = dict(Cpad=2, stride=100)
        for name, kw in c.items():
            cases[f"{op}/{name}"] = (lambda lib, op=op, kw=kw: _crop(lib, op, **kw))
    return cases


PASTE_OPS = ("paste", "paste_color", "paste_boxes", "paste_color_boxes", "paste_rboxes", "paste_color_rboxes")
MB_OPS = ("multiband", "multiband_color", "multiband_boxes", "multiband_color_boxes")


def _paste(lib, op, patch=P, B=3, H=64, W=64, stride=192, frame=D, src_h=90, src_w=160, box=GOOD[0], boxes=GOOD, rot=ROT,
           feather=3, coef=COEF, out=E, levels=2, ws=WS, ws_bytes=1 << 40):
    head = (patch, B, H, W, stride, frame, src_h, src_w)
    if op == "paste":
        return lib.d3f_paste_resize_cubic_u8(*head, *box, feather, out, None)
    if op == "paste_color":
        return lib.d3f_paste_resize_cubic_color_u8(*head, *box, feather, coef, out, None)
    if op == "paste_boxes":
        return lib.d3f_paste_resize_cubic_boxes_u8(*head, _table(boxes), feather, out, None)
    if op == "paste_color_boxes":
        return lib.d3f_paste_resize_cubic_color_boxes_u8(*head, _table(boxes), feather, coef, out, None)
    if op == "paste_rboxes":
        return lib.d3f_paste_resize_cubic_rboxes_u8(*head, _table(boxes), _table(rot), feather, out, None)
    if op == "paste_color_rboxes":
        return lib.d3f_paste_resize_cubic_color_rboxes_u8(*head, _table(boxes), _table(rot), feather, coef, out, None)
    if op == "multiband":
        return lib.d3f_paste_multiband_u8(*head, *box, feather, levels, ws, ws_bytes, out, None)
    if op == "multiband_color":
        return lib.d3f_paste_multiband_color_u8(*head, *box, feather, levels, coef, ws, ws_bytes, out, None)
    if op == "multiband_boxes":
        return lib.d3f_paste_multiband_boxes_u8(*head, _table(boxes), feather, levels, ws, ws_bytes, out, None)
    assert op == "multiband_color_boxes"
    return lib.d3f_paste_multiband_color_boxes_u8(*head, _table(boxes), feather, levels, coef, ws, ws_bytes, out, None)


def _paste_cases():
    cases = {}
    for op in PASTE_OPS + MB_OPS:
        one, rotated, color, mb = "boxes" not in op, "rboxes" in op, "color" in op, op in MB_OPS
        c = {
            "no_frames": dict(B=0),
            "negative_B": dict(B=-1),
            "too_many_frames": dict(B=70000),
            "zero_H": dict(H=0),
            "zero_frame": dict(src_h=0),
            "extent": dict(src_w=20000),
            "extent_patch": dict(H=16385),
            "feather_negative": dict(feather=-1),
            "feather_large": dict(feather=20000),
            "stride": dict(stride=100),
            "overlap_in_part": dict(out=D + 3),
            "patch_overlaps_out": dict(patch=E + 1000),
            "extent_and_stride": dict(src_w=20000, stride=100),
            "feather_and_overlap": dict(feather=-1, out=D + 3),
            "feather_and_patch_overlap": dict(feather=20000, patch=E),
            "stride_and_overlap": dict(stride=100, out=D + 3),
        }
        if one:
            c.update({
                "box_outside": dict(box=BOX_OUT),
                "box_empty": dict(box=BOX_EMPTY),
                "box_outside_and_feather": dict(box=BOX_OUT, feather=-1),
            })
        else:
            c.update({
                "null_boxes": dict(boxes=None),
                "null_boxes_no_frames": dict(boxes=None, B=0) if not rotated else dict(boxes=None, rot=None, B=0),
                "null_boxes_and_feather": dict(boxes=None, feather=-1),
                "frame1_empty": dict(boxes=_swap(GOOD, 1, BOX_EMPTY)),
                "frame2_outside": dict(boxes=_swap(GOOD, 2, BOX_OUT)),
                "frame1_outside_frame2_empty": dict(boxes=[GOOD[0], BOX_OUT, BOX_EMPTY]),
                "frame2_outside_and_overlap": dict(boxes=_swap(GOOD, 2, BOX_OUT), out=D + 3),
            })
        if color:
            c.update({
                "null_coef": dict(coef=None),
                "coef_overlaps_out": dict(coef=E + 8),
                "null_coef_and_bad_box": dict(coef=None, box=BOX_OUT, boxes=_swap(GOOD, 0, BOX_OUT)),
                "coef_overlap_and_bad_box": dict(coef=E + 8, box=BOX_OUT, boxes=_swap(GOOD, 0, BOX_OUT)),
                "coef_overlap_and_patch_overlap": dict(coef=E + 8, patch=E),
            })
        if rotated:
            c.update({
                "null_rot": dict(rot=None),
                "null_rot_no_frames": dict(rot=None, B=0),
                "frame1_no_rotation": dict(rot=_swap(ROT, 1, NO_ROT)),
                "frame1_outside_frame0_no_rotation": dict(boxes=_swap(GOOD, 1, BOX_OUT), rot=_swap(ROT, 0, NO_ROT)),
                "no_rotation_and_feather": dict(rot=_swap(ROT, 0, NO_ROT), feather=-1),
            })
            if color:
                c["coef_overlap_and_no_rotation"] = dict(coef=E + 8, rot=_swap(ROT, 0, NO_ROT))
        if mb:
            c.update({
                "levels_zero": dict(levels=0),
                "levels_seven": dict(levels=7),
                "levels_and_feather": dict(levels=0, feather=-1),
                "box_below_levels": dict(box=(35, 0, 90, 3), boxes=_swap(GOOD, 1, (35, 0, 3, 90))),
                "box_below_levels_no_frames": dict(box=(35, 0, 90, 3), boxes=_swap(GOOD, 1, (35, 0, 3, 90)), B=0),
                "box_below_levels_and_null_workspace": dict(box=(35, 0, 90, 3), boxes=_swap(GOOD, 1, (35, 0, 3, 90)), ws=None),
                "null_workspace": dict(ws=None),
                "workspace_alignment": dict(ws=WS + 8),
                "workspace_small": dict(ws_bytes=16),
                "workspace_overlaps_out": dict(ws=E),
                "workspace_overlaps_frame": dict(ws=D + 16),
                "workspace_overlaps_patch": dict(ws=P),
                "null_workspace_and_feather": dict(ws=None, feather=-1),
                "alignment_and_small": dict(ws=WS + 8, ws_bytes=16),
                "small_and_overlap": dict(ws=E, ws_bytes=16),
            })
            if color:
                c["workspace_overlaps_coef"] = dict(ws=COEF)
        for name, kw in c.items():
            cases[f"{op}/{name}"] = (lambda lib, op=op, kw=kw: _paste(lib, op, **kw))
    return cases


# ---- the six engine entries, as far as they answer without a device ----

ENGINE_OPS = ("frames", "frames_full", "frames_boxes", "frames_full_boxes", "frames_rboxes", "frames_full_rboxes")


def _engine(lib, h, op, raw=D, src_h=90, src_w=160, box=GOOD[0], boxes=GOOD, rot=ROT, feather=3, full_out=0x1100000, graph=0):
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    pair, ws = E, D
    if op == "frames":
        return lib.d3f_unet_predict_frames_u8(h, D, D, raw, src_h, src_w, *box, pair, ms, ms, ws, graph, None)
    if op == "frames_full":
        return lib.d3f_unet_predict_frames_full_u8(h, D, D, raw, src_h, src_w, *box, feather, pair, full_out, ms, ms, ws, graph,
                                                   None)
    if op == "frames_boxes":
        return lib.d3f_unet_predict_frames_boxes_u8(h, D, D, raw, src_h, src_w, _table(boxes), pair, ms, ms, ws, graph, None)
    if op == "frames_full_boxes":
        return lib.d3f_unet_predict_frames_full_boxes_u8(h, D, D, raw, src_h, src_w, _table(boxes), feather, pair, full_out, ms,
                                                         ms, ws, graph, None)
    if op == "frames_rboxes":
        return lib.d3f_unet_predict_frames_rboxes_u8(h, D, D, raw, src_h, src_w, _table(boxes), _table(rot), pair, ms, ms, ws,
                                                     graph, None)
    assert op == "frames_full_rboxes"
    return lib.d3f_unet_predict_frames_full_rboxes_u8(h, D, D, raw, src_h, src_w, _table(boxes), _table(rot), feather, pair,
                                                      full_out, ms, ms, ws, graph, None)


def _engine_cases():
    """name -> (settings, call): settings are applied to a fresh 3 x 64 x 64 resnet18 engine of 3 frames"""
    cases = {}
    for op in ENGINE_OPS:
        one, rotated, full = "boxes" not in op, "rboxes" in op, "full" in op
        c = {
            "null_argument": ({}, dict(raw=None)),
            "extent": ({}, dict(src_w=20000)),
            "zero_frame": ({}, dict(src_h=0)),
            "aa/extent": (dict(aa=True), dict(src_w=20000)) if not rotated else None,
        }
        if one:
            c.update({
                "box_outside": ({}, dict(box=BOX_OUT)),
                "box_empty": ({}, dict(box=BOX_EMPTY)),
                "aa/box_outside": (dict(aa=True), dict(box=BOX_OUT)),
                "aa/ratio": (dict(aa=True), dict(src_h=3000, src_w=3000, box=(0, 0, 2049, 2049))),
            })
        else:
            c.update({
                "null_boxes": ({}, dict(boxes=None)),
                "graph": ({}, dict(graph=1)),
                "graph_and_bad_box": ({}, dict(graph=1, boxes=_swap(GOOD, 2, BOX_OUT))),
                "frame2_outside": ({}, dict(boxes=_swap(GOOD, 2, BOX_OUT))),
                "frame2_empty": ({}, dict(boxes=_swap(GOOD, 2, BOX_EMPTY))),
                "aa/frame2_outside": (dict(aa=True), dict(boxes=_swap(GOOD, 2, BOX_OUT))),
            })
            if not rotated:
                c["aa/frame1_ratio"] = (dict(aa=True), dict(src_h=3000, src_w=3000, boxes=_swap(GOOD, 1, (0, 0, 2049, 2049))))
        if rotated:
            c.update({
                "null_rot": ({}, dict(rot=None)),
                "frame1_no_rotation": ({}, dict(rot=_swap(ROT, 1, NO_ROT))),
                "frame1_outside_frame0_no_rotation": ({}, dict(boxes=_swap(GOOD, 1, BOX_OUT), rot=_swap(ROT, 0, NO_ROT))),
                "aa/any": (dict(aa=True), {}),
                "aa/bad_box": (dict(aa=True), dict(boxes=_swap(GOOD, 0, BOX_OUT))),
            })
            if full:
                c["multiband/any"] = (dict(multiband=2), {})
                c["aa_multiband/any"] = (dict(aa=True, multiband=2), {})
        if full:
            c.update({
                "feather": ({}, dict(feather=-1)),
                "overlap_in_part": ({}, dict(full_out=D + 3)),
                "feather_and_overlap": ({}, dict(feather=-1, full_out=D + 3)),
                "patch_overlaps_out": ({}, dict(full_out=E)),
            })
            if one:
                c["graph_in_place"] = ({}, dict(graph=1, full_out=D))
                c["graph_in_place_and_feather"] = ({}, dict(graph=1, full_out=D, feather=-1))
        for name, sc in c.items():
            if sc is not None:
                cases[f"{op}/{name}"] = sc + (op,)
    return cases


def _run_engine(lib, settings, kw, op):
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 3, 64, 64, _lib.F32, C.byref(h)))
    try:
        if settings.get("aa"):
            _lib.check(lib.d3f_unet_set_frame_resample(h, _lib.RESAMPLE_CUBIC_AA))
        if settings.get("multiband"):
            _lib.check(lib.d3f_unet_set_frame_blend(h, _lib.BLEND_MULTIBAND, settings["multiband"]))
        return _engine(lib, h, op, **kw)
    finally:
        lib.d3f_unet_destroy(h)


def all_cases():
    cases = {}
    cases.update(_crop_cases())
    cases.update(_paste_cases())
    for name, (settings, kw, op) in _engine_cases().items():
        cases[f"engine/{name}"] = (lambda lib, s=settings, kw=kw, op=op: _run_engine(lib, s, kw, op))
    return cases


def answer(lib, call):
    """the whole message of a refused call; None for a call that returns 0"""
    return None if call(lib) == 0 else lib.d3f_last_error().decode()


CASES = all_cases()
RECORDED = json.loads(GOLDEN.read_text())


def test_every_case_is_recorded_and_every_record_has_its_case():
    assert sorted(CASES) == sorted(RECORDED)
    # nothing here may reach a launch: a call that is not refused has no frames
    assert all(name.endswith("no_frames") for name, text in RECORDED.items() if text is None)


@pytest.mark.parametrize("group", sorted({name.split("/")[0] + ("/" + name.split("/")[1] if name.startswith("engine/") else "")
                                          for name in CASES}))
def test_refusals_are_the_recorded_text(group):
    lib = _lib.lib()
    for name in sorted(n for n in CASES if n.startswith(group + "/")):
        assert answer(lib, CASES[name]) == RECORDED[name], name
