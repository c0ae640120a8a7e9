"""CPU: rotated crop boxes without a device -- ops.box_rotation, ops.read_rbox_track, ops.smooth_rbox_track and the tracker
tool's key-angle interpolation pinned by hand; the host-side guards of the _rboxes_ operators and the two rboxes entries of
the engine (everything is refused before a device call: the dummy pointers are never dereferenced); the argument handling of
the Python entries and the tools; and tests/rotation_restatement.py against an independent float64 oracle, torch's
grid_sample on the real cos / sin, within the bound DESIGN.md section 4 "Rotated crop" derives from the two quantisations."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rotation_restatement as R
from denoising_diffusion_deep_fake_amd import _lib, ops


def _table(rows):
    return (C.c_int32 * (len(rows) * len(rows[0])))(*[v for row in rows for v in row])


# ---- box_rotation, the track readers, the key angles ----

def test_box_rotation_by_hand():
    assert ops.box_rotation(0) == (65536, 0)
    assert ops.box_rotation(90) == (0, 65536)
    assert ops.box_rotation(180) == (-65536, 0)
    assert ops.box_rotation(-90) == (0, -65536)
    assert ops.box_rotation(30) == (56756, 32768)   # cos 30 * 65536 = 56755.84, sin 30 = 0.5
    assert ops.box_rotation(45) == (46341, 46341)   # 65536 / sqrt 2 = 46340.95
    assert ops.box_rotation(-30) == (56756, -32768) and ops.box_rotation(150) == (-56756, 32768)
    # rounded to hundredths first, wrapped to (-180, 180]
    assert ops.box_rotation(30.004) == ops.box_rotation(30) and ops.box_rotation(29.996) == ops.box_rotation(30)
    assert ops.box_rotation(30.006) == ops.box_rotation(30.01) != ops.box_rotation(30)
    assert ops.box_rotation(270) == ops.box_rotation(-90) and ops.box_rotation(-180) == (-65536, 0)
    assert ops.box_rotation(360 + 45) == (46341, 46341) and ops.box_rotation(-315) == (46341, 46341)
    assert ops.angle_hundredths(180) == 18000 and ops.angle_hundredths(-180) == 18000 and ops.angle_hundredths(180.01) == -17999
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.box_rotation(bad)
    # every hundredth gives a table the library takes as a rotation: |c16^2 + s16^2 - 2^32| <= 2^17
    for h in range(-17999, 18001, 7):
        c16, s16 = ops.box_rotation(h / 100.0)
        assert abs(c16 * c16 + s16 * s16 - (1 << 32)) <= 1 << 17, h
        assert (c16, s16) == R.box_rotation(h / 100.0), h


def test_read_rbox_track(tmp_path):
    path = tmp_path / "track.txt"
    path.write_text("# x y w h a\n"
                    "-\n"
                    "10 20 30 40 12.5\n"
                    "11,21,31,41   # four fields among five: angle 0\n"
                    "-\n"
                    "  12, 22 ,32  42, -7.256  # rounded to hundredths\n"
                    "13 23 33 43 270\n"
                    "-\n")
    faces = ops.read_rbox_track(path)
    assert faces == [(10, 20, 30, 40, 12.5)] * 2 + [(11, 21, 31, 41, 0.0)] * 2 + [(12, 22, 32, 42, -7.26)] + \
        [(13, 23, 33, 43, -90.0)] * 2  # 270 wraps to -90
    assert ops.read_rbox_track(str(path)) == faces
    assert ops.box_of_frame(faces, 100) == (13, 23, 33, 43, -90.0)
    path.write_text("# only gaps\n-\n")
    with pytest.raises(ValueError, match="no detection"):
        ops.read_rbox_track(path)
    for bad in ("1 2 3\n", "1 2 3 4 5 6\n", "1 2 3 x 5\n", "1.5 2 3 4 5\n", "1 2 3 4 five\n", "1 2 3 4 nan\n", "- -\n"):
        path.write_text("1 2 3 4 5\n" + bad)
        with pytest.raises(ValueError, match="line 2"):
            ops.read_rbox_track(path)
    # read_box_track itself keeps refusing a fifth field
    path.write_text("1 2 3 4\n1 2 3 4 5\n")
    with pytest.raises(ValueError, match="line 2"):
        ops.read_box_track(path)
    assert ops.read_rbox_track(path) == [(1, 2, 3, 4, 0.0), (1, 2, 3, 4, 5.0)]


def test_smooth_rbox_track_by_hand():
    boxes = [(0, 0, 10, 10), (10, 2, 10, 10), (20, 0, 12, 10), (30, 5, 10, 11), (40, 0, 10, 10)]
    angles = [0.0, 10.0, 10.01, -5.0, -5.02]
    faces = [b + (a,) for b, a in zip(boxes, angles)]
    assert ops.smooth_rbox_track(faces, 0) == faces
    got = ops.smooth_rbox_track(faces, 1)
    assert [f[:4] for f in got] == ops.smooth_box_track(boxes, 1)
    # hundredths 0, 1000, 1001, -500, -502 over the truncated window, floor division:
    #   1000 // 2 = 500, 2001 // 3 = 667, 1501 // 3 = 500, -1 // 3 = -1, -1002 // 2 = -501
    assert [f[4] for f in got] == [5.0, 6.67, 5.0, -0.01, -5.01]
    assert [f[4] for f in ops.smooth_rbox_track(faces, 100)] == [999 // 5 / 100.0] * 5
    with pytest.raises(ValueError):
        ops.smooth_rbox_track(faces, -1)


def test_track_crop_rboxes_takes_the_box_of_the_entry_and_its_angle():
    track = [(40, 30, 20, 30, 12.5), (100, 60, 40, 40, -3.0)]
    boxes, angles = ops.track_crop_rboxes(track, 0, 4, 150, 200, 64, 64)
    assert boxes == [ops.track_crop_box(150, 200, 64, 64, track[k][:4]) for k in (0, 1, 1, 1)]
    assert angles == [12.5, -3.0, -3.0, -3.0]


def test_key_angle_interpolation_by_hand(tmp_path):
    import denoising_diffusion_deep_fake_amd.script_tools.track_face_box as tool
    keys = tool.sorted_key_angles([("6", "-5"), (2, 10.0), ("10", "-5.5")])
    assert keys == {2: 1000, 6: -500, 10: -550} and list(keys) == [2, 6, 10]
    # constant before the first key and after the last; between: a0 + (a1 - a0) * (k - k0) // (k1 - k0), floor division
    #   k = 3: 1000 + (-1500 * 1) // 4 = 625; 4: 250; 5: 1000 + (-4500 // 4) = -125; 7: -500 + (-50 // 4) = -513; 9: -538
    assert tool.interpolate_key_angles(keys, 13) == [1000, 1000, 1000, 625, 250, -125, -500, -513, -525, -538, -550, -550, -550]
    assert tool.interpolate_key_angles({4: 123}, 3) == [123, 123, 123]
    assert tool.sorted_key_angles(None) is None and tool.sorted_key_angles([]) is None
    for bad in ([(-1, 3)], [(2, 3), (2, 4)], [(2, "x")], [(2, float("nan"))], [("k", 1)]):
        with pytest.raises(ValueError, match="key-angle"):
            tool.sorted_key_angles(bad)
    # the file: a fifth column in decimal degrees, `-` stays `-`; without angles it is byte for byte the four-column file
    track = [None, (1, 2, 3, 4), (5, 6, 7, 8), None, (9, 10, 11, 12)]
    path = tmp_path / "t.txt"
    tool.write_track(path, track, ("head",))
    assert path.read_text() == "# head\n-\n1 2 3 4\n5 6 7 8\n-\n9 10 11 12\n"
    tool.write_track(path, track, ("head",), [1000, 625, -125, 0, -5])
    assert path.read_text() == "# head\n-\n1 2 3 4 6.25\n5 6 7 8 -1.25\n-\n9 10 11 12 -0.05\n"
    assert ops.read_rbox_track(path) == [(1, 2, 3, 4, 6.25)] * 2 + [(5, 6, 7, 8, -1.25)] * 2 + [(9, 10, 11, 12, -0.05)]
    argv = ["clip.mp4", "--key", "0", "1", "2", "3", "4"]
    assert tool.parse_command_line_arguments(argv).key_angle is None
    a = tool.parse_command_line_arguments(argv + ["--key-angle", "0", "10", "--key-angle", "8", "-2.5"])
    assert tool.sorted_key_angles(a.key_angle) == {0: 1000, 8: -250}
    for bad in (["--key-angle", "0"], ["--key-angle", "0", "x"], ["--key-angle", "1", "2", "--key-angle", "1", "3"]):
        with pytest.raises(SystemExit):
            tool.parse_command_line_arguments(argv + bad)


# ---- refusals of the C operators: no device ----

GOOD = [(35, 0, 90, 90), (0, 0, 160, 90), (70, 10, 33, 47)]
ROT = [ops.box_rotation(a) for a in (12.5, -30.0, 0.0)]


def _operators(lib):
    """the four _rboxes_ operators as call(B, boxes, rot) on 3 frames of 90 x 160 and 64 x 64 patches"""
    d, e, p, coef, act = 0x100000, 0x900000, 0x500000, 0x700000, 0xb00000
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    return {
        "crop": lambda B, boxes, rot: lib.d3f_crop_resize_cubic_rboxes_u8(d, B, 90, 160, boxes, rot, e, 64, 64, 192, None),
        "crop_nhwc": lambda B, boxes, rot: lib.d3f_crop_resize_cubic_rboxes_u8_nhwc(_lib.F32, d, B, 90, 160, boxes, rot, e, 64,
                                                                                   64, 192, act, 8, ms, ms, None),
        "paste": lambda B, boxes, rot: lib.d3f_paste_resize_cubic_rboxes_u8(p, B, 64, 64, 192, d, 90, 160, boxes, rot, 3, e,
                                                                            None),
        "paste_color": lambda B, boxes, rot: lib.d3f_paste_resize_cubic_color_rboxes_u8(p, B, 64, 64, 192, d, 90, 160, boxes,
                                                                                        rot, 3, coef, e, None),
    }


@pytest.mark.parametrize("name", ["crop", "crop_nhwc", "paste", "paste_color"])
def test_rboxes_operators_refuse_before_any_device_call(name):
    lib = _lib.lib()
    call = _operators(lib)[name]
    assert call(3, None, _table(ROT)) != 0 and b"null boxes" in lib.d3f_last_error(), lib.d3f_last_error()
    assert call(3, _table(GOOD), None) != 0 and b"null rot" in lib.d3f_last_error(), lib.d3f_last_error()
    # whatever the _boxes_ forms refuse, the frame named
    for bad, word in (((71, 0, 90, 90), b"outside"), ((35, 1, 90, 90), b"outside"), ((-1, 0, 90, 90), b"outside"),
                      ((35, 0, 0, 90), b"non-positive"), ((35, 0, 90, -3), b"non-positive")):
        for at in (0, 1, 2):
            rows = list(GOOD)
            rows[at] = bad
            assert call(3, _table(rows), _table(ROT)) != 0, (bad, at)
            err = lib.d3f_last_error()
            assert word in err and b"frame %d:" % at in err, (bad, at, err)
    # a table that would scale, not rotate: c16^2 + s16^2 further than 2^17 from 2^32
    for bad in ((65536, 400), (65534, 0), (65538, 0), (0, 0), (46341, 46345), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 0)):
        for at in (0, 2):
            rows = list(ROT)
            rows[at] = bad
            assert call(3, _table(GOOD), _table(rows)) != 0, (bad, at)
            err = lib.d3f_last_error()
            assert b"no rotation" in err and b"frame %d:" % at in err, (bad, at, err)
    # the first bad frame is the one named, and a bad box is found before a bad rotation
    assert call(3, _table(GOOD), _table([ROT[0], (0, 0), (1, 1)])) != 0 and b"frame 1:" in lib.d3f_last_error()
    assert call(3, _table([GOOD[0], GOOD[1], (71, 0, 90, 90)]), _table([(0, 0)] * 3)) != 0
    assert b"outside" in lib.d3f_last_error()


def test_rotation_tables_at_the_edge_of_the_norm_bound():
    """(65537, 0): 65537^2 - 2^32 = 2^17 + 1 is refused, (65535, 0): 2^32 - 65535^2 = 2^17 - 1 is not; (65536, 362): 362^2 = 131044 <= 2^17 passes the norm check (and is
    then refused for what is checked behind it, not for the rotation)"""
    lib = _lib.lib()
    assert lib.d3f_crop_resize_cubic_rboxes_u8(0x100000, 1, 90, 160, _table(GOOD[:1]), _table([(65537, 0)]), 0x900000, 64, 64,
                                               192, None) != 0
    assert b"no rotation" in lib.d3f_last_error()
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    for passes in ((65536, 362), (65535, 0)):  # the fused form checks its channel count behind the tables
        assert lib.d3f_crop_resize_cubic_rboxes_u8_nhwc(_lib.F32, 0x100000, 1, 90, 160, _table(GOOD[:1]), _table([passes]),
                                                        0x900000, 64, 64, 192, 0xb00000, 2, ms, ms, None) != 0
        assert b"activation of 2 channels" in lib.d3f_last_error(), lib.d3f_last_error()
    assert lib.d3f_crop_resize_cubic_rboxes_u8(0x100000, 1, 90, 160, _table(GOOD[:1]), _table([(65536, 363)]), 0x900000, 64, 64,
                                               192, None) != 0
    assert b"no rotation" in lib.d3f_last_error()


def _engine_calls(lib, h):
    d, e, f = C.c_void_p(0x100000), C.c_void_p(0x500000), C.c_void_p(0x900000)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)

    def pair(boxes, rot, graph=0, raw=d):
        return lib.d3f_unet_predict_frames_rboxes_u8(h, d, d, raw, 90, 160, boxes, rot, e, ms, ms, d, graph, None)

    def full(boxes, rot, graph=0, raw=d):
        return lib.d3f_unet_predict_frames_full_rboxes_u8(h, d, d, raw, 90, 160, boxes, rot, 3, e, f, ms, ms, d, graph, None)

    return pair, full


def test_engine_rboxes_entries_refuse_before_any_device_call():
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 3, 64, 64, _lib.F32, C.byref(h)))
    try:
        pair, full = _engine_calls(lib, h)
        for call in (pair, full):
            assert call(None, _table(ROT)) != 0 and b"null boxes" in lib.d3f_last_error(), lib.d3f_last_error()
            assert call(_table(GOOD), None) != 0 and b"null rot" in lib.d3f_last_error(), lib.d3f_last_error()
            assert call(_table(GOOD), _table(ROT), raw=None) != 0 and b"null argument" in lib.d3f_last_error()
            assert call(_table(GOOD), _table(ROT), graph=1) != 0
            err = lib.d3f_last_error()
            assert b"graph" in err and b"kernel arguments" in err and b"use_graph = 0" in err, err
            assert call(_table([GOOD[0], GOOD[1], (71, 0, 90, 90)]), _table(ROT)) != 0
            err = lib.d3f_last_error()
            assert b"outside" in err and b"frame 2:" in err, err
            assert call(_table(GOOD), _table([ROT[0], (65536, 400), ROT[2]])) != 0
            err = lib.d3f_last_error()
            assert b"no rotation" in err and b"frame 1:" in err, err
        # the antialiased crop and the multiband pyramid of a rotated box are out of scope, and the message says so
        _lib.check(lib.d3f_unet_set_frame_resample(h, _lib.RESAMPLE_CUBIC_AA))
        for call in (pair, full):
            assert call(_table(GOOD), _table(ROT)) != 0
            err = lib.d3f_last_error()
            assert b"D3F_RESAMPLE_CUBIC_AA" in err and b"out of scope" in err, err
        _lib.check(lib.d3f_unet_set_frame_resample(h, _lib.RESAMPLE_CUBIC))
        _lib.check(lib.d3f_unet_set_frame_blend(h, _lib.BLEND_MULTIBAND, 2))
        assert full(_table(GOOD), _table(ROT)) != 0
        err = lib.d3f_last_error()
        assert b"D3F_BLEND_MULTIBAND" in err and b"out of scope" in err, err
    finally:
        lib.d3f_unet_destroy(h)
    pair_handle = C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 3, 64, 64, _lib.F32, 2, 2, C.byref(pair_handle)))
    try:
        for call in _engine_calls(lib, pair_handle):
            assert call(_table(GOOD), _table(ROT)) != 0 and b"pair" in lib.d3f_last_error(), lib.d3f_last_error()
    finally:
        lib.d3f_unet_destroy(pair_handle)


# ---- argument handling ----

def test_python_entries_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet
    frames = torch.zeros((3, 90, 160, 3), dtype=torch.uint8)
    patch = torch.zeros((3, 64, 64, 3), dtype=torch.uint8)
    angles = [12.5, -30.0, 0.0]
    with pytest.raises(ValueError, match="needs boxes"):
        ops.crop_resize_cubic_u8(frames, (64, 64), angles=angles)
    with pytest.raises(ValueError, match="needs boxes"):
        ops.crop_resize_cubic_u8(frames, (64, 64), box=GOOD[0], angles=angles)
    with pytest.raises(ValueError, match="needs boxes"):
        ops.paste_resize_cubic_u8(patch, frames, GOOD[0], angles=angles)
    with pytest.raises(ValueError, match="antialias"):
        ops.crop_resize_cubic_u8(frames, (64, 64), boxes=GOOD, angles=angles, antialias=True)
    for bad in (angles[:2], [1.0, 2.0, float("nan")], [1.0, 2.0, "x"], 5.0):
        with pytest.raises(ValueError):
            ops.crop_resize_cubic_u8(frames, (64, 64), boxes=GOOD, angles=bad)
        with pytest.raises(ValueError):
            ops.paste_resize_cubic_u8(patch, frames, boxes=GOOD, angles=bad)
    with pytest.raises(D3FError):                     # good arguments get as far as the missing device
        ops.crop_resize_cubic_u8(frames, (64, 64), boxes=GOOD, angles=angles)
    with pytest.raises(D3FError):
        ops.paste_resize_cubic_u8(patch, frames, boxes=GOOD, angles=angles)
    with pytest.raises(D3FError):                     # ... and all zero with antialias is the boxes call: no ValueError
        ops.crop_resize_cubic_u8(frames, (64, 64), boxes=GOOD, angles=[0, 0.004, -0.004], antialias=True)
    assert ops._rot_arg([0.0, 0.004, -0.0], 3, "test") is None
    assert list(ops._rot_arg(torch.tensor([30.0, 0.0, -90.0]), 3, "test")) == [56756, 32768, 65536, 0, 0, -65536]
    net = Unet("resnet18", None, 3, 3, None).eval()
    half = [0.5] * 3
    for call in (net.predict_frames_u8, net.predict_frames_full_u8):
        with pytest.raises(ValueError, match="box per frame"):
            call(frames, (64, 64), half, half, angles=angles)
        with pytest.raises(ValueError, match="box per frame"):
            call(frames, (64, 64), half, half, boxes=GOOD[0], angles=angles)
        with pytest.raises(ValueError, match="antialias"):
            call(frames, (64, 64), half, half, boxes=GOOD, angles=angles, antialias=True)
        with pytest.raises(ValueError, match="angles"):
            call(frames, (64, 64), half, half, boxes=GOOD, angles=angles[:2])
        with pytest.raises(D3FError):
            call(frames, (64, 64), half, half, boxes=GOOD, angles=angles)
    with pytest.raises(ValueError, match="multiband"):
        net.predict_frames_full_u8(frames, (64, 64), half, half, boxes=GOOD, angles=angles, blend="multiband")
    with pytest.raises(D3FError):                     # zero angles: the boxes call, multiband and all
        net.predict_frames_full_u8(frames, (64, 64), half, half, boxes=GOOD, angles=[0.0] * 3, blend="multiband")


def test_tools_track_rotate_arguments(tmp_path):
    import denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model as render
    import denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images as images
    base = {render: ["in.mp4", "last.ckpt", "a", "64", "64"], images: ["in.mp4", "64", "64"]}
    for tool, argv in base.items():
        assert tool.parse_command_line_arguments(argv).track_rotate is False
        assert tool.parse_command_line_arguments(argv + ["--track", "t.txt"]).track_rotate is False
        assert tool.parse_command_line_arguments(argv + ["--track", "t.txt", "--track-rotate"]).track_rotate is True
        for bad in (["--track-rotate"], ["--track", "t.txt", "--track-rotate", "--antialias"]):
            with pytest.raises(SystemExit):
                tool.parse_command_line_arguments(argv + bad)
    with pytest.raises(SystemExit):
        render.parse_command_line_arguments(base[render] + ["--track", "t.txt", "--track-rotate", "--output", "full", "--blend",
                                                            "multiband"])
    faces = [(40, 30, 20, 30, 12.5)]
    with pytest.raises(ValueError, match="track"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), track_rotate=True)
    with pytest.raises(ValueError, match="antialias"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), track=faces,
                               track_rotate=True, antialias=True)
    with pytest.raises(ValueError, match="multiband"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), track=faces,
                               track_rotate=True, output="full", blend="multiband")
    with pytest.raises(ValueError, match="track"):
        images.VideoToImages(tmp_path / "clip.mp4", 64, 64, frames=[], track_rotate=True)
    with pytest.raises(ValueError, match="antialias"):
        images.VideoToImages(tmp_path / "clip.mp4", 64, 64, frames=[], track=faces, track_rotate=True, antialias=True)
    # both tools read the same entries off the same five-column file
    track = tmp_path / "t.txt"
    track.write_text("40 30 20 30 12.5\n-\n100 60 40 40\n90 50 40 40 -20\n")
    entries = render.load_rtrack(track, 0)
    assert entries == [(40, 30, 20, 30, 12.5)] * 2 + [(100, 60, 40, 40, 0.0), (90, 50, 40, 40, -20.0)]
    assert images.load_rtrack(track, 0) == entries
    assert render.load_rtrack(track, 1) == ops.smooth_rbox_track(entries, 1)
    assert render.load_rtrack([(1, 2, 3, 4), (1, 2, 3, 4, 5.004)], 0) == [(1, 2, 3, 4, 0.0), (1, 2, 3, 4, 5.0)]
    # without the flag the same file is refused as ever: five fields are an error to read_box_track
    with pytest.raises(ValueError, match="line 1"):
        render.load_track(track, 1.6, 0)


# ---- the restatement against an independent float64 oracle ----
# torch.nn.functional.grid_sample(mode="bicubic", padding_mode="border", align_corners=False) in float64 on a grid built from
# the real cos / sin: torch's bicubic uses A = -0.75 and clamps tap indices under `border`.  The bound (DESIGN.md section 4
# "Rotated crop", derived, not tuned): with w_k(t) the four Keys weights, S = max_t sum_k |w_k(t)| = 1.375 and
# G = max_t sum_k |w_k'(t)| = 3 (both at t = 0.5), the interpolant of bytes moves by at most 255 * G * S = 1051.875 grey levels
# per unit of position on an axis.  The position is off by the two quantisations: cos and sin each by at most 2^-17 (rounding
# to 2^-16), which the lever arm multiplies, and the floor to 16 fractional bits, below 2^-16.

GRADIENT = 255.0 * 3.0 * 1.375
HW = (48, 64)
CASES = [((3, 5, 40, 30), 7.5), ((24, 18, 40, 30), -33.0), ((10, 8, 24, 24), 90.0), ((30, 0, 34, 40), 179.99),
         ((12, 9, 37, 29), 123.45), ((0, 0, 40, 40), -0.01)]


def test_the_bound_s_constants_are_the_keys_kernel_s():
    t = np.linspace(0.0, 1.0, 20001)
    x = np.stack([t + 1, t, 1 - t, 2 - t])
    A = -0.75
    w = np.where(x <= 1, ((A + 2) * x - (A + 3)) * x * x + 1, ((A * x - 5 * A) * x + 8 * A) * x - 4 * A)
    dw = np.where(x <= 1, 3 * (A + 2) * x * x - 2 * (A + 3) * x, 3 * A * x * x - 10 * A * x + 8 * A)
    assert abs(np.abs(w).sum(0).max() - 1.375) < 1e-9 and abs(np.abs(dw).sum(0).max() - 3.0) < 1e-9
    assert np.allclose(R.keys_weights(t, np.float64), w.T, atol=1e-15)


def _frame(seed, hw):
    return np.random.default_rng(seed).integers(0, 256, size=hw + (3,), dtype=np.uint8)


def _grid_sample(img, x, y):
    """img [h, w, 3] uint8, positions x, y in tap-index units (float64 [N]) -> float64 [N, 3]"""
    h, w = img.shape[:2]
    grid = torch.from_numpy(np.stack([(2 * x + 1) / w - 1, (2 * y + 1) / h - 1], axis=-1))[None, None]
    src = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    out = torch.nn.functional.grid_sample(src, grid, mode="bicubic", padding_mode="border", align_corners=False)
    return out[0, :, 0].T.numpy()


@pytest.mark.parametrize("size", [(16, 16), (16, 24)])
def test_crop_restatement_against_grid_sample(size):
    H, W = size
    worst = 0.0
    for n, (box, angle) in enumerate(CASES):
        frame = _frame(100 + n, HW)
        x1, y1, cw, ch = box
        a = math.radians(ops.angle_hundredths(angle) / 100.0)
        ox, oy = np.meshgrid(np.arange(W), np.arange(H))
        u, v = cw * (2 * ox + 1 - W) / (2 * W), ch * (2 * oy + 1 - H) / (2 * H)
        x = x1 + (cw - 1) / 2 + math.cos(a) * u - math.sin(a) * v
        y = y1 + (ch - 1) / 2 + math.sin(a) * u + math.cos(a) * v
        want = _grid_sample(frame, x.reshape(-1), y.reshape(-1)).reshape(H, W, 3)
        got = R.rot_crop(frame, box, ops.box_rotation(angle), size, dtype=np.float64)
        # |u| <= cw / 2, |v| <= ch / 2: each coordinate is off by at most 2^-17 (cw + ch) / 2 + 2^-16
        e = 2.0 ** -17 * (cw + ch) / 2 + 2.0 ** -16
        bound = GRADIENT * 2 * e
        assert bound < 0.75, bound  # near one grey level: the comparison is not vacuous on noise
        err = float(np.abs(got - want).max())
        assert err <= bound, (box, angle, err, bound)
        worst = max(worst, err)
        # the float32 form, the kernels' own, sits on the float64 form: 24 products and sums of values below 2^10
        assert float(np.abs(R.rot_crop(frame, box, ops.box_rotation(angle), size).astype(np.float64) - got).max()) < 1e-2
    assert worst > 1e-4  # the quantisations are seen: the oracle is not the restatement in disguise


@pytest.mark.parametrize("feather", [0, 5])
def test_paste_restatement_against_grid_sample(feather):
    H = W = 16
    for n, (box, angle) in enumerate(CASES):
        frame, patch = _frame(200 + n, HW), _frame(300 + n, (H, W))
        x1, y1, cw, ch = box
        a = math.radians(ops.angle_hundredths(angle) / 100.0)
        px, py = np.meshgrid(np.arange(HW[1], dtype=np.float64), np.arange(HW[0], dtype=np.float64))
        dx, dy = px - (x1 + (cw - 1) / 2), py - (y1 + (ch - 1) / 2)
        j = (cw - 1) / 2 + math.cos(a) * dx + math.sin(a) * dy
        i = (ch - 1) / 2 - math.sin(a) * dx + math.cos(a) * dy
        mask = (j >= -0.5) & (j < cw - 0.5) & (i >= -0.5) & (i < ch - 0.5)
        got, got_mask = R.rot_paste(patch, frame, box, ops.box_rotation(angle), feather, dtype=np.float64)
        # inside the rectangle |dx| + |dy| <= sqrt((cw^2 + ch^2) / 2): j' and i' are off by at most e_j
        e_j = 2.0 ** -17 * math.sqrt((cw * cw + ch * ch) / 2.0)
        edge = np.minimum(np.minimum(j + 0.5, cw - 0.5 - j), np.minimum(i + 0.5, ch - 0.5 - i))
        assert bool((np.abs(edge[mask != got_mask]) <= e_j).all())  # the two rectangles differ on their very border only
        both = mask & got_mask
        assert int(both.sum()) > 0.5 * cw * ch
        v = np.clip(_grid_sample(patch, (j[both] + 0.5) * W / cw - 0.5, (i[both] + 0.5) * H / ch - 0.5), 0.0, 255.0)
        ramp = lambda d: np.minimum(d + 1, feather + 1) / (feather + 1)  # noqa: E731
        alpha = ramp(np.minimum(i[both], ch - 1 - i[both])) * ramp(np.minimum(j[both], cw - 1 - j[both]))
        want = alpha[:, None] * v + (1 - alpha)[:, None] * frame[both].astype(np.float64)
        # the patch position is off by e_j W / cw + 2^-16 per axis; a ramp by (e_j + 2^-16) / (feather + 1) and its float32
        # arithmetic (two conversions and a division: 2^-22), their product and 1 - a by 2^-24 each
        e_v = GRADIENT * ((e_j * W / cw + 2.0 ** -16) + (e_j * H / ch + 2.0 ** -16))
        e_a = 2 * ((e_j + 2.0 ** -16) / (feather + 1) + 2.0 ** -22) + 2.0 ** -23
        bound = e_v + 255.0 * e_a
        assert bound < 1.0, bound
        err = float(np.abs(got[both] - want).max())
        assert err <= bound, (box, angle, err, bound)
        assert np.array_equal(got[~got_mask], frame[~got_mask].astype(np.float64))
