"""CPU: the tracked crop without a device -- ops.track_crop_box, ops.read_box_track and ops.smooth_box_track pinned by hand,
the host-side guards of the four _boxes_ operators and the two boxes entries of the engine (everything is refused before a
device call: the dummy pointers are never dereferenced), and the argument handling of the Python entries and both tools."""
import ctypes as C

import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib, ops


def _table(rows):
    return (C.c_int32 * (4 * len(rows)))(*[v for row in rows for v in row])


# ---- track_crop_box ----

FACES = [(900, 400, 200, 300), (-50, -80, 200, 300), (1800, 900, 300, 400), (0, 0, 1, 1), (5, 5, 4000, 3000),
         (-500, 300, 200, 200), (960, 540, 37, 91), (1919, 1079, 1, 1)]


@pytest.mark.parametrize("hw", [(1080, 1920), (150, 200), (333, 77)])
@pytest.mark.parametrize("size", [(256, 256), (448, 320), (64, 96)])
@pytest.mark.parametrize("margin", [1.0, 1.6, 3.0])
def test_track_crop_box_lies_inside_the_frame_with_the_target_aspect(hw, size, margin):
    """faces inside, partly outside and larger than the frame; |cw * height - ch * width| < width + height: both extents are
    int() of the same scale times width and height, so each is less than 1 below its exact value"""
    h, w = hw
    width, height = size
    for face in FACES:
        x1, y1, cw, ch = ops.track_crop_box(h, w, width, height, face, margin)
        assert cw >= 1 and ch >= 1 and x1 >= 0 and y1 >= 0 and x1 + cw <= w and y1 + ch <= h, (face, (x1, y1, cw, ch))
        assert abs(cw * height - ch * width) < width + height, (face, (cw, ch))
        assert all(isinstance(v, int) for v in (x1, y1, cw, ch))


@pytest.mark.parametrize("hw, size", [((1080, 1920), (256, 256)), ((1080, 1920), (448, 320)), ((150, 200), (64, 64)),
                                      ((333, 77), (64, 96))])
def test_a_centred_face_wider_than_the_frame_gives_the_centre_crop(hw, size):
    h, w = hw
    width, height = size
    for face in ((-w, -h, 3 * w, 3 * h), (0, 0, w, h), (-10, -10, w + 20, h + 20)):
        assert ops.track_crop_box(h, w, width, height, face) == ops.center_crop_box(h, w, width, height)


def test_track_crop_box_by_hand():
    # s = max(200 / 256, 300 / 256) * 1.6 = 1.875: 480 x 480 around the face's centre (1000, 550)
    assert ops.track_crop_box(1080, 1920, 256, 256, (900, 400, 200, 300)) == (760, 310, 480, 480)
    # the same face at the frame's corner: the box is moved inside
    assert ops.track_crop_box(1080, 1920, 256, 256, (-50, -80, 200, 300)) == (0, 0, 480, 480)
    assert ops.track_crop_box(1080, 1920, 256, 256, (1800, 900, 200, 300)) == (1440, 600, 480, 480)
    # margin 1: s = 300 / 256, int(256 * 1.171875) = 300
    assert ops.track_crop_box(1080, 1920, 256, 256, (900, 400, 200, 300), margin=1.0) == (850, 400, 300, 300)
    # 448 x 320 target: s = max(100 / 448, 100 / 320) * 1.6 = 0.5: 224 x 160 around (150, 100)
    assert ops.track_crop_box(600, 800, 448, 320, (100, 50, 100, 100)) == (38, 20, 224, 160)
    # s = 101 / 320 * 1.6 = 0.505: int(226.24) x int(161.6); x1 = (202 + 101 - 226) // 2 = 77 // 2, an odd sum floors
    assert ops.track_crop_box(600, 800, 448, 320, (101, 51, 101, 101)) == (38, 21, 226, 161)
    # a face of one pixel: the extents never drop below 1
    assert ops.track_crop_box(100, 100, 64, 64, (50, 50, 1, 1), margin=0.5) == (50, 50, 1, 1)
    # capped by the centre crop's scale: 150 x 150 of a 150 x 200 frame, x follows the face, y cannot move
    assert ops.track_crop_box(150, 200, 64, 64, (120, 10, 100, 100)) == (50, 0, 150, 150)
    assert ops.TRACK_MARGIN == 1.6
    with pytest.raises(ValueError):
        ops.track_crop_box(100, 100, 64, 64, (5, 5, 0, 10))


# ---- read_box_track, smooth_box_track ----

def test_read_box_track(tmp_path):
    path = tmp_path / "track.txt"
    path.write_text("# x y w h\n"
                    "-\n"
                    "- # nothing found yet\n"
                    "\n"
                    "10 20 30 40\n"
                    "11,21,31,41   # commas\n"
                    "-\n"
                    "  12, 22 ,32  42\n"
                    "-\n")
    faces = ops.read_box_track(path)
    # leading gaps take the first detection, inner and trailing ones the previous; comment and blank lines are no frames
    assert faces == [(10, 20, 30, 40)] * 3 + [(11, 21, 31, 41)] * 2 + [(12, 22, 32, 42)] * 2
    assert ops.read_box_track(str(path)) == faces
    assert ops.box_of_frame(faces, 0) == (10, 20, 30, 40) and ops.box_of_frame(faces, 6) == (12, 22, 32, 42)
    assert ops.box_of_frame(faces, 7) == (12, 22, 32, 42) and ops.box_of_frame(faces, 1000) == (12, 22, 32, 42)  # a short file
    path.write_text("# only gaps\n-\n-\n")
    with pytest.raises(ValueError, match="no detection"):
        ops.read_box_track(path)
    path.write_text("")
    with pytest.raises(ValueError, match="no detection"):
        ops.read_box_track(path)
    for bad in ("1 2 3\n", "1 2 3 4 5\n", "1 2 3 x\n", "1.5 2 3 4\n", "- -\n"):
        path.write_text("1 2 3 4\n" + bad)
        with pytest.raises(ValueError, match="line 2"):
            ops.read_box_track(path)


def test_smooth_box_track_by_hand():
    faces = [(0, 0, 10, 10), (10, 2, 10, 10), (20, 0, 12, 10), (30, 5, 10, 11), (40, 0, 10, 10)]
    assert ops.smooth_box_track(faces, 0) == faces
    assert ops.smooth_box_track([list(f) for f in faces], 0) == [list(f) for f in faces]  # n = 0: the input, untouched
    # n = 1, sums of (2 fx + fw, 2 fy + fh, fw, fh) over the truncated window, floor division by its length:
    #   k = 0: (10 + 30) // 2 = 20, (10 + 14) // 2 = 12, 10, 10              -> fx = (20 - 10) // 2 = 5, fy = 1
    #   k = 1: (10 + 30 + 52) // 3 = 30, (10 + 14 + 10) // 3 = 11, 32 // 3 = 10, 10 -> fx = 10, fy = (11 - 10) // 2 = 0
    #   k = 2: (30 + 52 + 70) // 3 = 50, (14 + 10 + 21) // 3 = 15, 10, 31 // 3 = 10 -> fx = 20, fy = 2
    #   k = 3: (52 + 70 + 90) // 3 = 70, (10 + 21 + 10) // 3 = 13, 10, 10    -> fx = 30, fy = 1
    #   k = 4: (70 + 90) // 2 = 80, (21 + 10) // 2 = 15, 10, 21 // 2 = 10    -> fx = 35, fy = 2
    assert ops.smooth_box_track(faces, 1) == [(5, 1, 10, 10), (10, 0, 10, 10), (20, 2, 10, 10), (30, 1, 10, 10),
                                              (35, 2, 10, 10)]
    # n = 2 at the middle is the mean of all five: 252 // 5 = 50, 65 // 5 = 13, 52 // 5 = 10, 51 // 5 = 10
    assert ops.smooth_box_track(faces, 2)[2] == (20, 1, 10, 10)
    assert ops.smooth_box_track(faces, 100) == [ops.smooth_box_track(faces, 2)[2]] * 5  # every window is the whole track
    assert ops.smooth_box_track([(3, 4, 5, 6)] * 4, 3) == [(3, 4, 5, 6)] * 4
    with pytest.raises(ValueError):
        ops.smooth_box_track(faces, -1)


# ---- refusals of the C operators: no device ----

GOOD = [(35, 0, 90, 90), (0, 0, 160, 90), (70, 10, 33, 47)]


def _operators(lib):
    """the four _boxes_ operators as call(B, boxes) on 3 frames of 90 x 160 and 64 x 64 patches, and their names"""
    d, e, p, coef = 0x100000, 0x900000, 0x500000, 0x700000

    def crop(fn):
        return lambda B, boxes, W=64: fn(d, B, 90, 160, boxes, e, 64, W, 3 * W, None)

    return {
        "crop": crop(lib.d3f_crop_resize_cubic_boxes_u8),
        "crop_aa": crop(lib.d3f_crop_resize_cubic_aa_boxes_u8),
        "paste": lambda B, boxes: lib.d3f_paste_resize_cubic_boxes_u8(p, B, 64, 64, 192, d, 90, 160, boxes, 3, e, None),
        "paste_color": lambda B, boxes: lib.d3f_paste_resize_cubic_color_boxes_u8(p, B, 64, 64, 192, d, 90, 160, boxes, 3,
                                                                                 coef, e, None),
    }


@pytest.mark.parametrize("name", ["crop", "crop_aa", "paste", "paste_color"])
def test_boxes_operators_refuse_before_any_device_call(name):
    lib = _lib.lib()
    call = _operators(lib)[name]
    assert call(3, None) != 0 and b"null boxes" in lib.d3f_last_error(), lib.d3f_last_error()
    assert call(0, None) == 0  # nothing to do, nothing launched
    for bad, word in (((71, 0, 90, 90), b"outside"), ((35, 1, 90, 90), b"outside"), ((-1, 0, 90, 90), b"outside"),
                      ((0, -1, 90, 90), b"outside"), ((35, 0, 0, 90), b"non-positive"), ((35, 0, 90, -3), b"non-positive")):
        for at in (0, 1, 2):
            rows = list(GOOD)
            rows[at] = bad
            assert call(3, _table(rows)) != 0, (bad, at)
            err = lib.d3f_last_error()
            assert word in err and b"frame %d:" % at in err, (bad, at, err)
    # the first bad frame is the one named
    assert call(3, _table([GOOD[0], (71, 0, 90, 90), (35, 0, 0, 90)])) != 0 and b"frame 1:" in lib.d3f_last_error()


def test_aa_boxes_operator_refuses_a_box_above_32_times_the_output():
    lib = _lib.lib()
    ops_ = _operators(lib)
    rows = [GOOD[0], GOOD[2], (0, 0, 160, 90)]
    assert ops_["crop_aa"](3, _table(rows), W=4) != 0  # 160 > 32 * 4
    err = lib.d3f_last_error()
    assert b"32 times" in err and b"frame 2:" in err, err


def _engine_calls(lib, h):
    d, e, f = C.c_void_p(0x100000), C.c_void_p(0x500000), C.c_void_p(0x900000)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)

    def pair(boxes, graph=0, raw=d):
        return lib.d3f_unet_predict_frames_boxes_u8(h, d, d, raw, 90, 160, boxes, e, ms, ms, d, graph, None)

    def full(boxes, graph=0, raw=d):
        return lib.d3f_unet_predict_frames_full_boxes_u8(h, d, d, raw, 90, 160, boxes, 3, e, f, ms, ms, d, graph, None)

    return pair, full


def test_engine_boxes_entries_refuse_before_any_device_call():
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 3, 64, 64, _lib.F32, C.byref(h)))
    try:
        for call in _engine_calls(lib, h):
            assert call(None) != 0 and b"null boxes" in lib.d3f_last_error(), lib.d3f_last_error()
            assert call(_table(GOOD), raw=None) != 0 and b"null argument" in lib.d3f_last_error()
            assert call(_table(GOOD), graph=1) != 0
            err = lib.d3f_last_error()
            assert b"graph" in err and b"kernel arguments" in err and b"use_graph = 0" in err, err
            rows = [GOOD[0], GOOD[1], (71, 0, 90, 90)]
            assert call(_table(rows)) != 0
            err = lib.d3f_last_error()
            assert b"outside" in err and b"frame 2:" in err, err
            rows[2] = (35, 0, 90, 0)
            assert call(_table(rows)) != 0
            err = lib.d3f_last_error()
            assert b"non-positive" in err and b"frame 2:" in err, err
        _lib.check(lib.d3f_unet_set_frame_resample(h, _lib.RESAMPLE_CUBIC_AA))
        for call in _engine_calls(lib, h):  # 64 x 64 output: nothing of a 90 x 160 frame is above 32 times it; a bad box still is
            assert call(_table([GOOD[0], GOOD[1], (0, 0, 161, 90)])) != 0
            err = lib.d3f_last_error()
            assert b"outside" in err and b"frame 2:" in err, err
    finally:
        lib.d3f_unet_destroy(h)
    pair_handle = C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 3, 64, 64, _lib.F32, 2, 2, C.byref(pair_handle)))
    try:
        for call in _engine_calls(lib, pair_handle):
            assert call(_table(GOOD)) != 0 and b"pair" in lib.d3f_last_error(), lib.d3f_last_error()
    finally:
        lib.d3f_unet_destroy(pair_handle)


def test_frame_boxes_max_is_the_header_s():
    text = _lib.HEADER_PATH.read_text()
    assert "#define D3F_FRAME_BOXES_MAX 64" in text


# ---- argument handling ----

def test_python_entries_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet
    frames = torch.zeros((3, 90, 160, 3), dtype=torch.uint8)
    patch = torch.zeros((3, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="exclude"):
        ops.crop_resize_cubic_u8(frames, (64, 64), box=GOOD[0], boxes=GOOD)
    with pytest.raises(ValueError, match="exactly one"):
        ops.paste_resize_cubic_u8(patch, frames, GOOD[0], boxes=GOOD)
    with pytest.raises(ValueError, match="exactly one"):
        ops.paste_resize_cubic_u8(patch, frames)
    with pytest.raises(D3FError):                     # good arguments get as far as the missing device
        ops.crop_resize_cubic_u8(frames, (64, 64), boxes=GOOD)
    with pytest.raises(D3FError):
        ops.paste_resize_cubic_u8(patch, frames, boxes=GOOD)
    for bad in (GOOD[:2], [GOOD[0], GOOD[1], (1, 2, 3)], [GOOD[0], GOOD[1], (1, 2, 3, 2 ** 31)]):
        with pytest.raises(ValueError, match="boxes"):
            ops._boxes_arg(bad, 3, "test")
    table, rows = ops._boxes_arg(torch.tensor(GOOD), 3, "test")
    assert list(table) == [v for row in GOOD for v in row] and rows == GOOD
    net = Unet("resnet18", None, 3, 3, None).eval()
    for call in (net.predict_frames_u8, net.predict_frames_full_u8):
        with pytest.raises(D3FError):
            call(frames, (64, 64), [0.5] * 3, [0.5] * 3, boxes=GOOD)
        with pytest.raises(D3FError):
            call(frames, (64, 64), [0.5] * 3, [0.5] * 3, boxes=GOOD[0])


def test_tools_track_arguments(tmp_path):
    import d3f.script_tools.put_video_through_fake_model as render
    import d3f.script_tools.video_to_center_cropped_images as images
    base = {render: ["in.mp4", "last.ckpt", "a", "64", "64"], images: ["in.mp4", "64", "64"]}
    for tool, argv in base.items():
        a = tool.parse_command_line_arguments(argv)
        assert a.track is None and a.track_margin is None and a.track_smooth is None
        a = tool.parse_command_line_arguments(argv + ["--track", "t.txt"])
        assert a.track == "t.txt" and a.track_margin is None and a.track_smooth is None
        a = tool.parse_command_line_arguments(argv + ["--track", "t.txt", "--track-margin", "2.5", "--track-smooth", "3"])
        assert a.track_margin == 2.5 and a.track_smooth == 3
        for bad in (["--track-margin", "2"], ["--track-smooth", "1"], ["--track", "t.txt", "--track-margin", "0"],
                    ["--track", "t.txt", "--track-smooth", "-1"], ["--track", "t.txt", "--track-margin", "wide"]):
            with pytest.raises(SystemExit):
                tool.parse_command_line_arguments(argv + bad)
    with pytest.raises(ValueError, match="track"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), track_margin=2.0)
    with pytest.raises(ValueError, match="track"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), track_smooth=1)
    with pytest.raises(ValueError, match="track"):
        images.VideoToImages(tmp_path / "clip.mp4", 64, 64, frames=[], track_smooth=1)
    with pytest.raises(ValueError, match="no detection"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), track=[])
    # the two tools read the same boxes off the same track, the frame counter carried across batches
    track = tmp_path / "t.txt"
    track.write_text("40 30 20 30\n-\n100 60 40 40\n")
    faces = render.load_track(track, 1.6, 0)
    assert faces == [(40, 30, 20, 30), (40, 30, 20, 30), (100, 60, 40, 40)]
    boxes = ops.track_crop_boxes(faces, 1, 4, 150, 200, 64, 64)
    assert boxes == [ops.track_crop_box(150, 200, 64, 64, faces[k]) for k in (1, 2, 2, 2)]
    assert render.load_track(track, 1.6, 1) == ops.smooth_box_track(faces, 1)
