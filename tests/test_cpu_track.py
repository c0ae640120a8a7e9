"""CPU: the template tracker without a device -- the geometry by hand, the restatement (tests/track_restatement.py) on the
moving-patch recipe and on hand-made images (ties, a lost frame, adapt), the tool's arguments and its file, and the
refusals of the four C entries (everything is refused before a device call: the dummy pointers are never dereferenced)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import track_restatement as tr
from denoising_diffusion_deep_fake_amd import _lib, ops


# ---- geometry ----

def test_geometry_by_hand():
    # 200 x 300 at side 48: s = ceil(300 / 48) = 7; tx = 900 // 7 = 128, ty = 400 // 7 = 57, tw = 1100 // 7 - 128 = 29,
    # th = 700 // 7 - 57 = 43; ox = 900 - 896 = 4, oy = 400 - 399 = 1
    assert ops.track_template_geometry(1080, 1920, (900, 400, 200, 300)) == (7, 128, 57, 29, 43, 4, 1, 200, 300)
    # clipped at the top-left corner: (0, 0, 150, 220), s = ceil(220 / 48) = 5
    assert ops.track_template_geometry(1080, 1920, (-50, -80, 200, 300)) == (5, 0, 0, 30, 44, 0, 0, 150, 220)
    # clipped at the bottom-right: (1800, 900, 120, 180): s = 4, tx = 450, ty = 225, tw = 480 - 450, th = 270 - 225
    assert ops.track_template_geometry(1080, 1920, (1800, 900, 300, 400)) == (4, 450, 225, 30, 45, 0, 0, 120, 180)
    # a small face: s = 1, the template is the box
    assert ops.track_template_geometry(96, 160, (31, 17, 20, 24)) == (1, 31, 17, 20, 24, 0, 0, 20, 24)
    # side 64, the largest: s = ceil(300 / 64) = 5
    assert ops.track_template_geometry(1080, 1920, (900, 400, 200, 300), side=64) == (5, 180, 80, 40, 60, 0, 0, 200, 300)
    # the default side keeps both extents at most 64: tw <= fw / s + 1 <= 48 + 1
    for face in ((3, 5, 1531, 977), (7, 9, 333, 1000), (0, 0, 1500, 1080)):
        s, tx, ty, tw, th, ox, oy, fw, fh = ops.track_template_geometry(1080, 1920, face)
        assert 4 <= tw <= 64 and 4 <= th <= 64 and 0 <= ox < s and 0 <= oy < s
        assert (tx + tw) * s <= 1920 and (ty + th) * s <= 1080
    assert ops.track_template_geometry(1080, 1920, (900, 401, 200, 21))[4] == 4  # s = 5: th = 422 // 5 - 401 // 5
    assert ops.TRACK_TEMPLATE_SIDE == 48 and ops.TRACK_SEARCH == 16 and ops.TRACK_ADAPT == 1 and ops.TRACK_LOST == 16
    for h, w, face, side in ((1080, 1920, (900, 400, 200, 300), 48), (96, 160, (150, 90, 30, 30), 48),
                             (333, 77, (-5, 7, 80, 300), 17)):
        assert ops.track_template_geometry(h, w, face, side) == tr.geometry(h, w, face, side)


@pytest.mark.parametrize("h, w, face, side", [
    (100, 100, (100, 10, 20, 20), 48),     # nothing inside the frame
    (100, 100, (10, -30, 20, 30), 48),
    (100, 100, (10, 10, 0, 20), 48),
    (4000, 4000, (0, 0, 1600, 100), 48),   # s = 34
    (100, 100, (10, 10, 3, 40), 48),       # tw = 3
    (1080, 1920, (900, 401, 200, 18), 48),  # s = 5: th = 419 // 5 - 401 // 5 = 3
    (100, 100, (10, 10, 40, 40), 65),      # side above D3F_TRACK_MAX_SIDE
    (100, 100, (10, 10, 40, 40), 0),
])
def test_geometry_value_errors(h, w, face, side):
    with pytest.raises(ValueError):
        ops.track_template_geometry(h, w, face, side)


# ---- the restatement on the recipe ----

@pytest.mark.parametrize("s, absent", [(2, ()), (1, (5,))])
def test_the_restatement_recovers_the_recipes_trajectory(s, absent):
    """96 x 160, step 3, R = 8: every frame with the patch is found where the recipe put it, at 1..3 levels a sample; the
    frame without it costs above lost = 16 a sample, is written as not found and moves nothing; the next frame's true
    position is within R of the stale one, and the tracker has it again"""
    ph, pw = (12, 10) if s == 2 else (24, 20)
    frames, positions = tr.moving_patch_frames(1234 + s, 10, 96, 160, s, 3, absent=absent, patch=(ph, pw))
    gray = tr.gray_decimate(frames, s)
    assert gray.shape == (10, 96 // s, 160 // s)
    T, pos = tr.seed(gray[0], positions[0][0], positions[0][1], pw, ph)
    n = pw * ph
    T1, pos1, rows = tr.search(gray[1:], T, pos, 8, 1, 16)
    last = positions[0]
    for k, row in enumerate(rows.tolist(), 1):
        if k in absent:
            assert row[3] == 0 and tuple(row[:2]) == last and row[2] > 16 * n, (k, row)
        else:
            assert row[3] == 1 and tuple(row[:2]) == positions[k] and row[2] <= 3 * n, (k, row, positions[k])
            last = positions[k]
    assert pos1 == last
    assert len(set(positions)) > 5, "the patch moves"


def test_a_constant_image_gives_no_displacement():
    G = np.full((3, 40, 50), 77, dtype=np.uint8)
    T, pos = tr.seed(G[0], 11, 9, 13, 7)
    T1, pos1, rows = tr.search(G, T, pos, 16, 1, 0)
    assert pos1 == (11, 9) and rows.tolist() == [[11, 9, 0, 1]] * 3 and np.array_equal(T1, T)


def test_the_tie_order():
    """equal costs: the smaller displacement, then the smaller dy, then the smaller dx"""
    T = np.full((4, 4), 200, dtype=np.uint8)

    def run(marks, pos=(10, 10)):
        G = np.zeros((24, 24), dtype=np.uint8)  # cost 3200 everywhere ...
        for x, y in marks:
            G[y:y + 4, x:x + 4] = 200           # ... except at the marks and around them
        return tr.search_frame(G, T, pos, 8, 0, 255)[2]

    # two perfect matches: the nearer one
    assert run([(10 + 5, 10), (10 - 4, 10)]) == (6, 10, 0, 1)
    # the same distance, dy = -4 against dy = +4 and dx = -4 against dx = +4: the smaller dy, whatever dx
    assert run([(10, 14), (10, 6), (14, 10), (6, 10)]) == (10, 6, 0, 1)
    # dy equal (0): the smaller dx
    assert run([(14, 10), (6, 10)]) == (6, 10, 0, 1)
    # the key's own order: (dx, dy) = (3, -4) and (-3, -4) and (4, 3): all 25; dy = -4 first, then dx = -3
    assert run([(13, 6), (7, 6), (14, 13)]) == (7, 6, 0, 1)


def test_a_lost_frame_leaves_template_and_position_untouched():
    rng = np.random.default_rng(5)
    G0 = rng.integers(0, 256, size=(30, 40), dtype=np.uint8)
    T, pos = tr.seed(G0, 12, 8, 9, 6)
    other = (255 - G0).astype(np.uint8)
    T1, pos1, row = tr.search_frame(other, T, pos, 4, 8, 16)
    assert row[3] == 0 and pos1 == pos == (12, 8) and row[:2] == (12, 8) and np.array_equal(T1, T)
    assert row[2] > 16 * 54
    # the same frame under lost = 255 is found, and adapt = 8 replaces the template by the window
    T2, pos2, row2 = tr.search_frame(other, T, pos, 4, 8, 255)
    assert row2[3] == 1 and row2[2] == row[2]
    assert np.array_equal(T2, other[pos2[1]:pos2[1] + 6, pos2[0]:pos2[0] + 9])


def test_adapt_by_hand():
    G = np.zeros((8, 8), dtype=np.uint8)
    G[2:6, 2:6] = [[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120], [255, 0, 7, 9]]
    T = np.array([[12, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 125], [250, 3, 0, 9]], dtype=np.uint8)
    T0, pos, row = tr.search_frame(G, T, (2, 2), 1, 0, 255)
    assert pos == (2, 2) and row == (2, 2, 2 + 5 + 5 + 3 + 7, 1) and np.array_equal(T0, T)  # adapt 0: T stays
    T8 = tr.search_frame(G, T, (2, 2), 1, 8, 255)[0]
    assert np.array_equal(T8, G[2:6, 2:6])                                                   # adapt 8: T = W
    T1 = tr.search_frame(G, T, (2, 2), 1, 1, 255)[0]
    # (T * 7 + W + 4) >> 3: 12, 10 -> 98 >> 3 = 12; 125, 120 -> 999 >> 3 = 124; 250, 255 -> 2009 >> 3 = 251;
    # 3, 0 -> 25 >> 3 = 3; 0, 7 -> 11 >> 3 = 1
    assert (T1[0, 0], T1[2, 3], T1[3, 0], T1[3, 1], T1[3, 2]) == (12, 124, 251, 3, 1)
    T4 = tr.search_frame(G, T, (2, 2), 1, 4, 255)[0]
    assert (T4[0, 0], T4[2, 3], T4[3, 0], T4[3, 1], T4[3, 2]) == (11, 123, 253, 2, 4)  # (T * 4 + W * 4 + 4) >> 3


def test_gray_reduction_by_hand():
    f = np.zeros((5, 7, 3), dtype=np.uint8)
    f[0, 0] = (1, 2, 3)       # 1 + 4 + 3 = 8
    f[0, 1] = (255, 255, 255)  # 1020
    f[1, 0] = (0, 1, 0)       # 2
    f[1, 1] = (9, 0, 0)       # 9
    g = tr.gray_decimate(f, 2)
    assert g.shape == (2, 3) and g[0, 0] == (8 + 1020 + 2 + 9) // 16 and not g[1:].any() and not g[0, 1:].any()
    assert np.array_equal(tr.gray_decimate(f, 1)[0, :2], [2, 255])
    assert tr.gray_decimate(np.full((2, 64, 96, 3), 255, dtype=np.uint8), 32).tolist() == [[[255] * 3] * 2] * 2


# ---- track_faces, the tool's arguments and its file ----

def test_track_faces():
    state = SimpleNamespace(geometry=(7, 128, 57, 29, 43, 4, 1, 200, 300))
    rows = [(128, 57, 100, 1), (130, 56, 99999, 0), (0, 0, 0, 1)]
    assert ops.track_faces(rows, state) == [(900, 400, 200, 300), None, (4, 1, 200, 300)]
    assert ops.track_faces(torch.tensor(rows).tolist(), state.geometry) == ops.track_faces(rows, state)
    assert ops.track_faces(rows, state) == tr.faces(rows, state.geometry)


def test_tool_arguments():
    import d3f.script_tools.track_face_box as tool
    a = tool.parse_command_line_arguments(["in.mp4", "--key", "0", "10", "20", "30", "40"])
    assert a.key == [[0, 10, 20, 30, 40]] and a.output is None and a.batch_frames == 8
    assert (a.search, a.adapt, a.lost, a.template_side) == (16, 1, 16, 48)
    a = tool.parse_command_line_arguments(["in.mp4", "--key", "7", "1", "2", "30", "40", "--key", "0", "10", "20", "30", "40",
                                           "-o", "t.txt", "--batch-frames", "3", "--search", "64", "--adapt", "0",
                                           "--lost", "255", "--template-side", "64"])
    assert tool.sorted_keys(a.key) == {0: (10, 20, 30, 40), 7: (1, 2, 30, 40)} and a.output == "t.txt"
    key = ["--key", "0", "10", "20", "30", "40"]
    for bad in ([], ["--key", "0", "10", "20", "30"], key + key, key + ["--key", "-1", "1", "2", "3", "4"],
                ["--key", "0", "10", "20", "0", "40"], key + ["--search", "0"], key + ["--search", "65"],
                key + ["--adapt", "9"], key + ["--adapt", "-1"], key + ["--lost", "256"], key + ["--template-side", "65"],
                key + ["--template-side", "3"], key + ["--batch-frames", "0"], key + ["--lost", "many"]):
        with pytest.raises(SystemExit):
            tool.parse_command_line_arguments(["in.mp4"] + bad)
    for keys in ([], [(0, 1, 2, 3)], [(3, 1, 2, 30, 40), (3, 5, 6, 30, 40)], [(-2, 1, 2, 30, 40)], [(0, 1, 2, 30, -40)]):
        with pytest.raises(ValueError, match="key"):
            tool.TrackFaceBox("clip.mp4", keys, frames=[])
    with pytest.raises(ValueError, match="search"):
        tool.TrackFaceBox("clip.mp4", [(0, 1, 2, 30, 40)], frames=[], search=0)
    with pytest.raises(ValueError, match="adapt"):
        tool.TrackFaceBox("clip.mp4", [(0, 1, 2, 30, 40)], frames=[], adapt=1.5)


def test_a_key_past_the_last_frame_is_an_error_after_the_run(tmp_path):
    """three frames, the only key at frame 5: nothing to follow (and no device needed), the file is written, then the error"""
    import d3f.script_tools.track_face_box as tool
    frames = [np.zeros((20, 30, 3), dtype=np.uint8)] * 3
    got = []
    with pytest.raises(ValueError, match="frame 5 is past"):
        tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames, sink=got.append,
                          output_path=tmp_path / "t.txt")
    assert got == [None] * 3
    lines = (tmp_path / "t.txt").read_text().splitlines()
    assert [line for line in lines if not line.startswith("#")] == ["-"] * 3
    # the default path lies next to the video; a sink alone writes no file
    with pytest.raises(ValueError, match="past"):
        tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames)
    assert (tmp_path / "clip_track.txt").exists()
    (tmp_path / "clip_track.txt").unlink()
    with pytest.raises(ValueError, match="past"):
        tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames, sink=got.append)
    assert not (tmp_path / "clip_track.txt").exists()


def test_the_written_file_round_trips_through_read_box_track(tmp_path):
    import d3f.script_tools.track_face_box as tool
    track = [None, None, (10, 20, 30, 40), (11, 21, 30, 40), None, (13, 19, 30, 40), None]
    path = tmp_path / "t.txt"
    tool.write_track(path, track, header=("settings: search 16, adapt 1", "keys (frame x y w h): 2 10 20 30 40"))
    text = path.read_text().splitlines()
    assert text[:2] == ["# settings: search 16, adapt 1", "# keys (frame x y w h): 2 10 20 30 40"]
    assert text[2:] == ["-", "-", "10 20 30 40", "11 21 30 40", "-", "13 19 30 40", "-"]
    filled = [(10, 20, 30, 40)] * 3 + [(11, 21, 30, 40)] * 2 + [(13, 19, 30, 40)] * 2
    assert ops.read_box_track(path) == filled
    assert ops.track_crop_boxes(ops.read_box_track(path), 0, 7, 100, 180, 64, 64)  # and feeds the crop boxes


# ---- refusals of the C entries: no device ----

def test_the_header_declares_the_tracker():
    names = {"d3f_gray_decimate_u8", "d3f_track_seed_u8", "d3f_track_search_u8", "d3f_track_template_u8"}
    lib = _lib.lib()
    assert names <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES) and all(hasattr(lib, n) for n in names)
    text = _lib.HEADER_PATH.read_text()
    for line in ("#define D3F_TRACK_MAX_SIDE 64", "#define D3F_TRACK_MAX_SEARCH 64", "#define D3F_TRACK_MAX_STRIDE 32",
                 "#define D3F_TRACK_TEMPLATE_SIDE 48", "#define D3F_TRACK_SEARCH 16", "#define D3F_TRACK_ADAPT 1",
                 "#define D3F_TRACK_LOST 16"):
        assert line in text, line
    assert (_lib.TRACK_MAX_SIDE, _lib.TRACK_MAX_SEARCH, _lib.TRACK_MAX_STRIDE) == (64, 64, 32)


F, G, T, P, O = 0x100000, 0x900000, 0x500000, 0x700000, 0x800000  # frames, grey, template, pos, out: never dereferenced


def _refused(lib, rc, word):
    err = lib.d3f_last_error()
    assert rc != 0 and word in err, (rc, err)


def test_gray_decimate_refuses_before_any_device_call():
    lib = _lib.lib()
    call = lib.d3f_gray_decimate_u8
    _refused(lib, call(None, 1, 8, 8, 1, G, None), b"null argument")
    _refused(lib, call(F, 1, 8, 8, 1, None, None), b"null argument")
    for s in (0, 33, -1):
        _refused(lib, call(F, 1, 64, 64, s, G, None), b"stride")
    for B in (-1, 65536):
        _refused(lib, call(F, B, 64, 64, 2, G, None), b"65535")
    for h, w in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        _refused(lib, call(F, 1, h, w, 1, G, None), b"16384")
    assert call(F, 0, 64, 64, 2, G, None) == 0  # B = 0: nothing to do, nothing launched
    assert call(F, 3, 5, 64, 6, G, None) == 0   # gh = 0: nothing to write


def test_track_seed_refuses_before_any_device_call():
    lib = _lib.lib()
    call = lib.d3f_track_seed_u8
    _refused(lib, call(None, 64, 96, 2, 0, 0, 8, 8, T, P, None), b"null argument")
    _refused(lib, call(F, 64, 96, 2, 0, 0, 8, 8, None, P, None), b"null argument")
    _refused(lib, call(F, 64, 96, 2, 0, 0, 8, 8, T, None, None), b"null argument")
    _refused(lib, call(F, 64, 96, 33, 0, 0, 8, 8, T, P, None), b"stride")
    _refused(lib, call(F, 64, 96, 0, 0, 0, 8, 8, T, P, None), b"stride")
    for tw, th in ((3, 8), (8, 3), (65, 8), (8, 65)):
        _refused(lib, call(F, 1000, 1000, 2, 0, 0, tw, th, T, P, None), b"template")
    for tx, ty, tw, th in ((-1, 0, 8, 8), (0, -1, 8, 8), (41, 0, 8, 8), (0, 25, 8, 8), (40, 24, 9, 8), (40, 24, 8, 9)):
        _refused(lib, call(F, 64, 96, 2, tx, ty, tw, th, T, P, None), b"outside the reduced image")
    _refused(lib, call(F, 64, 96, 2, 0, 0, 8, 8, T, P + 2, None), b"aligned")


GOOD_SEARCH = dict(B=2, gh=40, gw=50, tw=13, th=7, search=16, adapt=1, lost=16)


@pytest.mark.parametrize("fused", [False, True], ids=["search", "template"])
def test_track_search_and_template_refuse_before_any_device_call(fused):
    lib = _lib.lib()

    def call(pos=P, out=O, templ=T, src=G, ws=G, **change):
        a = dict(GOOD_SEARCH, **change)
        if fused:  # the frames are 2 x the reduced image, plus one pixel that the reduction drops
            return lib.d3f_track_template_u8(F if src else None, a["B"], a["gh"] * 2 + 1, a["gw"] * 2 + 1, 2, a["tw"], a["th"],
                                             a["search"], a["adapt"], a["lost"], templ, pos, ws, out, None)
        return lib.d3f_track_search_u8(src, a["B"], a["gh"], a["gw"], a["tw"], a["th"], a["search"], a["adapt"], a["lost"],
                                       templ, pos, out, None)

    for null in ("pos", "out", "templ", "src"):
        _refused(lib, call(**{null: None}), b"null argument")
    for B in (-1, 65536):
        _refused(lib, call(B=B), b"65535")
    for tw, th in ((3, 7), (13, 3), (65, 7), (13, 65)):
        _refused(lib, call(tw=tw, th=th), b"template")
    _refused(lib, call(gw=12), b"larger than the reduced image")
    _refused(lib, call(gh=6), b"larger than the reduced image")
    for search in (0, 65, -3):
        _refused(lib, call(search=search), b"search")
    for adapt in (-1, 9):
        _refused(lib, call(adapt=adapt), b"adapt")
    for lost in (-1, 256):
        _refused(lib, call(lost=lost), b"lost")
    _refused(lib, call(pos=P + 1), b"aligned")
    _refused(lib, call(out=O + 2), b"aligned")
    assert call(B=0) == 0  # nothing to do, nothing launched
    if fused:
        _refused(lib, call(ws=None), b"null argument")
        _refused(lib, lib.d3f_track_template_u8(F, 2, 81, 101, 33, 13, 7, 16, 1, 16, T, P, G, O, None), b"stride")
        _refused(lib, lib.d3f_track_template_u8(F, 2, 16385, 101, 2, 13, 7, 16, 1, 16, T, P, G, O, None), b"16384")
    else:
        _refused(lib, call(gh=16385), b"16384")


def test_python_entries_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError
    frames = torch.zeros((2, 40, 60, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        ops.gray_decimate_u8(frames.float(), 2)
    with pytest.raises(ValueError, match="stride"):
        ops.gray_decimate_u8(frames, 33)
    with pytest.raises(D3FError):          # good arguments get as far as the missing device
        ops.gray_decimate_u8(frames, 2)
    with pytest.raises(D3FError):
        ops.TrackState("cpu")
    with pytest.raises(ValueError, match="seeded"):
        ops.track_template_u8(frames, None)
    with pytest.raises(ValueError, match="TrackState"):
        ops.track_seed(None, frames[0], (1, 2, 20, 20))
