"""CPU: the scale search of the template tracker -- its restatement (tests/track_scale_restatement.py) against the plain
tracker's restatement and against the quality it is there for, the way back to the frame, the tool's arguments and the
refusals of the C entries (no device call is made before them)."""
from types import SimpleNamespace

import numpy as np
import pytest

import track_restatement as tr
import track_scale_restatement as ts
from denoising_diffusion_deep_fake_amd import _lib, ops


def test_resample_is_the_identity_at_equal_size():
    rng = np.random.default_rng(0)
    for h, w in ((4, 4), (7, 13), (40, 48), (64, 64)):
        A = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        assert np.array_equal(ts.resample(A, h, w), A)
        assert ts.axis_taps(w, w) == [(i, min(i + 1, w - 1), 0) for i in range(w)]


def test_resample_by_hand():
    # 2 -> 4 samples: centres at -0.25, 0.25, 0.75, 1.25: the ends are clamped, the inner weights are 16/64 and 48/64
    assert ts.axis_taps(2, 4) == [(0, 1, 0), (0, 1, 16), (0, 1, 48), (1, 1, 16)]
    A = np.array([[0, 128]], dtype=np.uint8)
    assert ts.resample(A, 1, 4).tolist() == [[0, 32, 96, 128]]
    # 4 -> 2: each output lies half way between two inputs
    assert ts.axis_taps(4, 2) == [(0, 1, 32), (2, 3, 32)]
    assert ts.resample(np.array([[10, 20, 30, 41]], dtype=np.uint8), 1, 2).tolist() == [[15, 36]]  # 35.5 rounds up
    # a constant stays a constant, and the range is kept
    assert (ts.resample(np.full((9, 5), 255, dtype=np.uint8), 13, 4) == 255).all()


def test_level_sizes_and_their_limits():
    assert ts.level_size(48, 40, 48) == (48, 40) and ts.level_size(40, 48, 48) == (40, 48)
    assert ts.level_size(48, 40, 49) == (49, 41) and ts.level_size(48, 40, 47) == (47, 39)
    assert ts.level_size(48, 40, 64) == (64, 53) and ts.level_size(48, 40, 5) == (5, 4)
    for tw0, th0 in ((48, 40), (13, 9), (64, 48), (4, 4), (20, 24), (5, 64)):
        L0 = max(tw0, th0)
        assert ts.level_size(tw0, th0, L0) == (tw0, th0)
        sizes = [ts.level_size(tw0, th0, L) for L in range(1, 65)]
        assert all(0 <= b[0] - a[0] <= 1 and 0 <= b[1] - a[1] <= 1 for a, b in zip(sizes, sizes[1:]))
        assert all(max(size) == L for L, size in enumerate(sizes, 1))  # one level is one sample on the longer side
    assert ts.level_range(48, 40, 1000, 1000) == (5, 64)       # th(4) = 3 is below 4 samples
    assert ts.level_range(64, 48, 1000, 1000) == (5, 64)       # cannot grow
    assert ts.level_range(4, 4, 1000, 1000) == (4, 64)         # cannot shrink
    assert ts.level_range(5, 64, 1000, 1000) == (45, 64)       # tw(45) = 4, tw(44) = 3
    assert ts.level_range(48, 40, 45, 50) == (5, 50)           # the image is 50 wide
    assert ts.level_range(48, 40, 41, 1000) == (5, 49)         # and 41 high: th(49) = 41
    assert not ts.level_valid(48, 40, 65, 1000, 1000) and not ts.level_valid(48, 40, 0, 1000, 1000)


def test_the_way_back_to_the_frame():
    geo = (7, 128, 57, 29, 43, 4, 1, 200, 300)  # L0 = 43
    rows = [(128, 57, 29, 43, 100, 1, 43, 5), (130, 56, 29, 43, 99999, 0, 43, 9), (0, 0, 29, 43, 0, 1, 43, 0)]
    plain = [(r[0], r[1], r[7], r[5]) for r in rows]
    assert ts.faces(rows, geo, 2000, 3000) == tr.faces(plain, geo) == [(900, 400, 200, 300), None, (4, 1, 200, 300)]
    state = SimpleNamespace(geometry=geo, h=2000, w=3000)
    assert ops.track_scale_faces(rows, state) == ts.faces(rows, geo, 2000, 3000)
    assert ops.track_scale_faces(rows, geo, frame=(2000, 3000)) == ops.track_scale_faces(rows, state)
    # a level up: 30 x 44 samples around the same centre (its corner half a sample further out: one sample, rounded down)
    up = (127, 56, 30, 44, 100, 1, 44, 5)
    fw1, fh1 = (200 * 44 + 21) // 43, (300 * 44 + 21) // 43
    assert (fw1, fh1) == (205, 307)
    x = ((2 * 127 + 30) * 7 + 2 * 4 + 200 - 29 * 7 - 205) // 2
    y = ((2 * 56 + 44) * 7 + 2 * 1 + 300 - 43 * 7 - 307) // 2
    assert ts.face_of_row(up, geo, 2000, 3000) == (x, y, 205, 307) == ops.track_scale_faces([up], state)[0]
    assert abs((2 * x + 205) - (2 * 900 + 200)) <= 7 and abs((2 * y + 307) - (2 * 400 + 300)) <= 7  # the centre: half a sample
    # a box that would leave the frame keeps one pixel inside it
    small = SimpleNamespace(geometry=geo, h=350, w=880)
    out = ops.track_scale_faces([rows[0]], small)[0]
    assert out == (879, 349, 200, 300) == ts.face_of_row(rows[0], geo, 350, 880)
    rng = np.random.default_rng(3)
    for _ in range(50):
        L = int(rng.integers(30, 60))
        tw, th = ts.level_size(29, 43, L)
        row = (int(rng.integers(0, 300)), int(rng.integers(0, 200)), tw, th, 7, 1, L, 9)
        assert ops.track_scale_faces([row], small) == ts.faces([row], geo, 350, 880)


@pytest.mark.parametrize("seed, adapt", [(7, 1), (8, 8), (9, 0)])
def test_levels_0_is_the_plain_search(seed, adapt):
    frames, positions = tr.moving_patch_frames(seed, 8, 96, 160, 2, 3, absent=(4,), patch=(12, 10))
    gray = tr.gray_decimate(frames, 2)
    T, pos = tr.seed(gray[0], positions[0][0], positions[0][1], 10, 12)
    T1, pos1, rows = tr.search(gray[1:], T, pos, 8, adapt, 16)
    for penalty in (0, 512, 65535):
        S1, spos, L, srows = ts.search(gray[1:], T, pos, 12, 8, adapt, 16, levels=0, penalty=penalty)
        assert np.array_equal(S1, T1) and spos == pos1 and L == 12
        assert np.array_equal(srows[:, [0, 1, 7, 5]], rows)
        assert (srows[:, 2] == 10).all() and (srows[:, 3] == 12).all() and (srows[:, 6] == 12).all()
        assert np.array_equal(srows[:, 4], (srows[:, 7].astype(np.int64) << 12) // 120)
    assert rows[:, 3].tolist() == [1, 1, 1, 0, 1, 1, 1]


def _errors(rows, boxes):
    """per frame: twice the centre's error per axis, and the error of both sides, in samples"""
    return np.array([(abs(2 * r[0] + r[2] - 2 * b[0] - b[2]), abs(2 * r[1] + r[3] - 2 * b[1] - b[3]), abs(r[2] - b[2]),
                      abs(r[3] - b[3])) for r, b in zip(rows, boxes)])


@pytest.mark.parametrize("grow", [0.2, -0.2], ids=["grows", "shrinks"])
def test_the_scale_search_follows_a_face_that_changes_size_and_the_fixed_size_does_not(grow):
    """a 48 x 40 patch in 128 x 160, R = 8, motion of at most 3 samples a frame, +-20 % over 12 frames, noise of +-6, seeds
    0..9.  levels=1: found in every frame, the centre and both sides within 1 sample.  levels=0: every seed loses a frame
    or ends at least 3 samples off."""
    for seed in range(10):
        gray, boxes = ts.scaling_patch_frames(seed, 12, 128, 160, 3, grow)
        x, y, pw, ph = boxes[0]
        assert (pw, ph) == (40, 48) and boxes[-1][2:] == ((48, 58) if grow > 0 else (32, 38))
        T0, pos = ts.seed(gray[0], x, y, pw, ph)
        rows = ts.search(gray[1:], T0, pos, 48, 8, 1, 16, levels=1)[3]
        e = _errors(rows, boxes[1:])
        assert rows[:, 5].all() and (e[:, :2] <= 2).all() and (e[:, 2:] <= 1).all(), (seed, e.max(axis=0))
        fixed = ts.search(gray[1:], T0, pos, 48, 8, 1, 16, levels=0)[3]
        e = _errors(fixed, boxes[1:])
        assert not fixed[:, 5].all() or e[-1, :2].max() >= 6 or e[-1, 2:].max() >= 3, (seed, e[-1])


def test_a_lost_frame_changes_nothing_and_the_penalty_holds_the_size_on_flat_content():
    gray, boxes = ts.scaling_patch_frames(4, 6, 96, 120, 2, 0.1, patch=(24, 20), absent=(3,))
    x, y, pw, ph = boxes[0]
    T0, pos = ts.seed(gray[0], x, y, pw, ph)
    T1, pos1, L1, rows = ts.search(gray[1:3], T0, pos, 24, 8, 1, 16)
    T2, pos2, L2, lost = ts.search(gray[3:4], T1, pos1, L1, 8, 1, 16)
    assert lost[0, 5] == 0 and np.array_equal(T2, T1) and pos2 == pos1 and L2 == L1
    assert lost[0, :4].tolist() == rows[-1, :4].tolist() and lost[0, 6] == L1
    assert ts.search(gray[4:], T2, pos2, L2, 8, 1, 16)[3][:, 5].all()
    # a constant image: every candidate of a level costs the same; without a penalty the tie still goes to no change of size
    flat = np.full((3, 40, 50), 77, dtype=np.uint8)
    for penalty in (0, 512):
        for value, ncost in ((77, 0), (78, 4096)):
            T = np.full((9, 13), value, dtype=np.uint8)
            rows = ts.search(flat, T, (11, 9), 13, 16, 1, 255, penalty=penalty)[3]
            assert rows.tolist() == [[11, 9, 13, 9, ncost, 1, 13, ncost * 117 >> 12]] * 3


def test_tool_arguments():
    import d3f.script_tools.track_face_box as tool
    key = ["--key", "0", "10", "20", "30", "40"]
    a = tool.parse_command_line_arguments(["in.mp4"] + key)
    assert a.scale is False and a.scale_penalty == 512 == ops.TRACK_SCALE_PENALTY == _lib.TRACK_SCALE_PENALTY
    a = tool.parse_command_line_arguments(["in.mp4"] + key + ["--scale", "--scale-penalty", "0"])
    assert a.scale is True and a.scale_penalty == 0
    assert tool.parse_command_line_arguments(["in.mp4"] + key + ["--scale-penalty", "65535"]).scale_penalty == 65535
    for bad in (["--scale-penalty", "65536"], ["--scale-penalty", "-1"], ["--scale-penalty", "much"], ["--scale", "1"]):
        with pytest.raises(SystemExit):
            tool.parse_command_line_arguments(["in.mp4"] + key + bad)
    with pytest.raises(ValueError, match="scale-penalty"):
        tool.TrackFaceBox("clip.mp4", [(0, 1, 2, 30, 40)], frames=[], scale=True, scale_penalty=65536)
    with pytest.raises(ValueError, match="scale-penalty"):
        tool.TrackFaceBox("clip.mp4", [(0, 1, 2, 30, 40)], frames=[], scale_penalty=1.5)
    with pytest.raises(ValueError, match="--scale is"):
        tool.TrackFaceBox("clip.mp4", [(0, 1, 2, 30, 40)], frames=[], scale=1)
    assert "#define D3F_TRACK_SCALE_PENALTY 512" in _lib.HEADER_PATH.read_text()


def test_the_header_line_of_the_scale_search(tmp_path):
    """three frames and a key past them: no device needed; --scale adds one header line, without it the header is as before"""
    import d3f.script_tools.track_face_box as tool
    frames = [np.zeros((20, 30, 3), dtype=np.uint8)] * 3
    headers = {}
    for scale in (False, True):
        path = tmp_path / f"t{int(scale)}.txt"
        with pytest.raises(ValueError, match="past"):
            tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames, output_path=path, scale=scale,
                              scale_penalty=300)
        headers[scale] = [line for line in path.read_text().splitlines() if line.startswith("#")]
    assert headers[False] == ["# track_face_box clip.mp4: x y w h per frame, - where the face was not found",
                              "# keys (frame x y w h): 5 1 2 10 10", "# search 16, adapt 1, lost 16, template side 48"]
    assert headers[True] == headers[False] + ["# scale search: one level a frame, penalty 300"]


# ---- refusals of the C entries: no device ----

F, G, T, P, O = 0x100000, 0x900000, 0x500000, 0x700000, 0x800000  # frames, grey, template, pos, out: never dereferenced
GOOD = dict(B=2, gh=40, gw=50, tw=13, th=7, search=16, adapt=1, lost=16, levels=1, penalty=512)


def _refused(lib, rc, word):
    err = lib.d3f_last_error()
    assert rc != 0 and word in err, (rc, err)


@pytest.mark.parametrize("fused", [False, True], ids=["search", "template"])
def test_the_scale_entries_refuse_before_any_device_call(fused):
    names = {"d3f_track_seed_scale_u8", "d3f_track_search_scale_u8", "d3f_track_template_scale_u8"}
    lib = _lib.lib()
    assert names <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES) and all(hasattr(lib, n) for n in names)

    def call(pos=P, out=O, templ=T, src=G, ws=G, **change):
        a = dict(GOOD, **change)
        if fused:
            return lib.d3f_track_template_scale_u8(F if src else None, a["B"], a["gh"] * 2 + 1, a["gw"] * 2 + 1, 2, a["tw"],
                                                   a["th"], a["search"], a["adapt"], a["lost"], a["levels"], a["penalty"],
                                                   templ, pos, ws, out, None)
        return lib.d3f_track_search_scale_u8(src, a["B"], a["gh"], a["gw"], a["tw"], a["th"], a["search"], a["adapt"],
                                             a["lost"], a["levels"], a["penalty"], templ, pos, out, None)

    for null in ("pos", "out", "templ", "src"):
        _refused(lib, call(**{null: None}), b"null argument")
    for levels in (-1, 2):
        _refused(lib, call(levels=levels), b"levels")
    for penalty in (-1, 65536):
        _refused(lib, call(penalty=penalty), b"penalty")
    _refused(lib, call(pos=P + 2), b"aligned")
    _refused(lib, call(out=O + 1), b"aligned")
    for B in (-1, 65536):
        _refused(lib, call(B=B), b"65535")
    for tw, th in ((3, 7), (13, 3), (65, 7), (13, 65)):
        _refused(lib, call(tw=tw, th=th), b"template")
    _refused(lib, call(gw=12), b"larger than the reduced image")
    for search in (0, 65):
        _refused(lib, call(search=search), b"search")
    for adapt in (-1, 9):
        _refused(lib, call(adapt=adapt), b"adapt")
    for lost in (-1, 256):
        _refused(lib, call(lost=lost), b"lost")
    assert call(B=0) == 0  # nothing to do, nothing launched
    if fused:
        _refused(lib, call(ws=None), b"null argument")
    seed = lib.d3f_track_seed_scale_u8
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, T, None, None), b"null argument")
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, T, P + 2, None), b"aligned")
    _refused(lib, seed(F, 64, 96, 2, 40, 24, 9, 8, T, P, None), b"outside the reduced image")
