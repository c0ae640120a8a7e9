"""CPU: the rotation search of the template tracker -- its restatement (tests/track_rot_restatement.py) against the quality it
is there for and against the plain tracker's restatement, the disc and the rotation, the table, the way back to the frame,
the tool's arguments and files, and the refusals of the C entries (no device call is made before them)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import track_restatement as tr
import track_rot_restatement as trr
from denoising_diffusion_deep_fake_amd import _lib, ops

SIZES = ((4, 4), (13, 9), (9, 13), (20, 24), (30, 31), (31, 30), (48, 40), (64, 48), (48, 64), (64, 64), (5, 64))


def test_the_rows_of_the_disc_are_contiguous_spans_inside_the_box():
    for tw0, th0 in SIZES:
        spans = trr.disc_spans(tw0, th0)  # (asserts that every row is one run)
        mask = trr.disc_mask(tw0, th0)
        D = min(tw0, th0)
        assert len(spans) == th0 and all(lo + n <= tw0 and (n == 0 or n == tw0 - 2 * lo) for lo, n in spans)
        assert np.array_equal(mask, mask[::-1, ::-1]) and np.array_equal(mask, mask[:, ::-1])
        # the disc of diameter D: its area to within its rim, and no sample further than D / 2 from the centre
        assert abs(int(mask.sum()) - np.pi * D * D / 4) <= 2 * D and mask.sum() >= 12
        j, i = np.nonzero(mask)
        assert ((2 * i + 1 - tw0) ** 2 + (2 * j + 1 - th0) ** 2).max() <= D * D
    assert trr.disc_spans(4, 4) == [(1, 2), (0, 4), (0, 4), (1, 2)]
    assert trr.disc_spans(5, 64)[:29] == [(0, 0)] * 29 and trr.disc_spans(5, 64)[31] == (0, 5)


def test_rot_at_angle_0_is_the_identity_on_the_disc():
    rng = np.random.default_rng(0)
    assert trr.table()[1][0] == (65536, 0) and ops.box_rotation(0.0) == (65536, 0)
    for tw0, th0 in SIZES:
        A = rng.integers(0, 256, size=(th0, tw0), dtype=np.uint8)
        assert np.array_equal(trr.rot(A, 65536, 0), np.where(trr.disc_mask(tw0, th0), A, 0))
        assert (trr.rot(np.full((th0, tw0), 255, dtype=np.uint8), 46341, -46341)[trr.disc_mask(tw0, th0)] == 255).all()


def test_rot_turns_clockwise_on_the_screen_and_the_inverse_turns_back():
    # a bright spot to the right of the centre: turned by +90 degrees (x right, y down: clockwise) it lies below the centre
    A = np.zeros((41, 41), dtype=np.uint8)
    A[20, 30] = 255
    c, s = ops.box_rotation(90.0)
    assert (c, s) == (0, 65536)
    T = trr.rot(A, c, s)
    assert T[30, 20] == 255 and T.sum() == 255
    assert np.array_equal(trr.rot(T, c, -s), A)
    # a smooth texture survives a turn and its inverse to within a few levels on the inner disc
    face = np.rint(trr._smooth(np.random.default_rng(1), 40, 48, 8)).astype(np.uint8)
    amax, tab = trr.table()
    assert amax == 30 and len(tab) == 61
    for a in (-30, -7, 1, 13):
        c, s = tab[a]
        back = trr.rot(trr.rot(face, c, s), c, -s).astype(int)
        inner = trr.disc_mask(34, 34)
        err = np.abs(back - face)[3:37, 7:41][inner]
        assert err.max() <= 12 and err.mean() <= 2, (a, err.max(), err.mean())


def test_the_table_is_box_rotation_of_every_index():
    for step, reach in ((200, 60), (100, 60), (150, 45), (200, 0), (281, 180), (300, 61.5)):
        amax, tab = trr.table(step, reach)
        got = ops.track_rot_table(step, reach)
        assert got == [tab[a] for a in range(-amax, amax + 1)] and len(got) == 2 * amax + 1
        assert all(abs(c) <= 65536 and abs(s) <= 65536 for c, s in got)
    assert len(ops.track_rot_table()) == 61 and ops.track_rot_table()[31] == ops.box_rotation(2.0)
    assert (ops.TRACK_ROT_STEP, ops.TRACK_ROT_MAX, ops.TRACK_ROT_PENALTY) == (trr.STEP, trr.MAX_DEGREES, trr.PENALTY)
    assert _lib.TRACK_ROT_MAX_INDEX == trr.MAX_INDEX == 64
    header = _lib.HEADER_PATH.read_text()
    for line in ("#define D3F_TRACK_ROT_MAX_INDEX 64", "#define D3F_TRACK_ROT_STEP 200", "#define D3F_TRACK_ROT_MAX 60",
                 "#define D3F_TRACK_ROT_PENALTY 512"):
        assert line in header
    for step, reach in ((0, 60), (-200, 60), (2.0, 60), (True, 60), (200, -1), (200, 181), (200, float("nan")), (200, "wide"),
                        (90, 60), (200, 130)):  # the last two: 66 and 65 indices
        with pytest.raises(ValueError, match="track_rot_table"):
            ops.track_rot_table(step, reach)
    assert len(ops.track_rot_table(200, 128)) == 129


def _track_errors(rows, boxes, step=trr.STEP):
    """(every frame found, the worst angle error in degrees, the worst error of the corner per axis in samples)"""
    angle = max(abs(int(r[6]) * step / 100.0 - b[4]) for r, b in zip(rows, boxes))
    corner = max(max(abs(int(r[0]) - b[0]), abs(int(r[1]) - b[1])) for r, b in zip(rows, boxes))
    return bool(rows[:, 5].all()), angle, corner


def test_the_rotation_search_follows_a_rolling_face_and_the_plain_search_does_not():
    """a 48 x 40 patch in 128 x 160 that rolls 1.5 degrees a frame over 12 frames and moves up to 2 samples per axis and
    frame, noise of +-6, R = 8, adapt 1, lost 16, seeds 0..9.  The rotation search: found in every frame, the angle within
    one step (2.00 degrees) and the box within one sample in every frame (measured: 1.0 degree and 0 samples).  The plain
    search on the same frames loses frames or ends more than 2 samples off (measured: 30 of the 110 frames lost, 8 of the
    ten seeds lose one; the other two stay within 2 samples)."""
    lost_frames = off = 0
    for seed in range(10):
        gray, boxes = trr.rolling_patch_frames(seed, 12, 128, 160, 2, 1.5)
        x, y, pw, ph, _ = boxes[0]
        assert (pw, ph) == (40, 48) and boxes[-1][4] == 16.5
        T0, pos, a = trr.seed_rot(gray[0], x, y, pw, ph)
        assert a == 0 and np.array_equal(T0, gray[0][y:y + ph, x:x + pw])
        rows = trr.search(gray[1:], T0, pos, a, 8, 1, 16)[3]
        found, angle, corner = _track_errors(rows, boxes[1:])
        assert found and angle <= 2.0 and corner <= 1, (seed, found, angle, corner)
        plain = tr.search(gray[1:], T0, pos, 8, 1, 16)[2]
        lost_frames += int((plain[:, 3] == 0).sum())
        off += max(abs(int(plain[-1, 0]) - boxes[-1][0]), abs(int(plain[-1, 1]) - boxes[-1][1])) > 2
    assert lost_frames >= 1 or off >= 1, (lost_frames, off)


def test_a_lost_frame_changes_nothing_a_constant_image_moves_nothing_and_the_angle_stops_at_the_table():
    gray, boxes = trr.rolling_patch_frames(4, 6, 96, 120, 2, 2.0, patch=(24, 20), absent=(3,))
    x, y, pw, ph, _ = boxes[0]
    T0, pos, a = trr.seed_rot(gray[0], x, y, pw, ph)
    T1, pos1, a1, rows = trr.search(gray[1:3], T0, pos, a, 8, 1, 16)
    T2, pos2, a2, lost = trr.search(gray[3:4], T1, pos1, a1, 8, 1, 16)
    assert lost[0, 5] == 0 and np.array_equal(T2, T1) and pos2 == pos1 and a2 == a1
    assert lost[0, :4].tolist() == rows[-1, :4].tolist() and lost[0, 6] == a1
    assert trr.search(gray[4:], T2, pos2, a2, 8, 1, 16)[3][:, 5].all()
    # the samples outside the disc are never blended
    outside = ~trr.disc_mask(pw, ph)
    assert np.array_equal(T1[outside], T0[outside]) and not np.array_equal(T1, T0)
    # a constant image: every candidate costs the same; the tie goes to no turn and no move, with and without a penalty
    flat = np.full((3, 40, 50), 77, dtype=np.uint8)
    n = int(trr.disc_mask(13, 9).sum())
    for penalty in (0, 512):
        for value, ncost in ((77, 0), (78, 4096)):
            T = np.full((9, 13), value, dtype=np.uint8)
            rows = trr.search(flat, T, (11, 9), 3, 16, 1, 255, penalty=penalty)[3]
            assert rows.tolist() == [[11, 9, 13, 9, ncost, 1, 3, ncost * n >> 12]] * 3
    # a table of +-2 steps: the angle follows a roll of 2 degrees a frame up to index 2 and stays there
    gray, boxes = trr.rolling_patch_frames(3, 6, 96, 120, 0, 2.0, patch=(40, 40))
    x, y, pw, ph, _ = boxes[0]
    T0, pos, a = trr.seed_rot(gray[0], x, y, pw, ph)
    rows = trr.search(gray[1:], T0, pos, a, 4, 1, 255, max_degrees=4)[3]
    assert rows[:, 6].tolist() == [1, 2, 2, 2, 2]
    assert trr.clamp_state((-3, 500), 9, 96, 120, 40, 40, max_degrees=4) == ((0, 56), 2)


def test_the_seed_with_an_angle():
    gray, boxes = trr.rolling_patch_frames(2, 1, 96, 120, 0, 0.0, patch=(40, 48), start=7.0)
    x, y, pw, ph, _ = boxes[0]
    plain, pos = tr.seed(gray[0], x, y, pw, ph)
    for angle, a0 in ((None, 0), (0, 0), (99, 0), (100, 1), (-100, -1), (700, 4), (-299, -1), (-300, -2), (12000, 60)):
        T0, p, a = trr.seed_rot(gray[0], x, y, pw, ph, angle, max_degrees=120)
        assert a == a0 and p == pos
        assert np.array_equal(T0, plain) == (a0 == 0)
        assert np.array_equal(T0[~trr.disc_mask(pw, ph)], plain[~trr.disc_mask(pw, ph)])
    with pytest.raises(ValueError):
        trr.seed_rot(gray[0], x, y, pw, ph, 6100)
    # turned back by the patch's angle the template is the upright patch: closer to it than the unturned grey is
    upright = trr.rolling_patch_frames(2, 1, 96, 120, 0, 0.0, patch=(40, 48), noise=0)[0][0][y:y + ph, x:x + pw]
    mask = trr.disc_mask(pw, ph)
    turned = trr.seed_rot(gray[0], x, y, pw, ph, 700)[0]
    assert np.abs(turned.astype(int) - upright)[mask].mean() < 0.6 * np.abs(plain.astype(int) - upright)[mask].mean()


def test_the_way_back_to_the_frame():
    geo = (7, 128, 57, 29, 43, 4, 1, 200, 300)
    rows = [(128, 57, 29, 43, 100, 1, 5, 9), (130, 56, 29, 43, 99999, 0, 5, 9), (0, 0, 29, 43, 0, 1, -30, 0)]
    want = [(900, 400, 200, 300, 1000), None, (4, 1, 200, 300, -6000)]
    assert trr.faces(rows, geo) == want == ops.track_rot_faces(rows, geo) == ops.track_rot_faces(rows, geo, 200)
    assert ops.track_rot_faces(rows, SimpleNamespace(geometry=geo), 150) == trr.faces(rows, geo, 150)
    assert ops.track_rot_faces(rows, geo, 150)[2] == (4, 1, 200, 300, -4500)
    plain = [(r[0], r[1], r[7], r[5]) for r in rows]
    assert [f and f[:4] for f in want] == ops.track_faces(plain, geo)  # the box is the plain tracker's


def test_tool_arguments():
    import d3f.script_tools.track_face_box as tool
    key = ["--key", "0", "10", "20", "30", "40"]
    a = tool.parse_command_line_arguments(["in.mp4"] + key)
    assert a.rotate is False and (a.rotate_step, a.rotate_max, a.rotate_penalty) == (200, 60, 512)
    a = tool.parse_command_line_arguments(["in.mp4"] + key + ["--rotate", "--rotate-step", "150", "--rotate-max", "45",
                                                               "--rotate-penalty", "0", "--key-angle", "0", "-7.5"])
    assert a.rotate is True and (a.rotate_step, a.rotate_max, a.rotate_penalty) == (150, 45, 0) and a.key_angle == [["0", "-7.5"]]
    for bad in (["--rotate", "--scale"], ["--rotate", "1"], ["--rotate-penalty", "65536"], ["--rotate-penalty", "-1"],
                ["--rotate-step", "0"], ["--rotate-step", "2.0"], ["--rotate-max", "181"], ["--rotate-max", "-1"],
                ["--rotate", "--rotate-step", "50"],                  # 120 steps: above 64 indices
                ["--rotate", "--key-angle", "3", "10"],               # frame 3 has no --key
                ["--rotate", "--key-angle", "0", "61"]):              # beyond --rotate-max
        with pytest.raises(SystemExit):
            tool.parse_command_line_arguments(["in.mp4"] + key + bad)
    # without --rotate a key angle needs no key, a step too fine for the table is no error, and --scale stands alone
    a = tool.parse_command_line_arguments(["in.mp4"] + key + ["--key-angle", "3", "10", "--rotate-step", "50", "--scale"])
    assert a.rotate is False and a.scale is True
    box = [(0, 1, 2, 30, 40)]
    with pytest.raises(ValueError, match="--rotate with --scale"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate=True, scale=True)
    with pytest.raises(ValueError, match="frame 3 has no --key"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate=True, key_angles=[(3, 10.0)])
    with pytest.raises(ValueError, match="beyond --rotate-max"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate=True, key_angles=[(0, -61.0)])
    with pytest.raises(ValueError, match="--rotate is"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate=1)
    with pytest.raises(ValueError, match="rotate-penalty"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate=True, rotate_penalty=65536)
    with pytest.raises(ValueError, match="rotate-step"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate_step=2.0)
    with pytest.raises(ValueError, match="--rotate-step 50 with --rotate-max 60"):
        tool.TrackFaceBox("clip.mp4", box, frames=[], rotate=True, rotate_step=50)


def test_the_header_line_of_the_rotation_search_and_the_file_without_it(tmp_path):
    """three frames and a key past them: no device needed.  --rotate adds one header line (one more with key angles);
    without it the header, and the file --key-angle writes by interpolation, are what they were"""
    import d3f.script_tools.track_face_box as tool
    frames = [np.zeros((20, 30, 3), dtype=np.uint8)] * 3
    head = ["# track_face_box clip.mp4: x y w h per frame, - where the face was not found",
            "# keys (frame x y w h): 5 1 2 10 10", "# search 16, adapt 1, lost 16, template side 48"]
    texts = {}
    for name, more in (("plain", dict(rotate=False)), ("angles", dict(rotate=False, key_angles=[(0, 10.0), (2, -3.5)])),
                       ("rotate", dict(rotate=True, rotate_penalty=300)),
                       ("both", dict(rotate=True, rotate_step=150, rotate_max=45, key_angles=[(5, 10.0)]))):
        path = tmp_path / f"{name}.txt"
        with pytest.raises(ValueError, match="past"):
            tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames, output_path=path, **more)
        texts[name] = path.read_text().splitlines()
    assert texts["plain"] == head + ["-"] * 3
    assert texts["angles"] == head + ["# fifth column: the box's angle in degrees, interpolated between the key angles (frame "
                                      "angle): 0 10.00, 2 -3.50"] + ["-"] * 3
    assert texts["rotate"] == head + ["# rotation search: one step of 2.00 degrees a frame within +-60, penalty 300; fifth "
                                      "column: the box's angle in degrees"] + ["-"] * 3
    assert texts["both"] == head + ["# rotation search: one step of 1.50 degrees a frame within +-45, penalty 512; fifth "
                                    "column: the box's angle in degrees", "# key angles (frame angle): 5 10.00"] + ["-"] * 3
    # the interpolated column itself, as write_track has written it all along
    angles = tool.interpolate_key_angles(tool.sorted_key_angles([(0, 10.0), (2, -3.5)]), 4)
    assert angles == [1000, 325, -350, -350]
    path = tmp_path / "column.txt"
    tool.write_track(path, [(1, 2, 3, 4), None, (5, 6, 7, 8), (9, 10, 11, 12)], ("h",), angles)
    assert path.read_text() == "# h\n1 2 3 4 10.00\n-\n5 6 7 8 -3.50\n9 10 11 12 -3.50\n"
    assert ops.read_rbox_track(path)[0] == (1, 2, 3, 4, 10.0)


# ---- refusals of the C entries: no device ----

F, G, T, P, O = 0x100000, 0x900000, 0x500000, 0x700000, 0x800000  # frames, grey, template, pos, out: never dereferenced
GOOD = dict(B=2, gh=40, gw=50, tw=13, th=7, search=16, adapt=1, lost=16, steps=1, penalty=512, amax=30)


def _refused(lib, rc, word):
    err = lib.d3f_last_error()
    assert rc != 0 and word in err, (rc, err)


def _table(amax, **change):
    flat = [v for pair in ops.track_rot_table(200, 2 * amax) for v in pair]
    for at, value in change.items():
        flat[int(at[1:])] = value
    return (C.c_int32 * len(flat))(*flat)


@pytest.mark.parametrize("fused", [False, True], ids=["search", "template"])
def test_the_rot_entries_refuse_before_any_device_call(fused):
    names = {"d3f_track_seed_rot_u8", "d3f_track_search_rot_u8", "d3f_track_template_rot_u8"}
    lib = _lib.lib()
    assert names <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES) and all(hasattr(lib, n) for n in names)

    def call(pos=P, out=O, templ=T, src=G, ws=G, table=True, entries=None, **change):
        a = dict(GOOD, **change)
        tab = _table(min(max(a["amax"], 0), 64), **(entries or {})) if table else None
        if fused:
            return lib.d3f_track_template_rot_u8(F if src else None, a["B"], a["gh"] * 2 + 1, a["gw"] * 2 + 1, 2, a["tw"],
                                                 a["th"], a["search"], a["adapt"], a["lost"], a["steps"], a["penalty"],
                                                 a["amax"], tab, templ, pos, ws, out, None)
        return lib.d3f_track_search_rot_u8(src, a["B"], a["gh"], a["gw"], a["tw"], a["th"], a["search"], a["adapt"], a["lost"],
                                           a["steps"], a["penalty"], a["amax"], tab, templ, pos, out, None)

    for null in ("pos", "out", "templ", "src"):
        _refused(lib, call(**{null: None}), b"null argument")
    _refused(lib, call(table=False), b"null table")
    for steps in (-1, 2):
        _refused(lib, call(steps=steps), b"steps")
    for penalty in (-1, 65536):
        _refused(lib, call(penalty=penalty), b"penalty")
    for amax in (-1, 65):
        _refused(lib, call(amax=amax), b"amax")
    for entries in ({"e0": 65537}, {"e121": -65537}, {"e60": 1 << 30}):
        _refused(lib, call(entries=entries), b"table entry")
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
    assert call(B=0) == 0 and call(B=0, amax=0) == 0 and call(B=0, amax=64) == 0  # nothing to do, nothing launched
    if fused:
        _refused(lib, call(ws=None), b"null argument")
    seed = lib.d3f_track_seed_rot_u8
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, 0, 65536, 0, T, None, None), b"null argument")
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, 0, 65536, 0, T, P + 2, None), b"aligned")
    _refused(lib, seed(F, 64, 96, 2, 40, 24, 9, 8, 0, 65536, 0, T, P, None), b"outside the reduced image")
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, 65, 65536, 0, T, P, None), b"angle index")
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, -65, 65536, 0, T, P, None), b"angle index")
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, 1, 65537, 0, T, P, None), b"rot")
    _refused(lib, seed(F, 64, 96, 2, 0, 0, 8, 8, 1, 0, -65537, T, P, None), b"rot")
