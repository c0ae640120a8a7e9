"""CPU: the template tracker's re-acquisition without a device -- the restatement (tests/track_reacq_restatement.py) on the
recipe of the teleporting patch, ten seeds, against the plain restatement on the same input; hand-made whole-frame
searches (ties, a constant image); the tool's arguments; and the refusals of the three C entries (everything is refused
before a device call: the dummy pointers are never dereferenced)."""
import numpy as np
import pytest
import torch

import track_reacq_restatement as rr
import track_restatement as tr
from denoising_diffusion_deep_fake_amd import _lib, ops

SEEDS = range(10)


@pytest.fixture(scope="module")
def recipe():
    """seed -> (gray [24, 72, 100], positions, K, the whole-frame keys of frames 1..23): computed once, never changed"""
    out = {}
    for seed in SEEDS:
        frames, positions = rr.teleporting_patch_frames(seed)
        gray = tr.gray_decimate(frames, 1)
        K, pos = tr.seed(gray[0], positions[0][0], positions[0][1], rr.PATCH[1], rr.PATCH[0])
        out[seed] = (gray, positions, K, rr.global_keys(gray[1:], K))
    return out


# ---- the recipe ----

def test_the_recipe_jumps_out_of_reach_and_hides_the_patch():
    frames, positions = rr.teleporting_patch_frames(3)
    assert frames.shape == (rr.FRAMES, rr.H, rr.W, 3) and frames.dtype == np.uint8
    shown = positions[0]
    for k in range(1, rr.FRAMES):
        dx, dy = positions[k][0] - shown[0], positions[k][1] - shown[1]
        if k in rr.JUMPS:
            assert max(abs(dx), abs(dy)) > 2 * rr.SEARCH, (k, dx, dy)
        elif k not in rr.ABSENT and k - 1 not in rr.ABSENT:
            assert max(abs(dx), abs(dy)) <= 2, (k, dx, dy)
        if k not in rr.ABSENT:
            shown = positions[k]
        assert 0 <= positions[k][0] <= rr.W - rr.PATCH[1] and 0 <= positions[k][1] <= rr.H - rr.PATCH[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_restatement_finds_every_frame_that_holds_the_patch(recipe, seed):
    """search 8, adapt 1, lost 16, relost 8 on 24 frames: the 20 tracked frames that hold the patch are found at the
    recipe's position, exactly the three jump frames of them re-acquired, and exactly the three absent frames lost.  The
    key template costs 2.4 .. 2.9 grey levels a sample where the patch is (two draws of noise in -6..6 on three bytes, through
    (B + 2 G + R) / 4: a mean absolute difference of about 2.6, so 4 a sample is far out over 480 samples) and 30.8 .. 33.0 at
    the best place of a frame without it (unrelated texture: the grey of uniform bytes in 40..215 has a standard deviation
    of 31, two of them differ by about 35 on average, and the smallest of 3969 means over 480 samples lies a few levels under
    that -- above 24 by a wide margin): relost = 8 and lost = 16 both lie between the two with room to spare."""
    gray, positions, K, keys = recipe[seed]
    n = K.size
    T1, pos1, rows = rr.search_reacq(gray[1:], K.copy(), K, positions[0], rr.SEARCH, rr.ADAPT, rr.LOST, rr.RELOST, keys)
    held = positions[0]
    for k, row in enumerate(rows.tolist(), 1):
        if k in rr.ABSENT:
            assert row[3] == 0 and tuple(row[:2]) == held and row[2] > rr.LOST * n, (k, row)
            assert rr.decode(keys[k - 1])[0] > 24 * n, (k, rr.decode(keys[k - 1]))
        else:
            assert row[3] == (2 if k in rr.JUMPS else 1) and tuple(row[:2]) == positions[k], (k, row, positions[k])
            assert row[2] <= 4 * n, (k, row)
            held = positions[k]
    assert pos1 == positions[-1]
    assert [k for k, row in enumerate(rows.tolist(), 1) if row[3] == 0] == list(rr.ABSENT)
    assert [k for k, row in enumerate(rows.tolist(), 1) if row[3] == 2] == list(rr.JUMPS)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_plain_restatement_finds_at_most_half_of_the_same_frames(recipe, seed):
    """without re-acquisition the first jump is the end: the five frames before it are found, and more only where a later
    jump happens to land within the window of the place the tracker stayed at"""
    gray, positions, K, _ = recipe[seed]
    rows = tr.search(gray[1:], K.copy(), positions[0], rr.SEARCH, rr.ADAPT, rr.LOST)[2]
    assert rows[:5, 3].all() and not rows[5, 3]
    assert int(rows[:, 3].sum()) <= (rr.FRAMES - 1) // 2


def test_without_a_jump_or_an_absent_frame_the_rows_are_the_plain_rows():
    frames, positions = rr.teleporting_patch_frames(11, jumps=(), absent=())
    gray = tr.gray_decimate(frames, 1)
    K, pos = tr.seed(gray[0], positions[0][0], positions[0][1], rr.PATCH[1], rr.PATCH[0])
    want = tr.search(gray[1:], K.copy(), pos, rr.SEARCH, rr.ADAPT, rr.LOST)
    got = rr.search_reacq(gray[1:], K.copy(), K, pos, rr.SEARCH, rr.ADAPT, rr.LOST, rr.RELOST)
    assert np.array_equal(got[2], want[2]) and got[1] == want[1] and np.array_equal(got[0], want[0])
    assert want[2][:, 3].all()


def test_relost_0_re_acquires_only_an_exact_copy():
    frames, positions = rr.teleporting_patch_frames(5)
    gray = tr.gray_decimate(frames, 1)
    K, pos = tr.seed(gray[0], positions[0][0], positions[0][1], rr.PATCH[1], rr.PATCH[0])
    want = tr.search(gray[1:], K.copy(), pos, rr.SEARCH, rr.ADAPT, rr.LOST)
    got = rr.search_reacq(gray[1:], K.copy(), K, pos, rr.SEARCH, rr.ADAPT, rr.LOST, 0)
    assert np.array_equal(got[2], want[2]) and 2 not in got[2][:, 3]
    # frame 0 itself, the key frame, behind a lost frame: cost 0 at the key's place, found 2, and the template is K again
    T, p, row = rr.search_reacq_frame(gray[0], K // 2, K, (0, 0), rr.global_key(gray[0], K), 4, 1, 0, 0)
    assert row == (positions[0][0], positions[0][1], 0, 2) and p == positions[0] and np.array_equal(T, K)


# ---- the whole-frame search by hand ----

def test_the_global_key_by_hand():
    K = np.array([[10, 20, 30, 40, 50]] * 4, dtype=np.uint8)
    G = np.full((9, 12), 100, dtype=np.uint8)
    # a constant image: every position costs the same, the key is (cost, 0, 0)
    assert rr.global_key(G, K) == (4 * (90 + 80 + 70 + 60 + 50)) << 32
    # two exact copies, the upper one further right: the top-most wins; in one row: the left-most
    G[4:8, 1:6] = K
    G[2:6, 7:12] = K
    assert rr.decode(rr.global_key(G, K)) == (0, 7, 2)
    G[:] = 100
    G[3:7, 6:11] = K
    G[3:7, 0:5] = K
    assert rr.decode(rr.global_key(G, K)) == (0, 0, 3)
    # the image is the template: one candidate
    assert rr.global_key(K + 1, K) == 20 << 32
    assert rr.global_keys(np.stack([G, G + 1]), K) == [3 << 16, 20 << 32 | 3 << 16]


# ---- ops and the tool ----

def test_track_faces_takes_a_re_acquired_row_as_found():
    geometry = (7, 128, 57, 29, 43, 4, 1, 200, 300)
    rows = [(128, 57, 100, 1), (130, 56, 99999, 0), (0, 0, 0, 2), (3, 2, 50, 2)]
    assert ops.track_faces(rows, geometry) == [(900, 400, 200, 300), None, (4, 1, 200, 300), (25, 15, 200, 300)]
    assert ops.TRACK_RELOST == _lib.TRACK_RELOST == rr.RELOST == 8 and 2 * ops.TRACK_RELOST == ops.TRACK_LOST


def test_tool_arguments():
    import d3f.script_tools.track_face_box as tool
    key = ["in.mp4", "--key", "0", "10", "20", "30", "40"]
    assert tool.parse_command_line_arguments(key).reacquire is None
    assert tool.parse_command_line_arguments(key + ["--reacquire"]).reacquire == 8
    assert tool.parse_command_line_arguments(key + ["--reacquire", "12"]).reacquire == 12
    assert tool.parse_command_line_arguments(key + ["--reacquire", "0"]).reacquire == 0
    for bad in (["--reacquire", "256"], ["--reacquire", "-1"], ["--reacquire", "some"], ["--reacquire", "--scale"],
                ["--scale", "--reacquire", "8"], ["--reacquire", "--rotate"]):
        with pytest.raises(SystemExit):
            tool.parse_command_line_arguments(key + bad)
    keys = [(0, 1, 2, 30, 40)]
    with pytest.raises(ValueError, match="--reacquire with --scale.*keeps a level.*cannot restore"):
        tool.TrackFaceBox("clip.mp4", keys, frames=[], scale=True, reacquire=8)
    with pytest.raises(ValueError, match="--reacquire with --rotate.*keeps an angle.*cannot restore"):
        tool.TrackFaceBox("clip.mp4", keys, frames=[], rotate=True, reacquire=8)
    for bad in (256, -1, 1.5, True):
        with pytest.raises(ValueError, match="--reacquire is an integer in 0..255"):
            tool.TrackFaceBox("clip.mp4", keys, frames=[], reacquire=bad)


def test_the_tool_without_frames_to_follow_needs_no_device(tmp_path):
    """three frames, the only key at frame 5: the file is written with the setting in its header, the counts say lost"""
    import d3f.script_tools.track_face_box as tool
    frames = [np.zeros((20, 30, 3), dtype=np.uint8)] * 3
    path = tmp_path / "t.txt"
    with pytest.raises(ValueError, match="frame 5 is past"):
        tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames, output_path=path, reacquire=8)
    lines = path.read_text().splitlines()
    assert any("re-acquisition" in line and "at most 8 a sample" in line for line in lines if line.startswith("#"))
    assert [line for line in lines if not line.startswith("#")] == ["-"] * 3
    # without the flag the header is what it was
    with pytest.raises(ValueError, match="past"):
        tool.TrackFaceBox(tmp_path / "clip.mp4", [(5, 1, 2, 10, 10)], frames=frames, output_path=path)
    assert "re-acquisition" not in path.read_text()


def test_python_entries_argument_errors_need_no_device():
    frames = torch.zeros((2, 40, 60, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="seeded"):
        ops.track_template_reacq_u8(frames, None)
    with pytest.raises(ValueError, match="uint8 grey image"):
        ops.track_global_u8(frames, torch.zeros(64, dtype=torch.uint8), 8, 8)


# ---- refusals of the C entries: no device ----

def test_the_header_declares_the_entries():
    names = {"d3f_track_global_u8", "d3f_track_search_reacq_u8", "d3f_track_template_reacq_u8"}
    lib = _lib.lib()
    assert names <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES) and all(hasattr(lib, n) for n in names)
    assert "#define D3F_TRACK_RELOST 8" in _lib.HEADER_PATH.read_text()


F, G, T, K, P, O, KEYS = 0x100000, 0x900000, 0x500000, 0x600000, 0x700000, 0x800000, 0xA00000  # never dereferenced


def _refused(lib, rc, word):
    err = lib.d3f_last_error()
    assert rc != 0 and word in err, (rc, err)


GOOD = dict(B=2, gh=40, gw=50, tw=13, th=7, search=16, adapt=1, lost=16, relost=8)


def test_track_global_refuses_before_any_device_call():
    lib = _lib.lib()

    def call(src=G, key_templ=K, keys=KEYS, **change):
        a = dict(GOOD, **change)
        return lib.d3f_track_global_u8(src, a["B"], a["gh"], a["gw"], a["tw"], a["th"], key_templ, keys, None)

    for null in ("src", "key_templ", "keys"):
        _refused(lib, call(**{null: None}), b"null argument")
    for B in (-1, 65536):
        _refused(lib, call(B=B), b"65535")
    for gh, gw in ((0, 50), (40, 0), (16385, 50), (40, 16385)):
        _refused(lib, call(gh=gh, gw=gw), b"16384")
    for tw, th in ((3, 7), (13, 3), (65, 7), (13, 65)):
        _refused(lib, call(tw=tw, th=th), b"template")
    _refused(lib, call(gw=12), b"larger than the reduced image")
    _refused(lib, call(gh=6), b"larger than the reduced image")
    for off in (1, 2, 4):
        _refused(lib, call(keys=KEYS + off), b"aligned to 8")
    assert call(B=0) == 0  # nothing to do, nothing launched


@pytest.mark.parametrize("fused", [False, True], ids=["search_reacq", "template_reacq"])
def test_track_search_reacq_and_template_reacq_refuse_before_any_device_call(fused):
    lib = _lib.lib()

    def call(pos=P, out=O, templ=T, key_templ=K, keys=KEYS, src=G, ws=G, **change):
        a = dict(GOOD, **change)
        if fused:  # the frames are 2 x the reduced image, plus one pixel that the reduction drops
            return lib.d3f_track_template_reacq_u8(F if src else None, a["B"], a["gh"] * 2 + 1, a["gw"] * 2 + 1, 2, a["tw"],
                                                   a["th"], a["search"], a["adapt"], a["lost"], a["relost"], templ, key_templ,
                                                   pos, ws, keys, out, None)
        return lib.d3f_track_search_reacq_u8(src, a["B"], a["gh"], a["gw"], a["tw"], a["th"], a["search"], a["adapt"],
                                             a["lost"], a["relost"], templ, key_templ, pos, keys, out, None)

    # what d3f_track_search_u8 refuses
    for null in ("pos", "out", "templ", "src", "key_templ", "keys"):
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
    # and what is new
    for relost in (-1, 256):
        _refused(lib, call(relost=relost), b"relost")
    for off in (1, 4, 7):
        _refused(lib, call(keys=KEYS + off), b"aligned to 8")
    for key_templ in (T, T + 1, T + 90, T - 90):  # 13 x 7 = 91 bytes each
        _refused(lib, call(key_templ=key_templ), b"overlaps")
    assert call(B=0) == 0                    # nothing to do, nothing launched
    assert call(B=0, key_templ=T + 91) == 0  # back to back is no overlap
    assert call(B=0, key_templ=T - 91) == 0
    if fused:
        _refused(lib, call(ws=None), b"null argument")
        _refused(lib, lib.d3f_track_template_reacq_u8(F, 2, 81, 101, 33, 13, 7, 16, 1, 16, 8, T, K, P, G, KEYS, O, None), b"stride")
        _refused(lib, lib.d3f_track_template_reacq_u8(F, 2, 16385, 101, 2, 13, 7, 16, 1, 16, 8, T, K, P, G, KEYS, O, None), b"16384")
    else:
        _refused(lib, call(gh=16385), b"16384")
