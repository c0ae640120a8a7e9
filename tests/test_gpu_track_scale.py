"""GPU: the scale search of the template tracker against its restatement (tests/track_scale_restatement.py) -- the search on
grey input, the fused entry, the Python entries and the tool with scale=True.  Everything is integer arithmetic, so every
comparison is array_equal: int32 rows, template bytes, the position and the level."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_restatement as tr
import track_scale_restatement as ts

pytestmark = pytest.mark.gpu


def _at_odd_offset(array, offset=33):
    """the array's bytes on the device at an odd byte offset into a larger buffer, as a tensor of the array's shape"""
    flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1))
    buf = torch.zeros(flat.numel() + offset + 7, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 2 == 1
    return view.view(array.shape)


def _search(gray, T0, pos, L, R, adapt, lost, levels=1, penalty=ts.PENALTY, odd=False):
    """d3f_track_search_scale_u8 on host arrays -> (T0, pos, L, rows) as the restatement returns them; the bytes of the
    template buffer behind T0 and the int32 around pos and the rows are guard bands"""
    from denoising_diffusion_deep_fake_amd import _lib
    B, gh, gw = gray.shape
    th0, tw0 = T0.shape
    if B == 0:
        g = torch.zeros(1, dtype=torch.uint8, device="cuda")  # (an empty tensor has no pointer to hand over)
    else:
        g = _at_odd_offset(gray) if odd else torch.from_numpy(gray).cuda()
    templ = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    templ[:tw0 * th0] = torch.from_numpy(T0.reshape(-1)).cuda()
    ints = torch.full((4 + 3 + 5 + 8 * B + 4,), -77, dtype=torch.int32, device="cuda")
    ints[4:7] = torch.tensor([pos[0], pos[1], L], dtype=torch.int32)
    p, o = ints.data_ptr() + 16, ints.data_ptr() + 48
    _lib.check(_lib.lib().d3f_track_search_scale_u8(C.c_void_p(g.data_ptr()), B, gh, gw, tw0, th0, R, adapt, lost, levels,
                                                    penalty, _lib.ptr(templ), C.c_void_p(p), C.c_void_p(o),
                                                    _lib.stream_ptr()))
    host, t = ints.cpu().numpy(), templ.cpu().numpy()
    assert (host[:4] == -77).all() and (host[7:12] == -77).all() and (host[12 + 8 * B:] == -77).all()
    assert (t[tw0 * th0:] == 0xA5).all()
    return t[:tw0 * th0].reshape(th0, tw0), (int(host[4]), int(host[5])), int(host[6]), host[12:12 + 8 * B].reshape(B, 8)


def _check(gray, T0, pos, L, R, adapt, lost, levels=1, penalty=ts.PENALTY, odd=False, want=None):
    want = want or ts.search(gray, T0, pos, L, R, adapt, lost, levels, penalty)
    got = _search(gray, T0, pos, L, R, adapt, lost, levels, penalty, odd)
    assert np.array_equal(got[3], want[3]), (got[3].tolist(), want[3].tolist())
    assert got[1] == want[1] and got[2] == want[2] and np.array_equal(got[0], want[0])
    return want


def _zooming(seed, B, gh, gw, tw0, th0, pos, grow, noise=3):
    """a smooth random image; in frame k the tw0 x th0 box at `pos` holds what frame 0 holds there, resized by 1 + grow k
    about the box's centre and moved by (2 k, -k); noise of a few levels"""
    rng = np.random.default_rng(seed)
    base = ts._smooth(rng, gh, gw, 5)
    cut = ts._smooth(rng, 2 * th0, 2 * tw0, 10)
    out = []
    for k in range(B):
        f = 1 + grow * k
        w, h = min(max(int(round(tw0 * f)), 2), gw), min(max(int(round(th0 * f)), 2), gh)
        x = int(np.clip(pos[0] + (tw0 - w) // 2 + 2 * k, 0, gw - w))
        y = int(np.clip(pos[1] + (th0 - h) // 2 - k, 0, gh - h))
        g = base.copy()
        g[y:y + h, x:x + w] = ts._render(cut, h, w)
        out.append(np.clip(np.rint(g) + rng.integers(-noise, noise + 1, size=g.shape), 0, 255))
    return np.stack(out).astype(np.uint8)


SEARCH = [
    # tw0, th0, R, gh, gw, pos, adapt, lost, grow per frame
    (13, 9, 1, 40, 50, (20, 15), 1, 255, 0.08),      # tw = 1 mod 4: the tail dword; up a level a frame
    (13, 9, 16, 40, 50, (0, 0), 1, 255, 0.08),       # a corner: anchors and windows are clipped on two sides
    (13, 9, 16, 40, 50, (37, 31), 8, 255, -0.08),    # the opposite corner, shrinking, the template replaced
    (13, 9, 64, 200, 210, (100, 90), 0, 255, 0.08),  # the widest radius, the template kept
    (48, 40, 1, 70, 83, (5, 3), 1, 16, 0.021),
    (48, 40, 16, 100, 131, (40, 30), 1, 16, 0.021),
    (48, 40, 16, 100, 131, (40, 30), 1, 16, -0.021),
    (48, 40, 64, 200, 210, (80, 80), 1, 255, 0.021),
    (64, 48, 16, 100, 131, (30, 20), 1, 255, 0.02),  # cannot grow: the upper level is dropped
    (64, 48, 64, 200, 210, (70, 66), 1, 255, -0.02),  # the whole union window, 193 x 178
    (64, 48, 64, 200, 210, (146, 152), 8, 255, -0.02),  # in the corner
    (48, 64, 16, 64, 50, (1, 0), 1, 255, -0.02),     # gh == th0: one row of candidates at the seed's level
    (4, 4, 1, 40, 50, (0, 0), 1, 255, 0.3),          # cannot shrink
    (4, 4, 16, 40, 50, (23, 18), 8, 255, 0.3),
    (4, 4, 64, 200, 210, (100, 100), 1, 255, 0.3),
    (20, 24, 1, 40, 50, (15, 8), 0, 16, 0.045),
    (20, 24, 16, 40, 50, (15, 8), 1, 16, 0.045),
    (20, 24, 16, 40, 50, (30, 16), 8, 16, -0.045),   # the corner
    (20, 24, 64, 200, 210, (90, 100), 1, 16, 0.045),
    (30, 31, 16, 64, 66, (10, 12), 1, 0, 0.0),       # tw = 2 mod 4; lost 0: found only at cost 0
    (31, 30, 8, 64, 67, (10, 12), 2, 16, 0.035),     # tw = 3 mod 4
]


@pytest.mark.parametrize("tw0, th0, R, gh, gw, pos, adapt, lost, grow", SEARCH)
def test_search_against_the_restatement(tw0, th0, R, gh, gw, pos, adapt, lost, grow):
    gray = _zooming(tw0 * 1000 + th0 * 10 + R, 3 if gh >= 200 else 4, gh, gw, tw0, th0, pos, grow)
    T0 = ts.seed(gray[0], pos[0], pos[1], tw0, th0)[0]
    L0 = max(tw0, th0)
    want = ts.search(gray[1:], T0, pos, L0, R, adapt, lost)
    for odd in (False, True):
        _check(gray[1:], T0, pos, L0, R, adapt, lost, odd=odd, want=want)
    rows = want[3]
    if lost == 255:
        assert rows[:, 5].all()
    if (tw0, th0) == (64, 48) and grow > 0 or (tw0, th0) == (4, 4) and grow < 0:
        assert (rows[:, 6] == L0).all()
    if (tw0, th0, R, adapt) == (48, 40, 16, 1):  # the size is followed, a level a frame
        assert rows[:, 5].all() and rows[:, 6].tolist() == [L0 + k * (1 if grow > 0 else -1) for k in (1, 2, 3)]


def test_a_level_and_a_position_the_host_never_saw_are_moved_inside_first():
    """the level above the valid ones (and below them), the position outside the image: as the restatement from the
    nearest valid state"""
    gray = _zooming(5, 3, 40, 50, 13, 9, (20, 15), 0.0)
    T0 = ts.seed(gray[0], 20, 15, 13, 9)[0]
    lo, hi = ts.level_range(13, 9, 40, 50)
    assert (lo, hi) == (6, 50)
    for L, pos, L_in, pos_in in ((99, (45, 35), 50, (0, 5)), (-3, (-7, 38), 6, (0, 36)), (13, (1000, -1000), 13, (37, 0))):
        want = ts.search(gray[1:], T0, pos_in, L_in, 16, 1, 255)
        got = _search(gray[1:], T0, pos, L, 16, 1, 255)
        assert np.array_equal(got[3], want[3]) and got[1] == want[1] and got[2] == want[2] and np.array_equal(got[0], want[0])


def test_penalties_and_levels_0():
    gray = _zooming(11, 4, 64, 66, 20, 24, (20, 18), 0.045)
    T0 = ts.seed(gray[0], 20, 18, 20, 24)[0]
    for levels, penalty in ((0, 512), (0, 0), (1, 0), (1, 4096), (1, 65535)):
        rows = _check(gray[1:], T0, (20, 18), 24, 8, 1, 255, levels, penalty)[3]
        if levels == 0 or penalty == 65535:
            assert (rows[:, 6] == 24).all()


@pytest.mark.parametrize("s", [1, 2])
def test_levels_0_is_track_template_u8_bit_for_bit(s):
    from denoising_diffusion_deep_fake_amd import ops
    patch = (24 // s, 20 // s)
    frames, positions = tr.moving_patch_frames(40 + s, 8, 96, 160, s, 3, absent=(5,), patch=patch)
    dev = torch.from_numpy(frames).cuda()
    face = (positions[0][0] * s, positions[0][1] * s, patch[1] * s, patch[0] * s)
    plain, scale = ops.TrackState(), ops.TrackState()
    for state in (plain, scale):
        geo = ops.track_seed(state, dev[0], face, 24 // s)
    assert geo[0] == s and scale.pos_level.cpu().tolist() == [positions[0][0], positions[0][1], patch[0]]
    want = ops.track_template_u8(dev[1:], plain, search=8, adapt=2).cpu().numpy()
    rows = ops.track_template_scale_u8(dev[1:], scale, search=8, adapt=2, levels=0).cpu().numpy()
    assert rows.shape == (7, 8) and np.array_equal(rows[:, [0, 1, 7, 5]], want) and want[:, 3].tolist() == [1, 1, 1, 1, 0, 1, 1]
    assert (rows[:, 2:4] == (patch[1], patch[0])).all() and (rows[:, 6] == patch[0]).all()
    assert np.array_equal(scale.templ.cpu().numpy(), plain.templ.cpu().numpy())
    assert np.array_equal(scale.pos.cpu().numpy(), plain.pos.cpu().numpy()) and int(scale.pos_level[2]) == patch[0]
    assert ops.track_scale_faces(rows.tolist(), scale) == ops.track_faces(want.tolist(), plain)


def test_the_plain_seed_entry_leaves_the_level_alone():
    from denoising_diffusion_deep_fake_amd import _lib
    frame = np.random.default_rng(1).integers(0, 256, size=(64, 96, 3), dtype=np.uint8)
    dev = torch.from_numpy(frame).cuda()
    T, pos = tr.seed(tr.gray_decimate(frame, 2), 7, 5, 13, 9)
    for name, level in (("d3f_track_seed_u8", -77), ("d3f_track_seed_scale_u8", 13)):
        templ = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        ints = torch.full((8,), -77, dtype=torch.int32, device="cuda")
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(dev), 64, 96, 2, 7, 5, 13, 9, _lib.ptr(templ),
                                             C.c_void_p(ints.data_ptr() + 8), _lib.stream_ptr()))
        assert ints.cpu().tolist() == [-77, -77, 7, 5, level, -77, -77, -77]
        t = templ.cpu().numpy()
        assert np.array_equal(t[:117].reshape(9, 13), T) and (t[117:] == 0xA5).all()


def test_on_a_constant_image_the_position_and_the_level_stay():
    gray = np.full((3, 40, 50), 77, dtype=np.uint8)
    for R in (1, 16, 64):
        for value, ncost, penalty in ((77, 0, 512), (78, 4096, 512), (78, 4096, 0)):
            T0 = np.full((9, 13), value, dtype=np.uint8)
            T1, pos, L, rows = _check(gray, T0, (11, 9), 13, R, 1, 255, 1, penalty)
            assert pos == (11, 9) and L == 13 and rows.tolist() == [[11, 9, 13, 9, ncost, 1, 13, ncost * 117 >> 12]] * 3
    T1, pos, L, rows = _check(gray, np.full((9, 13), 78, dtype=np.uint8), (11, 9), 13, 16, 1, 0)  # lost 0: not found
    assert pos == (11, 9) and L == 13 and rows.tolist() == [[11, 9, 13, 9, 4096, 0, 13, 117]] * 3


def test_an_absent_frame_mid_call_changes_nothing_and_the_next_frame_picks_the_face_up():
    gray, boxes = ts.scaling_patch_frames(4, 7, 96, 120, 2, 0.15, patch=(24, 20), absent=(3,))
    x, y, pw, ph = boxes[0]
    T0, pos = ts.seed(gray[0], x, y, pw, ph)
    T1, pos1, L1, rows = _check(gray[1:], T0, pos, 24, 8, 1, 16)
    assert rows[:, 5].tolist() == [1, 1, 0, 1, 1, 1] and rows[2, [0, 1, 2, 3, 6]].tolist() == rows[1, [0, 1, 2, 3, 6]].tolist()
    assert L1 > 24 and abs(rows[-1, 2] - boxes[-1][2]) <= 1 and abs(rows[-1, 3] - boxes[-1][3]) <= 1
    # the state behind the absent frame is the state in front of it
    before = _search(gray[1:3], T0, pos, 24, 8, 1, 16)
    behind = _search(gray[3:4], before[0], before[1], before[2], 8, 1, 16)
    assert behind[3][0, 5] == 0 and np.array_equal(behind[0], before[0]) and behind[1:3] == before[1:3]


def _growing_on_device(seed, B, grow=0.2, absent=()):
    """frames of 96 x 160 whose reduced grey image at stride 2 holds a patch of 20 x 24 samples that grows"""
    gray, boxes = ts.scaling_patch_frames(seed, B, 48, 80, 2, grow, patch=(24, 20), absent=absent)
    frames = ts.bgr_at_stride(gray, 2)
    return frames, torch.from_numpy(frames).cuda(), gray, boxes


def test_cutting_a_call_changes_nothing():
    """9 frames as one call, as nine and as 4 + 5: the same rows and the same final state"""
    from denoising_diffusion_deep_fake_amd import ops
    frames, dev, gray, boxes = _growing_on_device(31, 10, absent=(6,))
    face = tuple(2 * v for v in boxes[0])
    results = []
    for cuts in ([9], [1] * 9, [4, 5]):
        state = ops.TrackState()
        assert ops.track_seed(state, dev[0], face, 24)[:5] == (2,) + boxes[0]
        rows, at = [], 1
        for n in cuts:
            rows.append(ops.track_template_scale_u8(dev[at:at + n], state, search=8))
            at += n
        results.append((torch.cat(rows).cpu().numpy(), state.templ.cpu().numpy(), state.pos_level.cpu().numpy()))
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    geo = ts.geometry(96, 160, face, 24)
    T0, pos = ts.seed(gray[0], *geo[1:5])
    T1, pos1, L1, rows = ts.search(gray[1:], T0, pos, 24, 8, ops.TRACK_ADAPT, ops.TRACK_LOST)
    assert np.array_equal(results[0][0], rows) and tuple(results[0][2]) == pos1 + (L1,)
    assert np.array_equal(results[0][1][:T1.size].reshape(T1.shape), T1)
    assert rows[:, 5].tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1] and L1 > 24
    assert ops.track_scale_faces(rows.tolist(), state) == ts.faces(rows, geo, 96, 160)
    assert ops.track_scale_faces(rows.tolist(), geo, frame=(96, 160)) == ts.faces(rows, geo, 96, 160)


def test_the_fused_entry_is_decimate_then_search_at_odd_addresses():
    from denoising_diffusion_deep_fake_amd import ops
    rng = np.random.default_rng(8)
    gray, boxes = ts.scaling_patch_frames(5, 6, 48, 80, 2, -0.2, patch=(24, 20))
    # (not flat inside a 2 x 2 block, one more row and column than the reduction keeps)
    frames = np.pad(ts.bgr_at_stride(gray, 2), ((0, 0), (0, 1), (0, 1), (0, 0)), mode="edge")
    frames = np.clip(frames.astype(np.int64) + rng.integers(-9, 10, size=frames.shape), 0, 255).astype(np.uint8)
    dev = _at_odd_offset(frames)
    face = tuple(2 * v for v in boxes[0])
    fused, parts = ops.TrackState(), ops.TrackState()
    for state in (fused, parts):
        geo = ops.track_seed(state, dev[0], face, 24)
    s, _, _, tw, th = geo[:5]
    assert (s, tw, th) == (2, 20, 24)
    rows = ops.track_template_scale_u8(dev[1:], fused, search=8, adapt=2, lost=20, levels=1, penalty=100)
    g = tr.gray_decimate(frames[1:], 2)
    assert np.array_equal(ops.gray_decimate_u8(dev[1:], s).cpu().numpy(), g)
    T0 = parts.templ.cpu().numpy()[:tw * th].reshape(th, tw)
    x, y, L = parts.pos_level.cpu().tolist()
    T1, pos1, L1, want = _search(g, T0, (x, y), L, 8, 2, 20, 1, 100, odd=True)
    assert np.array_equal(rows.cpu().numpy(), want) and fused.pos_level.cpu().tolist() == list(pos1) + [L1]
    assert np.array_equal(fused.templ.cpu().numpy()[:tw * th].reshape(th, tw), T1)
    assert np.array_equal(want, ts.search(g, T0, (x, y), L, 8, 2, 20, 1, 100)[3]) and L1 < 24 and want[:, 5].all()
    assert rows.dtype == torch.int32 and rows.shape == (5, 8) and rows.is_cuda
    assert ops.track_template_scale_u8(dev[:0], fused).shape == (0, 8)
    with pytest.raises(ValueError, match="seeded"):
        ops.track_template_scale_u8(dev, ops.TrackState())
    with pytest.raises(ValueError, match="seeded on"):
        ops.track_template_scale_u8(dev[:, :90], fused)


def test_search_of_no_frames_touches_nothing():
    gray = np.zeros((0, 40, 50), dtype=np.uint8)
    T0 = np.arange(117, dtype=np.uint8).reshape(9, 13)
    T1, pos, L, rows = _search(gray, T0, (3, 4), 99, 16, 8, 255)
    assert np.array_equal(T1, T0) and pos == (3, 4) and L == 99 and rows.shape == (0, 8)


def test_the_host_refuses_levels_2_a_penalty_of_65536_and_a_misaligned_pos():
    from denoising_diffusion_deep_fake_amd import _lib
    lib = _lib.lib()
    g = torch.zeros((2, 40, 50), dtype=torch.uint8, device="cuda")
    templ = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ints = torch.full((32,), -77, dtype=torch.int32, device="cuda")
    p, o = ints.data_ptr() + 16, ints.data_ptr() + 48

    def call(levels=1, penalty=512, pos=p):
        return lib.d3f_track_search_scale_u8(_lib.ptr(g), 2, 40, 50, 13, 9, 16, 1, 16, levels, penalty, _lib.ptr(templ),
                                             C.c_void_p(pos), C.c_void_p(o), _lib.stream_ptr())

    for change, word in ((dict(levels=2), b"levels"), (dict(penalty=65536), b"penalty"), (dict(pos=p + 2), b"aligned")):
        assert call(**change) != 0 and word in lib.d3f_last_error()
    torch.cuda.synchronize()
    assert (ints.cpu().numpy() == -77).all() and (templ.cpu().numpy() == 0xA5).all()  # nothing ran


def test_the_tool_with_scale_writes_the_restatements_track_whatever_the_batch(tmp_path):
    """16 frames of 96 x 160 at stride 2, the patch growing, keys at frames 1 and 9: the track is the restatement's for
    batch_frames 1, 5 and 16, its boxes grow, and scale=False writes what the plain tracker's restatement gives"""
    from denoising_diffusion_deep_fake_amd.script_tools.track_face_box import TrackFaceBox
    frames, _, gray, boxes = _growing_on_device(2024, 16, grow=0.25)
    keys = {k: tuple(2 * v for v in boxes[k]) for k in (1, 9)}
    want = ts.tool_track(frames, keys, R=8, side=32)
    assert want[0] is None and want[1] == keys[1] and want[9] == keys[9] and None not in want[1:]
    assert ts.geometry(96, 160, keys[1], 32)[0] == ts.geometry(96, 160, keys[9], 32)[0] == 2
    for a, b in ((1, 8), (9, 15)):  # the boxes grow between the keys, to within a sample (two pixels) of the patch
        assert want[b][2] > want[a][2] and want[b][3] > want[a][3]
        assert all(want[k + 1][2] >= want[k][2] and want[k + 1][3] >= want[k][3] for k in range(a, b))
        assert abs(want[b][2] - 2 * boxes[b][2]) <= 2 and abs(want[b][3] - 2 * boxes[b][3]) <= 2
    texts = []
    for batch_frames in (1, 5, 16):
        path = tmp_path / f"track_{batch_frames}.txt"
        got = []
        tool = TrackFaceBox(tmp_path / "clip.mp4", [(k,) + box for k, box in keys.items()], output_path=path,
                            batch_frames=batch_frames, frames=iter(frames), sink=got.append, search=8, template_side=32,
                            scale=True)
        assert tool.track == want and got == want
        texts.append(path.read_text())
    assert texts[0] == texts[1] == texts[2]
    lines = texts[0].splitlines()
    assert lines[3] == "# scale search: one level a frame, penalty 512" and not lines[4].startswith("#")
    assert lines[4:] == ["-" if box is None else "{} {} {} {}".format(*box) for box in want]
    # without scale: the plain tracker's file, header included
    plain = tr.tool_track(frames, keys, R=8, side=32)
    path = tmp_path / "plain.txt"
    tool = TrackFaceBox(tmp_path / "clip.mp4", [(k,) + box for k, box in keys.items()], output_path=path, batch_frames=5,
                        frames=iter(frames), search=8, template_side=32)
    assert tool.track == plain and all(box[2:] == keys[1 if k < 9 else 9][2:] for k, box in enumerate(plain) if box)
    keys_line = ", ".join("{} {} {} {} {}".format(k, *box) for k, box in keys.items())
    assert path.read_text().splitlines() == [
        "# track_face_box clip.mp4: x y w h per frame, - where the face was not found",
        f"# keys (frame x y w h): {keys_line}", "# search 8, adapt 1, lost 16, template side 32",
    ] + ["-" if box is None else "{} {} {} {}".format(*box) for box in plain]
