"""GPU: the rotation search of the template tracker against its restatement (tests/track_rot_restatement.py) -- the search on
grey input, the seed with an angle, the fused entry, the Python entries, the sign of the angle against the frame path's
rotated paste, and the tool with rotate=True.  Everything is integer arithmetic, so every comparison is array_equal: int32
rows, template bytes, the position and the angle index."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_restatement as tr
import track_rot_restatement as trr

pytestmark = pytest.mark.gpu


def _at_odd_offset(array, offset=33):
    """the array's bytes on the device at an odd byte offset into a larger buffer, as a tensor of the array's shape"""
    flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1))
    buf = torch.zeros(flat.numel() + offset + 7, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 2 == 1
    return view.view(array.shape)


def _table(step, reach):
    amax, tab = trr.table(step, reach)
    flat = [v for a in range(-amax, amax + 1) for v in tab[a]]
    return amax, (C.c_int32 * len(flat))(*flat)


def _search(gray, T0, pos, a, R, adapt, lost, steps=1, penalty=trr.PENALTY, step=trr.STEP, reach=trr.MAX_DEGREES, odd=False):
    """d3f_track_search_rot_u8 on host arrays -> (T0, pos, a, rows) as the restatement returns them; the bytes of the
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
    ints[4:7] = torch.tensor([pos[0], pos[1], a], dtype=torch.int32)
    p, o = ints.data_ptr() + 16, ints.data_ptr() + 48
    amax, table = _table(step, reach)
    _lib.check(_lib.lib().d3f_track_search_rot_u8(C.c_void_p(g.data_ptr()), B, gh, gw, tw0, th0, R, adapt, lost, steps, penalty,
                                                  amax, table, _lib.ptr(templ), C.c_void_p(p), C.c_void_p(o),
                                                  _lib.stream_ptr()))
    host, t = ints.cpu().numpy(), templ.cpu().numpy()
    assert (host[:4] == -77).all() and (host[7:12] == -77).all() and (host[12 + 8 * B:] == -77).all()
    assert (t[tw0 * th0:] == 0xA5).all()
    return t[:tw0 * th0].reshape(th0, tw0), (int(host[4]), int(host[5])), int(host[6]), host[12:12 + 8 * B].reshape(B, 8)


def _check(gray, T0, pos, a, R, adapt, lost, steps=1, penalty=trr.PENALTY, step=trr.STEP, reach=trr.MAX_DEGREES, odd=False,
           want=None):
    want = want or trr.search(gray, T0, pos, a, R, adapt, lost, steps, penalty, step, reach)
    got = _search(gray, T0, pos, a, R, adapt, lost, steps, penalty, step, reach, odd)
    assert np.array_equal(got[3], want[3]), (got[3].tolist(), want[3].tolist())
    assert got[1] == want[1] and got[2] == want[2] and np.array_equal(got[0], want[0])
    return want


def _rolling(seed, B, gh, gw, tw0, th0, pos, roll, noise=3):
    """a smooth random image; in frame k the tw0 x th0 box at `pos`, moved by (2 k, -k) and kept inside the image, holds one
    smooth texture turned by roll k degrees about the box's centre; noise of a few levels"""
    rng = np.random.default_rng(seed)
    base = trr._smooth(rng, gh, gw, 5)
    cut = trr._smooth(rng, 2 * th0, 2 * tw0, 10)
    out = []
    for k in range(B):
        x = int(np.clip(pos[0] + 2 * k, 0, gw - tw0))
        y = int(np.clip(pos[1] - k, 0, gh - th0))
        g = base.copy()
        trr.turned_patch(g, cut, x, y, tw0, th0, roll * k)
        out.append(np.clip(np.rint(g) + rng.integers(-noise, noise + 1, size=g.shape), 0, 255))
    return np.stack(out).astype(np.uint8)


SEARCH = [
    # tw0, th0, R, gh, gw, pos, adapt, lost, roll per frame, (step, reach), the first index
    (13, 9, 1, 40, 50, (20, 15), 1, 255, 2.0, (200, 60), 0),       # spans of 1, 3 mod 4: the tail dword
    (13, 9, 16, 40, 50, (0, 0), 8, 255, -2.0, (200, 60), 0),       # a corner: the window is clipped on two sides
    (13, 9, 64, 200, 210, (100, 90), 0, 255, 2.0, (200, 60), 0),   # the widest radius, the template kept
    (4, 4, 1, 40, 50, (0, 0), 1, 255, 8.0, (800, 180), 0),         # the smallest disc, 12 samples
    (4, 4, 16, 40, 50, (46, 36), 8, 255, -8.0, (800, 180), 0),     # the opposite corner
    (4, 4, 64, 200, 210, (100, 100), 1, 255, 8.0, (800, 180), 0),
    (20, 24, 1, 40, 50, (15, 8), 0, 16, 2.0, (200, 60), 0),
    (20, 24, 16, 40, 50, (30, 16), 8, 16, -2.0, (200, 60), 0),     # the corner
    (20, 24, 64, 200, 210, (90, 100), 1, 16, 2.0, (200, 60), 0),
    (30, 31, 1, 64, 66, (10, 12), 1, 255, 1.0, (200, 60), 0),
    (30, 31, 16, 64, 66, (10, 12), 1, 0, 0.0, (200, 60), 0),       # spans of 2 mod 4; lost 0: found only at cost 0
    (30, 31, 64, 200, 210, (80, 80), 1, 255, -3.0, (100, 2), -2),  # pinned at -amax
    (31, 30, 1, 64, 67, (10, 12), 2, 16, 1.5, (150, 45), 0),
    (31, 30, 16, 64, 67, (10, 12), 2, 255, 4.5, (150, 3), 2),      # pinned at +amax: the upper angle is dropped
    (31, 30, 64, 200, 210, (150, 160), 2, 255, 1.5, (150, 45), 0),
    (48, 40, 1, 70, 83, (5, 3), 1, 16, 2.0, (200, 60), 0),
    (48, 40, 16, 100, 131, (40, 30), 1, 16, 2.0, (200, 60), 0),    # turning up, a step a frame
    (48, 40, 16, 100, 131, (40, 30), 1, 16, -2.0, (200, 60), 0),   # turning down
    (48, 40, 64, 200, 210, (80, 80), 1, 255, 2.0, (200, 60), 0),
    (64, 48, 1, 100, 131, (30, 20), 1, 255, 128.0, (200, 128), 63),  # up to the last index of the longest table
    (64, 48, 16, 100, 131, (30, 20), 1, 255, -2.0, (200, 60), 0),
    (64, 48, 64, 200, 210, (70, 66), 1, 255, 2.0, (200, 60), 0),   # the whole window, 192 x 176
    (64, 48, 64, 200, 210, (146, 152), 8, 255, -2.0, (200, 60), 0),  # in the corner
    (48, 64, 1, 64, 50, (1, 0), 1, 255, 2.0, (200, 60), 0),        # gh == th0: one row of candidates; empty rows of the disc
    (48, 64, 16, 64, 50, (1, 0), 1, 255, -2.0, (200, 60), 0),
    (48, 64, 64, 200, 210, (100, 70), 1, 255, 2.0, (200, 60), 0),
]


@pytest.mark.parametrize("tw0, th0, R, gh, gw, pos, adapt, lost, roll, table, first", SEARCH)
def test_search_against_the_restatement(tw0, th0, R, gh, gw, pos, adapt, lost, roll, table, first):
    gray = _rolling(tw0 * 1000 + th0 * 10 + R, 3 if gh >= 200 else 4, gh, gw, tw0, th0, pos, roll)
    T0 = trr.seed_rot(gray[0], pos[0], pos[1], tw0, th0)[0]
    step, reach = table
    want = trr.search(gray[1:], T0, pos, first, R, adapt, lost, 1, trr.PENALTY, step, reach)
    for odd in (False, True):
        _check(gray[1:], T0, pos, first, R, adapt, lost, step=step, reach=reach, odd=odd, want=want)
    rows = want[3]
    amax = trr.table(step, reach)[0]
    assert (np.abs(rows[:, 6]) <= amax).all()
    if lost == 255:
        assert rows[:, 5].all()
    if first and reach < 128:  # pinned: the roll goes on, the index cannot
        assert (rows[:, 6] == first).all() and abs(first) == amax
    if reach == 128:
        assert rows[0, 6] == amax == 64
    if (tw0, th0, R, adapt) == (48, 40, 16, 1):  # the roll is followed, a step a frame
        assert rows[:, 5].all() and rows[:, 6].tolist() == [k * (1 if roll > 0 else -1) for k in (1, 2, 3)]


def test_an_angle_and_a_position_the_host_never_saw_are_moved_inside_first():
    gray = _rolling(5, 3, 40, 50, 13, 9, (20, 15), 0.0)
    T0 = trr.seed_rot(gray[0], 20, 15, 13, 9)[0]
    for a, pos in ((99, (45, 35)), (-99, (-7, 38)), (3, (1000, -1000)), (-(1 << 31), (1 << 30, -(1 << 30)))):
        pos_in, a_in = trr.clamp_state(pos, a, 40, 50, 13, 9)
        assert abs(a_in) <= 30 and 0 <= pos_in[0] <= 37 and 0 <= pos_in[1] <= 31
        want = trr.search(gray[1:], T0, pos_in, a_in, 16, 1, 255)
        got = _search(gray[1:], T0, pos, a, 16, 1, 255)
        assert np.array_equal(got[3], want[3]) and got[1] == want[1] and got[2] == want[2] and np.array_equal(got[0], want[0])


def test_penalties_and_steps_0():
    gray = _rolling(11, 4, 64, 66, 20, 24, (20, 18), 2.0)
    T0 = trr.seed_rot(gray[0], 20, 18, 20, 24)[0]
    for steps, penalty in ((0, 512), (0, 0), (1, 0), (1, 4096), (1, 65535)):
        rows = _check(gray[1:], T0, (20, 18), 0, 8, 1, 255, steps, penalty)[3]
        if steps == 0 or penalty == 65535:
            assert (rows[:, 6] == 0).all()


def test_on_a_constant_image_the_position_and_the_angle_stay():
    gray = np.full((3, 40, 50), 77, dtype=np.uint8)
    n = int(trr.disc_mask(13, 9).sum())
    for R in (1, 16, 64):
        for value, ncost, penalty in ((77, 0, 512), (78, 4096, 512), (78, 4096, 0)):
            T0 = np.full((9, 13), value, dtype=np.uint8)
            T1, pos, a, rows = _check(gray, T0, (11, 9), -4, R, 1, 255, 1, penalty)
            assert pos == (11, 9) and a == -4 and rows.tolist() == [[11, 9, 13, 9, ncost, 1, -4, ncost * n >> 12]] * 3
    T1, pos, a, rows = _check(gray, np.full((9, 13), 78, dtype=np.uint8), (11, 9), 7, 16, 1, 0)  # lost 0: not found
    assert pos == (11, 9) and a == 7 and rows.tolist() == [[11, 9, 13, 9, 4096, 0, 7, n]] * 3


def test_an_absent_frame_mid_call_changes_nothing_and_the_next_frame_picks_the_face_up():
    gray, boxes = trr.rolling_patch_frames(4, 7, 96, 120, 2, 2.0, patch=(24, 20), absent=(3,))
    x, y, pw, ph, _ = boxes[0]
    T0, pos, a = trr.seed_rot(gray[0], x, y, pw, ph)
    T1, pos1, a1, rows = _check(gray[1:], T0, pos, a, 8, 1, 16)
    assert rows[:, 5].tolist() == [1, 1, 0, 1, 1, 1] and rows[2, [0, 1, 6]].tolist() == rows[1, [0, 1, 6]].tolist()
    # the state behind the absent frame is the state in front of it
    before = _search(gray[1:3], T0, pos, a, 8, 1, 16)
    behind = _search(gray[3:4], before[0], before[1], before[2], 8, 1, 16)
    assert behind[3][0, 5] == 0 and np.array_equal(behind[0], before[0]) and behind[1:3] == before[1:3]


def _rolling_on_device(seed, B, roll=2.0, absent=()):
    """frames of 96 x 160 whose reduced grey image at stride 2 holds a patch of 20 x 24 samples that rolls"""
    gray, boxes = trr.rolling_patch_frames(seed, B, 48, 80, 2, roll, patch=(24, 20), absent=absent)
    frames = trr.bgr_at_stride(gray, 2)
    return frames, torch.from_numpy(frames).cuda(), gray, boxes


def test_cutting_a_call_changes_nothing():
    """9 frames as one call, as nine and as 4 + 5: the same rows and the same final state"""
    from denoising_diffusion_deep_fake_amd import ops
    frames, dev, gray, boxes = _rolling_on_device(31, 10, absent=(6,))
    face = tuple(2 * v for v in boxes[0][:4])
    results = []
    for cuts in ([9], [1] * 9, [4, 5]):
        state = ops.TrackState()
        assert ops.track_seed(state, dev[0], face, 24, angle=0.0)[:5] == (2,) + boxes[0][:4]
        rows, at = [], 1
        for n in cuts:
            rows.append(ops.track_template_rot_u8(dev[at:at + n], state, search=8))
            at += n
        results.append((torch.cat(rows).cpu().numpy(), state.templ.cpu().numpy(), state.pos_level.cpu().numpy()))
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    geo = trr.geometry(96, 160, face, 24)
    T0, pos, a = trr.seed_rot(gray[0], *geo[1:5])
    T1, pos1, a1, rows = trr.search(gray[1:], T0, pos, a, 8, ops.TRACK_ADAPT, ops.TRACK_LOST)
    assert np.array_equal(results[0][0], rows) and tuple(results[0][2]) == pos1 + (a1,)
    assert np.array_equal(results[0][1][:T1.size].reshape(T1.shape), T1)
    assert rows[:, 5].tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1] and a1 > 0
    assert ops.track_rot_faces(rows.tolist(), state) == trr.faces(rows, geo) == ops.track_rot_faces(rows.tolist(), geo, 200)


def test_the_fused_entry_is_decimate_then_search_at_odd_addresses():
    from denoising_diffusion_deep_fake_amd import ops
    rng = np.random.default_rng(8)
    gray, boxes = trr.rolling_patch_frames(5, 6, 48, 80, 2, -3.0, patch=(24, 20))
    # (not flat inside a 2 x 2 block, one more row and column than the reduction keeps)
    frames = np.pad(trr.bgr_at_stride(gray, 2), ((0, 0), (0, 1), (0, 1), (0, 0)), mode="edge")
    frames = np.clip(frames.astype(np.int64) + rng.integers(-9, 10, size=frames.shape), 0, 255).astype(np.uint8)
    dev = _at_odd_offset(frames)
    face = tuple(2 * v for v in boxes[0][:4])
    fused, parts = ops.TrackState(), ops.TrackState()
    for state in (fused, parts):
        geo = ops.track_seed(state, dev[0], face, 24, angle=0.0, step=300, max_degrees=45)
    s, _, _, tw, th = geo[:5]
    assert (s, tw, th) == (2, 20, 24) and fused.rot == (300, 45)
    rows = ops.track_template_rot_u8(dev[1:], fused, search=8, adapt=2, lost=20, steps=1, penalty=100, step=300, max_degrees=45)
    g = tr.gray_decimate(frames[1:], 2)
    assert np.array_equal(ops.gray_decimate_u8(dev[1:], s).cpu().numpy(), g)
    T0 = parts.templ.cpu().numpy()[:tw * th].reshape(th, tw)
    x, y, a = parts.pos_level.cpu().tolist()
    T1, pos1, a1, want = _search(g, T0, (x, y), a, 8, 2, 20, 1, 100, 300, 45, odd=True)
    assert np.array_equal(rows.cpu().numpy(), want) and fused.pos_level.cpu().tolist() == list(pos1) + [a1]
    assert np.array_equal(fused.templ.cpu().numpy()[:tw * th].reshape(th, tw), T1)
    assert np.array_equal(want, trr.search(g, T0, (x, y), a, 8, 2, 20, 1, 100, 300, 45)[3]) and a1 < 0 and want[:, 5].all()
    assert rows.dtype == torch.int32 and rows.shape == (5, 8) and rows.is_cuda
    assert ops.track_template_rot_u8(dev[:0], fused, step=300, max_degrees=45).shape == (0, 8)
    with pytest.raises(ValueError, match="seeded"):
        ops.track_template_rot_u8(dev, ops.TrackState())
    with pytest.raises(ValueError, match="seeded on"):
        ops.track_template_rot_u8(dev[:, :90], fused, step=300, max_degrees=45)
    with pytest.raises(ValueError, match="the state was seeded with"):
        ops.track_template_rot_u8(dev, fused)  # another step than the seed's
    plain = ops.TrackState()
    ops.track_seed(plain, dev[0], face, 24)
    with pytest.raises(ValueError, match="without angle="):
        ops.track_template_rot_u8(dev, plain)
    with pytest.raises(ValueError, match="outside the table"):
        ops.track_seed(plain, dev[0], face, 24, angle=-61.0)


def test_search_of_no_frames_touches_nothing():
    gray = np.zeros((0, 40, 50), dtype=np.uint8)
    T0 = np.arange(117, dtype=np.uint8).reshape(9, 13)
    T1, pos, a, rows = _search(gray, T0, (3, 4), 99, 16, 8, 255)
    assert np.array_equal(T1, T0) and pos == (3, 4) and a == 99 and rows.shape == (0, 8)


def test_every_refusal_runs_nothing():
    from denoising_diffusion_deep_fake_amd import _lib
    lib = _lib.lib()
    g = torch.zeros((2, 40, 50), dtype=torch.uint8, device="cuda")
    frame = torch.zeros((64, 96, 3), dtype=torch.uint8, device="cuda")
    templ = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ints = torch.full((32,), -77, dtype=torch.int32, device="cuda")
    p, o = ints.data_ptr() + 16, ints.data_ptr() + 48
    amax, good = _table(200, 60)
    bad = (C.c_int32 * len(good))(*good)
    bad[7] = 65537

    def call(steps=1, penalty=512, amax=amax, table=good, pos=p, search=16, adapt=1, lost=16, tw=13, fused=False):
        if fused:
            return lib.d3f_track_template_rot_u8(_lib.ptr(frame), 1, 64, 96, 2, tw, 9, search, adapt, lost, steps, penalty, amax,
                                                 table, _lib.ptr(templ), C.c_void_p(pos), _lib.ptr(g), C.c_void_p(o),
                                                 _lib.stream_ptr())
        return lib.d3f_track_search_rot_u8(_lib.ptr(g), 2, 40, 50, tw, 9, search, adapt, lost, steps, penalty, amax, table,
                                           _lib.ptr(templ), C.c_void_p(pos), C.c_void_p(o), _lib.stream_ptr())

    for fused in (False, True):
        for change, word in ((dict(steps=2), b"steps"), (dict(penalty=65536), b"penalty"), (dict(amax=65), b"amax"),
                             (dict(table=bad), b"table entry"), (dict(table=None), b"null table"), (dict(pos=p + 2), b"aligned"),
                             (dict(search=65), b"search"), (dict(adapt=9), b"adapt"), (dict(lost=256), b"lost"),
                             (dict(tw=65), b"template")):
            assert call(fused=fused, **change) != 0 and word in lib.d3f_last_error(), (fused, change, lib.d3f_last_error())
    seed = lib.d3f_track_seed_rot_u8
    for args, word in (((0, 0, 13, 9, 65, 65536, 0), b"angle index"), ((0, 0, 13, 9, 1, 65537, 0), b"rot"),
                       ((40, 24, 13, 9, 1, 65500, 2287), b"outside the reduced image")):
        assert seed(_lib.ptr(frame), 64, 96, 2, *args, _lib.ptr(templ), C.c_void_p(p), _lib.stream_ptr()) != 0
        assert word in lib.d3f_last_error()
    torch.cuda.synchronize()
    assert (ints.cpu().numpy() == -77).all() and (templ.cpu().numpy() == 0xA5).all() and (g.cpu().numpy() == 0).all()


def test_the_seed_with_an_angle_is_the_restatements_and_without_one_the_plain_seeds_bytes():
    from denoising_diffusion_deep_fake_amd import _lib, ops
    gray, boxes = trr.rolling_patch_frames(6, 1, 32, 48, 0, 0.0, patch=(20, 16), start=10.0, cell=4)
    frame = trr.bgr_at_stride(gray, 2)[0]
    frame = np.clip(frame.astype(np.int64) + np.random.default_rng(1).integers(-9, 10, size=frame.shape), 0, 255).astype(np.uint8)
    dev = torch.from_numpy(frame).cuda()
    g = tr.gray_decimate(frame, 2)
    amax, tab = trr.table()

    def seeded(name, box, *more):
        templ = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        ints = torch.full((8,), -77, dtype=torch.int32, device="cuda")
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(dev), 64, 96, 2, *box, *more, _lib.ptr(templ),
                                             C.c_void_p(ints.data_ptr() + 8), _lib.stream_ptr()))
        return templ.cpu().numpy(), ints.cpu().tolist()

    for box in ((7, 5, 13, 9), boxes[0][:4], (0, 0, 4, 4), (0, 0, 48, 32)):
        x, y, tw, th = box
        plain, ints = seeded("d3f_track_seed_u8", box)
        assert ints == [-77, -77, x, y, -77, -77, -77, -77]
        for a0 in (0, 5, -5, 30, -30):
            T0, pos, a = trr.seed_rot(g, x, y, tw, th, a0 * 200)
            t, ints = seeded("d3f_track_seed_rot_u8", box, a0, *tab[a0])
            assert a == a0 and ints == [-77, -77, x, y, a0, -77, -77, -77]
            assert np.array_equal(t[:tw * th].reshape(th, tw), T0) and (t[tw * th:] == 0xA5).all()
            assert np.array_equal(t, plain) == (a0 == 0)
    # the Python entry: the index is the angle rounded to the step, halves away from zero
    state = ops.TrackState()
    face = tuple(2 * v for v in boxes[0][:4])
    for angle, a0 in ((10.0, 5), (-9.0, -5), (0.99, 0), (-1.0, -1), (0.0, 0)):
        geo = ops.track_seed(state, dev, face, 24, angle=angle)
        T0 = trr.seed_rot(g, *geo[1:5], int(round(angle * 100)))[0]
        assert state.pos_level.cpu().tolist() == [geo[1], geo[2], a0] and state.rot == (200, 60)
        assert np.array_equal(state.templ.cpu().numpy()[:T0.size].reshape(T0.shape), T0)
    ops.track_seed(state, dev, face, 24)
    assert state.rot is None and state.pos_level.cpu().tolist() == [geo[1], geo[2], max(geo[3:5])]


def test_the_tracked_angle_has_the_sign_of_the_frame_paths_rotated_paste():
    """one patch pasted by paste_resize_cubic_u8(..., angles=) at 2 k degrees in frame k, and at -2 k: the tracker, seeded on
    frame 0, writes angles within one step of the paste's"""
    from denoising_diffusion_deep_fake_amd import ops
    rng = np.random.default_rng(12)
    B, box = 8, (70, 40, 80, 96)
    back = np.rint(trr._smooth(rng, 96, 120, 6)).astype(np.uint8)
    frames = torch.from_numpy(np.repeat(trr.bgr_at_stride(back[None], 2), B, axis=0)).cuda()
    patch = np.rint(trr._smooth(rng, 96, 80, 12)).astype(np.uint8)
    patch = torch.from_numpy(np.ascontiguousarray(np.repeat(patch[None, :, :, None], 3, axis=3))).cuda().expand(B, 96, 80, 3)
    for sign in (1, -1):
        angles = [2.0 * sign * k for k in range(B)]
        pasted = ops.paste_resize_cubic_u8(patch.contiguous(), frames, boxes=[box] * B, angles=angles)
        state = ops.TrackState()
        geo = ops.track_seed(state, pasted[0], box, 48, angle=0.0)
        assert geo[:5] == (2, 35, 20, 40, 48)
        rows = ops.track_template_rot_u8(pasted[1:], state, search=8).cpu().tolist()
        faces = ops.track_rot_faces(rows, state)
        assert None not in faces
        for k, face in enumerate(faces, 1):
            assert abs(face[4] - 200 * sign * k) <= 200, (sign, k, face)
            assert abs(face[0] - box[0]) <= 2 and abs(face[1] - box[1]) <= 2 and face[2:4] == box[2:]
        assert faces[-1][4] * sign >= 1200


def test_the_tool_with_rotate_writes_the_restatements_track_whatever_the_batch(tmp_path):
    """16 frames of 96 x 160 at stride 2, the patch rolling 2 degrees a frame, keys at frames 1 and 9, the second with its
    angle: the track is the restatement's for batch_frames 1, 5 and 16, and rotate=False writes the plain tracker's file"""
    from denoising_diffusion_deep_fake_amd.script_tools.track_face_box import TrackFaceBox
    frames, _, gray, boxes = _rolling_on_device(2024, 16)
    keys = {k: tuple(2 * v for v in boxes[k][:4]) for k in (1, 9)}
    want = trr.tool_track(frames, keys, {9: 1800}, R=8, side=32)
    assert want[0] is None and want[1] == keys[1] + (0,) and want[9] == keys[9] + (1800,) and None not in want[1:]
    assert trr.geometry(96, 160, keys[1], 32)[0] == trr.geometry(96, 160, keys[9], 32)[0] == 2
    assert want[8][4] > 0 and want[15][4] > 1800  # the angle is followed from both keys
    texts = []
    for batch_frames in (1, 5, 16):
        path = tmp_path / f"track_{batch_frames}.txt"
        got = []
        tool = TrackFaceBox(tmp_path / "clip.mp4", [(k,) + box for k, box in keys.items()], output_path=path,
                            batch_frames=batch_frames, frames=iter(frames), sink=got.append, search=8, template_side=32,
                            rotate=True, key_angles=[(9, 18.0)])
        assert tool.track == [e and e[:4] for e in want] == got and tool.angles == [e[4] if e else 0 for e in want]
        texts.append(path.read_text())
    assert texts[0] == texts[1] == texts[2]
    lines = texts[0].splitlines()
    assert lines[3] == ("# rotation search: one step of 2.00 degrees a frame within +-60, penalty 512; fifth column: the box's "
                        "angle in degrees")
    assert lines[4] == "# key angles (frame angle): 9 18.00" and not lines[5].startswith("#")
    assert lines[5:] == ["-" if e is None else "{} {} {} {} {:.2f}".format(*e[:4], e[4] / 100.0) for e in want]
    from denoising_diffusion_deep_fake_amd import ops
    assert ops.read_rbox_track(tmp_path / "track_5.txt")[2] == want[2][:4] + (want[2][4] / 100.0,)
    # without rotate: the plain tracker's file, header included
    plain = tr.tool_track(frames, keys, R=8, side=32)
    path = tmp_path / "plain.txt"
    tool = TrackFaceBox(tmp_path / "clip.mp4", [(k,) + box for k, box in keys.items()], output_path=path, batch_frames=5,
                        frames=iter(frames), search=8, template_side=32, rotate=False)
    assert tool.track == plain and tool.angles is None
    keys_line = ", ".join("{} {} {} {} {}".format(k, *box) for k, box in keys.items())
    assert path.read_text().splitlines() == [
        "# track_face_box clip.mp4: x y w h per frame, - where the face was not found",
        f"# keys (frame x y w h): {keys_line}", "# search 8, adapt 1, lost 16, template side 32",
    ] + ["-" if box is None else "{} {} {} {}".format(*box) for box in plain]
