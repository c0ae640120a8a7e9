"""GPU: the template tracker's re-acquisition against its restatement (tests/track_reacq_restatement.py) -- the whole-frame
search, the serial search that takes a lost frame from it, the fused entry, the Python entries and the tool.  Everything
is integer arithmetic, so every comparison is array_equal: keys, int32 rows, template bytes and the position.  The
whole-frame kernel takes tiles of 16 x 8 candidate positions; the shapes below are chosen around that."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_reacq_restatement as rr
import track_restatement as tr

pytestmark = pytest.mark.gpu

GUARD = 64
TILE_X, TILE_Y = 16, 8


def _with_guards(array, offset):
    """the array's bytes on the device between two guard bands of 0xA5, `offset` bytes (odd: an odd byte address) into the
    buffer -> (the buffer, the view of the array's shape)"""
    flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1))
    buf = torch.full((flat.numel() + offset + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 2 == offset % 2
    return buf, view.view(array.shape)


def _guards_hold(buf, array, offset):
    host = buf.cpu().numpy()
    n = array.size
    assert (host[:offset] == 0xA5).all() and (host[offset + n:] == 0xA5).all()
    assert np.array_equal(host[offset:offset + n], np.ascontiguousarray(array).reshape(-1))


def _templ_buffer(T):
    buf = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:T.size] = torch.from_numpy(np.ascontiguousarray(T).reshape(-1)).cuda()
    return buf


def _global(gray, K, odd=False):
    """d3f_track_global_u8 on host arrays -> the keys as Python integers; the grey buffer, the key template and the keys lie
    between guard bands, and the first two come back as they went in"""
    from denoising_diffusion_deep_fake_amd import _lib
    B, gh, gw = gray.shape
    th, tw = K.shape
    offset = GUARD + 1 if odd else GUARD
    gbuf, g = _with_guards(gray if B else np.zeros((1,), dtype=np.uint8), offset)
    kt = _templ_buffer(K)
    keys = torch.full((2 + B + 2,), -77, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().d3f_track_global_u8(C.c_void_p(g.data_ptr()), B, gh, gw, tw, th, _lib.ptr(kt),
                                              C.c_void_p(keys.data_ptr() + 16), _lib.stream_ptr()))
    host = keys.cpu().numpy()
    assert (host[:2] == -77).all() and (host[2 + B:] == -77).all()
    if B:
        _guards_hold(gbuf, gray, offset)
    t = kt.cpu().numpy()
    assert np.array_equal(t[:tw * th].reshape(th, tw), K) and (t[tw * th:] == 0xA5).all()
    return [int(v) for v in host[2:2 + B]]


def _check_global(gray, K):
    want = rr.global_keys(gray, K)
    for odd in (False, True):
        got = _global(gray, K, odd)
        assert got == want, ([rr.decode(k) for k in got], [rr.decode(k) for k in want])
    return want


def _random(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---- the whole-frame search ----

GLOBAL = [
    # tw, th, gh, gw, B
    (9, 7, 40, 53, 2),     # tw no multiple of 4, an odd gw: the rows lie at every byte phase
    (64, 64, 64, 64, 2),   # the image is the template: one candidate
    (64, 64, 70, 131, 1),  # the largest template, 7 x 68 candidates
    (13, 7, 50, 13, 2),    # gw == tw: one column of candidates
    (7, 13, 13, 50, 2),    # gh == th: one row of them
    (9, 7, 2 * TILE_Y + 7, 2 * TILE_X + 9, 2),          # 33 x 17 candidates: one more than two tiles on each axis
    (9, 7, 2 * TILE_Y + 5, 2 * TILE_X + 7, 2),          # 31 x 15: one fewer
    (30, 31, 45, 66, 1),   # tw = 2 mod 4
    (31, 5, 20, 67, 1),    # tw = 3 mod 4; th below the eight parts of a group
    (4, 4, 4, 5, 1),       # the smallest template, two candidates
]


@pytest.mark.parametrize("tw, th, gh, gw, B", GLOBAL)
def test_global_against_the_restatement(tw, th, gh, gw, B):
    """random images, the template a noisy cut of the first one: the first frame's winner is the cut's place, the others'
    wherever chance puts it"""
    gray = _random(1000 * tw + 10 * th + gw, B, gh, gw)
    x, y = (gw - tw) // 2, (gh - th) // 3
    noise = np.random.default_rng(7).integers(-3, 4, size=(th, tw))
    K = np.clip(gray[0, y:y + th, x:x + tw].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    want = _check_global(gray, K)
    assert rr.decode(want[0])[1:] == (x, y)


def test_global_with_a_different_winner_in_every_frame():
    """B = 3, an exact copy of the template planted per frame: the first candidate, one in the middle of a tile, and the very
    last candidate, alone in the last partial tile of both axes (38 x 19 candidates: tiles of 16 + 16 + 6 by 8 + 8 + 3)"""
    tw, th, gh, gw = 12, 10, 28, 49
    gray = _random(5, 3, gh, gw)
    K = _random(6, th, tw)
    places = [(0, 0), (21, 11), (gw - tw, gh - th)]
    assert places[2] == (37, 18)
    for b, (x, y) in enumerate(places):
        gray[b, y:y + th, x:x + tw] = K
    want = _check_global(gray, K)
    assert [rr.decode(k) for k in want] == [(0, x, y) for x, y in places]


def test_global_on_a_constant_image_and_with_two_exact_copies():
    K = _random(8, 7, 9)
    const = np.full((2, 30, 45), 77, dtype=np.uint8)
    cost = int(np.abs(K.astype(np.int64) - 77).sum())
    assert _check_global(const, K) == [cost << 32] * 2  # (cost, 0, 0)
    # two exact copies: the top-most wins whatever its column; in one row of candidates the left-most; tiles apart each time
    gray = _random(9, 2, 30, 45)
    gray[0, 20:27, 3:12] = K
    gray[0, 4:11, 30:39] = K
    gray[1, 12:19, 33:42] = K
    gray[1, 12:19, 2:11] = K
    assert [rr.decode(k) for k in _check_global(gray, K)] == [(0, 30, 4), (0, 2, 12)]


def test_global_of_no_frames_touches_nothing():
    assert _global(np.zeros((0, 40, 50), dtype=np.uint8), _random(1, 7, 13)) == []


def test_the_python_entry_returns_the_keys_as_int64():
    from denoising_diffusion_deep_fake_amd import ops
    gray = _random(21, 2, 33, 47)
    K = _random(22, 9, 11)
    want = rr.global_keys(gray, K)
    kt = _templ_buffer(K)
    keys = ops.track_global_u8(torch.from_numpy(gray).cuda(), kt, 11, 9)
    assert keys.dtype == torch.int64 and keys.shape == (2,) and keys.is_cuda and keys.tolist() == want
    assert [(k >> 32, k & 0xffff, (k >> 16) & 0xffff) for k in keys.tolist()] == [rr.decode(k) for k in want]
    assert ops.track_global_u8(torch.from_numpy(gray[1]).cuda(), kt, 11, 9).tolist() == want[1:]
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert ops.track_global_u8(torch.from_numpy(gray).cuda(), kt, 11, 9, out=out).data_ptr() == out.data_ptr()
    assert out.tolist() == want
    assert ops.track_global_u8(torch.from_numpy(gray[:0]).cuda(), kt, 11, 9).shape == (0,)


# ---- the serial form ----

def _search_reacq(gray, T, K, pos, keys, R, adapt, lost, relost):
    """d3f_track_search_reacq_u8 on host arrays -> (T, pos, rows) as the restatement returns them; the bytes behind either
    template and the int32 around pos and the rows are guard bands, K and the keys come back as they went in"""
    from denoising_diffusion_deep_fake_amd import _lib
    B, gh, gw = gray.shape
    th, tw = T.shape
    gbuf, g = _with_guards(gray, GUARD + 1)
    templ, kt = _templ_buffer(T), _templ_buffer(K)
    k = torch.tensor([-77] + list(keys) + [-77], dtype=torch.int64, device="cuda")
    ints = torch.full((4 + 2 + 4 + 4 * B + 4,), -77, dtype=torch.int32, device="cuda")
    ints[4:6] = torch.tensor(pos, dtype=torch.int32)
    p, o = ints.data_ptr() + 16, ints.data_ptr() + 40
    _lib.check(_lib.lib().d3f_track_search_reacq_u8(C.c_void_p(g.data_ptr()), B, gh, gw, tw, th, R, adapt, lost, relost,
                                                    _lib.ptr(templ), _lib.ptr(kt), C.c_void_p(p), C.c_void_p(k.data_ptr() + 8),
                                                    C.c_void_p(o), _lib.stream_ptr()))
    host, t, kh = ints.cpu().numpy(), templ.cpu().numpy(), kt.cpu().numpy()
    assert (host[:4] == -77).all() and (host[6:10] == -77).all() and (host[10 + 4 * B:] == -77).all()
    assert (t[tw * th:] == 0xA5).all() and np.array_equal(kh[:tw * th].reshape(th, tw), K) and (kh[tw * th:] == 0xA5).all()
    assert k.tolist() == [-77] + list(keys) + [-77]
    _guards_hold(gbuf, gray, GUARD + 1)
    return t[:tw * th].reshape(th, tw), (int(host[4]), int(host[5])), host[10:10 + 4 * B].reshape(B, 4)


@pytest.fixture(scope="module")
def recipe():
    """the teleporting patch, seed 0: (frames, positions, gray, K, the keys of frames 1..23, the restatement's (T, pos, rows)
    of frames 1..23): computed once, never changed"""
    frames, positions = rr.teleporting_patch_frames(0)
    gray = tr.gray_decimate(frames, 1)
    K, pos = tr.seed(gray[0], positions[0][0], positions[0][1], rr.PATCH[1], rr.PATCH[0])
    keys = rr.global_keys(gray[1:], K)
    want = rr.search_reacq(gray[1:], K.copy(), K, pos, rr.SEARCH, rr.ADAPT, rr.LOST, rr.RELOST, keys)
    assert [k for k, row in enumerate(want[2].tolist(), 1) if row[3] == 2] == list(rr.JUMPS)
    assert [k for k, row in enumerate(want[2].tolist(), 1) if row[3] == 0] == list(rr.ABSENT)
    return frames, positions, gray, K, keys, want


def _face(positions):
    return (positions[0][0], positions[0][1], rr.PATCH[1], rr.PATCH[0])


def _seeded(dev, positions):
    from denoising_diffusion_deep_fake_amd import ops
    state = ops.TrackState()
    geo = ops.track_seed(state, dev[0], _face(positions), reacquire=True)
    assert geo[:5] == (1, positions[0][0], positions[0][1], rr.PATCH[1], rr.PATCH[0])
    return state


def _state(state, n):
    return state.templ.cpu().numpy()[:n], tuple(state.pos.cpu().tolist())


def test_the_serial_search_on_the_recipe_row_for_row(recipe):
    frames, positions, gray, K, keys, want = recipe
    assert _global(gray[1:], K, odd=True) == keys
    T1, pos1, rows = _search_reacq(gray[1:], K.copy(), K, positions[0], keys, rr.SEARCH, rr.ADAPT, rr.LOST, rr.RELOST)
    assert np.array_equal(rows, want[2]), (rows.tolist(), want[2].tolist())
    assert pos1 == want[1] and np.array_equal(T1, want[0])


def test_the_python_entry_on_the_recipe_and_cut_at_every_third_frame(recipe):
    from denoising_diffusion_deep_fake_amd import ops
    frames, positions, gray, K, keys, want = recipe
    dev = torch.from_numpy(frames).cuda()
    results = []
    for cuts in ([23], [3] * 7 + [2], [1] * 23):
        state = _seeded(dev, positions)
        assert np.array_equal(state.key_templ.cpu().numpy()[:K.size].reshape(K.shape), K)
        rows, at = [], 1
        for n in cuts:
            rows.append(ops.track_template_reacq_u8(dev[at:at + n], state, rr.SEARCH, rr.ADAPT, rr.LOST))
            at += n
        assert rows[0].dtype == torch.int32 and rows[0].shape == (cuts[0], 4) and rows[0].is_cuda
        results.append((torch.cat(rows).cpu().numpy(),) + _state(state, K.size))
        assert np.array_equal(state.key_templ.cpu().numpy()[:K.size].reshape(K.shape), K)  # never adapted
    for got in results:
        assert np.array_equal(got[0], want[2]), (got[0].tolist(), want[2].tolist())
        assert got[2] == want[1] and np.array_equal(got[1].reshape(K.shape), want[0])
    geo = state.geometry
    assert ops.track_faces(want[2].tolist(), state) == tr.faces([r[:3] + [1 if r[3] else 0] for r in want[2].tolist()], geo)
    assert ops.track_template_reacq_u8(dev[:0], state).shape == (0, 4)
    plain = ops.TrackState()
    ops.track_seed(plain, dev[0], _face(positions))
    assert plain.key_templ is None
    with pytest.raises(ValueError, match="without reacquire=True"):
        ops.track_template_reacq_u8(dev[1:], plain)
    with pytest.raises(ValueError, match="reacquire=True with angle="):
        ops.track_seed(plain, dev[0], _face(positions), angle=0.0, reacquire=True)
    ops.track_seed(state, dev[0], _face(positions))  # every seed replaces the key template: this one by none
    assert state.key_templ is None


def test_the_fused_entry_is_its_three_parts(recipe):
    from denoising_diffusion_deep_fake_amd import ops
    frames, positions, gray, K, keys, want = recipe
    dev = torch.from_numpy(frames).cuda()
    state = _seeded(dev, positions)
    rows = ops.track_template_reacq_u8(dev[1:13], state, rr.SEARCH, 2, 20, 9)
    g = ops.gray_decimate_u8(dev[1:13], 1)
    assert np.array_equal(g.cpu().numpy(), gray[1:13])
    k = ops.track_global_u8(g, _templ_buffer(K), rr.PATCH[1], rr.PATCH[0]).tolist()
    assert k == keys[:12]
    T1, pos1, parts = _search_reacq(gray[1:13], K.copy(), K, positions[0], k, rr.SEARCH, 2, 20, 9)
    assert np.array_equal(rows.cpu().numpy(), parts) and 2 in parts[:, 3] and 0 in parts[:, 3]
    t, pos = _state(state, K.size)
    assert pos == pos1 and np.array_equal(t.reshape(K.shape), T1)
    assert np.array_equal(parts, rr.search_reacq(gray[1:13], K.copy(), K, positions[0], rr.SEARCH, 2, 20, 9, keys[:12])[2])


def test_after_a_re_acquired_frame_the_template_is_the_key_template(recipe):
    from denoising_diffusion_deep_fake_amd import ops
    frames, positions, gray, K, keys, want = recipe
    dev = torch.from_numpy(frames).cuda()
    state = _seeded(dev, positions)
    rows = ops.track_template_reacq_u8(dev[1:6], state, rr.SEARCH, rr.ADAPT, rr.LOST).cpu().numpy()
    assert rows[:, 3].tolist() == [1] * 5
    assert not torch.equal(state.templ, state.key_templ), "five frames of adapt = 1 have moved the template"
    rows = ops.track_template_reacq_u8(dev[6:7], state, rr.SEARCH, rr.ADAPT, rr.LOST).cpu().numpy()
    assert rows.tolist() == [[positions[6][0], positions[6][1], rr.decode(keys[5])[0], 2]]
    assert torch.equal(state.templ, state.key_templ) and tuple(state.pos.tolist()) == positions[6]


def test_relost_0_gives_the_plain_rows(recipe):
    """the frames are noisy, so no place costs 0: nothing is re-acquired, and the rows, the template and the position are
    the plain search's"""
    from denoising_diffusion_deep_fake_amd import ops
    frames, positions, gray, K, keys, want = recipe
    dev = torch.from_numpy(frames).cuda()
    state, plain = _seeded(dev, positions), ops.TrackState()
    ops.track_seed(plain, dev[0], _face(positions))
    rows = ops.track_template_reacq_u8(dev[1:], state, rr.SEARCH, rr.ADAPT, rr.LOST, 0).cpu().numpy()
    want_plain = tr.search(gray[1:], K.copy(), positions[0], rr.SEARCH, rr.ADAPT, rr.LOST)
    assert np.array_equal(rows, want_plain[2]) and 2 not in rows[:, 3] and 0 in rows[:, 3]
    assert np.array_equal(rows, ops.track_template_u8(dev[1:], plain, rr.SEARCH, rr.ADAPT, rr.LOST).cpu().numpy())
    assert torch.equal(state.templ, plain.templ) and torch.equal(state.pos, plain.pos)


def test_the_plain_entries_before_and_after_a_re_acquiring_call(recipe):
    from denoising_diffusion_deep_fake_amd import ops
    frames, positions, gray, K, keys, want = recipe
    dev = torch.from_numpy(frames).cuda()

    def plain_run():
        state = ops.TrackState()
        ops.track_seed(state, dev[0], _face(positions))
        rows = ops.track_template_u8(dev[1:], state, rr.SEARCH, rr.ADAPT, rr.LOST).cpu().numpy()
        scale = ops.TrackState()
        ops.track_seed(scale, dev[0], _face(positions))
        rows_scale = ops.track_template_scale_u8(dev[1:9], scale, rr.SEARCH, rr.ADAPT, rr.LOST).cpu().numpy()
        return rows, state.templ.cpu().numpy(), state.pos.cpu().numpy(), rows_scale

    before = plain_run()
    state = _seeded(dev, positions)
    assert np.array_equal(ops.track_template_reacq_u8(dev[1:], state, rr.SEARCH, rr.ADAPT, rr.LOST).cpu().numpy(), want[2])
    after = plain_run()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(before[0], tr.search(gray[1:], K.copy(), positions[0], rr.SEARCH, rr.ADAPT, rr.LOST)[2])


# ---- the tool ----

def test_the_tool_with_reacquire_writes_the_restatements_track_whatever_the_batch(recipe, tmp_path):
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.track_face_box import TrackFaceBox
    frames, positions, gray, K, keys, _ = recipe
    boxes = {0: _face(positions)}
    want, flags = rr.tool_track(frames, boxes, R=rr.SEARCH)
    assert [w[:2] if w else None for w in want] == [None if k in rr.ABSENT else positions[k] for k in range(rr.FRAMES)]
    assert [k for k, f in enumerate(flags) if f == 2] == list(rr.JUMPS)
    texts = []
    for batch_frames in (1, 5, 24):
        path = tmp_path / f"track_{batch_frames}.txt"
        got = []
        tool = TrackFaceBox(tmp_path / "clip.mp4", [(0,) + boxes[0]], output_path=path, batch_frames=batch_frames,
                            frames=iter(frames), sink=got.append, search=rr.SEARCH, reacquire=ops.TRACK_RELOST)
        assert tool.track == want and got == want and tool.reacquired == 3
        assert tool.summary() == "24 frames: 18 found, 3 re-acquired, 3 lost"
        texts.append(path.read_text())
    assert texts[0] == texts[1] == texts[2]
    lines = texts[0].splitlines()
    assert [line for line in lines if not line.startswith("#")] == ["-" if b is None else "{} {} {} {}".format(*b) for b in want]
    assert any("re-acquisition" in line for line in lines if line.startswith("#"))
    # without the flag the same frames lose the face at the first jump, and the file says nothing of re-acquisition
    plain = TrackFaceBox(tmp_path / "clip.mp4", [(0,) + boxes[0]], output_path=tmp_path / "plain.txt", batch_frames=5,
                         frames=iter(frames), search=rr.SEARCH)
    assert plain.track == tr.tool_track(frames, boxes, R=rr.SEARCH) and plain.track[6] is None
    assert "re-acquisition" not in (tmp_path / "plain.txt").read_text()
