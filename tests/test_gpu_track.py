"""GPU: the template tracker against its restatement (tests/track_restatement.py) -- the reduced grey image, the seed, the
search, the fused entry and the tool.  Everything is integer arithmetic, so every comparison is array_equal: bytes, int32
rows, template bytes and the position."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_restatement as tr

pytestmark = pytest.mark.gpu

GUARD = 64


def _frames(seed, B, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)


def _at_odd_offset(array, offset=33):
    """the array's bytes on the device at an odd byte offset into a larger buffer, as a tensor of the array's shape"""
    flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1))
    buf = torch.zeros(flat.numel() + offset + 7, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 2 == 1
    return view.view(array.shape)


# ---- the reduced grey image ----

DECIMATE = [(1, 1, 1, 1), (5, 7, 1, 3), (37, 53, 3, 2), (64, 96, 4, 3), (33, 130, 32, 1), (40, 41, 2, 2)]


@pytest.mark.parametrize("h, w, s, B", DECIMATE)
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
def test_decimate_against_the_restatement(h, w, s, B, odd):
    from denoising_diffusion_deep_fake_amd import ops
    frames = _frames(100 * h + s, B, h, w)
    want = tr.gray_decimate(frames, s)
    dev = _at_odd_offset(frames) if odd else torch.from_numpy(frames).cuda()
    assert np.array_equal(ops.gray_decimate_u8(dev, s).cpu().numpy(), want)
    assert np.array_equal(ops.gray_decimate_u8(dev[0], s).cpu().numpy(), want[0])
    # into a buffer with guard bands, at an odd offset too: no byte outside out is written
    n = want.size
    buf = torch.full((n + 2 * GUARD + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + 1:GUARD + 1 + n].view(want.shape)
    got = ops.gray_decimate_u8(dev, s, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    host = buf.cpu().numpy()
    assert (host[:GUARD + 1] == 0xA5).all() and (host[GUARD + 1 + n:] == 0xA5).all()


def test_decimate_over_more_than_one_tile_of_columns_and_every_staging_depth():
    """262 to 301 reduced columns are two workgroups a row and 700 are three, the last one partial; strides 5, 8, 16 and 32 stage
    5, 4, 2 and 1 source rows at a time"""
    from denoising_diffusion_deep_fake_amd import ops
    for h, w, s in ((6, 301, 1), (10, 1503, 5), (17, 2403, 8), (33, 4200, 16), (64, 8999, 32), (9, 2101, 3)):
        frames = _frames(h + w, 1, h, w)
        assert np.array_equal(ops.gray_decimate_u8(_at_odd_offset(frames, 3), s).cpu().numpy(), tr.gray_decimate(frames, s)), (h, w, s)


# ---- the seed ----

@pytest.mark.parametrize("h, w, face, side", [
    (64, 96, (0, 0, 33, 21), 48),      # the top-left corner, s = 1
    (64, 96, (66, 24, 30, 40), 20),    # the bottom-right corner, s = 2
    (90, 131, (7, 5, 40, 50), 17),     # an odd origin, s = 3: ox = 1, oy = 2
    (70, 140, (1, 3, 128, 64), 64),    # s = 2, a template of 64 x 32
])
def test_seed_against_the_restatement(h, w, face, side):
    from denoising_diffusion_deep_fake_amd import ops
    frame = _frames(h * w, 1, h, w)[0]
    geo = tr.geometry(h, w, face, side)
    s, tx, ty, tw, th = geo[:5]
    T, pos = tr.seed(tr.gray_decimate(frame, s), tx, ty, tw, th)
    for dev in (torch.from_numpy(frame).cuda(), _at_odd_offset(frame)):
        state = ops.TrackState()
        state.templ.fill_(0xA5)
        assert ops.track_seed(state, dev, face, side) == geo and state.seeded and state.geometry == geo
        templ = state.templ.cpu().numpy()
        assert np.array_equal(templ[:tw * th].reshape(th, tw), T) and (templ[tw * th:] == 0xA5).all()
        assert tuple(state.pos.cpu().tolist()) == pos


# ---- the search ----

def _search(gray, T, pos, R, adapt, lost, odd=False):
    """d3f_track_search_u8 on host arrays -> (T, pos, rows) as the restatement returns them; the bytes of the template
    buffer behind T and the int32 around pos and the rows are guard bands"""
    from denoising_diffusion_deep_fake_amd import _lib
    B, gh, gw = gray.shape
    th, tw = T.shape
    if B == 0:
        g = torch.zeros(1, dtype=torch.uint8, device="cuda")  # (an empty tensor has no pointer to hand over)
    else:
        g = _at_odd_offset(gray) if odd else torch.from_numpy(gray).cuda()
    templ = torch.full((64 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    templ[:tw * th] = torch.from_numpy(T.reshape(-1)).cuda()
    ints = torch.full((4 + 2 + 4 + 4 * B + 4,), -77, dtype=torch.int32, device="cuda")
    ints[4:6] = torch.tensor(pos, dtype=torch.int32)
    p, o = ints.data_ptr() + 16, ints.data_ptr() + 40
    _lib.check(_lib.lib().d3f_track_search_u8(C.c_void_p(g.data_ptr()), B, gh, gw, tw, th, R, adapt, lost, _lib.ptr(templ),
                                              C.c_void_p(p), C.c_void_p(o), _lib.stream_ptr()))
    host, t = ints.cpu().numpy(), templ.cpu().numpy()
    assert (host[:4] == -77).all() and (host[6:10] == -77).all() and (host[10 + 4 * B:] == -77).all()
    assert (t[tw * th:] == 0xA5).all()
    return t[:tw * th].reshape(th, tw), (int(host[4]), int(host[5])), host[10:10 + 4 * B].reshape(B, 4)


def _drifting(seed, B, gh, gw, noise=3):
    """a random image that drifts by (2, -3) a frame under noise of a few levels: frame k's content is frame 0's, moved"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(gh, gw))
    out = [np.clip(np.roll(base, (2 * k, -3 * k), axis=(0, 1)) + rng.integers(-noise, noise + 1, size=base.shape), 0, 255)
           for k in range(B)]
    return np.stack(out).astype(np.uint8)


def _check(gray, T, pos, R, adapt, lost, odd=False, want=None):
    want = want or tr.search(gray, T, pos, R, adapt, lost)
    got = _search(gray, T, pos, R, adapt, lost, odd)
    assert np.array_equal(got[2], want[2]), (got[2].tolist(), want[2].tolist())
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    return want


SEARCH = [
    # tw, th, R, gh, gw, pos, adapt, lost
    (4, 4, 1, 9, 11, (3, 2), 1, 16),
    (4, 4, 16, 40, 51, (20, 18), 1, 16),
    (13, 7, 16, 50, 61, (30, 20), 1, 16),
    (13, 7, 64, 90, 101, (40, 30), 1, 255),
    (64, 64, 1, 70, 83, (5, 3), 1, 16),
    (64, 64, 16, 100, 131, (30, 20), 1, 16),
    (64, 64, 64, 200, 211, (70, 66), 1, 16),     # the whole 192 x 192 window
    (5, 64, 16, 80, 37, (12, 9), 1, 16),
    (5, 64, 64, 80, 150, (100, 8), 8, 255),
    (13, 7, 16, 50, 61, (0, 0), 1, 16),          # a corner: the candidates are clipped on two sides
    (13, 7, 16, 50, 61, (48, 43), 1, 16),        # the opposite corner
    (13, 7, 16, 50, 13, (0, 20), 1, 16),         # gw == tw: one column of candidates
    (64, 64, 64, 64, 64, (0, 0), 1, 16),         # the image is the template: one candidate
    (13, 7, 16, 50, 61, (30, 20), 0, 16),
    (13, 7, 16, 50, 61, (30, 20), 8, 16),
    (13, 7, 16, 50, 61, (30, 20), 1, 0),         # lost 0: found only at cost 0
    (13, 7, 16, 50, 61, (30, 20), 3, 255),       # lost 255: always found
    (30, 31, 16, 64, 66, (10, 12), 1, 16),       # tw = 2 mod 4
    (31, 30, 8, 64, 67, (10, 12), 2, 16),        # tw = 3 mod 4
]


@pytest.mark.parametrize("tw, th, R, gh, gw, pos, adapt, lost", SEARCH)
def test_search_against_the_restatement(tw, th, R, gh, gw, pos, adapt, lost):
    gray = _drifting(tw * 1000 + th * 10 + R, 2 if gh >= 200 else 3, gh, gw)
    T = tr.seed(gray[0], pos[0], pos[1], tw, th)[0]
    want = tr.search(gray, T, pos, R, adapt, lost)
    rows = want[2]
    for odd in (False, True):
        _check(gray, T, pos, R, adapt, lost, odd, want)
    if lost == 255:
        assert rows[:, 3].all()
    if (tw, th, R, pos, adapt, lost) == (13, 7, 16, (30, 20), 1, 16):  # the drift is followed: (-3, 2) a frame
        assert rows[:, :2].tolist() == [[30, 20], [27, 22], [24, 24]] and rows[:, 3].all()  # (13, 7, 16 is 3 frames)


def test_search_on_a_constant_image_stays_where_it_is():
    gray = np.full((3, 40, 50), 77, dtype=np.uint8)
    T = np.full((7, 13), 77, dtype=np.uint8)
    for R in (1, 16, 64):
        T1, pos, rows = _check(gray, T, (11, 9), R, 1, 0)
        assert pos == (11, 9) and rows.tolist() == [[11, 9, 0, 1]] * 3
    # every candidate costs the same, and not 0: still no displacement; lost 0 says not found
    T1, pos, rows = _check(gray, T + 1, (11, 9), 16, 1, 0)
    assert pos == (11, 9) and rows.tolist() == [[11, 9, 91, 0]] * 3


def test_search_ties_go_to_the_smaller_displacement_then_dy_then_dx():
    T = np.full((4, 4), 200, dtype=np.uint8)
    gray = np.zeros((4, 24, 24), dtype=np.uint8)
    for k, marks in enumerate([[(15, 10), (6, 10)], [(6, 14), (6, 6), (10, 10), (2, 10)], [(10, 6), (2, 6)],
                               [(5, 2), (-1, 2), (6, 9)]]):
        for x, y in marks:  # relative to where the previous frame's winner left the position
            if x >= 0:
                gray[k, y:y + 4, x:x + 4] = 200
    rows = _check(gray, T, (10, 10), 8, 0, 255)[2]
    assert rows[:, :3].tolist() == [[6, 10, 0], [6, 6, 0], [2, 6, 0], [5, 2, 0]]


def test_search_through_the_recipe_with_an_absent_frame_mid_call():
    frames, positions = tr.moving_patch_frames(77, 10, 96, 160, 2, 3, absent=(4,), patch=(12, 10))
    gray = tr.gray_decimate(frames, 2)
    T, pos = tr.seed(gray[0], positions[0][0], positions[0][1], 10, 12)
    T1, pos1, rows = _check(gray[1:], T, pos, 8, 1, 16)
    assert rows[:, 3].tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert [tuple(r) for r in rows[:, :2].tolist()] == positions[1:4] + [positions[3]] + positions[5:]


def test_search_of_no_frames_touches_nothing():
    gray = np.zeros((0, 40, 50), dtype=np.uint8)
    T = np.arange(91, dtype=np.uint8).reshape(7, 13)
    T1, pos, rows = _search(gray, T, (3, 4), 16, 8, 255)
    assert np.array_equal(T1, T) and pos == (3, 4) and rows.shape == (0, 4)


# ---- the Python entries: call cutting, the fused call ----

def _recipe_on_device(seed, B, s, absent=()):
    patch = (24 // s, 20 // s)
    frames, positions = tr.moving_patch_frames(seed, B, 96, 160, s, 3, absent=absent, patch=patch)
    face = (positions[0][0] * s, positions[0][1] * s, patch[1] * s, patch[0] * s)
    return frames, torch.from_numpy(frames).cuda(), face, positions


@pytest.mark.parametrize("s", [1, 2])
def test_cutting_a_call_changes_nothing(s):
    """9 frames as one call, as nine and as 4 + 5: the same rows and the same final state"""
    from denoising_diffusion_deep_fake_amd import ops
    frames, dev, face, positions = _recipe_on_device(31 + s, 10, s, absent=(6,))
    side = 24 // s  # the longer side of the face over the stride: a stride of s
    results = []
    for cuts in ([9], [1] * 9, [4, 5]):
        state = ops.TrackState()
        assert ops.track_seed(state, dev[0], face, side)[0] == s
        rows, at = [], 1
        for n in cuts:
            rows.append(ops.track_template_u8(dev[at:at + n], state, search=8))
            at += n
        results.append((torch.cat(rows).cpu().numpy(), state.templ.cpu().numpy(), state.pos.cpu().numpy()))
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    geo = tr.geometry(96, 160, face, side)
    T, pos = tr.seed(tr.gray_decimate(frames[0], s), *geo[1:5])
    T1, pos1, rows = tr.search(tr.gray_decimate(frames[1:], s), T, pos, 8, ops.TRACK_ADAPT, ops.TRACK_LOST)
    assert np.array_equal(results[0][0], rows) and tuple(results[0][2]) == pos1
    assert np.array_equal(results[0][1][:T1.size].reshape(T1.shape), T1)
    assert rows[:, 3].tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1]
    assert ops.track_faces(rows.tolist(), state) == tr.faces(rows, geo)


def test_the_fused_entry_is_decimate_then_search():
    from denoising_diffusion_deep_fake_amd import ops
    frames, dev, face, _ = _recipe_on_device(5, 6, 2)
    fused, parts = ops.TrackState(), ops.TrackState()
    for state in (fused, parts):
        geo = ops.track_seed(state, dev[0], face, 12)
    s, _, _, tw, th = geo[:5]
    rows = ops.track_template_u8(dev[1:], fused, search=8, adapt=2, lost=20)
    gray = ops.gray_decimate_u8(dev[1:], s).cpu().numpy()
    T = parts.templ.cpu().numpy()[:tw * th].reshape(th, tw)
    T1, pos1, want = _search(gray, T, tuple(parts.pos.cpu().tolist()), 8, 2, 20)
    assert np.array_equal(rows.cpu().numpy(), want) and tuple(fused.pos.cpu().tolist()) == pos1
    assert np.array_equal(fused.templ.cpu().numpy()[:tw * th].reshape(th, tw), T1)
    assert rows.dtype == torch.int32 and rows.shape == (5, 4) and rows.is_cuda
    assert ops.track_template_u8(dev[:0], fused).shape == (0, 4)
    with pytest.raises(ValueError, match="seeded"):
        ops.track_template_u8(dev, ops.TrackState())
    with pytest.raises(ValueError, match="seeded on"):
        ops.track_template_u8(dev[:, :90], fused)


# ---- the tool ----

def test_the_tool_writes_the_restatements_track_whatever_the_batch(tmp_path):
    """24 frames of 96 x 160, the patch absent from frame 9, keys at frames 2 and 13 (the second one moved by hand: a
    correction): frames 0 and 1 are `-`, the key frames carry the key's box, and the file does not depend on batch_frames"""
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.track_face_box import TrackFaceBox
    frames, positions = tr.moving_patch_frames(2024, 24, 96, 160, 1, 3, absent=(9,), patch=(24, 20))
    keys = {2: (positions[2][0], positions[2][1], 20, 24), 13: (positions[13][0] - 1, positions[13][1], 22, 24)}
    want = tr.tool_track(frames, keys, R=8)
    assert want[:2] == [None, None] and want[2] == keys[2] and want[13] == keys[13] and want[9] is None
    assert [w[:2] for w in want[3:9]] == positions[3:9] and sum(w is None for w in want) == 3
    texts = []
    for batch_frames in (1, 3, 8):
        path = tmp_path / f"track_{batch_frames}.txt"
        got = []
        tool = TrackFaceBox(tmp_path / "clip.mp4", [(k,) + box for k, box in keys.items()], output_path=path,
                            batch_frames=batch_frames, frames=iter(frames), sink=got.append, search=8)
        assert tool.track == want and got == want
        texts.append(path.read_text())
    assert texts[0] == texts[1] == texts[2]
    lines = [line for line in texts[0].splitlines() if not line.startswith("#")]
    assert lines == ["-" if box is None else "{} {} {} {}".format(*box) for box in want]
    track = ops.read_box_track(tmp_path / "track_3.txt")
    assert len(track) == 24 and track[0] == track[2] == want[2] and track[9] == want[8]
    boxes = ops.track_crop_boxes(track, 0, 24, 96, 160, 64, 64)
    assert len(boxes) == 24 and all(x >= 0 and y >= 0 and x + cw <= 160 and y + ch <= 96 for x, y, cw, ch in boxes)


def test_the_three_commands_of_the_workflow_run_end_to_end(tmp_path):
    """INTEGRATION.md's order through the frames= and sink= hooks: track the face, cut the training images at its boxes,
    render --output full --track: the render pastes inside the tracked box of every frame and leaves the rest as it was"""
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    from denoising_diffusion_deep_fake_amd.script_tools.track_face_box import TrackFaceBox
    from denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images import VideoToImages
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    frames, positions = tr.moving_patch_frames(99, 6, 96, 160, 1, 3, patch=(24, 20))
    track_path = tmp_path / "clip_track.txt"
    tool = TrackFaceBox(tmp_path / "clip.mp4", [(0, positions[0][0], positions[0][1], 20, 24)], batch_frames=4,
                        frames=iter(frames), search=8)
    assert tool.output_path == track_path and [box[:2] for box in tool.track] == positions
    images = VideoToImages(tmp_path / "clip.mp4", 64, 64, batch_frames=4, frames=iter(frames), track=str(track_path))
    assert len((images.output_dir_path / "images.txt").read_text().splitlines()) == 6
    torch.manual_seed(6)
    lit = LitModule(precision="f32", mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999,
                    max_epochs=1, cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet18",
                    noise_exponential_sampling_lambda=3, mean_a=[0.4, 0.5, 0.6], std_a=[0.5, 0.45, 0.55],
                    mean_b=[0.45, 0.4, 0.55], std_b=[0.6, 0.5, 0.4], synthetic=True, image_size=64, synthetic_length=4,
                    ema_beta=0.9999, ema_update_every=1, augment=False).cuda().eval()
    got = []
    RenderFakeVideo("clip.mp4", None, "a", 64, 64, batch_frames=4, frames=iter(frames), sink=got.append, model=lit,
                    output="full", track=str(track_path))
    assert len(got) == 6
    boxes = ops.track_crop_boxes(ops.read_box_track(track_path), 0, 6, 96, 160, 64, 64)
    assert len(set(boxes)) > 1, "the crop follows the face"
    for k, (x, y, cw, ch) in enumerate(boxes):
        changed = got[k] != frames[k]
        assert changed[y:y + ch, x:x + cw].any()
        changed[y:y + ch, x:x + cw] = False
        assert not changed.any(), k
