"""GPU: rotated crop boxes through the crop kernels (u8 and the fused activation form, staged and from global memory), the
paste (plain, colour, in place), the engine's two rboxes entries and both tools.  The oracle is tests/rotation_restatement.py
in its float32 form, which follows the kernels operation for operation: every comparison is torch.equal unless it says
otherwise.  One oracle is not the restatement: at 90 / 180 / 270 degrees with a box twice the output, the rotated crop is
np.rot90 of the crop the axis-aligned kernel makes -- that pins the sign convention against code that predates rotation."""
import ctypes as C

import numpy as np
import pytest
import torch

import rotation_restatement as R

pytestmark = pytest.mark.gpu

HW = (48, 64)
ANGLES = [7.5, -33.0, 90.0, 179.99]
# two boxes touch two frame edges each (their rotated corners leave the frame: taps clamp to the frame); the last has angle 0
CROP_BOXES = [(0, 0, 40, 30), (24, 18, 40, 30), (10, 8, 24, 24), (30, 0, 34, 40), (5, 5, 37, 29)]
CROP_ANGLES = ANGLES + [0.0]

RESIZE_LDS_BYTES, TW, TH = 32 * 1024, 32, 8


def _frames(seed, B, hw):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(B,) + hw + (3,), dtype=np.uint8)).cuda()


def _crop_want(frames, boxes, angles, size):
    f = frames.cpu().numpy()
    return torch.from_numpy(np.stack([R.round_u8(R.rot_crop(f[b], boxes[b], R.box_rotation(angles[b]), size))
                                      for b in range(len(boxes))]))


def _crop_lds(box, angle, hw, size):
    """rot_crop_launch_one's bound (csrc/resize.hip): rows * pitch of the largest footprint a tile of this box may stage"""
    c16, s16 = (abs(v) for v in R.box_rotation(angle))
    H, W = size
    du, dv, den = (TW - 1) * box[2] * H, (TH - 1) * box[3] * W, 65536 * W * H
    cols = min((c16 * du + s16 * dv) // den + 5, hw[1])
    rows = min((s16 * du + c16 * dv) // den + 5, hw[0])
    return rows * ((cols * 3 + 6) // 4 * 4)


def _rot_crop_one(frame, box, angle, size):
    """one frame through the rotated entry itself (ops sends an angle of zero to the boxes entry)"""
    from denoising_diffusion_deep_fake_amd import _lib
    out = torch.empty((1,) + size + (3,), dtype=torch.uint8, device="cuda")
    frame = frame.contiguous()
    _lib.check(_lib.lib().d3f_crop_resize_cubic_rboxes_u8(_lib.ptr(frame), 1, frame.shape[0], frame.shape[1],
                                                          (C.c_int32 * 4)(*box), (C.c_int32 * 2)(*R.box_rotation(angle)),
                                                          _lib.ptr(out), size[0], size[1], 3 * size[1], _lib.stream_ptr()))
    return out


# ---- the crop ----

@pytest.mark.parametrize("size", [(16, 16), (16, 24)])
def test_rotated_crop_equals_the_restatement(size):
    from denoising_diffusion_deep_fake_amd import ops
    frames = _frames(900, 5, HW)
    want = _crop_want(frames, CROP_BOXES, CROP_ANGLES, size)
    assert len({bytes(w.numpy()) for w in want}) == 5
    got = ops.crop_resize_cubic_u8(frames, size, boxes=CROP_BOXES, angles=CROP_ANGLES)
    assert got.shape == (5,) + size + (3,) and torch.equal(got.cpu(), want)
    assert max(_crop_lds(b, a, HW, size) for b, a in zip(CROP_BOXES, CROP_ANGLES)) <= RESIZE_LDS_BYTES  # staged
    # the rotation moves something: the same boxes without angles give other bytes on every turned frame
    plain = ops.crop_resize_cubic_u8(frames, size, boxes=CROP_BOXES).cpu()
    assert all(not torch.equal(plain[b], want[b]) for b in range(4))
    # a strided out: the left half of a side-by-side buffer; the right half stays
    pair = torch.full((5, size[0], 2 * size[1], 3), 7, dtype=torch.uint8, device="cuda")
    ret = ops.crop_resize_cubic_u8(frames, size, boxes=CROP_BOXES, angles=CROP_ANGLES, out=pair[:, :, :size[1]])
    assert ret.data_ptr() == pair.data_ptr() and torch.equal(pair[:, :, :size[1]].cpu(), want)
    assert bool((pair[:, :, size[1]:] == 7).all())
    # a single frame takes one box and one angle
    assert torch.equal(ops.crop_resize_cubic_u8(frames[1], size, boxes=[CROP_BOXES[1]], angles=[CROP_ANGLES[1]]).cpu(), want[1])


def test_rotated_crop_from_global_memory_and_staged_give_the_restatement():
    from denoising_diffusion_deep_fake_amd import ops
    hw, box, angle = (200, 200), (4, 4, 192, 192), 20.0
    assert _crop_lds(box, angle, hw, (16, 16)) > RESIZE_LDS_BYTES   # a tile's footprint passes the 32 KB of LDS
    assert _crop_lds(box, angle, hw, (96, 96)) <= RESIZE_LDS_BYTES  # the same box and angle at a size that stages
    frames = _frames(901, 2, hw)
    for size in ((16, 16), (96, 96)):
        got = ops.crop_resize_cubic_u8(frames[:1], size, boxes=[box], angles=[angle])
        assert torch.equal(got.cpu(), _crop_want(frames[:1], [box], [angle], size)), size
    # one launch has one route: a small box staged alone reads from global memory next to the large one -- the same bytes
    small = (50, 60, 40, 40)
    assert _crop_lds(small, angle, hw, (16, 16)) <= RESIZE_LDS_BYTES
    both = ops.crop_resize_cubic_u8(frames, (16, 16), boxes=[small, box], angles=[angle, angle])
    alone = ops.crop_resize_cubic_u8(frames[:1], (16, 16), boxes=[small], angles=[angle])
    assert torch.equal(both[:1], alone) and torch.equal(both.cpu(), _crop_want(frames, [small, box], [angle, angle], (16, 16)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_activation_form_equals_the_u8_form_then_the_normalisation(dtype):
    from denoising_diffusion_deep_fake_amd import _lib, ops
    frames = _frames(902, 5, HW)
    size, cpad = (16, 24), 8
    want = ops.crop_resize_cubic_u8(frames, size, boxes=CROP_BOXES, angles=CROP_ANGLES)
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    table, _ = ops._boxes_arg(CROP_BOXES, 5, "test")
    rot = ops._rot_arg(CROP_ANGLES, 5, "test")

    def fused(mean, std):
        dst = torch.zeros_like(want)
        act = torch.full((5,) + size + (cpad,), 3.0, dtype=tdt, device="cuda")
        m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        _lib.check(_lib.lib().d3f_crop_resize_cubic_rboxes_u8_nhwc(_lib.F32 if dtype == "f32" else _lib.BF16, _lib.ptr(frames), 5,
                                                                   HW[0], HW[1], table, rot, _lib.ptr(dst), size[0], size[1],
                                                                   3 * size[1], _lib.ptr(act), cpad, m, s, _lib.stream_ptr()))
        assert torch.equal(dst, want) and bool((act[..., 3:] == 0).all())
        return act[..., :3]

    # mean 0, std 1: the engine's (byte - 0) / 255 and u8rgb_normalise's (byte / 255 - 0) / 1 are the same fp32 operations
    rgb = want.flip(-1)
    norm = ops.u8rgb_normalise(rgb, [0.0] * 3, [1.0] * 3).permute(0, 2, 3, 1)
    assert torch.equal(fused([0.0] * 3, [1.0] * 3), norm.to(tdt))
    # any mean and std: the header's expression, (byte - mean * 255) / (std * 255) in fp32, RGB order
    mean, std = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    m255 = torch.tensor(mean, dtype=torch.float32) * 255.0
    s255 = torch.tensor(std, dtype=torch.float32) * 255.0
    expect = ((rgb.cpu().float() - m255) / s255).to(tdt)
    assert torch.equal(fused(mean, std).cpu(), expect)


def _moving_boxes(B, hw=(24, 32)):
    """a box and an angle per frame, drawn as the 70-frame test draws them"""
    rng = np.random.default_rng(922)
    boxes, angles = [], []
    for b in range(B):
        cw, ch = int(rng.integers(6, 20)), int(rng.integers(6, 20))
        boxes.append((int(rng.integers(0, hw[1] - cw + 1)), int(rng.integers(0, hw[0] - ch + 1)), cw, ch))
        angles.append(float(rng.integers(-17999, 18001)) / 100.0)
    return boxes, angles


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_activation_form_behind_the_first_launch_of_a_call(dtype):
    """65 frames are two launches: frame 64 is the second one's first, where the source, the bytes and the activation have
    each advanced by 64 frames.  It equals the call on frame 64 alone with box 64, and not the one with box 0."""
    from denoising_diffusion_deep_fake_amd import _lib, ops
    B, hw, size, cpad = 65, (24, 32), (8, 8), 4
    frames = _frames(920, B, hw)
    boxes, angles = _moving_boxes(B)
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    m, s = (C.c_float * 3)(0.4, 0.5, 0.6), (C.c_float * 3)(0.5, 0.45, 0.55)

    def fused(fr, bx, an):
        n = fr.shape[0]
        dst = torch.zeros((n,) + size + (3,), dtype=torch.uint8, device="cuda")
        act = torch.full((n,) + size + (cpad,), 3.0, dtype=tdt, device="cuda")
        table, _ = ops._boxes_arg(bx, n, "test")
        _lib.check(_lib.lib().d3f_crop_resize_cubic_rboxes_u8_nhwc(_lib.F32 if dtype == "f32" else _lib.BF16, _lib.ptr(fr), n,
                                                                   hw[0], hw[1], table, ops._rot_arg(an, n, "test"),
                                                                   _lib.ptr(dst), size[0], size[1], 3 * size[1], _lib.ptr(act),
                                                                   cpad, m, s, _lib.stream_ptr()))
        return dst, act

    dst, act = fused(frames, boxes, angles)
    last = frames[64:].contiguous()
    dst_own, act_own = fused(last, boxes[64:], angles[64:])
    assert torch.equal(dst[64:], dst_own) and torch.equal(act[64:], act_own)
    dst_first, act_first = fused(last, boxes[:1], angles[:1])
    assert not torch.equal(dst[64:], dst_first) and not torch.equal(act[64:], act_first)


@pytest.mark.parametrize("angle, k", [(90.0, 1), (180.0, 2), (270.0, 3), (-90.0, 3)])
def test_quarter_turns_are_rot90_of_the_axis_aligned_kernel_s_crop(angle, k):
    """cw = 2 W, ch = 2 H, a square box: every t is 0.5, all weights and sums are dyadic, so fp32 is exact in either pass
    order.  By the convention (x right, y down, positive = clockwise on the screen) k = 1 at +90.  The outermost ring of output
    pixels is left out: there the two clamp rules (the box / the frame) differ."""
    from denoising_diffusion_deep_fake_amd import ops
    frames = _frames(903, 1, HW)
    box = (21, 9, 32, 32)
    plain = ops.crop_resize_cubic_u8(frames, (16, 16), boxes=[box])[0].cpu().numpy()
    got = ops.crop_resize_cubic_u8(frames, (16, 16), boxes=[box], angles=[angle])[0].cpu().numpy()
    want = np.rot90(plain, k=k, axes=(0, 1))
    assert np.array_equal(got[1:-1, 1:-1], want[1:-1, 1:-1])
    assert not np.array_equal(got[1:-1, 1:-1], plain[1:-1, 1:-1])


# ---- the paste ----

PASTE_BOXES = [(30, 20, 34, 28), (0, 0, 40, 30), (12, 10, 24, 31), (20, 6, 29, 36)]  # the first two turn out of the frame
PASTE_ANGLES = [40.0, -33.0, 90.0, 7.5]


def _coef(seed, B):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([rng.uniform(0.6, 1.6, size=(B, 3)), rng.uniform(-40, 40, size=(B, 3))],
                                     axis=-1).astype(np.float32)).cuda()


@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("feather", [0, 5])
def test_rotated_paste_equals_the_restatement(feather, color):
    from denoising_diffusion_deep_fake_amd import ops
    frames, patch = _frames(910, 4, HW), _frames(911, 4, (16, 16))
    coef = _coef(912, 4) if color else None
    f, p = frames.cpu().numpy(), patch.cpu().numpy()
    want, masks = [], []
    for b in range(4):
        v, mask = R.rot_paste(p[b], f[b], PASTE_BOXES[b], R.box_rotation(PASTE_ANGLES[b]), feather,
                              coef[b].cpu().numpy() if color else None)
        want.append(R.round_u8(v))
        masks.append(mask)
    want, outside = torch.from_numpy(np.stack(want)), ~torch.from_numpy(np.stack(masks))
    # the rotated rectangle of box b holds about cw * ch pixel centres, less what left the frame
    for b in range(4):
        n, area = int(masks[b].sum()), PASTE_BOXES[b][2] * PASTE_BOXES[b][3]
        assert 0.5 * area < n <= area + 2 * (PASTE_BOXES[b][2] + PASTE_BOXES[b][3]), (b, n, area)
    assert int(masks[0].sum()) < PASTE_BOXES[0][2] * PASTE_BOXES[0][3] - 20  # corners outside the frame
    got = ops.paste_resize_cubic_u8(patch, frames, boxes=PASTE_BOXES, angles=PASTE_ANGLES, feather=feather, color=coef)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got.cpu()[outside], frames.cpu()[outside])
    # in place: the same bytes, and every byte whose pixel centre lies outside the rotated rectangle is the frame's
    work = frames.clone()
    ret = ops.paste_resize_cubic_u8(patch, work, boxes=PASTE_BOXES, angles=PASTE_ANGLES, feather=feather, color=coef, out=work)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work.cpu(), want)
    assert torch.equal(work.cpu()[outside], frames.cpu()[outside])
    # the patch as the right half of a pair buffer
    pair = torch.zeros((4, 16, 32, 3), dtype=torch.uint8, device="cuda")
    pair[:, :, 16:] = patch
    assert torch.equal(ops.paste_resize_cubic_u8(pair[:, :, 16:], frames, boxes=PASTE_BOXES, angles=PASTE_ANGLES,
                                                 feather=feather, color=coef).cpu(), want)


def test_rotated_paste_from_global_memory_equals_the_restatement():
    """a 200 x 200 patch into a 14 x 14 box: a frame tile's footprint in the patch passes the 32 KB of LDS"""
    from denoising_diffusion_deep_fake_amd import ops
    frames, patch = _frames(913, 1, HW), _frames(914, 1, (200, 200))
    box, angle = (20, 16, 14, 14), 20.0
    c16, s16 = (abs(v) for v in R.box_rotation(angle))
    cols = min((c16 * 31 + s16 * 7) * 200 // (65536 * 14) + 5, 200)
    rows = min((s16 * 31 + c16 * 7) * 200 // (65536 * 14) + 5, 200)
    assert rows * ((cols * 3 + 6) // 4 * 4) > RESIZE_LDS_BYTES
    v, _ = R.rot_paste(patch[0].cpu().numpy(), frames[0].cpu().numpy(), box, R.box_rotation(angle), 2)
    got = ops.paste_resize_cubic_u8(patch, frames, boxes=[box], angles=[angle], feather=2)
    assert torch.equal(got[0].cpu(), torch.from_numpy(R.round_u8(v)))


def test_a_call_of_70_frames_equals_its_frames_one_by_one():
    from denoising_diffusion_deep_fake_amd import ops
    B, hw = 70, (24, 32)
    frames, patch = _frames(920, B, hw), _frames(921, B, (8, 8))
    rng = np.random.default_rng(922)
    boxes, angles = [], []
    for b in range(B):
        cw, ch = int(rng.integers(6, 20)), int(rng.integers(6, 20))
        boxes.append((int(rng.integers(0, 32 - cw + 1)), int(rng.integers(0, 24 - ch + 1)), cw, ch))
        angles.append(float(rng.integers(-17999, 18001)) / 100.0)
    angles[3] = angles[66] = 0.0
    got = ops.crop_resize_cubic_u8(frames, (8, 8), boxes=boxes, angles=angles)
    want = torch.cat([_rot_crop_one(frames[b], boxes[b], angles[b], (8, 8)) for b in range(B)])
    assert torch.equal(got, want)
    assert torch.equal(got[64:].cpu(), _crop_want(frames[64:], boxes[64:], angles[64:], (8, 8)))  # behind the split
    coef = _coef(923, B)
    for color in (None, coef):
        pasted = ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, angles=angles, feather=2, color=color)
        for b in list(range(0, B, 9)) + [63, 64, 65, 69]:
            v, _ = R.rot_paste(patch[b].cpu().numpy(), frames[b].cpu().numpy(), boxes[b], R.box_rotation(angles[b]), 2,
                               None if color is None else coef[b].cpu().numpy())
            assert torch.equal(pasted[b].cpu(), torch.from_numpy(R.round_u8(v))), b
        work = frames.clone()
        ops.paste_resize_cubic_u8(patch, work, boxes=boxes, angles=angles, feather=2, color=color, out=work)
        assert torch.equal(work, pasted)


def test_angle_zero_inside_a_rotated_call_is_within_one_level_of_the_axis_aligned_call():
    """DESIGN.md section 4 "Rotated crop": the rotated form holds t to 16 fractional bits where the plain form divides exact
    integers, a position difference below 2^-16 per axis, worth at most 255 * 4.125 * 2 * 2^-16 = 0.033 grey levels before
    rounding: the bytes differ by at most ONE level.  Byte equality is not claimed.  The crop is compared away from the box's
    border ring (one output pixel at these down-scales), where the plain form clamps to the box and this one to the frame."""
    from denoising_diffusion_deep_fake_amd import ops
    frames, patch = _frames(930, 2, HW), _frames(931, 2, (16, 16))
    boxes, angles = [(9, 7, 37, 29), (20, 10, 30, 30)], [0.0, 10.0]
    got = ops.crop_resize_cubic_u8(frames, (16, 16), boxes=boxes, angles=angles)[0].int()
    plain = ops.crop_resize_cubic_u8(frames, (16, 16), boxes=boxes)[0].int()
    assert int((got - plain)[1:-1, 1:-1].abs().max()) <= 1
    for feather in (0, 5):
        got = ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, angles=angles, feather=feather)[0].int()
        plain = ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, feather=feather)[0].int()
        assert int((got - plain).abs().max()) <= 1
        x1, y1, cw, ch = boxes[0]
        outside = torch.ones(HW, dtype=torch.bool)
        outside[y1:y1 + ch, x1:x1 + cw] = False
        assert torch.equal(got.cpu()[outside], frames[0].int().cpu()[outside])  # the same pixels belong to the box
    # all angles zero after rounding: the boxes= call itself, byte for byte
    assert torch.equal(ops.crop_resize_cubic_u8(frames, (16, 16), boxes=boxes, angles=[0.0, 0.004]),
                       ops.crop_resize_cubic_u8(frames, (16, 16), boxes=boxes))
    assert torch.equal(ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, angles=[0, -0.0049], feather=3),
                       ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, feather=3))


def test_rotated_refusals_raise():
    from denoising_diffusion_deep_fake_amd import D3FError, _lib, ops
    frames, patch = _frames(940, 3, (90, 160)), _frames(941, 3, (16, 16))
    bad = [(35, 0, 90, 90), (0, 0, 160, 90), (71, 0, 90, 90)]
    with pytest.raises(D3FError, match="frame 2"):
        ops.crop_resize_cubic_u8(frames, (16, 16), boxes=bad, angles=[1, 2, 3])
    with pytest.raises(D3FError, match="frame 2"):
        ops.paste_resize_cubic_u8(patch, frames, boxes=bad, angles=[1, 2, 3])
    with pytest.raises(ValueError, match="angles"):
        ops.crop_resize_cubic_u8(frames, (16, 16), boxes=bad[:2] + [(0, 0, 9, 9)], angles=[1, 2])
    with pytest.raises(ValueError, match="antialias"):
        ops.crop_resize_cubic_u8(frames, (16, 16), boxes=bad[:2] + [(0, 0, 9, 9)], angles=[1, 2, 3], antialias=True)
    # a table that would scale: refused by the library, the frame named
    table, _ = ops._boxes_arg(bad[:2] + [(0, 0, 9, 9)], 3, "test")
    rot = (C.c_int32 * 6)(65536, 0, 65536, 400, 0, 65536)  # 400^2 > 2^17
    out = torch.zeros((3, 16, 16, 3), dtype=torch.uint8, device="cuda")
    assert _lib.lib().d3f_crop_resize_cubic_rboxes_u8(_lib.ptr(frames), 3, 90, 160, table, rot, _lib.ptr(out), 16, 16, 48,
                                                      _lib.stream_ptr()) != 0
    assert b"frame 1:" in _lib.lib().d3f_last_error() and b"no rotation" in _lib.lib().d3f_last_error()
    assert not bool(out.any())


# ---- the engine ----

MEAN, STD = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
ENGINE_HW = (150, 200)
ENGINE_BOXES = [(0, 0, 64, 64), (37, 11, 150, 139), (101, 50, 99, 100)]
ENGINE_ANGLES = [12.5, -30.0, 0.0]


def _net(dtype):
    from denoising_diffusion_deep_fake_amd import Unet
    torch.manual_seed(11)
    net = Unet("resnet18", None, 3, 3, None, compute_dtype=dtype).cuda().eval()
    with torch.no_grad():
        for name, buf in net.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0, 0.1)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    net.mark_params_changed()
    return net


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("color_match", [None, "meanstd"], ids=["plain", "colour"])
def test_engine_rboxes_entries_are_bit_exact_against_the_ops_they_fuse(dtype, color_match):
    from denoising_diffusion_deep_fake_amd import _lib, ops
    net = _net(dtype)
    raw = _frames(950, 3, ENGINE_HW)
    boxes, angles = ENGINE_BOXES, ENGINE_ANGLES
    left = ops.crop_resize_cubic_u8(raw, (64, 64), boxes=boxes, angles=angles)
    assert not torch.equal(left[:2], ops.crop_resize_cubic_u8(raw, (64, 64), boxes=boxes)[:2])
    right = net.predict_u8(left, MEAN, STD, graph=False)
    pair = net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=angles)  # graph=True is ignored: eager
    assert pair.shape == (3, 64, 128, 3)
    assert torch.equal(pair[:, :, :64], left) and torch.equal(pair[:, :, 64:], right)
    coef = None
    if color_match:
        coef = ops.color_match_coef(ops.channel_sums_u8(pair[:, :, 64:]), ops.channel_sums_u8(pair[:, :, :64]), 64 * 64)
    for f in (None, 0, 9):
        want = ops.paste_resize_cubic_u8(right, raw, boxes=boxes, angles=angles, color=coef,
                                         feather=ops.default_feather(64, 64) if f is None else f)
        pair_out = torch.zeros_like(pair)
        full = net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, feather=f, boxes=boxes, angles=angles, pair_out=pair_out,
                                          color_match=color_match)
        assert torch.equal(pair_out, pair) and torch.equal(full, want), f
    work = raw.clone()
    net.predict_frames_full_u8(work, (64, 64), MEAN, STD, feather=9, boxes=boxes, angles=angles, out=work, graph=False,
                               color_match=color_match)
    assert torch.equal(work, want)
    # angles all zero (after rounding) is the boxes= call
    for zero in ([0.0] * 3, [0.0, 0.004, -0.004]):
        assert torch.equal(net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=zero),
                           net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes))
        assert torch.equal(net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=zero, color_match=color_match),
                           net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, boxes=boxes, color_match=color_match))
    # what Python refuses before the call
    with pytest.raises(ValueError, match="antialias"):
        net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=angles, antialias=True)
    with pytest.raises(ValueError, match="multiband"):
        net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=angles, blend="multiband")
    with pytest.raises(ValueError, match="boxes"):
        net.predict_frames_u8(raw, (64, 64), MEAN, STD, angles=angles)
    # a graph together with angles is refused by the entry itself
    L = _lib.lib()
    eng, rt = net._u8_engine(3, 64, 64, raw.device), net._rt
    table, _ = ops._boxes_arg(boxes, 3, "test")
    rot = ops._rot_arg(angles, 3, "test")
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    before = pair.clone()
    assert L.d3f_unet_predict_frames_rboxes_u8(eng.h, _lib.ptr(rt["flat"]), _lib.ptr(rt["flat_bn"]), _lib.ptr(raw), 150, 200,
                                               table, rot, _lib.ptr(pair), m, s, _lib.ptr(eng.workspace), 1,
                                               _lib.stream_ptr()) != 0
    assert b"graph" in L.d3f_last_error() and torch.equal(pair, before)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_rboxes_with_colour_match_and_temporal_filter_equal_the_chain_of_ops(dtype):
    from denoising_diffusion_deep_fake_amd import ops
    net, untouched = _net(dtype), _net(dtype)
    raws = [_frames(960 + it, 3, ENGINE_HW) for it in range(2)]
    noise = torch.from_numpy(np.random.default_rng(969).integers(-3, 4, size=ENGINE_HW + (3,))).cuda()
    raws[1][2] = (raws[1][1].int() + noise).clamp(0, 255).to(torch.uint8)  # a crop that stands still: the filter averages
    calls = [(ENGINE_BOXES, ENGINE_ANGLES), ([(1, 0, 64, 64), (37, 11, 150, 139), (37, 11, 150, 139)], [12.5, 21.0, 21.0])]
    state = ops.TemporalState(64, 64)
    n = 64 * 64
    net.reset_frame_temporal()
    for it, (raw, (boxes, angles)) in enumerate(zip(raws, calls)):
        pair = untouched.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=angles)
        unfiltered = pair.clone()
        ops.temporal_filter_u8(pair[:, :, :64], pair[:, :, 64:], state, 0.75, 8)
        s_to, s_from = ops.channel_sums_u8(pair[:, :, :64]), ops.channel_sums_u8(pair[:, :, 64:])
        coef = ops.color_match_coef(s_from, s_to, n)
        ops.color_coef_smooth(coef, s_to, n, state, 0.75)
        want = ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, boxes=boxes, angles=angles, feather=5, color=coef)
        pair_out = torch.zeros_like(pair)
        full = net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, feather=5, boxes=boxes, angles=angles,
                                          color_match="meanstd", temporal=0.75, pair_out=pair_out)
        assert torch.equal(pair_out, pair), (it, "pair")
        assert torch.equal(full, want), (it, "full")
        assert it == 0 or not torch.equal(pair, unfiltered), "the filter moves the second call's fake"
    net.reset_frame_temporal()
    state = ops.TemporalState(64, 64)
    for raw, (boxes, angles) in zip(raws, calls):
        pair = untouched.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=angles)
        ops.temporal_filter_u8(pair[:, :, :64], pair[:, :, 64:], state, 0.75, 8)
        assert torch.equal(net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, angles=angles, temporal=0.75), pair)


# ---- the tools ----

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet18",
               noise_exponential_sampling_lambda=3, mean_a=[0.4, 0.5, 0.6], std_a=[0.5, 0.45, 0.55],
               mean_b=[0.45, 0.4, 0.55], std_b=[0.6, 0.5, 0.4], synthetic=True, image_size=64, synthetic_length=4,
               ema_beta=0.9999, ema_update_every=1, augment=False)
TRACK_TEXT = "# x y w h a\n20 10 30 40 12.5\n-\n90,30,50,50\n150 60 40 30 -20\n"  # frame 4 keeps the last line's box and angle
TRACK_ENTRIES = [(20, 10, 30, 40, 12.5), (20, 10, 30, 40, 12.5), (90, 30, 50, 50, 0.0), (150, 60, 40, 30, -20.0),
                 (150, 60, 40, 30, -20.0)]


@pytest.mark.parametrize("output", ["pair", "full"])
def test_both_tools_cut_the_same_rotated_boxes_from_one_five_column_file(output, tmp_path):
    """5 frames, 2 at a time: the sink gets what the Unet calls with the track's boxes and angles give, the frame counter runs
    across batches, the padded last batch repeats the last box AND angle; VideoToImages cuts the crops the render tool's
    pair shows on its left"""
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    from denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images import VideoToImages
    from denoising_diffusion_deep_fake_amd.script_tools.video_writer_context_manager import load_rtrack
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    torch.manual_seed(6)
    lit = LitModule(precision="f32", **HP_FAKE).cuda().eval()
    model, mean, std = lit.model_a, lit.hparams.mean_b, lit.hparams.std_b
    track = tmp_path / "track.txt"
    track.write_text(TRACK_TEXT)
    assert load_rtrack(track, 0) == TRACK_ENTRIES[:4]
    rng = np.random.default_rng(980)
    frames = [rng.integers(0, 256, size=(100, 180, 3), dtype=np.uint8) for _ in range(5)]
    got = []
    RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                    output=output, track=str(track), track_rotate=True)
    assert len(got) == 5
    boxes = [ops.track_crop_box(100, 180, 96, 64, e[:4]) for e in TRACK_ENTRIES]
    angles = [e[4] for e in TRACK_ENTRIES]
    feather = ops.default_feather(min(b[2] for b in boxes), min(b[3] for b in boxes))
    for k in range(5):
        first = k - k % 2
        other = min(first + 1, 4)  # the padding repeats frame 4, its box and its angle
        batch = torch.from_numpy(np.stack([frames[first], frames[other]])).cuda()
        both, turn = [boxes[first], boxes[other]], [angles[first], angles[other]]
        if output == "pair":
            want = model.predict_frames_u8(batch, (64, 96), mean, std, boxes=both, angles=turn)
        else:
            want = model.predict_frames_full_u8(batch, (64, 96), mean, std, feather=feather, boxes=both, angles=turn)
        assert np.array_equal(got[k], want[k % 2].cpu().numpy()), k
    # without the flag the five-column file is refused, as ever
    with pytest.raises(ValueError, match="line 2"):
        RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                        output=output, track=str(track))
    if output == "pair":
        tool = VideoToImages.__new__(VideoToImages)
        tool.image_width, tool.image_height, tool.device, tool.antialias = 96, 64, "cuda", False
        tool.track, tool.track_rotate, tool.track_margin, tool.frame_index = load_rtrack(track, 0), True, 1.6, 0
        cut = [tool.resize_frames(np.stack(frames[0:2]), 2), tool.resize_frames(np.stack(frames[2:4]), 2),
               tool.resize_frames(np.stack([frames[4], frames[4]]), 1)]
        assert tool.frame_index == 5
        for k in range(5):
            assert np.array_equal(cut[k // 2][k % 2], got[k][:, :96]), k
            # (frame 2 has angle 0 inside a rotated call: the rotated entry itself, not the boxes entry ops would take alone)
            want = _rot_crop_one(torch.from_numpy(frames[k]).cuda(), boxes[k], angles[k], (64, 96))[0]
            assert np.array_equal(cut[k // 2][k % 2], want.cpu().numpy()), k
        assert np.array_equal(cut[2][1], cut[2][0])  # the padding frame: the same frame, box and angle


def test_track_face_box_writes_the_key_angles_as_a_fifth_column(tmp_path):
    """without --key-angle the file is byte for byte what it was; with it every found frame gains the interpolated angle, and
    the two tools read the file with track_rotate"""
    import track_restatement as tr
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.track_face_box import TrackFaceBox
    frames, positions = tr.moving_patch_frames(2025, 10, 96, 160, 1, 3, absent=(5,), patch=(24, 20))
    keys = [(1, positions[1][0], positions[1][1], 20, 24)]
    plain, turned = tmp_path / "plain.txt", tmp_path / "turned.txt"
    a = TrackFaceBox(tmp_path / "clip.mp4", keys, output_path=plain, batch_frames=4, frames=iter(frames), search=8)
    b = TrackFaceBox(tmp_path / "clip.mp4", keys, output_path=turned, batch_frames=4, frames=iter(frames), search=8,
                     key_angles=[(2, 10), (6, -10.5)])
    assert a.track == b.track and a.angles is None and a.track[0] is None and a.track[5] is None
    # keys at 2 and 6: 1000 + (-2050 * d) // 4 for d = 1, 2, 3 is 487, -25, -538 (floor division)
    assert b.angles == [1000, 1000, 1000, 487, -25, -538, -1050, -1050, -1050, -1050]
    rows = [line for line in plain.read_text().splitlines() if not line.startswith("#")]
    assert rows == ["-" if box is None else "{} {} {} {}".format(*box) for box in a.track]
    assert "angle" not in plain.read_text()
    got = [line for line in turned.read_text().splitlines() if not line.startswith("#")]
    assert got == [r if r == "-" else f"{r} {b.angles[k] / 100:.2f}" for k, r in enumerate(rows)]
    assert [line for line in turned.read_text().splitlines() if line.startswith("#")][:-1] == \
        [line for line in plain.read_text().splitlines() if line.startswith("#")]
    entries = ops.read_rbox_track(turned)
    assert [e[:4] for e in entries] == ops.read_box_track(plain)
    assert [e[4] for e in entries][1:5] == [10.0, 10.0, 4.87, -0.25] and entries[5] == entries[4]  # the gap keeps box and angle
