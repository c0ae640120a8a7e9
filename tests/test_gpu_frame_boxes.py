"""GPU: a box per frame through the crop kernels (both resample forms), the paste (plain, colour, in place), the engine's two
frame entries and the render tool.  The single-box kernels are pinned bit for bit by their restatement tests, so the
per-frame form has an exact oracle: frame b of a boxes call equals the single-box call on frame b with box b.  Every
comparison is torch.equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# call A: the copy path (equal extents), enlarge on x / shrink on y at an odd byte offset, the frame's far corner, a plain one
BOXES_A = [(0, 0, 16, 16), (5, 3, 13, 29), (304, 240, 16, 16), (1, 2, 40, 24)]
# call B: the last box's staged patch is far over 32 KB in the plain form: the whole launch reads its taps from global memory
BOXES_B = BOXES_A[:3] + [(79, 15, 240, 240)]
HW, SIZE = (256, 320), (16, 16)

RESIZE_LDS_BYTES, TW, TH = 32 * 1024, 32, 8


def _patch_extent(n_h, n_w, out_h, out_w):
    """resize_patch_extent's formula (csrc/resize.hip): rows and pitch of the largest staged part of a tile"""
    cols, rows = (TW - 1) * n_w // out_w + 1 + 4, (TH - 1) * n_h // out_h + 1 + 4
    return rows, (cols * 3 + 3 + 3) // 4 * 4


def _launch_lds(boxes, size):
    extents = [_patch_extent(ch, cw, size[0], size[1]) for _, _, cw, ch in boxes]
    return max(r for r, _ in extents) * max(p for _, p in extents)


def _frames(seed, B, hw):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(B,) + hw + (3,), dtype=np.uint8)).cuda()


def test_the_two_calls_sit_on_both_sides_of_the_staging_limit():
    assert _launch_lds(BOXES_A, SIZE) <= RESIZE_LDS_BYTES
    rows, pitch = _patch_extent(240, 240, 16, 16)
    assert rows * pitch > 2 * RESIZE_LDS_BYTES and _launch_lds(BOXES_B, SIZE) > 2 * RESIZE_LDS_BYTES
    # and the paste's staged part of a 16 x 16 patch stays staged for every box of call A
    assert max(_patch_extent(16, 16, ch, cw)[0] for _, _, cw, ch in BOXES_A) * \
        max(_patch_extent(16, 16, ch, cw)[1] for _, _, cw, ch in BOXES_A) <= RESIZE_LDS_BYTES


@pytest.mark.parametrize("antialias", [False, True], ids=["cubic", "aa"])
@pytest.mark.parametrize("boxes", [BOXES_A, BOXES_B], ids=["A_staged", "B_global"])
def test_crop_boxes_equal_the_single_box_calls(boxes, antialias):
    from denoising_diffusion_deep_fake_amd import ops
    frames = _frames(700, 4, HW)
    want = torch.stack([ops.crop_resize_cubic_u8(frames[b], SIZE, box=boxes[b], antialias=antialias) for b in range(4)])
    assert len({bytes(w.cpu().numpy()) for w in want}) == 4  # four different crops
    assert torch.equal(want[0], frames[0, :16, :16]) and torch.equal(want[2], frames[2, 240:, 304:])  # the copy path
    got = ops.crop_resize_cubic_u8(frames, SIZE, boxes=boxes, antialias=antialias)
    assert got.shape == (4, 16, 16, 3) and torch.equal(got, want)
    assert torch.equal(ops.crop_resize_cubic_u8(frames, SIZE, boxes=np.asarray(boxes), antialias=antialias), want)
    # a strided out: the left half of a side-by-side buffer; the right half stays
    pair = torch.full((4, 16, 32, 3), 7, dtype=torch.uint8, device="cuda")
    ret = ops.crop_resize_cubic_u8(frames, SIZE, boxes=boxes, antialias=antialias, out=pair[:, :, :16])
    assert ret.data_ptr() == pair.data_ptr() and torch.equal(pair[:, :, :16], want) and bool((pair[:, :, 16:] == 7).all())
    # a single frame takes [1][4]
    assert torch.equal(ops.crop_resize_cubic_u8(frames[1], SIZE, boxes=[boxes[1]], antialias=antialias), want[1])


@pytest.mark.parametrize("antialias", [False, True], ids=["cubic", "aa"])
def test_crop_boxes_over_more_than_one_launch(antialias):
    """65 frames: the 65th is the second launch's first, and takes box 64, not box 0"""
    from denoising_diffusion_deep_fake_amd import ops
    B = 65
    frames = _frames(701, B, (40, 48))
    boxes = [(b % 9, b % 7, 24 + b % 5, 20 + b % 3) for b in range(B)]
    assert boxes[64] != boxes[0]
    want = torch.stack([ops.crop_resize_cubic_u8(frames[b], (8, 8), box=boxes[b], antialias=antialias) for b in range(B)])
    got = ops.crop_resize_cubic_u8(frames, (8, 8), boxes=boxes, antialias=antialias)
    assert torch.equal(got, want)
    assert not torch.equal(want[64], ops.crop_resize_cubic_u8(frames[64], (8, 8), box=boxes[0], antialias=antialias))


def _coef(seed, B):
    rng = np.random.default_rng(seed)
    coef = np.stack([rng.uniform(0.5, 2.0, size=(B, 3)), rng.uniform(-20.0, 20.0, size=(B, 3))], axis=-1)
    return torch.from_numpy(coef.astype(np.float32)).cuda()


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("feather", [0, 3])
def test_paste_boxes_equal_the_single_box_calls(feather, color):
    from denoising_diffusion_deep_fake_amd import ops
    boxes = BOXES_A
    frames = _frames(710, 4, HW)
    patch = _frames(711, 4, SIZE)
    coef = _coef(712, 4) if color else None
    want = torch.stack([ops.paste_resize_cubic_u8(patch[b], frames[b], boxes[b], feather,
                                                  color=None if coef is None else coef[b]) for b in range(4)])
    got = ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, feather=feather, color=coef)
    assert torch.equal(got, want)
    outside = torch.ones((4,) + HW, dtype=torch.bool, device="cuda")
    for b, (x1, y1, cw, ch) in enumerate(boxes):
        outside[b, y1:y1 + ch, x1:x1 + cw] = False
        assert not torch.equal(got[b, y1:y1 + ch, x1:x1 + cw], frames[b, y1:y1 + ch, x1:x1 + cw]), b
    assert torch.equal(got[outside], frames[outside])
    # the patch as the right half of a pair buffer
    pair = torch.zeros((4, 16, 32, 3), dtype=torch.uint8, device="cuda")
    pair[:, :, 16:] = patch
    assert torch.equal(ops.paste_resize_cubic_u8(pair[:, :, 16:], frames, boxes=boxes, feather=feather, color=coef), want)
    # in place: one tile grid for the launch, every frame's own first tile -- nothing outside a frame's own box is written
    work = frames.clone()
    ret = ops.paste_resize_cubic_u8(patch, work, boxes=boxes, feather=feather, out=work, color=coef)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work, want)
    assert torch.equal(work[outside], frames[outside])


def test_paste_boxes_over_more_than_one_launch_in_place():
    from denoising_diffusion_deep_fake_amd import ops
    B = 65
    frames = _frames(720, B, (40, 48))
    patch = _frames(721, B, (8, 8))
    coef = _coef(722, B)
    boxes = [(b % 9, b % 7, 24 + b % 5, 20 + b % 3) for b in range(B)]
    for color in (None, coef):
        want = torch.stack([ops.paste_resize_cubic_u8(patch[b], frames[b], boxes[b], 2,
                                                      color=None if color is None else color[b]) for b in range(B)])
        assert torch.equal(ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, feather=2, color=color), want)
        work = frames.clone()
        ops.paste_resize_cubic_u8(patch, work, boxes=boxes, feather=2, out=work, color=color)
        assert torch.equal(work, want)


def test_boxes_refusals_raise():
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    frames = _frames(730, 3, (90, 160))
    patch = _frames(731, 3, (16, 16))
    bad = [(35, 0, 90, 90), (0, 0, 160, 90), (71, 0, 90, 90)]
    with pytest.raises(D3FError, match="frame 2"):
        ops.crop_resize_cubic_u8(frames, SIZE, boxes=bad)
    with pytest.raises(D3FError, match="frame 2"):
        ops.paste_resize_cubic_u8(patch, frames, boxes=bad)
    with pytest.raises(ValueError):
        ops.crop_resize_cubic_u8(frames, SIZE, boxes=bad[:2])
    with pytest.raises(ValueError):
        ops.crop_resize_cubic_u8(frames, SIZE, box=bad[0], boxes=bad)


# ---- the engine ----

MEAN, STD = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
ENGINE_HW = (150, 200)
ENGINE_BOXES = [(0, 0, 64, 64), (37, 11, 150, 139), (101, 50, 99, 100)]


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
@pytest.mark.parametrize("antialias", [False, True], ids=["cubic", "aa"])
def test_engine_boxes_entries_are_bit_exact_against_the_ops_they_fuse(dtype, antialias):
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    net = _net(dtype)
    raw = _frames(740, 3, ENGINE_HW)
    boxes = ENGINE_BOXES
    left = ops.crop_resize_cubic_u8(raw, (64, 64), boxes=boxes, antialias=antialias)
    assert torch.equal(left, torch.stack([ops.crop_resize_cubic_u8(raw[b], (64, 64), box=boxes[b], antialias=antialias)
                                          for b in range(3)]))
    right = net.predict_u8(left, MEAN, STD, graph=False)
    pair = net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, antialias=antialias)  # graph=True is ignored: eager
    assert pair.shape == (3, 64, 128, 3)
    assert torch.equal(pair[:, :, :64], left) and torch.equal(pair[:, :, 64:], right)
    assert len({bytes(p.cpu().numpy()) for p in left}) == 3
    feather = ops.default_feather(64, 64)
    assert feather == 4
    for f in (None, 0, 9):
        want = ops.paste_resize_cubic_u8(right, raw, boxes=boxes, feather=feather if f is None else f)
        pair_out = torch.zeros_like(pair)
        full = net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, feather=f, boxes=boxes, antialias=antialias,
                                          pair_out=pair_out)
        assert torch.equal(pair_out, pair) and torch.equal(full, want), f
    work = raw.clone()
    net.predict_frames_full_u8(work, (64, 64), MEAN, STD, feather=9, boxes=boxes, antialias=antialias, out=work, graph=False)
    assert torch.equal(work, want)
    # one box as 4 ints is that box three times; it goes through the single-box entry, graph honoured
    for box in (boxes[1], torch.tensor(boxes[1])):
        for graph in (False, True):
            assert torch.equal(net.predict_frames_u8(raw, (64, 64), MEAN, STD, graph=graph, boxes=box, antialias=antialias),
                               net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=[boxes[1]] * 3, antialias=antialias))
            assert torch.equal(
                net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, graph=graph, boxes=box, antialias=antialias),
                net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, boxes=[boxes[1]] * 3, antialias=antialias))
    # boxes=None is the centre crop
    centre = ops.center_crop_box(150, 200, 64, 64)
    assert torch.equal(net.predict_frames_u8(raw, (64, 64), MEAN, STD, graph=False, antialias=antialias),
                       net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=[centre] * 3, antialias=antialias))
    assert torch.equal(net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, graph=False, antialias=antialias),
                       net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, boxes=[centre] * 3, antialias=antialias))
    with pytest.raises(D3FError, match="frame 1"):
        net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=[boxes[0], (150, 0, 64, 64), boxes[2]])
    with pytest.raises(ValueError):
        net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes[:2])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_boxes_with_colour_match_and_temporal_filter_equal_the_chain_of_ops(dtype):
    from denoising_diffusion_deep_fake_amd import ops
    net, untouched = _net(dtype), _net(dtype)
    raws = [_frames(750 + it, 3, ENGINE_HW) for it in range(2)]
    # the second call's last two frames differ by at most 3 levels and share a box: a crop that stands still, where the
    # filter averages
    noise = torch.from_numpy(np.random.default_rng(759).integers(-3, 4, size=ENGINE_HW + (3,))).cuda()
    raws[1][2] = (raws[1][1].int() + noise).clamp(0, 255).to(torch.uint8)
    calls = [ENGINE_BOXES, [(1, 0, 64, 64), (37, 11, 150, 139), (37, 11, 150, 139)]]
    state = ops.TemporalState(64, 64)
    n = 64 * 64
    net.reset_frame_temporal()
    for it, (raw, boxes) in enumerate(zip(raws, calls)):
        pair = untouched.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes)
        unfiltered = pair.clone()
        ops.temporal_filter_u8(pair[:, :, :64], pair[:, :, 64:], state, 0.75, 8)
        s_to, s_from = ops.channel_sums_u8(pair[:, :, :64]), ops.channel_sums_u8(pair[:, :, 64:])
        coef = ops.color_match_coef(s_from, s_to, n)
        ops.color_coef_smooth(coef, s_to, n, state, 0.75)
        want = ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, boxes=boxes, feather=5, color=coef)
        pair_out = torch.zeros_like(pair)
        full = net.predict_frames_full_u8(raw, (64, 64), MEAN, STD, feather=5, boxes=boxes, color_match="meanstd",
                                          temporal=0.75, pair_out=pair_out)
        assert torch.equal(pair_out, pair), (it, "pair")
        assert torch.equal(full, want), (it, "full")
        assert it == 0 or not torch.equal(pair, unfiltered), "the filter moves the second call's fake"
    # the pair entry with the filter on, from a fresh sequence
    net.reset_frame_temporal()
    state = ops.TemporalState(64, 64)
    for raw, boxes in zip(raws, calls):
        pair = untouched.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes)
        ops.temporal_filter_u8(pair[:, :, :64], pair[:, :, 64:], state, 0.75, 8)
        assert torch.equal(net.predict_frames_u8(raw, (64, 64), MEAN, STD, boxes=boxes, temporal=0.75), pair)


# ---- the tools ----

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet18",
               noise_exponential_sampling_lambda=3, mean_a=[0.4, 0.5, 0.6], std_a=[0.5, 0.45, 0.55],
               mean_b=[0.45, 0.4, 0.55], std_b=[0.6, 0.5, 0.4], synthetic=True, image_size=64, synthetic_length=4,
               ema_beta=0.9999, ema_update_every=1, augment=False)


@pytest.mark.parametrize("output", ["pair", "full"])
def test_render_fake_video_follows_a_track(output, tmp_path):
    """5 frames, 2 at a time, a track of 4 lines with a gap: the sink gets what the per-frame Unet calls with
    track_crop_box of the track's lines give; the frame counter runs across batches; the padded last batch writes 5"""
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    torch.manual_seed(6)
    lit = LitModule(precision="f32", **HP_FAKE).cuda().eval()
    model, mean, std = lit.model_a, lit.hparams.mean_b, lit.hparams.std_b
    track = tmp_path / "track.txt"
    track.write_text("# x y w h\n20 10 30 40\n-\n90,30,50,50\n150 60 40 30\n")  # frame 4 keeps the last line's box
    faces = [(20, 10, 30, 40), (20, 10, 30, 40), (90, 30, 50, 50), (150, 60, 40, 30), (150, 60, 40, 30)]
    rng = np.random.default_rng(760)
    frames = [rng.integers(0, 256, size=(100, 180, 3), dtype=np.uint8) for _ in range(5)]
    for margin, smooth in ((None, None), (2.0, 1)):
        got = []
        RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                        output=output, track=str(track), track_margin=margin, track_smooth=smooth)
        assert len(got) == 5
        used = ops.smooth_box_track(faces[:4], smooth or 0)
        used.append(used[-1])
        boxes = [ops.track_crop_box(100, 180, 96, 64, face, margin or 1.6) for face in used]
        assert len(set(boxes)) >= 3
        feather = ops.default_feather(min(b[2] for b in boxes), min(b[3] for b in boxes))
        for k in range(5):
            # frame k of its batch of two, with its batch's other frame (the padding repeats frame 4 and its box)
            first = k - k % 2
            other = min(first + 1, 4)
            batch = torch.from_numpy(np.stack([frames[first], frames[other]])).cuda()
            both = [boxes[first], boxes[other]]
            if output == "pair":
                want = model.predict_frames_u8(batch, (64, 96), mean, std, boxes=both)
            else:
                want = model.predict_frames_full_u8(batch, (64, 96), mean, std, feather=feather, boxes=both)
            assert np.array_equal(got[k], want[k % 2].cpu().numpy()), (margin, k)
            # ... which is the single-box call on that box
            if output == "pair":
                alone = model.predict_frames_u8(batch, (64, 96), mean, std, graph=False, boxes=boxes[k])
            else:
                alone = model.predict_frames_full_u8(batch, (64, 96), mean, std, graph=False, feather=feather, boxes=boxes[k])
            assert np.array_equal(got[k], alone[k % 2].cpu().numpy()), (margin, k, "single box")


def test_video_to_images_cuts_the_same_boxes(tmp_path):
    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images import VideoToImages
    rng = np.random.default_rng(770)
    frames = [rng.integers(0, 256, size=(100, 180, 3), dtype=np.uint8) for _ in range(5)]
    faces = [(20, 10, 30, 40), (90, 30, 50, 50), (150, 60, 40, 30)]
    tool = VideoToImages.__new__(VideoToImages)
    tool.image_width, tool.image_height, tool.device, tool.antialias = 96, 64, "cuda", False
    tool.track, tool.track_margin, tool.frame_index = faces, 1.6, 0
    got = [tool.resize_frames(np.stack(frames[0:2]), 2), tool.resize_frames(np.stack(frames[2:4]), 2),
           tool.resize_frames(np.stack([frames[4], frames[4]]), 1)]
    assert tool.frame_index == 5
    for k in range(5):
        box = ops.track_crop_box(100, 180, 96, 64, faces[min(k, 2)])
        want = ops.crop_resize_cubic_u8(torch.from_numpy(frames[k]).cuda(), (64, 96), box=box).cpu().numpy()
        assert np.array_equal(got[k // 2][k % 2], want), k
