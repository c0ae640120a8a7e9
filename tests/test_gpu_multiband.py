"""GPU: the multiband paste (csrc/multiband.hip; include/d3f_hip.h: d3f_paste_multiband_u8) against its restatement in numpy
integers (tests/multiband_restatement.py), byte for byte and with no pixel left out, at operator level and through the
full-frame entry.  The restatement takes the target bytes V from the plain paste at feather 0 on the device -- everything
behind V is integer arithmetic, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import multiband_restatement as mb

pytestmark = pytest.mark.gpu

FRAMES = {"67x91": (67, 91), "40x64": (40, 64)}  # (h, w)
ODD_BOX = (5, 3, 29, 37)                        # (x1, y1, cw, ch): 29 -> 15 -> 8 -> 4 columns, 37 -> 19 -> 10 -> 5 rows


def _rand(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)).cuda()


def _smooth_patch(seed, B, H, W):
    """a patch with structure at every scale, so that every band of the pyramid is busy"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin(x / 5.0 + rng.uniform(0, 3)) * np.cos(y / 7.0) + rng.normal(0, 25, (B, H, W, 3)).transpose(3, 0, 1, 2)
    return torch.from_numpy(np.clip(base.transpose(1, 2, 3, 0), 0, 255).astype(np.uint8)).cuda()


def _want(patch, frames, boxes, feather, levels, color=None):
    """the restatement on V = the plain (colour) paste at feather 0, frame by frame"""
    from denoising_diffusion_deep_fake_amd import ops
    B = frames.shape[0]
    V = ops.paste_resize_cubic_u8(patch, frames, boxes=boxes, feather=0, color=color).cpu().numpy()
    f = frames.cpu().numpy()
    out = []
    for b in range(B):
        x1, y1, cw, ch = boxes[b]
        out.append(mb.paste_multiband(V[b, y1:y1 + ch, x1:x1 + cw], f[b], boxes[b], feather, levels))
    return np.stack(out)


def _check(patch, frames, box, feather, levels, color=None, what=""):
    from denoising_diffusion_deep_fake_amd import ops
    got = ops.paste_multiband_u8(patch, frames, box, feather, levels, color=color)
    want = _want(patch, frames, [tuple(box)] * frames.shape[0], feather, levels, color)
    assert np.array_equal(got.cpu().numpy(), want), (what, box, feather, levels)
    return got


@pytest.mark.parametrize("hw", list(FRAMES), ids=list(FRAMES))
@pytest.mark.parametrize("B", [1, 3])
def test_every_level_count_and_feather_on_a_box_that_is_odd_at_every_level(hw, B):
    h, w = FRAMES[hw]
    frames, patch = _rand(1 + B, (B, h, w, 3)), _smooth_patch(2 + B, B, 24, 20)
    for levels in (1, 2, 3):
        for feather in (0, 1, 5, 12):
            _check(patch, frames, ODD_BOX, feather, levels)


@pytest.mark.parametrize("hw", list(FRAMES), ids=list(FRAMES))
def test_boxes_at_the_frame_edges_the_whole_frame_and_the_smallest_box(hw):
    from denoising_diffusion_deep_fake_amd import ops
    h, w = FRAMES[hw]
    B = 2
    frames, patch = _rand(11, (B, h, w, 3)), _smooth_patch(12, B, 32, 32)
    for box, levels, feather in (((0, 0, 33, 30), 2, 5),             # the top-left corner
                                 ((w - 41, h - 35, 41, 35), 3, 12),   # the bottom-right corner
                                 ((0, 0, w, h), 3, 5),                # the whole frame
                                 ((0, 0, w, h), 1, 12),
                                 ((7, 9, 20, 8), 3, 5),               # exactly 1 << N rows
                                 ((9, 7, 4, 23), 2, 1),               # exactly 1 << N columns
                                 ((3, 3, 2, 2), 1, 0)):
        _check(patch, frames, box, feather, levels)
    # more than one 64 x 16 tile of the pyramid kernels at level 1 needs more than 128 columns: one wide frame
    wide = _rand(13, (1, 40, 300, 3))
    _check(_smooth_patch(14, 1, 32, 200), wide, (1, 2, 297, 37), 12, 3, what="wide")
    assert ops.multiband_levels(12) == 2


def test_patch_scales_strides_and_the_colour_form():
    from denoising_diffusion_deep_fake_amd import ops
    h, w = FRAMES["67x91"]
    B = 3
    frames = _rand(21, (B, h, w, 3))
    small, large = _smooth_patch(22, B, 12, 16), _smooth_patch(23, B, 80, 70)
    _check(small, frames, ODD_BOX, 5, 2, what="up-scale")
    _check(large, frames, ODD_BOX, 5, 2, what="down-scale")
    pair = torch.cat([_rand(24, (B, 24, 20, 3)), _smooth_patch(25, B, 24, 20)], dim=2)  # [B, H, 2W, 3]
    half = pair[:, :, 20:]
    assert not half.is_contiguous()
    got = _check(half, frames, ODD_BOX, 12, 3, what="strided patch")
    assert torch.equal(got, ops.paste_multiband_u8(half.contiguous(), frames, ODD_BOX, 12, 3))
    coef = torch.tensor([[[1.25, -20.0], [0.75, 30.0], [1.0, 0.0]], [[0.5, 100.0], [2.0, -128.0], [1.1, 3.5]],
                         [[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]]], dtype=torch.float32, device="cuda")
    got = _check(half, frames, ODD_BOX, 5, 3, color=coef, what="colour")
    plain = ops.paste_multiband_u8(half, frames, ODD_BOX, 5, 3)
    assert not torch.equal(got[:2], plain[:2]) and torch.equal(got[2], plain[2])  # (1, 0) is the plain form
    # a single frame: [h, w, 3] in and out
    one = ops.paste_multiband_u8(half[0], frames[0], ODD_BOX, 5, 3, color=coef[0])
    assert one.shape == (h, w, 3) and torch.equal(one, got[0])
    # levels=None: the default from the feather
    assert torch.equal(ops.paste_multiband_u8(half, frames, ODD_BOX, 9), ops.paste_multiband_u8(half, frames, ODD_BOX, 9, 2))


def test_a_box_per_frame_equals_the_single_box_calls():
    from denoising_diffusion_deep_fake_amd import ops
    h, w = FRAMES["67x91"]
    B = 3
    frames, patch = _rand(31, (B, h, w, 3)), _smooth_patch(32, B, 24, 20)
    boxes = [(5, 3, 29, 37), (40, 20, 51, 16), (0, 50, 17, 17)]
    coef = torch.tensor([[[1.2, -10.0]] * 3, [[0.8, 25.0]] * 3, [[1.0, 4.0]] * 3], dtype=torch.float32, device="cuda")
    for color in (None, coef):
        for out_arg in ("new", "in place"):
            target = frames.clone()
            got = ops.paste_multiband_u8(patch, target, boxes=boxes, feather=5, levels=2, color=color,
                                         out=target if out_arg == "in place" else None)
            for b in range(B):
                alone = ops.paste_multiband_u8(patch[b], frames[b], boxes[b], 5, 2, color=None if color is None else color[b])
                assert torch.equal(got[b], alone), (b, out_arg, color is not None)
            assert np.array_equal(got.cpu().numpy(), _want(patch, frames, boxes, 5, 2, color))


def test_in_place_and_misaligned_buffers():
    from denoising_diffusion_deep_fake_amd import ops
    h, w = FRAMES["67x91"]
    B = 2
    frames, patch = _rand(41, (B, h, w, 3)), _smooth_patch(42, B, 24, 20)
    want = ops.paste_multiband_u8(patch, frames, ODD_BOX, 5, 3)
    work = frames.clone()
    ret = ops.paste_multiband_u8(patch, work, ODD_BOX, 5, 3, out=work)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work, want)
    # frame and out at byte addresses 1 and 3 past a dword, the patch at 2
    n = frames.numel()
    for off_f, off_o in ((1, 3), (2, 2), (3, 0)):
        sf = torch.zeros(n + 4, dtype=torch.uint8, device="cuda")
        so = torch.full((n + 4,), 9, dtype=torch.uint8, device="cuda")
        sp = torch.zeros(patch.numel() + 4, dtype=torch.uint8, device="cuda")
        f = sf[off_f:off_f + n].view(frames.shape)
        o = so[off_o:off_o + n].view(frames.shape)
        p = sp[2:2 + patch.numel()].view(patch.shape)
        f.copy_(frames)
        p.copy_(patch)
        ops.paste_multiband_u8(p, f, ODD_BOX, 5, 3, out=o)
        assert torch.equal(o, want), (off_f, off_o)
        assert int(so[:off_o].sum()) == 9 * off_o and int(so[off_o + n:].sum()) == 9 * (4 - off_o)  # nothing written outside


def _c_paste(patch, frames, box, feather, levels, ws, ws_bytes, out):
    from denoising_diffusion_deep_fake_amd import _lib
    from denoising_diffusion_deep_fake_amd._lib import ptr, stream_ptr
    B, H, W, _ = patch.shape
    return _lib.lib().d3f_paste_multiband_u8(ptr(patch), B, H, W, patch.stride(1), ptr(frames), frames.shape[1], frames.shape[2],
                                             *box, feather, levels, ptr(ws), ws_bytes, ptr(out), stream_ptr())


def test_a_poisoned_workspace_and_the_c_level_refusals():
    from denoising_diffusion_deep_fake_amd import _lib, ops
    L = _lib.lib()
    h, w = FRAMES["67x91"]
    B = 2
    frames, patch = _rand(51, (B, h, w, 3)), _smooth_patch(52, B, 24, 20)
    x1, y1, cw, ch = ODD_BOX
    for levels in (1, 3):
        need = L.d3f_paste_multiband_workspace_bytes(B, cw, ch, levels)
        assert need > 0 and need % 16 == 0
        ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        out = torch.empty_like(frames)
        assert _c_paste(patch, frames, ODD_BOX, 12, levels, ws, need, out) == 0
        assert torch.equal(out, ops.paste_multiband_u8(patch, frames, ODD_BOX, 12, levels)), levels
        assert bool((ws[need:] == 0xFF).all()), "nothing is written past the workspace"
        # a short workspace, a misaligned one, a null one
        assert _c_paste(patch, frames, ODD_BOX, 12, levels, ws, need - 1, out) != 0
        assert "workspace" in L.d3f_last_error().decode()
        assert _c_paste(patch, frames, ODD_BOX, 12, levels, ws[8:], need, out) != 0
        assert "16 bytes" in L.d3f_last_error().decode()
        assert _c_paste(patch, frames, ODD_BOX, 12, levels, None, need, out) != 0
    assert L.d3f_paste_multiband_workspace_bytes(B, cw, ch, 0) < 0 and L.d3f_paste_multiband_workspace_bytes(B, cw, ch, 7) < 0
    assert L.d3f_paste_multiband_workspace_bytes(B, 0, ch, 2) < 0
    # the workspace inside out
    need = L.d3f_paste_multiband_workspace_bytes(B, cw, ch, 1)
    big = torch.zeros((2 * B, h, w, 3), dtype=torch.uint8, device="cuda")
    assert big.numel() >= need + 16
    assert _c_paste(patch, frames, ODD_BOX, 12, 1, big.view(-1)[16:], need, big[:B]) != 0
    assert "overlaps" in L.d3f_last_error().decode()


def test_refusals():
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    frames, patch = _rand(61, (2, 67, 91, 3)), _rand(62, (2, 24, 20, 3))
    for levels in (0, 7):
        with pytest.raises(D3FError, match="levels"):
            ops.paste_multiband_u8(patch, frames, ODD_BOX, 5, levels)
    with pytest.raises(D3FError, match="below 8 on a side"):
        ops.paste_multiband_u8(patch, frames, (5, 3, 29, 7), 5, 3)
    with pytest.raises(D3FError, match="frame 1: box"):
        ops.paste_multiband_u8(patch, frames, boxes=[(5, 3, 29, 37), (5, 3, 3, 37)], feather=5, levels=2)
    with pytest.raises(D3FError, match="outside"):
        ops.paste_multiband_u8(patch, frames, (80, 3, 29, 37), 5, 2)
    with pytest.raises(D3FError, match="feather"):
        ops.paste_multiband_u8(patch, frames, ODD_BOX, -1, 2)
    with pytest.raises(D3FError, match="overlap"):  # out one frame further in the same buffer
        store = torch.zeros((3, 67, 91, 3), dtype=torch.uint8, device="cuda")
        ops.paste_multiband_u8(patch, store[:2], ODD_BOX, 5, 2, out=store[1:])
    with pytest.raises(D3FError, match="patch overlaps"):
        m = patch.numel()
        store = torch.zeros(m + frames.numel(), dtype=torch.uint8, device="cuda")
        ops.paste_multiband_u8(store[1:m + 1].view(patch.shape), frames, ODD_BOX, 5, 2, out=store[m:].view(frames.shape))
    with pytest.raises(ValueError, match="exactly one"):
        ops.paste_multiband_u8(patch, frames, feather=5)
    with pytest.raises(ValueError):
        ops.paste_multiband_u8(patch[:1], frames, ODD_BOX)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_feather_zero_is_the_plain_paste_at_feather_zero(levels):
    from denoising_diffusion_deep_fake_amd import ops
    frames, patch = _rand(71, (3, 67, 91, 3)), _smooth_patch(72, 3, 24, 20)
    for box in (ODD_BOX, (0, 0, 91, 67), (50, 40, 41, 27)):
        assert torch.equal(ops.paste_multiband_u8(patch, frames, box, 0, levels), ops.paste_resize_cubic_u8(patch, frames, box, 0))
    # D == 0 returns the frame: a frame that already holds the target bytes in the box, at any feather
    pasted = ops.paste_resize_cubic_u8(patch, frames, ODD_BOX, 0)
    assert not torch.equal(pasted, frames)
    assert torch.equal(ops.paste_multiband_u8(patch, pasted, ODD_BOX, 12, levels), pasted)
    same = ops.crop_resize_cubic_u8(frames, (24, 20), ODD_BOX)  # not D == 0, but close: the paste of the crop's own resize
    assert np.array_equal(ops.paste_multiband_u8(same, frames, ODD_BOX, 5, levels).cpu().numpy(),
                          _want(same, frames, [ODD_BOX] * 3, 5, levels))


# ---- the frame call: the smallest network shape of tests/test_gpu_frame_options.py ----
HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)
SIZE, RAW_HW, BOX = (64, 64), (96, 160), (32, 0, 96, 96)
MEAN, STD = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
B = 2
_lits, _raws = {}, []


def _lit(which="first"):
    """as tests/test_gpu_frame_options.py sets its module up; two modules of equal weights, so that one never has the blend set"""
    if which not in _lits:
        from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
        torch.manual_seed(6)
        lit = LitModule(precision="f32", **HP_FAKE).cuda().eval()
        with torch.no_grad():
            for net in (lit.model_a, lit.model_b):
                for name, buf in net.named_buffers():
                    if name.endswith("running_mean"):
                        buf.normal_(0, 0.1)
                    elif name.endswith("running_var"):
                        buf.uniform_(0.5, 1.5)
                net.mark_params_changed()
        _lits[which] = lit
    return _lits[which]


def _writes():
    if not _raws:
        from temporal_restatement import correlated_frames
        frames = correlated_frames(700, 2 * B, *RAW_HW)[0]
        _raws.extend(torch.from_numpy(frames[i * B:(i + 1) * B]).cuda() for i in range(2))
    return _raws


def _color_coef(pair):
    from denoising_diffusion_deep_fake_amd import ops
    real, fake = pair[:, :, :SIZE[1]], pair[:, :, SIZE[1]:]
    return ops.color_match_coef(ops.channel_sums_u8(fake), ops.channel_sums_u8(real), SIZE[0] * SIZE[1])


def test_full_entry_with_multiband_is_the_pair_entry_then_the_operator():
    """eager and replayed from a graph, plain and with the colour match; a change of the levels, of the feather and of the
    blend re-captures; blend="feather" and blend=None are today's bytes"""
    from denoising_diffusion_deep_fake_amd import _lib, ops
    net, other = _lit().model_a, _lit("untouched").model_a
    raw = torch.empty_like(_writes()[0])
    pair = torch.empty((B, SIZE[0], 2 * SIZE[1], 3), dtype=torch.uint8, device="cuda")
    full = torch.empty_like(raw)
    assert ops.default_feather(96, 96) == 6 and ops.multiband_levels(6) == 1
    steps = [("multiband", None, None, None), ("multiband", None, 12, 3), ("multiband", "meanstd", 12, 3),
             ("feather", "meanstd", 12, None), (None, None, 12, None), ("multiband", None, 12, 3), ("multiband", None, 12, 2)]
    for graph in (False, True):
        for step, (blend, color, feather, levels) in enumerate(steps):
            for it in range(2):
                raw.copy_(_writes()[it])
                pair.fill_(7)
                full.fill_(7)
                want_pair = other.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False)
                fake = want_pair[:, :, SIZE[1]:]
                coef = _color_coef(want_pair) if color else None
                fth = 6 if feather is None else feather
                if blend == "multiband":
                    want = ops.paste_multiband_u8(fake, raw, BOX, fth, levels, color=coef)
                    assert not torch.equal(want, ops.paste_resize_cubic_u8(fake, raw, BOX, fth, color=coef))
                else:
                    want = ops.paste_resize_cubic_u8(fake, raw, BOX, fth, color=coef)
                got = net.predict_frames_full_u8(raw, SIZE, MEAN, STD, feather=feather, graph=graph, out=full, pair_out=pair,
                                                 color_match=color, blend=blend, blend_levels=levels)
                assert got.data_ptr() == full.data_ptr()
                assert torch.equal(pair, want_pair), (graph, step, it, "pair")
                assert torch.equal(full, want), (graph, step, it, "full")
    eng = net._u8_engine(B, *SIZE, raw.device)
    lv = C.c_int(0)
    assert _lib.lib().d3f_unet_frame_blend(eng.h, C.byref(lv)) == _lib.BLEND_MULTIBAND and lv.value == 2
    # in place, eager; refused with a graph
    from denoising_diffusion_deep_fake_amd import D3FError
    work = _writes()[1].clone()
    net.predict_frames_full_u8(work, SIZE, MEAN, STD, feather=12, graph=False, out=work, blend="multiband", blend_levels=2)
    assert torch.equal(work, full)
    with pytest.raises(D3FError, match="in place"):
        net.predict_frames_full_u8(work, SIZE, MEAN, STD, graph=True, out=work, blend="multiband")
    # six levels need 64 pixels on a side: a 48 x 48 box is refused before any capture
    with pytest.raises(D3FError, match="below 64 on a side"):
        net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=True, blend="multiband", blend_levels=6, boxes=(40, 10, 48, 48))
    with pytest.raises(ValueError, match="blend_levels"):
        net.predict_frames_full_u8(raw, SIZE, MEAN, STD, blend_levels=2)
    with pytest.raises(ValueError, match="blend"):
        net.predict_frames_full_u8(raw, SIZE, MEAN, STD, blend="pyramid")


def test_full_entry_with_multiband_and_the_temporal_filter_and_a_box_per_frame():
    from denoising_diffusion_deep_fake_amd import ops
    net, other = _lit().model_a, _lit("untouched").model_a
    pair = torch.empty((B, SIZE[0], 2 * SIZE[1], 3), dtype=torch.uint8, device="cuda")
    # the filter acts on the pair before the paste: the same sequence through the pair entry of the other module
    for color in (None, "meanstd"):
        net.reset_frame_temporal()
        other.reset_frame_temporal()
        state = ops.TemporalState(*SIZE)
        for it in range(2):
            raw = _writes()[it]
            want_pair = other.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False, temporal=0.75)
            got = net.predict_frames_full_u8(raw, SIZE, MEAN, STD, feather=12, graph=False, pair_out=pair, temporal=0.75,
                                             color_match=color, blend="multiband", blend_levels=3)
            assert torch.equal(pair, want_pair), (color, it)
            coef = None
            if color:
                real, fake = want_pair[:, :, :SIZE[1]], want_pair[:, :, SIZE[1]:]
                s_to = ops.channel_sums_u8(real)
                coef = ops.color_match_coef(ops.channel_sums_u8(fake), s_to, SIZE[0] * SIZE[1])
                ops.color_coef_smooth(coef, s_to, SIZE[0] * SIZE[1], state, 0.75)
            assert torch.equal(got, ops.paste_multiband_u8(want_pair[:, :, SIZE[1]:], raw, BOX, 12, 3, color=coef)), (color, it)
    other.predict_frames_u8(_writes()[0], SIZE, MEAN, STD, graph=False)  # (the filter off again on the module that stays plain)
    boxes = [(32, 0, 96, 96), (10, 8, 80, 72)]
    raw = _writes()[0]
    for color in (None, "meanstd"):
        want_pair = other.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False, boxes=boxes)
        got = net.predict_frames_full_u8(raw, SIZE, MEAN, STD, feather=9, pair_out=pair, boxes=boxes, color_match=color,
                                         blend="multiband")
        assert torch.equal(pair, want_pair)
        coef = _color_coef(want_pair) if color else None
        assert torch.equal(got, ops.paste_multiband_u8(want_pair[:, :, SIZE[1]:], raw, boxes=boxes, feather=9, color=coef))


def test_a_larger_frame_grows_the_workspace_and_both_sizes_stay_right():
    from denoising_diffusion_deep_fake_amd import ops
    net, other = _lit().model_a, _lit("untouched").model_a
    small = _writes()[0]
    large = _rand(81, (B, 130, 200, 3))
    for raw in (small, large, small):
        box = ops.center_crop_box(raw.shape[1], raw.shape[2], SIZE[1], SIZE[0])
        for graph in (False, True):
            want_pair = other.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False)
            got = net.predict_frames_full_u8(raw, SIZE, MEAN, STD, feather=12, graph=graph, blend="multiband", blend_levels=3)
            assert torch.equal(got, ops.paste_multiband_u8(want_pair[:, :, SIZE[1]:], raw, box, 12, 3)), (raw.shape, graph)


def test_render_fake_video_with_multiband_over_two_batches():
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    lit = _lit()
    frames = [f for f in torch.cat(_writes()).cpu().numpy()[:3]]
    batches = [frames[0:2], [frames[2], frames[2]]]
    got = []
    RenderFakeVideo("clip.mp4", None, "a", "64", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                    output="full", blend="multiband", blend_levels=2)
    assert len(got) == 3 and all(f.shape == RAW_HW + (3,) and f.dtype == np.uint8 for f in got)
    mean, std = lit.hparams.mean_b, lit.hparams.std_b
    want = [lit.model_a.predict_frames_full_u8(torch.from_numpy(np.stack(b)).cuda(), SIZE, mean, std, graph=False,
                                               blend="multiband", blend_levels=2).cpu().numpy() for b in batches]
    plain = lit.model_a.predict_frames_full_u8(torch.from_numpy(np.stack(batches[0])).cuda(), SIZE, mean, std,
                                               graph=False).cpu().numpy()
    for i, (k, j) in enumerate([(0, 0), (0, 1), (1, 0)]):
        assert np.array_equal(got[i], want[k][j]), i
    assert not np.array_equal(want[0], plain)
