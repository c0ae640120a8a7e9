"""GPU: full-frame output -- the paste kernel against its float64 restatement and, where the definition is exact, byte
for byte; its forms (in place, strided patch, single frame, guard bands); the fused raw-frame inference call
(resize -> forward -> pair -> paste) bit for bit against the operators it fuses; and the render loop in full mode."""
import numpy as np
import pytest
import torch

from paste_restatement import paste_f64, ramp
from resize_restatement import round_u8

pytestmark = pytest.mark.gpu

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)

# tests/test_gpu_video.py's band: ~4x the fp32 accumulation bound of the 16 taps (~2e-4); the blend's two products and sum
# add three roundings of values <= 255, ~5e-5
TIE_BAND = 1e-3


def _lit(precision):
    """as tests/test_gpu_video.py sets its module up: non-trivial running statistics"""
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    torch.manual_seed(6)
    lit = LitModule(precision=precision, **HP_FAKE).cuda().eval()
    with torch.no_grad():
        for net in (lit.model_a, lit.model_b):
            for name, buf in net.named_buffers():
                if name.endswith("running_mean"):
                    buf.normal_(0, 0.1)
                elif name.endswith("running_var"):
                    buf.uniform_(0.5, 1.5)
            net.mark_params_changed()
    return lit

# (seed, batch, frame h x w, patch H x W, box, feather)
CASES = [
    (200, 1, (90, 160), (64, 64), (35, 0, 90, 90), 7),            # enlarge
    (201, 1, (90, 160), (64, 64), (35, 0, 90, 90), 0),            # enlarge, no feather
    (202, 1, (48, 40), (64, 64), (0, 4, 40, 40), 3),              # shrink, box flush with two frame edges
    (203, 1, (80, 120), (64, 64), (7, 3, 101, 70), 12),           # anisotropic, off centre, odd offsets
    (204, 2, (61, 77), (40, 70), (1, 2, 75, 58), 40),             # no pixel with a == 1, tiles cut by the edge
    (205, 1, (1080, 1920), (448, 448), (420, 0, 1080, 1080), 67),  # source indices that would expose an fp32 coordinate
    (206, 1, (700, 900), (448, 448), (100, 50, 24, 24), 2),       # a tiny box: the patch region passes the LDS budget
]

_cache = {}


def _case(case):
    """inputs, the device result and the float64 restatement of a case, computed once and shared (read only)"""
    if case not in _cache:
        from denoising_diffusion_deep_fake_amd import ops
        seed, batch, hw, patch_hw, box, feather = case
        rng = np.random.default_rng(seed)
        patch = rng.integers(0, 256, size=(batch,) + patch_hw + (3,), dtype=np.uint8)
        frames = rng.integers(0, 256, size=(batch,) + hw + (3,), dtype=np.uint8)
        dev_patch, dev_frames = torch.from_numpy(patch).cuda(), torch.from_numpy(frames).cuda()
        got = ops.paste_resize_cubic_u8(dev_patch, dev_frames, box, feather)
        assert got.shape == dev_frames.shape and got.dtype == torch.uint8 and got.data_ptr() != dev_frames.data_ptr()
        assert torch.equal(dev_frames.cpu(), torch.from_numpy(frames))  # the input is left alone
        want = np.stack([paste_f64(patch[b], frames[b], box, feather) for b in range(batch)])
        _cache[case] = (patch, frames, dev_patch, dev_frames, got, want)
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=[f"case{i + 1}" for i in range(len(CASES))])
def test_paste_against_the_restatement(case):
    """the tie rule of tests/test_gpu_video.py: bytes equal the rounded float64 value wherever it is farther than
    TIE_BAND from a .5 tie, inside the band at most one level off, the band holds under 1 % of the box's values; the
    bytes outside the box equal the frame exactly"""
    seed, batch, hw, patch_hw, (x1, y1, cw, ch), feather = case
    patch, frames, _, _, got, want = _case(case)
    got = got.cpu().numpy()
    outside = np.ones(hw, dtype=bool)
    outside[y1:y1 + ch, x1:x1 + cw] = False
    for b in range(batch):
        assert np.array_equal(got[b][outside], frames[b][outside]), b
        v = want[b][y1:y1 + ch, x1:x1 + cw]
        band = np.abs(v - np.floor(v) - 0.5) <= TIE_BAND
        diff = np.abs(got[b][y1:y1 + ch, x1:x1 + cw].astype(int) - round_u8(v).astype(int))
        print(f"frame {b}: patch {patch_hw} -> box {(x1, y1, cw, ch)} of {hw}, feather {feather}: tie band "
              f"{100 * band.mean():.3f} % of the box's values, {int((diff > 0).sum())} bytes differ (max {int(diff.max())})")
        assert band.mean() < 0.01
        assert not diff[~band].any(), (b, int((diff[~band] > 0).sum()), int(diff[~band].max()))
        assert diff.max() <= 1


@pytest.mark.parametrize("case", CASES, ids=[f"case{i + 1}" for i in range(len(CASES))])
def test_paste_interior_is_the_resize_operator_bit_for_bit(case):
    """where a == 1 the byte is rintf(v): what d3f_crop_resize_cubic_u8(patch -> ch x cw) writes"""
    from denoising_diffusion_deep_fake_amd import ops
    seed, batch, hw, patch_hw, (x1, y1, cw, ch), feather = case
    _, _, dev_patch, _, got, _ = _case(case)
    resized = ops.crop_resize_cubic_u8(dev_patch, (ch, cw), box=(0, 0, patch_hw[1], patch_hw[0]))
    inner = torch.from_numpy(ramp(cw, ch, feather) == 1).cuda()
    assert bool(inner.any()) == (2 * feather < min(cw, ch))
    assert torch.equal(got[:, y1:y1 + ch, x1:x1 + cw][:, inner], resized[:, inner])


def test_paste_exact_case_pins_half_to_even():
    """equal extents and feather + 1 = 4: v is an integer and a a multiple of 1/16, so the blend is exact in fp32 and the
    bytes equal the rounded restatement everywhere, the exact .5 ties (several per cent of the values) included"""
    from denoising_diffusion_deep_fake_amd import ops
    rng = np.random.default_rng(210)
    patch = rng.integers(0, 256, size=(1, 64, 64, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, size=(1, 64, 100, 3), dtype=np.uint8)
    box = (18, 0, 64, 64)
    got = ops.paste_resize_cubic_u8(torch.from_numpy(patch).cuda(), torch.from_numpy(frames).cuda(), box, 3).cpu().numpy()
    v = paste_f64(patch[0], frames[0], box, 3)
    ties = (v[:, 18:82] - np.floor(v[:, 18:82]) == 0.5).mean()
    print(f"exact ties: {100 * ties:.2f} % of the box's values")
    assert ties > 0.02
    assert np.array_equal(got[0], round_u8(v))


def test_paste_forms():
    """in place equals out of place; a strided patch (the right half of a pair buffer) equals the packed one; a single frame
    equals row 0 of the batch; a repeat is bit for bit; a guard band around out is untouched; out= is written and returned"""
    from denoising_diffusion_deep_fake_amd import ops
    seed, batch, hw, patch_hw, box, feather = CASES[4]
    _, _, dev_patch, dev_frames, got, _ = _case(CASES[4])
    H, W = patch_hw
    assert torch.equal(ops.paste_resize_cubic_u8(dev_patch, dev_frames, box, feather), got)  # a repeat
    work = dev_frames.clone()
    ret = ops.paste_resize_cubic_u8(dev_patch, work, box, feather, out=work)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work, got)
    pair = torch.full((batch, H, 2 * W, 3), 99, dtype=torch.uint8, device="cuda")
    pair[:, :, W:] = dev_patch
    assert torch.equal(ops.paste_resize_cubic_u8(pair[:, :, W:], dev_frames, box, feather), got)
    one = ops.paste_resize_cubic_u8(dev_patch[0], dev_frames[0], box, feather)
    assert one.shape == hw + (3,) and torch.equal(one, got[0])
    one_in_place = dev_frames[0].clone()
    ops.paste_resize_cubic_u8(pair[0, :, W:], one_in_place, box, feather, out=one_in_place)
    assert torch.equal(one_in_place, got[0])
    # guard bands: out inside a larger buffer of a sentinel byte, at an aligned and at an odd offset.  (Every tile of
    # this geometry meets the box: the copy tiles' paths are test_paste_copy_tiles_* below.)
    n = got.numel()
    for lead in (256, 259):
        store = torch.full((lead + n + 301,), 0xA5, dtype=torch.uint8, device="cuda")
        out = store[lead:lead + n].view(got.shape)
        ret = ops.paste_resize_cubic_u8(dev_patch, dev_frames, box, feather, out=out)
        assert ret.data_ptr() == out.data_ptr() and torch.equal(out, got)
        assert bool((store[:lead] == 0xA5).all()) and bool((store[lead + n:] == 0xA5).all())
    # in place inside guard bands: nothing outside the frames moves, nothing outside the box changes
    store = torch.full((256 + n + 300,), 0xA5, dtype=torch.uint8, device="cuda")
    work = store[256:256 + n].view(got.shape)
    work.copy_(dev_frames)
    ops.paste_resize_cubic_u8(dev_patch, work, box, feather, out=work)
    assert torch.equal(work, got) and bool((store[:256] == 0xA5).all()) and bool((store[256 + n:] == 0xA5).all())


# copy tiles: a frame whose row pitch (3 * 161 = 483 bytes) is no multiple of 4, so rows start 0, 3, 2, 1, ... bytes past
# a dword, with a box well inside it: tile columns 0, 4 and 5 (the last one a single pixel wide) and tile rows 0, 1 and
# 9 to 11 (the last one 2 rows high) lie wholly outside the box and are copied, B = 2
COPY_HW, COPY_PATCH_HW, COPY_BOX, COPY_FEATHER = (90, 161), (40, 70), (40, 20, 70, 45), 6


def _copy_case():
    if "copy" not in _cache:
        rng = np.random.default_rng(250)
        patch = rng.integers(0, 256, size=(2,) + COPY_PATCH_HW + (3,), dtype=np.uint8)
        frames = rng.integers(0, 256, size=(2,) + COPY_HW + (3,), dtype=np.uint8)
        want = np.stack([paste_f64(patch[b], frames[b], COPY_BOX, COPY_FEATHER) for b in range(2)])
        _cache["copy"] = (frames, torch.from_numpy(patch).cuda(), torch.from_numpy(frames).cuda(), want)
    return _cache["copy"]


@pytest.mark.parametrize("lead", [256, 257, 259], ids=["aligned", "one_past", "three_past"])
def test_paste_copy_tiles_out_of_place(lead):
    """out at `lead` bytes into a buffer of a sentinel byte, the frames allocator-aligned.  lead 256: frame and out sit
    alike within a dword, so the copy tiles move dwords, with ragged heads and tails of 1 to 3 bytes on three rows of
    four; lead 257 / 259: they sit differently and the copy tiles move bytes.  Outside the box the bytes are the frame's,
    inside it the restatement's under the tie rule, and the sentinels around out are untouched"""
    from denoising_diffusion_deep_fake_amd import ops
    frames, dev_patch, dev_frames, want = _copy_case()
    x1, y1, cw, ch = COPY_BOX
    n = dev_frames.numel()
    store = torch.full((lead + n + 301,), 0xA5, dtype=torch.uint8, device="cuda")
    out = store[lead:lead + n].view(dev_frames.shape)
    assert out.data_ptr() % 4 == lead % 4 and dev_frames.data_ptr() % 4 == 0
    ret = ops.paste_resize_cubic_u8(dev_patch, dev_frames, COPY_BOX, COPY_FEATHER, out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert bool((store[:lead] == 0xA5).all()) and bool((store[lead + n:] == 0xA5).all())
    got = out.cpu().numpy()
    outside = np.ones(COPY_HW, dtype=bool)
    outside[y1:y1 + ch, x1:x1 + cw] = False
    for b in range(2):
        assert np.array_equal(got[b][outside], frames[b][outside]), b
        v = want[b][y1:y1 + ch, x1:x1 + cw]
        band = np.abs(v - np.floor(v) - 0.5) <= TIE_BAND
        diff = np.abs(got[b][y1:y1 + ch, x1:x1 + cw].astype(int) - round_u8(v).astype(int))
        print(f"frame {b}, lead {lead}: tie band {100 * band.mean():.3f} % of the box's values, "
              f"{int((diff > 0).sum())} bytes differ (max {int(diff.max())})")
        assert band.mean() < 0.01 and not diff[~band].any() and diff.max() <= 1
    assert torch.equal(dev_frames.cpu(), torch.from_numpy(frames))  # the input is left alone


def test_paste_copy_tiles_in_place_and_misaligned_frames():
    """in place equals out of place on the copy-tile geometry, with sentinels around the frames; frames that start 3 bytes
    past a dword pasted into an out that starts 3 past too (the dword path with every row's head ragged) and into an
    aligned out (the byte path) give the same bytes; a patch that ends where out begins is accepted"""
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    frames, dev_patch, dev_frames, _ = _copy_case()
    ref = ops.paste_resize_cubic_u8(dev_patch, dev_frames, COPY_BOX, COPY_FEATHER)
    n = dev_frames.numel()
    store = torch.full((256 + n + 300,), 0xA5, dtype=torch.uint8, device="cuda")
    work = store[256:256 + n].view(dev_frames.shape)
    work.copy_(dev_frames)
    ops.paste_resize_cubic_u8(dev_patch, work, COPY_BOX, COPY_FEATHER, out=work)
    assert torch.equal(work, ref) and bool((store[:256] == 0xA5).all()) and bool((store[256 + n:] == 0xA5).all())
    shifted = torch.empty((n + 3,), dtype=torch.uint8, device="cuda")[3:].view(dev_frames.shape)
    shifted.copy_(dev_frames)
    for lead in (259, 256):
        store = torch.full((lead + n + 301,), 0xA5, dtype=torch.uint8, device="cuda")
        out = store[lead:lead + n].view(dev_frames.shape)
        ops.paste_resize_cubic_u8(dev_patch, shifted, COPY_BOX, COPY_FEATHER, out=out)
        assert torch.equal(out, ref), lead
        assert bool((store[:lead] == 0xA5).all()) and bool((store[lead + n:] == 0xA5).all())
    # patch and out in one buffer: adjacent is accepted, one byte of overlap refused
    m = dev_patch.numel()
    store = torch.empty((m + n,), dtype=torch.uint8, device="cuda")
    store[:m] = dev_patch.reshape(-1)
    out = store[m:].view(dev_frames.shape)
    ops.paste_resize_cubic_u8(store[:m].view(dev_patch.shape), dev_frames, COPY_BOX, COPY_FEATHER, out=out)
    assert torch.equal(out, ref) and torch.equal(store[:m].view(dev_patch.shape), dev_patch)
    with pytest.raises(D3FError, match="patch overlaps"):
        ops.paste_resize_cubic_u8(store[1:m + 1].view(dev_patch.shape), dev_frames, COPY_BOX, COPY_FEATHER, out=out)


def test_paste_argument_errors():
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    patch = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    frames = torch.zeros((2, 90, 160, 3), dtype=torch.uint8, device="cuda")
    box = (35, 0, 90, 90)
    with pytest.raises(D3FError, match="outside"):
        ops.paste_resize_cubic_u8(patch, frames, (100, 0, 61, 90))
    with pytest.raises(D3FError, match="non-positive"):
        ops.paste_resize_cubic_u8(patch, frames, (0, 0, 0, 90))
    with pytest.raises(D3FError, match="feather"):
        ops.paste_resize_cubic_u8(patch, frames, box, feather=-1)
    with pytest.raises(D3FError, match="overlap"):  # out one frame further in the same buffer
        store = torch.zeros((3, 90, 160, 3), dtype=torch.uint8, device="cuda")
        ops.paste_resize_cubic_u8(patch, store[:2], box, out=store[1:])
    with pytest.raises(ValueError):  # a wrong shape
        ops.paste_resize_cubic_u8(patch, frames, box, out=torch.empty((2, 90, 90, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):  # a batch of another size
        ops.paste_resize_cubic_u8(patch[:1], frames, box)
    with pytest.raises(ValueError):  # pixels that are not packed
        ops.paste_resize_cubic_u8(torch.zeros((2, 64, 64, 4), dtype=torch.uint8, device="cuda")[..., :3], frames, box)
    with pytest.raises(D3FError):    # no CPU fallback
        ops.paste_resize_cubic_u8(patch.cpu(), frames.cpu(), box)
    with pytest.raises(ValueError):
        ops.paste_resize_cubic_u8(patch.float(), frames, box)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
def test_predict_frames_full_u8_is_bit_exact_against_the_ops_it_fuses(precision, B):
    """no tolerance: pair_out equals predict_frames_u8, full_out the paste of its right half into the raw frames -- eager
    and graph-replayed, with new input bytes between replays and predict_frames_u8's own graph alternating with this one"""
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    net = _lit(precision).model_a
    mean, std = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    rng = np.random.default_rng(220 + B)
    size, hw = (64, 64), (90, 160)
    box = ops.center_crop_box(hw[0], hw[1], 64, 64)
    assert box == (35, 0, 90, 90) and ops.default_feather(90, 90) == 5
    raw = torch.empty((B,) + hw + (3,), dtype=torch.uint8, device="cuda")
    pair_buf = torch.empty((B, 64, 128, 3), dtype=torch.uint8, device="cuda")
    pair_buf2 = torch.empty_like(pair_buf)
    full_buf = torch.empty_like(raw)
    for it in range(3):
        raw.copy_(torch.from_numpy(rng.integers(0, 256, size=tuple(raw.shape), dtype=np.uint8)))
        feather = None if it < 2 else 11
        want_pair = net.predict_frames_u8(raw, size, mean, std, graph=False)
        want_full = ops.paste_resize_cubic_u8(want_pair[:, :, 64:], raw, box, 5 if feather is None else feather)
        assert not torch.equal(want_full, raw)
        pair_e = torch.zeros_like(pair_buf)
        eager = net.predict_frames_full_u8(raw, size, mean, std, feather=feather, graph=False, pair_out=pair_e)
        assert eager.shape == raw.shape and torch.equal(pair_e, want_pair), (it, "eager pair")
        assert torch.equal(eager, want_full), (it, "eager full")
        pair_buf.fill_(7)
        full_buf.fill_(7)
        replay = net.predict_frames_full_u8(raw, size, mean, std, feather=feather, graph=True, out=full_buf, pair_out=pair_buf)
        assert replay.data_ptr() == full_buf.data_ptr()
        assert torch.equal(pair_buf, want_pair) and torch.equal(replay, want_full), (it, "replay")
        # the other entry's graph between two replays of this one: each keeps its own slot and stays right
        pair_buf2.fill_(9)
        assert torch.equal(net.predict_frames_u8(raw, size, mean, std, graph=True, out=pair_buf2), want_pair), (it, "pair graph")
        full_buf.fill_(3)
        net.predict_frames_full_u8(raw, size, mean, std, feather=feather, graph=True, out=full_buf, pair_out=pair_buf)
        assert torch.equal(full_buf, want_full), (it, "second replay")
    # in place, eager; refused with a graph
    work = raw.clone()
    ret = net.predict_frames_full_u8(work, size, mean, std, feather=11, graph=False, out=work)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work, want_full)
    with pytest.raises(D3FError, match="in place"):
        net.predict_frames_full_u8(work, size, mean, std, graph=True, out=work)
    if B == 1:  # a single frame: [h, w, 3] in and out
        one = net.predict_frames_full_u8(raw[0], size, mean, std, feather=11, graph=False)
        assert one.shape == hw + (3,) and torch.equal(one, want_full[0])
    with pytest.raises(RuntimeError, match="divisible by 32"):
        net.predict_frames_full_u8(raw, (60, 96), mean, std)
    with pytest.raises(ValueError):
        net.predict_frames_full_u8(raw, size, mean, std, out=torch.empty((B, 64, 64, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        net.predict_frames_full_u8(raw, size, mean, std, pair_out=torch.empty((B, 64, 64, 3), dtype=torch.uint8, device="cuda"))


def test_predict_frames_full_u8_honours_a_sigmoid_head():
    """with an activation on the segmentation head the result is still the composition of the two entries"""
    from denoising_diffusion_deep_fake_amd import Unet, ops
    torch.manual_seed(8)
    net = Unet("resnet18", None, 3, 3, "sigmoid").cuda().eval()
    plain = Unet("resnet18", None, 3, 3, None).cuda().eval()
    plain.load_state_dict(net.state_dict())
    mean, std = [0.1, 0.2, 0.15], [0.9, 0.8, 0.85]
    raw = torch.from_numpy(np.random.default_rng(230).integers(0, 256, size=(2, 90, 160, 3), dtype=np.uint8)).cuda()
    pair = net.predict_frames_u8(raw, (64, 64), mean, std, graph=False)
    assert not torch.equal(pair, plain.predict_frames_u8(raw, (64, 64), mean, std, graph=False))  # the head matters
    want = ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, (35, 0, 90, 90), 5)
    for graph in (False, True):
        got_pair = torch.zeros_like(pair)
        got = net.predict_frames_full_u8(raw, (64, 64), mean, std, graph=graph, pair_out=got_pair)
        assert torch.equal(got_pair, pair) and torch.equal(got, want), graph


def test_render_fake_video_full_output_loop():
    """RenderFakeVideo(output="full") over 5 host frames, 2 at a time: 5 frames of the source's shape reach the sink, each
    equal to Unet.predict_frames_full_u8 of its batch; output="pair" through the same objects gives what it gives without
    the feature (predict_frames_u8 of the same batches)"""
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    lit = _lit("f32")
    lit.hparams.mean_a, lit.hparams.std_a = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    lit.hparams.mean_b, lit.hparams.std_b = [0.45, 0.4, 0.55], [0.6, 0.5, 0.4]
    rng = np.random.default_rng(240)
    frames = [rng.integers(0, 256, size=(100, 180, 3), dtype=np.uint8) for _ in range(5)]
    batches = [frames[0:2], frames[2:4], [frames[4], frames[4]]]
    order = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    model, mean, std = lit.model_a, lit.hparams.mean_b, lit.hparams.std_b
    for feather in (None, 9):
        got = []
        RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                        output="full", feather=feather)
        assert len(got) == 5 and all(f.shape == (100, 180, 3) and f.dtype == np.uint8 for f in got)
        want = [model.predict_frames_full_u8(torch.from_numpy(np.stack(b)).cuda(), (64, 96), mean, std, feather=feather,
                                             graph=False).cpu().numpy() for b in batches]
        for i, (k, j) in enumerate(order):
            assert np.array_equal(got[i], want[k][j]), (feather, i)
            assert not np.array_equal(got[i], frames[i])
    got = []
    RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                    output="pair")
    want = [model.predict_frames_u8(torch.from_numpy(np.stack(b)).cuda(), (64, 96), mean, std, graph=False).cpu().numpy()
            for b in batches]
    assert len(got) == 5
    for i, (k, j) in enumerate(order):
        assert got[i].shape == (64, 192, 3) and np.array_equal(got[i], want[k][j]), i
    full, pair = lit.predict_fake_frames_full(np.stack(frames[0:2]), "a", 96, 64, with_pair=True)
    assert np.array_equal(pair, want[0]) and np.array_equal(pair, lit.predict_fake_frames(np.stack(frames[0:2]), "a", 96, 64))
    assert full.shape == (2, 100, 180, 3)
    assert len(lit._frames_full_buffers) == 3  # in, full and pair staging of one (shape, model), reused by every call
