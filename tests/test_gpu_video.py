"""GPU: the script_tools frame path -- the crop + bicubic resize kernel against its float64 restatement, the fused
raw-frame inference call (resize -> forward -> real|fake pair) bit for bit against the operators it fuses, and the two
frame loops (RenderFakeVideo, VideoToImages) through their frames= / sink= hooks."""
import io

import numpy as np
import pytest
import torch

from resize_restatement import crop_resize_cubic_f64, round_u8

pytestmark = pytest.mark.gpu

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)

TIE_BAND = 1e-3  # ~4x the fp32 accumulation bound: 16 taps, weight sums <= 1.47, values <= 255, a few ulp each ~ 2e-4


def check_against_restatement(got, frames, box, size):
    """bytes equal the rounded float64 restatement wherever its value is farther than TIE_BAND from a .5 tie; inside
    the band at most one level off.  The band must hold under 1 % of the pixels (a condition on the inputs)."""
    for b in range(frames.shape[0]):
        v = crop_resize_cubic_f64(frames[b], box, size)
        want = round_u8(v)
        band = np.abs(v - np.floor(v) - 0.5) <= TIE_BAND
        diff = np.abs(got[b].astype(int) - want.astype(int))
        saturated = ((v < 0) | (v > 255)).mean()
        print(f"frame {b}: {frames.shape[1:3]} -> {size} box {box}: tie band {100 * band.mean():.3f} % of the values, "
              f"{100 * saturated:.2f} % saturate, {int((diff > 0).sum())} bytes differ (max {int(diff.max())})")
        assert band.mean() < 0.01
        assert saturated > 0 or frames.shape[1:3] == tuple(size)  # the clamp is exercised
        assert not diff[~band].any(), (b, int((diff[~band] > 0).sum()), int(diff[~band].max()))
        assert diff.max() <= 1


@pytest.mark.parametrize("seed, batch, hw, size, box", [
    (100, 1, (90, 160), (64, 64), None),              # shrink, crop on width
    (101, 1, (48, 40), (64, 64), None),               # enlarge, replicate border
    (102, 1, (67, 131), (32, 96), None),              # non-integer ratios, crop on height
    (104, 1, (80, 120), (64, 64), (7, 3, 101, 70)),   # an explicit off-centre box
    (105, 3, (90, 160), (64, 64), None),              # a batch of 3 different frames
    (106, 1, (1080, 1920), (448, 448), None),         # source indices large enough to expose an fp32 coordinate
    (107, 1, (700, 900), (32, 32), None),             # a patch beyond the LDS budget: taps read from global memory
    (108, 2, (61, 77), (40, 70), (1, 2, 75, 58)),     # tiles cut by the output's edge, odd row pitch, odd offsets
])
def test_crop_resize_cubic_against_the_restatement(seed, batch, hw, size, box):
    from denoising_diffusion_deep_fake_amd import ops
    frames = np.random.default_rng(seed).integers(0, 256, size=(batch,) + hw + (3,), dtype=np.uint8)
    box = box or ops.center_crop_box(hw[0], hw[1], size[1], size[0])
    dev = torch.from_numpy(frames).cuda()
    got = ops.crop_resize_cubic_u8(dev, size, box=box)
    assert got.shape == (batch,) + size + (3,) and got.dtype == torch.uint8
    check_against_restatement(got.cpu().numpy(), frames, box, size)
    single = ops.crop_resize_cubic_u8(dev[0], size, box=box)  # [h, w, 3] in, [H, W, 3] out
    assert single.shape == size + (3,) and torch.equal(single, got[0])


def test_crop_resize_identity_is_a_byte_copy_and_default_box_is_the_centre_crop():
    from denoising_diffusion_deep_fake_amd import ops
    rng = np.random.default_rng(103)
    frame = torch.from_numpy(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).cuda()
    assert torch.equal(ops.crop_resize_cubic_u8(frame, (64, 64)), frame)
    wide = torch.from_numpy(rng.integers(0, 256, size=(64, 100, 3), dtype=np.uint8)).cuda()
    assert ops.center_crop_box(64, 100, 64, 64) == (18, 0, 64, 64)
    assert torch.equal(ops.crop_resize_cubic_u8(wide, (64, 64)), wide[:, 18:82])  # box=None: a plain centre crop here
    assert torch.equal(ops.crop_resize_cubic_u8(wide, (64, 64), box=(36, 0, 64, 64)), wide[:, 36:])


def test_crop_resize_strided_output_and_argument_errors():
    """writing into the left half of a [B][H][2W][3] buffer leaves the right half untouched"""
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    rng = np.random.default_rng(109)
    frames = torch.from_numpy(rng.integers(0, 256, size=(2, 90, 160, 3), dtype=np.uint8)).cuda()
    packed = ops.crop_resize_cubic_u8(frames, (32, 64))
    pair = torch.full((2, 32, 128, 3), 171, dtype=torch.uint8, device="cuda")
    ret = ops.crop_resize_cubic_u8(frames, (32, 64), out=pair[:, :, :64])
    assert ret.data_ptr() == pair.data_ptr()
    assert torch.equal(pair[:, :, :64], packed) and bool((pair[:, :, 64:] == 171).all())
    ops.crop_resize_cubic_u8(frames, (32, 64), out=pair[:, :, 64:])  # ... and the right half the left one
    assert torch.equal(pair[:, :, 64:], packed) and torch.equal(pair[:, :, :64], packed)
    with pytest.raises(D3FError, match="outside"):
        ops.crop_resize_cubic_u8(frames, (32, 64), box=(100, 0, 61, 90))
    with pytest.raises(D3FError, match="non-positive"):
        ops.crop_resize_cubic_u8(frames, (32, 64), box=(0, 0, 0, 90))
    with pytest.raises(ValueError):  # a wrong shape
        ops.crop_resize_cubic_u8(frames, (32, 64), out=torch.empty((2, 32, 32, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):  # pixels that are not packed
        ops.crop_resize_cubic_u8(frames, (32, 64), out=torch.empty((2, 32, 64, 4), dtype=torch.uint8, device="cuda")[..., :3])
    with pytest.raises(D3FError):    # no CPU fallback
        ops.crop_resize_cubic_u8(frames.cpu(), (32, 64))
    with pytest.raises(ValueError):
        ops.crop_resize_cubic_u8(frames.float(), (32, 64))


def _lit(precision):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    torch.manual_seed(6)
    lit = LitModule(precision=precision, **HP_FAKE).cuda().eval()
    with torch.no_grad():  # non-trivial running statistics
        for net in (lit.model_a, lit.model_b):
            for name, buf in net.named_buffers():
                if name.endswith("running_mean"):
                    buf.normal_(0, 0.1)
                elif name.endswith("running_var"):
                    buf.uniform_(0.5, 1.5)
            net.mark_params_changed()
    return lit


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
def test_predict_frames_u8_is_bit_exact_against_the_ops_it_fuses(precision, B):
    """no tolerance: the left half of the pair equals the standalone resize, the right half predict_u8 of the left half
    at the same batch size -- eager and graph-replayed, four frames through the same buffers with a parameter update
    between replays; then a second raw size on the same module (a stale graph would keep the first geometry)"""
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    net = _lit(precision).model_a
    mean, std = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    rng = np.random.default_rng(11)
    size = (64, 96)

    store = torch.empty(B * 100 * 180 * 3, dtype=torch.uint8, device="cuda")
    buf_out = torch.empty((B, 64, 192, 3), dtype=torch.uint8, device="cuda")

    def run(raw_hw, iterations):
        # both raw sizes start at the same address and write the same output: only the geometry tells their graphs apart
        buf_in = store[:B * raw_hw[0] * raw_hw[1] * 3].view((B,) + raw_hw + (3,))
        for it in range(iterations):
            buf_in.copy_(torch.from_numpy(rng.integers(0, 256, size=tuple(buf_in.shape), dtype=np.uint8)))
            left = ops.crop_resize_cubic_u8(buf_in, size)
            right = net.predict_u8(left, mean, std, graph=False)
            eager = net.predict_frames_u8(buf_in, size, mean, std, graph=False)
            assert eager.shape == (B, 64, 192, 3)
            assert torch.equal(eager[:, :, :96], left), (it, "eager left")
            assert torch.equal(eager[:, :, 96:], right), (it, "eager right")
            buf_out.fill_(7)
            replay = net.predict_frames_u8(buf_in, size, mean, std, graph=True, out=buf_out)
            assert replay.data_ptr() == buf_out.data_ptr()
            assert torch.equal(replay, eager), (it, "replay")
            if it == 1:  # a parameter update between replays: the graph must see the re-packed weights
                with torch.no_grad():
                    net.segmentation_head[0].bias.add_(0.05)
                    next(iter(net.parameters())).mul_(1.01)
        return buf_in

    buf_in = run((100, 180), 4)
    engines = [e for pool in net._rt["engines"].values() for e in pool]  # the plan keeps what its graph baked in alive
    assert any(getattr(e, "keep", None) is not None and e.keep[0] is buf_in and e.keep[1] is buf_out for e in engines)
    assert run((75, 91), 2).data_ptr() == buf_in.data_ptr()  # another frame size and crop box, same module and plan
    run((100, 180), 1)
    # a single frame: [h, w, 3] in, [H, 2W, 3] out
    if B == 1:
        one = net.predict_frames_u8(buf_in[0], size, mean, std, graph=False)
        assert one.shape == (64, 192, 3) and torch.equal(one, net.predict_frames_u8(buf_in, size, mean, std, graph=False)[0])
    # the argument errors, as predict_u8's
    with pytest.raises(RuntimeError, match="divisible by 32"):
        net.predict_frames_u8(buf_in, (60, 96), mean, std)
    with pytest.raises(ValueError):
        net.predict_frames_u8(buf_in.float(), size, mean, std)
    with pytest.raises(ValueError):
        net.predict_frames_u8(buf_in[..., :2], size, mean, std)
    with pytest.raises(D3FError):
        net.predict_frames_u8(buf_in.cpu(), size, mean, std)
    with pytest.raises(ValueError):
        net.predict_frames_u8(buf_in, size, mean, std, out=torch.empty((B, 64, 96, 3), dtype=torch.uint8, device="cuda"))


def test_render_fake_video_loop_and_predict_fake_frames():
    """RenderFakeVideo over 5 host frames, 2 at a time: 5 frames reach the sink, each equal to Unet.predict_frames_u8 of
    the same batches (the last one padded by repeating its frame); predict_fake_frames feeds model a the statistics of
    domain b and the other way round"""
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    lit = _lit("f32")
    lit.hparams.mean_a, lit.hparams.std_a = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    lit.hparams.mean_b, lit.hparams.std_b = [0.45, 0.4, 0.55], [0.6, 0.5, 0.4]
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 256, size=(100, 180, 3), dtype=np.uint8) for _ in range(5)]
    for which, model, mean, std in (("a", lit.model_a, lit.hparams.mean_b, lit.hparams.std_b),
                                    ("b", lit.model_b, lit.hparams.mean_a, lit.hparams.std_a)):
        got = []
        RenderFakeVideo("clip.mp4", None, which, "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit)
        assert len(got) == 5 and all(f.shape == (64, 192, 3) and f.dtype == np.uint8 for f in got)
        batches = [frames[0:2], frames[2:4], [frames[4], frames[4]]]
        want = [model.predict_frames_u8(torch.from_numpy(np.stack(b)).cuda(), (64, 96), mean, std, graph=False).cpu().numpy()
                for b in batches]
        want = [want[0][0], want[0][1], want[1][0], want[1][1], want[2][0]]
        for i in range(5):
            assert np.array_equal(got[i], want[i]), (which, i)
        direct = lit.predict_fake_frames(np.stack(frames[0:2]), which, 96, 64)
        assert direct.shape == (2, 64, 192, 3) and np.array_equal(direct[0], want[0]) and np.array_equal(direct[1], want[1])
    # the two models differ, and so do the two domains' statistics: a mix-up would show
    a = lit.predict_fake_frames(np.stack(frames[0:2]), "a", 96, 64)
    b = lit.predict_fake_frames(np.stack(frames[0:2]), "b", 96, 64)
    assert np.array_equal(a[:, :, :96], b[:, :, :96]) and not np.array_equal(a[:, :, 96:], b[:, :, 96:])
    wrong = lit.model_a.predict_frames_u8(torch.from_numpy(np.stack(frames[0:2])).cuda(), (64, 96), lit.hparams.mean_a,
                                          lit.hparams.std_a, graph=False).cpu().numpy()
    assert not np.array_equal(a, wrong)
    assert len(lit._frames_buffers) == 2  # one set of staging buffers per (shape, model), reused


def test_video_to_images_writes_the_reference_layout(tmp_path):
    """VideoToImages(frames=...): <stem>_w<W>_h<H>/000000.jpg ... and images.txt with relative paths; a decoded JPEG
    equals a PIL round trip of the op's own bytes (the JPEG loss is PIL's, not an invented tolerance)"""
    from PIL import Image

    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images import VideoToImages
    rng = np.random.default_rng(13)
    frames = [rng.integers(0, 256, size=(90, 160, 3), dtype=np.uint8) for _ in range(5)]
    tool = VideoToImages(tmp_path / "clip.mp4", "64", "32", batch_frames=2, frames=iter(frames))
    out = tmp_path / "clip_w64_h32"
    assert tool.output_dir_path == out
    names = [f"{i:06}.jpg" for i in range(5)]
    assert sorted(p.name for p in out.iterdir()) == names + ["images.txt"]
    assert (out / "images.txt").read_text() == "".join(n + "\n" for n in names)
    resized = ops.crop_resize_cubic_u8(torch.from_numpy(np.stack(frames)).cuda(), (32, 64)).cpu().numpy()
    for i, name in enumerate(names):
        with Image.open(out / name) as im:
            assert im.size == (64, 32) and im.mode == "RGB"
            got = np.array(im)
        blob = io.BytesIO()
        Image.fromarray(resized[i][:, :, ::-1].copy()).save(blob, format="JPEG")  # BGR -> RGB, PIL's default quality
        with Image.open(blob) as im:
            want = np.array(im)
        assert np.array_equal(got, want), i
