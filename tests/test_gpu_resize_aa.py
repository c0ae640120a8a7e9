"""GPU: the antialiased crop + bicubic resize (d3f_crop_resize_cubic_aa_u8) against its float64 restatement, the default
path unchanged, the fused frame entries in the antialiased mode bit for bit against the operators they fuse -- eager and
graph-replayed with the mode alternating -- and the two frame loops with antialias=True."""
import io

import numpy as np
import pytest
import torch

from resize_aa_restatement import axis_taps_aa, axis_windows_aa, case_taps_aa, crop_resize_cubic_aa_f64, keys_weight_aa
from resize_restatement import round_u8

pytestmark = pytest.mark.gpu

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)

U = 2.0 ** -24  # unit roundoff of fp32, round to nearest

# TIE_BAND of a case: the worst-case error of the kernel's fp32 arithmetic against the exact value, derived from the
# order of operations include/d3f_hip.h fixes -- to first order in U (the second-order terms are below 1e-5 of it) and
# from nothing the kernel outputs.  Per axis and output index, x_t = |a_t| the exact tap offsets, w_t = keys(x_t),
# W = sum w_t, wn_t = w_t / W, L = sum |wn_t|:
#   * a_t: one correctly rounded division of exact integers, relative error U.  keys in Horner form, every operation
#     relative error U of its own result, carried through the remaining operations:
#       x < 1:       1.5 x | - 2.5 | * x | * x | + 1     errors 1.5x, 2.5, 5x - 1.5x^2, 7.5x^2 - 3x^3, then + |w| <= 1
#                    -> (1 + 5x^2 - 1.5x^3) U, and |keys'(x)| x U = (5x^2 - 4.5x^3) U from a_t:   eps(x) = 1 + 10x^2 - 6x^3
#       1 <= x < 2:  -0.5 x (exact) | + 2.5 | * x | - 4 | * x | + 2   errors 0, 2.5 - 0.5x, 5x - x^2, 4 + 2.5x - 0.5x^2, 8x,
#                    then + |w| -> (8x + |w|) U, and |-1.5x^2 + 5x - 4| x U from a_t:   eps(x) = 8x + |w| + |g(x)| x
#       x >= 2: the weight is an exact 0.
#     So |w^_t - w_t| <= eps(x_t) U; E = sum_t eps(x_t) / |W|.
#   * the weights' sum: eight interleaved partial sums and a three-level tree, d_s = ceil(n / 8) - 1 + 3 additions deep:
#     |sum^ - W| <= (E |W| + d_s sum |w_t|) U; one more rounding for the quotient:
#       omega = sum_t |wn^_t - wn_t| <= (E + L (E + d_s L) + L) U
#   * horizontal pass: a product and ceil(n / 4) - 1 + 2 additions on any term's way (the first addition is to an exact
#     0): d_h = ceil(n / 4) + 2;  |h^ - h| <= 255 (omega + d_h L) U, and |h| <= 255 L
#   * vertical pass: a product, at most 7 additions inside a chunk of 8 rows, one addition per chunk the window meets
#     (ceil((n - 1) / 8) + 1 of them): d_v = 9 + ceil((n - 1) / 8);
#       |v^ - v| <= L_y max|h^ - h| + 255 L_x (omega_y + d_v L_y) U
#   TIE_BAND = 255 U (L_y Om_x + L_x Om_y), Om = the axis' max over its output indices of omega + d L, L_x and L_y the
#   axes' largest L.  In units of 2^-24 * 255 * S with S = L_x L_y that is d_h(n_x) + d_v(n_y) plus 130 to 150 for the
#   weights -- the Horner form of the outer lobe loses 8x U against a value below 0.075 -- where plain left-to-right sums
#   of exact weights would give n_x + n_y + 6: 127 (seed 207) to 190 (seed 205) over the cases below.


def _eps(x):
    w = np.abs(keys_weight_aa(x))
    inner = 1 + 10 * x * x - 6 * x ** 3
    outer = 8 * x + w + np.abs(-1.5 * x * x + 5 * x - 4) * x
    return np.where(x < 1, inner, np.where(x < 2, outer, 0.0))


def _axis_bound(n_in, n_out, depth):
    """-> (Om, L) of an axis n_in -> n_out whose pass is `depth(n)` operations deep"""
    xmin, xmax, D = axis_windows_aa(n_in, n_out)
    _, count, wn = axis_taps_aa(n_in, n_out)
    i = np.arange(n_out, dtype=np.int64)
    k = xmin[:, None] + np.arange(int(count.max()), dtype=np.int64)[None, :]
    valid = k < xmax[:, None]
    x = np.abs((2 * k + 1) * n_out - ((2 * i + 1) * n_in)[:, None]) / D
    W = np.abs(np.where(valid, keys_weight_aa(x), 0.0).sum(axis=1))
    E = np.where(valid, _eps(x), 0.0).sum(axis=1) / W
    L = np.abs(wn).sum(axis=1)
    omega = E + L * (E + (np.ceil(count / 8) + 2) * L) + L
    return float((omega + depth(count) * L).max()), float(L.max())


def tie_band(box, size):
    _, _, cw, ch = box
    om_x, l_x = _axis_bound(cw, size[1], lambda n: np.ceil(n / 4) + 2)
    om_y, l_y = _axis_bound(ch, size[0], lambda n: 9 + np.ceil((n - 1) / 8))
    return 255 * U * (l_y * om_x + l_x * om_y)


def make_frames(seed, batch, hw):
    """uniform random bytes, then six blocks of h//4 x w//4 per frame set to 0 or 255 where the generator puts them: flat
    regions next to random ones overshoot on both sides, which exercises the clamp"""
    rng = np.random.default_rng(seed)
    h, w = hw
    frames = rng.integers(0, 256, size=(batch, h, w, 3), dtype=np.uint8)
    for b in range(batch):
        for _ in range(6):
            y, x = int(rng.integers(0, h - h // 4 + 1)), int(rng.integers(0, w - w // 4 + 1))
            frames[b, y:y + h // 4, x:x + w // 4] = 255 * int(rng.integers(0, 2))
    return frames


def check_against_restatement(got, frames, box, size):
    """bytes equal the rounded float64 restatement wherever its value is farther than the case's TIE_BAND from a .5 tie;
    inside the band at most one level off.  The band must hold under 1 % of the values (a condition on the inputs)."""
    band_width = tie_band(box, size)
    n_x, n_y, s = case_taps_aa(box, size)
    for b in range(frames.shape[0]):
        v = crop_resize_cubic_aa_f64(frames[b], box, size)
        want = round_u8(v)
        band = np.abs(v - np.floor(v) - 0.5) <= band_width
        diff = np.abs(got[b].astype(int) - want.astype(int))
        saturated = ((v < 0) | (v > 255)).mean()
        print(f"frame {b}: {frames.shape[1:3]} -> {size} box {box}: taps {n_x}, {n_y}, S {s:.3f}, TIE_BAND {band_width:.2e} "
              f"({band_width / (U * 255 * s):.0f} units): {100 * band.mean():.3f} % of the values in the band, "
              f"{100 * saturated:.2f} % saturate, {int((diff > 0).sum())} bytes differ (max {int(diff.max())})")
        assert band.mean() < 0.01
        assert saturated > 0  # the clamp is exercised
        assert not diff[~band].any(), (b, int((diff[~band] > 0).sum()), int(diff[~band].max()))
        assert diff.max() <= 1


@pytest.mark.parametrize("seed, batch, hw, size, box", [
    (200, 1, (90, 160), (64, 64), None),
    (201, 1, (48, 40), (64, 64), None),               # both axes enlarge: Pillow's up-sampling, truncated windows
    (202, 1, (67, 131), (32, 96), None),              # non-integer ratios, crop on height
    (203, 1, (80, 120), (64, 64), (7, 3, 101, 70)),   # an explicit off-centre box
    (206, 1, (61, 77), (40, 70), (1, 2, 75, 58)),     # tiles cut by the output's edge, odd row pitch, odd offsets
    (207, 1, (96, 40), (32, 64), (0, 0, 40, 96)),     # x enlarges, y shrinks
    (205, 1, (700, 900), (32, 32), None),             # 88 taps per axis, a footprint beyond LDS, 25 chunks of rows
    (204, 1, (1080, 1920), (256, 256), None),         # the workload's ratio, once
    (208, 3, (90, 160), (64, 64), None),              # a batch of 3 different frames
])
def test_crop_resize_cubic_aa_against_the_restatement(seed, batch, hw, size, box):
    from denoising_diffusion_deep_fake_amd import ops
    frames = make_frames(seed, batch, hw)
    box = box or ops.center_crop_box(hw[0], hw[1], size[1], size[0])
    dev = torch.from_numpy(frames).cuda()
    got = ops.crop_resize_cubic_u8(dev, size, box=box, antialias=True)
    assert got.shape == (batch,) + size + (3,) and got.dtype == torch.uint8
    check_against_restatement(got.cpu().numpy(), frames, box, size)
    single = ops.crop_resize_cubic_u8(dev[0], size, box=box, antialias=True)  # [h, w, 3] in, [H, W, 3] out
    assert single.shape == size + (3,) and torch.equal(single, got[0])


def test_aa_identity_is_a_byte_copy_and_one_equal_axis_leaves_that_axis_alone():
    from denoising_diffusion_deep_fake_amd import ops
    frames = make_frames(210, 2, (64, 100))
    dev = torch.from_numpy(frames).cuda()
    assert torch.equal(ops.crop_resize_cubic_u8(dev, (64, 64), antialias=True), dev[:, :, 18:82])  # the centre crop
    assert torch.equal(ops.crop_resize_cubic_u8(dev, (64, 64), box=(36, 0, 64, 64), antialias=True), dev[:, :, 36:])
    assert torch.equal(ops.crop_resize_cubic_u8(dev, (64, 100), box=(0, 0, 100, 64), antialias=True), dev)
    # rows equal, columns shrink: the vertical pass has weight 1 on its own row, so a row depends on that source row alone
    got = ops.crop_resize_cubic_u8(dev, (64, 40), box=(0, 0, 100, 64), antialias=True)
    rows = ops.crop_resize_cubic_u8(dev[:, 10:11].contiguous(), (1, 40), box=(0, 0, 100, 1), antialias=True)
    assert torch.equal(got[:, 10:11], rows)


def test_aa_strided_output_and_refusals():
    """writing into the left half of a [B][H][2W][3] buffer leaves the right half untouched; the host refusals reach
    Python as D3FError"""
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    frames = torch.from_numpy(make_frames(211, 2, (90, 160))).cuda()
    packed = ops.crop_resize_cubic_u8(frames, (32, 64), antialias=True)
    pair = torch.full((2, 32, 128, 3), 171, dtype=torch.uint8, device="cuda")
    ret = ops.crop_resize_cubic_u8(frames, (32, 64), out=pair[:, :, :64], antialias=True)
    assert ret.data_ptr() == pair.data_ptr()
    assert torch.equal(pair[:, :, :64], packed) and bool((pair[:, :, 64:] == 171).all())
    ops.crop_resize_cubic_u8(frames, (32, 64), out=pair[:, :, 64:], antialias=True)
    assert torch.equal(pair[:, :, 64:], packed) and torch.equal(pair[:, :, :64], packed)
    assert not torch.equal(packed, ops.crop_resize_cubic_u8(frames, (32, 64)))  # the filter differs from the plain one
    tall = torch.zeros((1, 66, 66, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(D3FError, match="32 times"):
        ops.crop_resize_cubic_u8(tall, (2, 64), box=(0, 0, 66, 66), antialias=True)  # n_in = 33 n_out
    with pytest.raises(D3FError, match="32 times"):
        ops.crop_resize_cubic_u8(tall, (64, 2), box=(0, 0, 66, 66), antialias=True)
    with pytest.raises(D3FError, match="outside"):
        ops.crop_resize_cubic_u8(frames, (32, 64), box=(100, 0, 61, 90), antialias=True)
    with pytest.raises(D3FError, match="stride"):  # rows 3 W - 3 bytes apart
        ops.crop_resize_cubic_u8(frames[:1], (32, 64), antialias=True,
                                 out=torch.empty(32 * 64 * 3, dtype=torch.uint8, device="cuda").as_strided(
                                     (1, 32, 64, 3), (32 * 63 * 3, 63 * 3, 3, 1)))
    with pytest.raises(D3FError):    # no CPU fallback
        ops.crop_resize_cubic_u8(frames.cpu(), (32, 64), antialias=True)


@pytest.mark.parametrize("hw, size, box", [((90, 160), (64, 64), None), ((61, 77), (40, 70), (1, 2, 75, 58))])
def test_default_is_unchanged(hw, size, box):
    from denoising_diffusion_deep_fake_amd import ops
    dev = torch.from_numpy(make_frames(212, 2, hw)).cuda()
    assert torch.equal(ops.crop_resize_cubic_u8(dev, size, box=box, antialias=False), ops.crop_resize_cubic_u8(dev, size, box=box))


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
def test_fused_entries_in_the_antialiased_mode_are_bit_exact_against_the_ops_they_fuse(precision, B):
    """no tolerance: the pair's left half is the standalone antialiased resize, its right half predict_u8 of the left half,
    the full frame the paste of that fake; graph replays with antialias alternating True, False, True on the same buffers
    equal their eager counterparts (a stale graph would keep the other filter); antialias=False equals a module that was
    never given the keyword"""
    from denoising_diffusion_deep_fake_amd import ops
    net = _lit(precision).model_a
    mean, std = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    size, feather = (64, 64), 5
    raw = torch.from_numpy(make_frames(213, B, (90, 160))).cuda()
    box = ops.center_crop_box(90, 160, 64, 64)

    eager = {}
    for aa in (True, False):
        pair = net.predict_frames_u8(raw, size, mean, std, graph=False, antialias=aa)
        left = ops.crop_resize_cubic_u8(raw, size, antialias=aa)
        assert pair.shape == (B, 64, 128, 3)
        assert torch.equal(pair[:, :, :64], left), (aa, "left")
        assert torch.equal(pair[:, :, 64:], net.predict_u8(left, mean, std, graph=False)), (aa, "right")
        pair_full = torch.empty_like(pair)
        full = net.predict_frames_full_u8(raw, size, mean, std, feather=feather, graph=False, pair_out=pair_full, antialias=aa)
        assert torch.equal(pair_full, pair), (aa, "pair of full")
        assert torch.equal(full, ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, box, feather=feather)), (aa, "full")
        eager[aa] = (pair, full)
    assert not torch.equal(eager[True][0], eager[False][0])

    pair_buf, pair_buf2 = torch.empty_like(eager[True][0]), torch.empty_like(eager[True][0])
    full_buf = torch.empty_like(raw)
    for it, aa in enumerate((True, False, True)):
        pair_buf.fill_(7)
        replay = net.predict_frames_u8(raw, size, mean, std, graph=True, out=pair_buf, antialias=aa)
        assert replay.data_ptr() == pair_buf.data_ptr() and torch.equal(replay, eager[aa][0]), (it, aa, "pair graph")
        full_buf.fill_(7)
        pair_buf2.fill_(7)
        net.predict_frames_full_u8(raw, size, mean, std, feather=feather, graph=True, out=full_buf, pair_out=pair_buf2,
                                   antialias=aa)
        assert torch.equal(full_buf, eager[aa][1]) and torch.equal(pair_buf2, eager[aa][0]), (it, aa, "full graph")
        # the same mode again: a replay of the graph just captured
        net.predict_frames_u8(raw, size, mean, std, graph=True, out=pair_buf, antialias=aa)
        assert torch.equal(pair_buf, eager[aa][0]), (it, aa, "pair replay")

    never = _lit(precision).model_a  # the same weights, never given the keyword
    assert torch.equal(never.predict_frames_u8(raw, size, mean, std, graph=False), eager[False][0])
    assert torch.equal(never.predict_frames_full_u8(raw, size, mean, std, feather=feather, graph=False), eager[False][1])
    assert torch.equal(never.predict_frames_u8(raw, size, mean, std, graph=True), eager[False][0])


def test_render_fake_video_with_antialias_in_both_outputs():
    """RenderFakeVideo(antialias=True) over 3 host frames, 2 at a time (a short last batch): every frame that reaches the
    sink equals the direct call on its batch, as the real|fake pair and as the full frame"""
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    lit = _lit("f32")
    frames = list(make_frames(214, 3, (100, 180)))
    mean, std = lit.hparams.mean_b, lit.hparams.std_b
    batches = [frames[0:2], [frames[2], frames[2]]]
    dev = [torch.from_numpy(np.stack(b)).cuda() for b in batches]
    want_pair = [lit.model_a.predict_frames_u8(d, (64, 96), mean, std, graph=False, antialias=True).cpu().numpy() for d in dev]
    want_full = [lit.model_a.predict_frames_full_u8(d, (64, 96), mean, std, feather=4, graph=False, antialias=True).cpu().numpy()
                 for d in dev]
    plain = lit.model_a.predict_frames_u8(dev[0], (64, 96), mean, std, graph=False).cpu().numpy()
    assert not np.array_equal(plain, want_pair[0])
    for output, want, shape in (("pair", want_pair, (64, 192, 3)), ("full", want_full, (100, 180, 3))):
        got = []
        RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                        output=output, feather=4, antialias=True)
        assert len(got) == 3 and all(f.shape == shape and f.dtype == np.uint8 for f in got)
        for i, w in enumerate((want[0][0], want[0][1], want[1][0])):
            assert np.array_equal(got[i], w), (output, i)
    direct = lit.predict_fake_frames(np.stack(frames[0:2]), "a", 96, 64, antialias=True)
    assert np.array_equal(direct, want_pair[0])
    direct = lit.predict_fake_frames_full(np.stack(frames[0:2]), "a", 96, 64, feather=4, antialias=True)
    assert np.array_equal(direct, want_full[0])


def test_video_to_images_with_antialias(tmp_path):
    """VideoToImages(antialias=True): a decoded JPEG equals a PIL round trip of the antialiased operator's own bytes"""
    from PIL import Image

    from denoising_diffusion_deep_fake_amd import ops
    from denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images import VideoToImages
    frames = list(make_frames(215, 3, (90, 160)))
    VideoToImages(tmp_path / "clip.mp4", "64", "32", batch_frames=2, frames=iter(frames), antialias=True)
    out = tmp_path / "clip_w64_h32"
    resized = ops.crop_resize_cubic_u8(torch.from_numpy(np.stack(frames)).cuda(), (32, 64), antialias=True).cpu().numpy()
    assert not np.array_equal(resized, ops.crop_resize_cubic_u8(torch.from_numpy(np.stack(frames)).cuda(), (32, 64)).cpu().numpy())
    for i in range(3):
        with Image.open(out / f"{i:06}.jpg") as im:
            got = np.array(im)
        blob = io.BytesIO()
        Image.fromarray(resized[i][:, :, ::-1].copy()).save(blob, format="JPEG")  # BGR -> RGB, PIL's default quality
        with Image.open(blob) as im:
            want = np.array(im)
        assert np.array_equal(got, want), i
