"""GPU: colour match of the full-frame output -- the channel sums exactly and the coefficients bit for bit against their
restatement (tests/color_match_restatement.py), the colour form of the paste kernel against its float64 restatement under
the tie rule of tests/test_gpu_paste.py, the fused raw-frame call against the operators it fuses, and the render loop."""
import numpy as np
import pytest
import torch

from color_match_restatement import channel_sums, color_match_coef, paste_color_f64, sums_array
from resize_restatement import round_u8

pytestmark = pytest.mark.gpu

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)

# The band of tests/test_gpu_paste.py, kept: the 16-tap fp32 accumulation bound quoted there (2.5e-4) times the largest gain
# (2), plus five more roundings (gain * v, + offset, the blend's two products and its sum) of values up to 510, each at most
# 510 * 2^-24 = 3.0e-5, is 6.5e-4
TIE_BAND = 1e-3


_lits = {}


def _lit(which="first"):
    """as tests/test_gpu_paste.py sets its module up: non-trivial running statistics, the same weights every time; two
    modules of equal weights are kept, so that one of them never has the colour mode set"""
    if which not in _lits:
        _lits[which] = _new_lit()
    return _lits[which]


def _new_lit():
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
    return lit


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, size=shape, dtype=np.uint8)


def _sums(img, **kw):
    from denoising_diffusion_deep_fake_amd import ops
    return ops.channel_sums_u8(img, **kw).cpu().numpy()


# ---- sums: exact --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed, shape", [(300, (1, 1, 1, 3)), (301, (3, 5, 37, 3)), (302, (2, 200, 67, 3))],
                         ids=["1x1x1", "3x5x37", "2x200x67_several_workgroups"])
def test_sums_packed(seed, shape):
    """a single pixel; rows of 111 bytes (every row starts another number of bytes past a dword); several workgroups per
    image with rows of 201 bytes"""
    img = _rand(seed, shape)
    got = _sums(torch.from_numpy(img).cuda())
    assert got.dtype == np.uint64 and np.array_equal(got, sums_array(channel_sums(img)))
    one = _sums(torch.from_numpy(img[0]).cuda())                 # a single image: [3, 2]
    assert one.shape == (3, 2) and np.array_equal(one, got[0])


def test_sums_of_the_halves_of_a_pair_buffer():
    """[2][32][64][3]: the right half starts 96 bytes in, rows 192 bytes apart; the left half likewise from 0"""
    pair = _rand(303, (2, 32, 64, 3))
    dev = torch.from_numpy(pair).cuda()
    assert np.array_equal(_sums(dev[:, :, 32:]), sums_array(channel_sums(pair[:, :, 32:])))
    assert np.array_equal(_sums(dev[:, :, :32]), sums_array(channel_sums(pair[:, :, :32])))


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_sums_from_any_byte_address_leave_their_surroundings_alone(lead):
    """a 64 x 96 image `lead` bytes past a dword inside a byte store (the image's first and last groups are read byte by
    byte), the sums inside a store of sentinel bytes"""
    from denoising_diffusion_deep_fake_amd import ops
    img = _rand(304, (64, 96, 3))
    n = img.size
    store = torch.full((256 + lead + n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    view = store[256 + lead:256 + lead + n].view(64, 96, 3)
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 4 == lead
    guard = torch.full((64 + 48 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = guard[64:112].view(torch.uint64).view(3, 2)
    ret = ops.channel_sums_u8(view, out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), sums_array(channel_sums(img))[0])
    assert bool((guard[:64] == 0xA5).all()) and bool((guard[112:] == 0xA5).all())
    assert bool((store[:256 + lead] == 0x5A).all()) and bool((store[256 + lead + n:] == 0x5A).all())


def test_sums_at_the_pixel_limit_and_beyond():
    """2048 x 2048 of all 255: the largest sums the contract allows, 255 * 2^22 and 65025 * 2^22 (a lane's 32-bit
    accumulators are the fullest they get); one more column is refused"""
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    img = torch.full((1, 2048, 2048, 3), 255, dtype=torch.uint8, device="cuda")
    got = _sums(img)
    assert np.array_equal(got, np.array([[[255 << 22, 65025 << 22]] * 3], dtype=np.uint64))
    with pytest.raises(D3FError, match="pixels"):
        ops.channel_sums_u8(torch.zeros((1, 2048, 2049, 3), dtype=torch.uint8, device="cuda"))


def test_sums_overwrite_their_output():
    """the same output, pre-filled with 0xA5 bytes, twice: the call resets it both times"""
    from denoising_diffusion_deep_fake_amd import ops
    img = _rand(305, (2, 70, 50, 3))
    dev = torch.from_numpy(img).cuda()
    out = torch.full((2 * 3 * 2 * 8,), 0xA5, dtype=torch.uint8, device="cuda").view(torch.uint64).view(2, 3, 2)
    want = sums_array(channel_sums(img))
    for _ in range(2):
        ops.channel_sums_u8(dev, out=out)
        assert np.array_equal(out.cpu().numpy(), want)
    assert ops.channel_sums_u8(dev[:0]).shape == (0, 3, 2)        # B == 0: nothing to do


# ---- coefficients: bit for bit ------------------------------------------------------------------------------------------

def _coef_case(src, dst):
    """device coefficients from device sums of (src, dst) and the restatement's, as raw bits"""
    from denoising_diffusion_deep_fake_amd import ops
    n = src.shape[1] * src.shape[2]
    s_from, s_to = ops.channel_sums_u8(torch.from_numpy(src).cuda()), ops.channel_sums_u8(torch.from_numpy(dst).cuda())
    got = ops.color_match_coef(s_from, s_to, n).cpu().numpy()
    want = color_match_coef(channel_sums(src), channel_sums(dst), n)
    assert got.dtype == np.float32 and got.shape == want.shape
    return got, want


def test_coefficients_of_random_images():
    """24 (frame, channel) pairs of unrelated statistics: float64 division and square root are correctly rounded on the
    device, so the float32 results agree in every bit"""
    src = np.stack([_rand(310 + b, (40, 52, 3), 10 * b, 140 + 12 * b) for b in range(8)])
    dst = np.stack([_rand(330 + b, (40, 52, 3), 5 * b, 250 - 15 * b) for b in range(8)])
    got, want = _coef_case(src, dst)
    print("gains", want[:, :, 0].min(), "..", want[:, :, 0].max())
    assert want[:, :, 0].min() > 0.5 and want[:, :, 0].max() < 2.0 and len(np.unique(want[:, :, 0])) == 24
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_coefficients_of_flat_images_and_at_both_clamp_ends():
    flat = np.full((1, 16, 24, 3), 77, dtype=np.uint8)
    rnd = _rand(340, (1, 16, 24, 3))
    narrow = _rand(341, (1, 16, 24, 3), 100, 110)
    for name, src, dst, gain in (("constant from", flat, rnd, 1.0), ("constant to", rnd, flat, 1.0),
                                 ("clamp at 2", narrow, rnd, 2.0), ("clamp at 0.5", rnd, narrow, 0.5)):
        got, want = _coef_case(src, dst)
        assert np.all(want[:, :, 0] == np.float32(gain)), name
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


def test_coefficients_of_an_empty_batch_and_a_single_frame():
    from denoising_diffusion_deep_fake_amd import ops
    empty = torch.zeros((0, 3, 2), dtype=torch.uint64, device="cuda")
    assert ops.color_match_coef(empty, empty, 64).shape == (0, 3, 2)
    src, dst = _rand(342, (1, 8, 8, 3)), _rand(343, (1, 8, 8, 3))
    a, b = ops.channel_sums_u8(torch.from_numpy(src[0]).cuda()), ops.channel_sums_u8(torch.from_numpy(dst[0]).cuda())
    one = ops.color_match_coef(a, b, 64)
    assert one.shape == (3, 2)
    assert np.array_equal(one.cpu().numpy(), color_match_coef(channel_sums(src), channel_sums(dst), 64)[0])


# ---- the colour paste ---------------------------------------------------------------------------------------------------

# (seed, frame h x w, patch H x W, box, feather, coefficients), B = 3: the shapes of tests/test_gpu_paste.py.  The first three
# stage the patch in LDS; the last one's tiny box reads a patch region beyond the LDS budget (taps from global memory).
# The restatement alone puts 0.1 % to 0.6 % of each frame's box values inside the band at these seeds (measured without a
# device).  "clip" coefficients run at feather 6, not that file's 7: with feather + 1 a power of two the ramp is a multiple
# of 1 / 64, and the values the colour step clips to exactly 0 or 255 then blend to EXACT .5 ties on over 1 % of the box
# whatever the seed.  That file's feather 7 runs with the "mild" coefficients, which clip nothing.
PASTE_CASES = [
    (400, (90, 160), (64, 64), (35, 0, 90, 90), 6, "clip"),
    (403, (90, 160), (64, 64), (35, 0, 90, 90), 7, "mild"),
    (401, (61, 77), (40, 70), (1, 2, 75, 58), 40, "clip"),
    (402, (700, 900), (448, 448), (100, 50, 24, 24), 2, "clip"),
]
PASTE_IDS = ["staged", "staged_feather_7", "staged_all_ramp", "global_taps"]
# per frame and byte-in-pixel (gain, offset).  clip: both clamp ends of the gain with offsets that drive values into both
# clips; mild: gain * 255 + offset <= 255 and offset >= 0, so that the second clamp never acts
COEF = {
    "clip": np.array([[[2, -255], [0.5, 100], [1, 0]],
                      [[1.25, -20.5], [0.75, 30.25], [1.6180339, -70.123]],
                      [[0.9, 12.3], [1.9999, -3.7], [0.5000001, 127.4]]], dtype=np.float32),
    "mild": np.array([[[0.9, 12.3], [0.75, 30.25], [1, 0]],
                      [[0.55, 90.3], [0.8, 40.7], [0.6180339, 70.123]],
                      [[0.95, 5.5], [0.5000001, 127.4], [0.7, 0.3]]], dtype=np.float32),
}

_cache = {}


def _paste_case(case):
    """inputs and the float64 restatement of a case, computed once and shared (read only)"""
    if case not in _cache:
        seed, hw, patch_hw, box, feather, which = case
        rng = np.random.default_rng(seed)
        patch = rng.integers(0, 256, size=(3,) + patch_hw + (3,), dtype=np.uint8)
        frames = rng.integers(0, 256, size=(3,) + hw + (3,), dtype=np.uint8)
        want = np.stack([paste_color_f64(patch[b], frames[b], box, feather, COEF[which][b]) for b in range(3)])
        _cache[case] = (patch, frames, torch.from_numpy(patch).cuda(), torch.from_numpy(frames).cuda(), want)
    return _cache[case]


@pytest.mark.parametrize("case", PASTE_CASES, ids=PASTE_IDS)
def test_colour_paste_with_identity_coefficients_is_the_plain_paste(case):
    """(1, 0): 1 * v and + 0 are exact, the second clamp changes nothing -- out of place and in place"""
    from denoising_diffusion_deep_fake_amd import ops
    seed, hw, patch_hw, box, feather, _ = case
    _, _, dev_patch, dev_frames, _ = _paste_case(case)
    identity = torch.tensor([[[1.0, 0.0]] * 3] * 3, device="cuda")
    plain = ops.paste_resize_cubic_u8(dev_patch, dev_frames, box, feather)
    assert torch.equal(ops.paste_resize_cubic_u8(dev_patch, dev_frames, box, feather, color=identity), plain)
    work = dev_frames.clone()
    ret = ops.paste_resize_cubic_u8(dev_patch, work, box, feather, out=work, color=identity)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work, plain)
    one = ops.paste_resize_cubic_u8(dev_patch[1], dev_frames[1], box, feather, color=identity[1])   # a single frame
    assert one.shape == hw + (3,) and torch.equal(one, plain[1])


@pytest.mark.parametrize("case", PASTE_CASES, ids=PASTE_IDS)
def test_colour_paste_against_the_restatement(case):
    """the tie rule of tests/test_gpu_paste.py with coefficients that differ per frame and channel: bytes equal the rounded
    float64 value wherever it is farther than TIE_BAND from a .5 tie, inside the band at most one level off, the band
    holds under 1 % of the box's values; outside the box the bytes are the frame's.  In place gives the same bytes."""
    from denoising_diffusion_deep_fake_amd import ops
    seed, hw, patch_hw, (x1, y1, cw, ch), feather, which = case
    patch, frames, dev_patch, dev_frames, want = _paste_case(case)
    coef = torch.from_numpy(COEF[which]).cuda()
    dev_got = ops.paste_resize_cubic_u8(dev_patch, dev_frames, (x1, y1, cw, ch), feather, color=coef)
    assert dev_got.data_ptr() != dev_frames.data_ptr() and torch.equal(dev_frames.cpu(), torch.from_numpy(frames))
    work = dev_frames.clone()
    ops.paste_resize_cubic_u8(dev_patch, work, (x1, y1, cw, ch), feather, out=work, color=coef)
    assert torch.equal(work, dev_got)
    assert not torch.equal(dev_got, ops.paste_resize_cubic_u8(dev_patch, dev_frames, (x1, y1, cw, ch), feather))
    got = dev_got.cpu().numpy()
    outside = np.ones(hw, dtype=bool)
    outside[y1:y1 + ch, x1:x1 + cw] = False
    for b in range(3):
        assert np.array_equal(got[b][outside], frames[b][outside]), b
        v = want[b][y1:y1 + ch, x1:x1 + cw]
        band = np.abs(v - np.floor(v) - 0.5) <= TIE_BAND
        diff = np.abs(got[b][y1:y1 + ch, x1:x1 + cw].astype(int) - round_u8(v).astype(int))
        print(f"frame {b}: patch {patch_hw} -> box {(x1, y1, cw, ch)} of {hw}, feather {feather}: tie band "
              f"{100 * band.mean():.3f} % of the box's values, {int((diff > 0).sum())} bytes differ (max {int(diff.max())})")
        assert band.mean() < 0.01
        assert not diff[~band].any(), (b, int((diff[~band] > 0).sum()), int(diff[~band].max()))
        assert diff.max() <= 1


def test_colour_paste_argument_errors():
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    patch = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    frames = torch.zeros((2, 90, 160, 3), dtype=torch.uint8, device="cuda")
    box = (35, 0, 90, 90)
    with pytest.raises(ValueError, match="color"):
        ops.paste_resize_cubic_u8(patch, frames, box, color=torch.zeros((3, 3, 2), device="cuda"))   # another batch size
    with pytest.raises(ValueError, match="color"):
        ops.paste_resize_cubic_u8(patch, frames, box, color=torch.zeros((2, 3, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="color"):
        ops.paste_resize_cubic_u8(patch, frames, box, color=torch.zeros((2, 3, 2)))                 # on the host
    with pytest.raises(D3FError, match="outside"):
        ops.paste_resize_cubic_u8(patch, frames, (100, 0, 61, 90), color=torch.zeros((2, 3, 2), device="cuda"))
    # coefficients inside the buffer that is written: refused
    store = torch.zeros((2 * 90 * 160 * 3 + 64,), dtype=torch.uint8, device="cuda")
    out = store[:2 * 90 * 160 * 3].view(2, 90, 160, 3)
    inside = store[48:96].view(torch.float32).view(2, 3, 2)
    with pytest.raises(D3FError, match="coef overlaps"):
        ops.paste_resize_cubic_u8(patch, frames, box, out=out, color=inside)


# ---- the fused call -----------------------------------------------------------------------------------------------------

SIZE, RAW_HW, BOX = (64, 64), (96, 160), (32, 0, 96, 96)
MEAN, STD = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]


def _composition(net, raw, feather):
    """predict_frames_u8, then the three operators on its pair: (pair, coefficients, full)"""
    from denoising_diffusion_deep_fake_amd import ops
    pair = net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False)
    s_to, s_from = ops.channel_sums_u8(pair[:, :, :64]), ops.channel_sums_u8(pair[:, :, 64:])
    coef = ops.color_match_coef(s_from, s_to, 64 * 64)
    return pair, coef, ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, BOX, feather, color=coef)


@pytest.mark.parametrize("B", [1, 3])
def test_predict_frames_full_u8_with_colour_match_is_the_composition_of_the_ops(B):
    """no tolerance: full_out equals predict_frames_u8 -> sums of both halves -> coefficients -> colour paste, eager and
    replayed.  The network stays in the mode over three writes of new bytes into the same input buffer and every call passes
    the same buffers, so nothing drops or re-keys the graph: it is captured at the first write and every later call,
    the first one after each new write included, is a replay of that capture.  pair_out is predict_frames_u8's; the result
    differs from the unmatched one (taken from a second network of equal weights that never has the mode set); and back at
    color_match=None the first network gives that second network's bytes, eager and from a graph on the same buffers"""
    from denoising_diffusion_deep_fake_amd import _lib, ops
    net, untouched = _lit().model_a, _lit("untouched").model_a
    assert ops.center_crop_box(RAW_HW[0], RAW_HW[1], 64, 64) == BOX and ops.default_feather(96, 96) == 6
    rng = np.random.default_rng(420 + B)
    raw = torch.empty((B,) + RAW_HW + (3,), dtype=torch.uint8, device="cuda")
    pair_buf = torch.empty((B, 64, 128, 3), dtype=torch.uint8, device="cuda")
    full_buf = torch.empty_like(raw)
    previous = None
    for it in range(3):
        raw.copy_(torch.from_numpy(rng.integers(0, 256, size=tuple(raw.shape), dtype=np.uint8)))
        want_pair, coef, want_full = _composition(untouched, raw, 6)   # (operators and the pair entry: no mode involved)
        if it == 0:
            print("coefficients", coef.cpu().numpy().reshape(-1, 2).tolist())
        plain = untouched.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=False)
        assert not torch.equal(want_full, plain), (it, "the match changes the frame")
        assert previous is None or not torch.equal(want_full, previous), (it, "new bytes give a new frame")
        previous = want_full
        pair_e = torch.zeros_like(pair_buf)
        eager = net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=False, pair_out=pair_e, color_match="meanstd")
        assert torch.equal(pair_e, want_pair), (it, "eager pair")
        assert torch.equal(eager, want_full), (it, "eager full")
        for call in range(2):  # it == 0, call == 0 captures; the other five calls replay
            pair_buf.fill_(7)
            full_buf.fill_(7)
            got = net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=True, out=full_buf, pair_out=pair_buf,
                                             color_match="meanstd")
            assert got.data_ptr() == full_buf.data_ptr()
            assert torch.equal(pair_buf, want_pair) and torch.equal(full_buf, want_full), (it, call, "graph")
        eng = net._engine(B, 64, 64, raw.device)
        assert _lib.lib().d3f_unet_frame_color_match(eng.h) == _lib.COLOR_MEANSTD   # nobody switched it in between
    # back to no match on the network that had it: the bytes of the one that never did, eager and from a graph on the same
    # buffers (the mode is part of the graph's key); then the match again, re-captured
    assert torch.equal(net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=False), plain), "mode off, eager"
    for call in range(2):
        full_buf.fill_(3)
        pair_buf.fill_(3)
        net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=True, out=full_buf, pair_out=pair_buf, color_match="none")
        assert torch.equal(full_buf, plain) and torch.equal(pair_buf, want_pair), (call, "graph, mode off")
    full_buf.fill_(3)
    net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=True, out=full_buf, pair_out=pair_buf, color_match="meanstd")
    assert torch.equal(full_buf, want_full), "graph, mode on again"
    # the pair entry ignores the mode
    net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=False, color_match="meanstd")
    assert torch.equal(net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False), want_pair)
    if B == 1:  # a single frame, in place
        work = raw[0].clone()
        ret = net.predict_frames_full_u8(work, SIZE, MEAN, STD, graph=False, out=work, color_match="meanstd")
        assert ret.data_ptr() == work.data_ptr() and torch.equal(work, want_full[0])
    with pytest.raises(ValueError, match="color_match"):
        net.predict_frames_full_u8(raw, SIZE, MEAN, STD, color_match="reinhard")


def test_render_fake_video_full_output_loop_with_colour_match():
    """RenderFakeVideo(output="full", color_match="meanstd") over 5 host frames, 2 at a time: each frame that reaches the sink
    equals Unet.predict_frames_full_u8(color_match="meanstd") of its batch, and differs from the unmatched one"""
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    lit = _lit()
    lit.hparams.mean_a, lit.hparams.std_a = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    lit.hparams.mean_b, lit.hparams.std_b = [0.45, 0.4, 0.55], [0.6, 0.5, 0.4]
    rng = np.random.default_rng(440)
    frames = [rng.integers(0, 256, size=(100, 180, 3), dtype=np.uint8) for _ in range(5)]
    batches = [frames[0:2], frames[2:4], [frames[4], frames[4]]]
    order = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    model, mean, std = lit.model_a, lit.hparams.mean_b, lit.hparams.std_b
    got = []
    RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                    output="full", color_match="meanstd")
    assert len(got) == 5 and all(f.shape == (100, 180, 3) and f.dtype == np.uint8 for f in got)
    want, plain = [], []
    for b in batches:
        dev = torch.from_numpy(np.stack(b)).cuda()
        want.append(model.predict_frames_full_u8(dev, (64, 96), mean, std, graph=False, color_match="meanstd").cpu().numpy())
        plain.append(model.predict_frames_full_u8(dev, (64, 96), mean, std, graph=False).cpu().numpy())
    for i, (k, j) in enumerate(order):
        assert np.array_equal(got[i], want[k][j]), i
        assert not np.array_equal(got[i], plain[k][j]), i
