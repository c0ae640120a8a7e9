"""GPU: the temporal filter -- the filter kernel and the coefficient smoothing against their numpy restatement
(tests/temporal_restatement.py), the fused raw-frame entries against the operators they fuse, and the render loop.  Every
comparison is exact: bytes, and the raw bits of the fp32 state and coefficients.  The frames are temporally correlated
(temporal_restatement.correlated_frames); tests/test_cpu_temporal.py shows that the filter is no identity on them."""
import numpy as np
import pytest
import torch

from temporal_restatement import (CoefState, FilterState, bits, color_coef_smooth, correlated_frames, temporal_filter)

pytestmark = pytest.mark.gpu

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)
SIZE, RAW_HW, BOX = (64, 64), (96, 160), (32, 0, 96, 96)
MEAN, STD = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]

_lits = {}


def _lit(which="first"):
    """as tests/test_gpu_color_match.py sets its module up: non-trivial running statistics, the same weights every time; two
    modules of equal weights are kept, so that one of them never has the temporal mode set"""
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


def _frames(seed, B, H, W):
    """the correlated recipe; below three columns there are no thirds, and the whole frame gets the middle third's noise"""
    if W >= 3:
        return correlated_frames(seed, B, H, W)
    rng = np.random.default_rng(seed)
    base, fbase = rng.integers(0, 256, size=(2, H, W, 3))
    real = np.clip(base + rng.integers(-6, 7, size=(B, H, W, 3)), 0, 255).astype(np.uint8)
    fake = np.clip(fbase + rng.integers(-20, 21, size=(B, H, W, 3)), 0, 255).astype(np.uint8)
    return real, fake


def _check_state(state, ref, what=""):
    assert state.valid.cpu().tolist()[0] == (1 if ref.valid else 0), what
    if ref.valid:
        assert np.array_equal(bits(state.fake.cpu().numpy()), bits(ref.fake)), (what, "state_fake bits")
        assert np.array_equal(state.real.cpu().numpy(), ref.real), (what, "state_real")


def _run(real, fake, cuts, strength, threshold, state=None):
    """the device filter over the frames cut into calls of `cuts` frames: (bytes, state)"""
    from denoising_diffusion_deep_fake_amd import ops
    state = state or ops.TemporalState(real.shape[1], real.shape[2])
    dr, df = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    at = 0
    for n in cuts:
        ret = ops.temporal_filter_u8(dr[at:at + n], df[at:at + n], state, strength, threshold)
        assert ret.data_ptr() == df[at:at + n].data_ptr()
        at += n
    assert torch.equal(dr.cpu(), torch.from_numpy(real)), "real is read only"
    return df.cpu().numpy(), state


# ---- part A against the restatement ---------------------------------------------------------------------------------------

CASES = [(520, 1, 1, 0.75, 8), (521, 8, 8, 0.75, 8), (522, 37, 53, 0.75, 8), (523, 64, 64, 0.25, 8), (524, 64, 64, 0.75, 1),
         (525, 64, 64, 0.999, 255), (526, 64, 64, 0.75, 8)]


@pytest.mark.parametrize("seed, H, W, strength, threshold", CASES,
                         ids=[f"{c[1]}x{c[2]}_s{c[3]}_t{c[4]}" for c in CASES])
def test_filter_against_the_restatement(seed, H, W, strength, threshold):
    """B = 5 in one call.  1 x 1: every neighbour is the clamped pixel; 37 x 53: ragged tiles in both directions and rows of 159
    bytes, so that every row starts another number of bytes past a dword; 64 x 64: several tiles, several settings"""
    real, fake = _frames(seed, 5, H, W)
    ref = FilterState(H, W)
    want = temporal_filter(real, fake, ref, strength, threshold)
    got, state = _run(real, fake, (5,), strength, threshold)
    print("bytes changed", (want != fake).mean())
    assert np.array_equal(got, want)
    assert W < 8 or not np.array_equal(want[1:], fake[1:])
    _check_state(state, ref)


def test_filter_on_the_halves_of_a_pair_buffer():
    """[5][64][128][3]: row stride 384, the fake half 192 bytes in; the real half and every byte outside the fake half stay"""
    from denoising_diffusion_deep_fake_amd import ops
    real, fake = _frames(530, 5, 64, 64)
    pair = np.concatenate([real, fake], axis=2)
    dev = torch.from_numpy(pair).cuda()
    state = ops.TemporalState(64, 64)
    ops.temporal_filter_u8(dev[:, :, :64], dev[:, :, 64:], state)
    ref = FilterState(64, 64)
    want = temporal_filter(real, fake, ref)
    got = dev.cpu().numpy()
    assert np.array_equal(got[:, :, :64], real) and np.array_equal(got[:, :, 64:], want)
    _check_state(state, ref)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_filter_from_any_byte_address_leaves_its_surroundings_alone(lead):
    """2 x 37 x 53 images `lead` bytes past a dword inside stores of sentinel bytes (the ragged ends of the rows are written
    byte by byte), and each state buffer inside a guard of its own"""
    from denoising_diffusion_deep_fake_amd import ops
    B, H, W = 2, 37, 53
    n = B * H * W * 3
    real, fake = _frames(540 + lead, B + 1, H, W)
    store_r = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    store_f = torch.full((n + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    at = 32 + lead
    assert (store_r.data_ptr() + at) % 4 == lead and (store_f.data_ptr() + at) % 4 == lead
    dr, df = store_r[at:at + n].view(B, H, W, 3), store_f[at:at + n].view(B, H, W, 3)
    state = ops.TemporalState(H, W)
    guard_f = torch.full((H * W * 3 + 16,), -7.0, dtype=torch.float32, device="cuda")
    guard_r = torch.full((H * W * 3 + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    guard_v = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    guard_v[3:5] = 0
    state.fake, state.real = guard_f[8:8 + H * W * 3].view(H, W, 3), guard_r[at:at + H * W * 3].view(H, W, 3)
    state.valid = guard_v[3:5]
    ref = FilterState(H, W)
    for k in (0, 1):   # the second call reads the state back from the odd addresses
        dr.copy_(torch.from_numpy(real[k:k + B]))
        df.copy_(torch.from_numpy(fake[k:k + B]))
        ops.temporal_filter_u8(dr, df, state)
        want = temporal_filter(real[k:k + B], fake[k:k + B], ref)
        assert np.array_equal(df.cpu().numpy(), want), k
        _check_state(state, ref, k)
        assert bool((store_f[:at] == 0xC3).all()) and bool((store_f[at + n:] == 0xC3).all()), "sentinels around fake"
        assert bool((store_r[:at] == 0x5A).all()) and bool((store_r[at + n:] == 0x5A).all())
        assert np.array_equal(dr.cpu().numpy(), real[k:k + B])
        assert bool((guard_f[:8] == -7.0).all()) and bool((guard_f[8 + H * W * 3:] == -7.0).all()), "guard of state_fake"
        assert bool((guard_r[:at] == 0x3C).all()) and bool((guard_r[at + H * W * 3:] == 0x3C).all()), "guard of state_real"
        assert guard_v.cpu().tolist() == [77, 77, 77, 1, 0, 77, 77, 77], "the filter's flag, and nothing else"


def test_state_hand_off_between_calls():
    """one call of 5, calls of 2 + 3 and five calls of 1: equal bytes and equal state bits"""
    real, fake = _frames(550, 5, 37, 53)
    ref = FilterState(37, 53)
    want = temporal_filter(real, fake, ref)
    for cuts in ((5,), (2, 3), (1, 1, 1, 1, 1)):
        got, state = _run(real, fake, cuts, 0.75, 8)
        assert np.array_equal(got, want), cuts
        _check_state(state, ref, cuts)


def test_first_frame_does_not_read_the_state():
    """the state buffers pre-filled with NaN and 0xA5 and invalid: the output is the fake, and the state is clean"""
    from denoising_diffusion_deep_fake_amd import ops
    real, fake = _frames(560, 1, 37, 53)
    state = ops.TemporalState(37, 53)
    state.fake.fill_(float("nan"))
    state.real.fill_(0xA5)
    got, state = _run(real, fake, (1,), 0.75, 8, state)
    assert np.array_equal(got, fake)
    assert np.array_equal(bits(state.fake.cpu().numpy()), bits(fake[0].astype(np.float32)))
    assert np.array_equal(state.real.cpu().numpy(), real[0]) and state.valid.cpu().tolist() == [1, 0]


def test_reset_in_the_middle_of_a_sequence_equals_a_fresh_state():
    real, fake = _frames(570, 5, 37, 53)
    got_a, state = _run(real[:2], fake[:2], (2,), 0.75, 8)
    assert state.reset() is state
    assert state.valid.cpu().tolist() == [0, 0]
    got_b, state = _run(real[2:], fake[2:], (3,), 0.75, 8, state)
    ref = FilterState(37, 53)
    want = temporal_filter(real[2:], fake[2:], ref)
    assert np.array_equal(got_b, want) and np.array_equal(got_b[0], fake[2])
    _check_state(state, ref)


def test_an_empty_batch_leaves_everything_alone():
    from denoising_diffusion_deep_fake_amd import ops
    state = ops.TemporalState(8, 8)
    state.fake.fill_(3.5)
    state.real.fill_(9)
    empty = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda")
    assert ops.temporal_filter_u8(empty, empty.clone(), state).shape[0] == 0
    assert state.valid.cpu().tolist() == [0, 0] and bool((state.fake == 3.5).all()) and bool((state.real == 9).all())
    coef = torch.empty((0, 3, 2), device="cuda")
    ops.color_coef_smooth(coef, torch.empty((0, 3, 2), dtype=torch.uint64, device="cuda"), 64, state)
    assert state.valid.cpu().tolist() == [0, 0]


def test_refusals_raise():
    from denoising_diffusion_deep_fake_amd import D3FError, ops
    real, fake = (torch.from_numpy(a).cuda() for a in _frames(580, 2, 8, 8))
    state = ops.TemporalState(8, 8)
    for kw in (dict(strength=1.0), dict(strength=-0.1), dict(strength=float("nan")), dict(threshold=0), dict(threshold=256),
               dict(state=ops.TemporalState(8, 9)), dict(fake=fake[:1]), dict(real=real.float())):
        args = dict(real=real, fake=fake, state=state)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.temporal_filter_u8(**args)
    pair = torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(D3FError, match="overlap"):
        ops.temporal_filter_u8(real, real, state)                               # fake is real
    with pytest.raises(D3FError, match="overlap"):
        ops.temporal_filter_u8(pair[:, :, :8], pair[:, :, 4:12], state)         # halves that share columns
    with pytest.raises(D3FError, match="overlap"):
        ops.temporal_filter_u8(pair[:, :, :8], pair.flatten()[1:2 * 8 * 8 * 3 + 1].view(2, 8, 8, 3), state)
    inside = ops.TemporalState(8, 8)
    inside.real = fake[0]
    with pytest.raises(D3FError, match="state buffer overlaps"):
        ops.temporal_filter_u8(real, fake, inside)
    inside = ops.TemporalState(8, 8)
    inside.real = inside.fake.view(torch.uint8).flatten()[:192].view(8, 8, 3)
    with pytest.raises(D3FError, match="state buffers overlap"):
        ops.temporal_filter_u8(real, fake, inside)
    assert state.valid.cpu().tolist() == [0, 0] and torch.equal(fake.cpu(), torch.from_numpy(_frames(580, 2, 8, 8)[1]))
    with pytest.raises(ValueError):
        ops.color_coef_smooth(torch.zeros((2, 3, 2), device="cuda"), torch.zeros((2, 3, 2), dtype=torch.uint64, device="cuda"),
                              64, state, strength=1.0)
    with pytest.raises(D3FError, match="pixels"):
        ops.color_coef_smooth(torch.zeros((2, 3, 2), device="cuda"), torch.zeros((2, 3, 2), dtype=torch.uint64, device="cuda"),
                              0, state)


# ---- part B against the restatement ---------------------------------------------------------------------------------------

def _coef_case(seed, B, n, cut_at=None):
    rng = np.random.default_rng(seed)
    coef = np.stack([rng.uniform(0.5, 2.0, size=(B, 3)), rng.uniform(-40, 40, size=(B, 3))], axis=2).astype(np.float32)
    mean = 100 + rng.integers(-3, 4, size=(B, 3))
    if cut_at is not None:
        mean[cut_at:, 1] += 20     # more than the 16 levels of a cut
    sums = np.zeros((B, 3, 2), dtype=np.uint64)
    sums[:, :, 0] = (mean * n).astype(np.uint64)
    sums[:, :, 1] = 0xFFFFFFFFFFFFFFF      # Q is not read
    return coef, sums


def _smooth(coef, sums, n, state, strength=0.75):
    from denoising_diffusion_deep_fake_amd import ops
    dev = torch.from_numpy(coef.copy()).cuda()
    ret = ops.color_coef_smooth(dev, torch.from_numpy(sums).cuda(), n, state, strength)
    assert ret.data_ptr() == dev.data_ptr()
    return dev.cpu().numpy()


def test_coefficient_smoothing_against_the_restatement():
    """8 frames with a cut at frame 4 on a garbage state (NaN coefficients, huge sums, invalid: not read); chunked 3 + 5 equals
    8; a single frame [3, 2]; strength 0 gives the coefficients back"""
    from denoising_diffusion_deep_fake_amd import ops
    n = 64 * 64
    coef, sums = _coef_case(590, 8, n, cut_at=4)
    ref = CoefState()
    want = color_coef_smooth(coef, sums, n, ref)
    assert np.array_equal(want[4], coef[4]) and np.array_equal(want[0], coef[0]) and not np.array_equal(want[5], coef[5])

    def garbage():
        state = ops.TemporalState(8, 8)
        state.coef.fill_(float("nan"))
        state.sums.copy_(torch.full((3,), 1 << 62, dtype=torch.int64).view(torch.uint64))
        return state

    state = garbage()
    got = _smooth(coef, sums, n, state)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(state.coef.cpu().numpy()), bits(ref.coef))
    assert state.sums.cpu().view(torch.int64).tolist() == ref.sums.tolist() and state.valid.cpu().tolist() == [0, 1]
    state = garbage()
    parts = [_smooth(coef[:3], sums[:3], n, state), _smooth(coef[3:], sums[3:], n, state)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(want))
    state = garbage()
    one = [_smooth(coef[b], sums[b], n, state) for b in range(8)]
    assert one[0].shape == (3, 2) and np.array_equal(bits(np.stack(one)), bits(want))
    assert np.array_equal(_smooth(coef, sums, n, garbage(), strength=0.0), coef)
    state.reset()
    assert np.array_equal(_smooth(coef[5:6], sums[5:6], n, state), coef[5:6]), "after a reset: a first frame"


# ---- the fused entries ------------------------------------------------------------------------------------------------------

def _reference(untouched, raws, color):
    """per write: (unfiltered pair, filtered pair, full) from the network that never has the mode set and the operators, the
    state held here"""
    from denoising_diffusion_deep_fake_amd import ops
    state = ops.TemporalState(64, 64)
    out = []
    for raw in raws:
        pair = untouched.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False)
        plain = pair.clone()
        ops.temporal_filter_u8(pair[:, :, :64], pair[:, :, 64:], state, 0.75, 8)
        if color:
            s_to, s_from = ops.channel_sums_u8(pair[:, :, :64]), ops.channel_sums_u8(pair[:, :, 64:])
            coef = ops.color_match_coef(s_from, s_to, 64 * 64)
            raw_coef = coef.clone()
            ops.color_coef_smooth(coef, s_to, 64 * 64, state, 0.75)
            assert len(out) == 0 or not torch.equal(coef, raw_coef), "the smoothing moves the coefficients"
            full = ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, BOX, 6, color=coef)
        else:
            full = ops.paste_resize_cubic_u8(pair[:, :, 64:], raw, BOX, 6)
        out.append((plain, pair, full))
    return out


@pytest.mark.parametrize("color", [None, "meanstd"], ids=["plain_paste", "colour_match"])
@pytest.mark.parametrize("B", [1, 3])
def test_fused_entries_are_the_composition_of_the_ops(B, color):
    """three successive writes of correlated raw frames into one input buffer: predict_frames_u8 and predict_frames_full_u8
    with temporal=0.75 give exactly the bytes of the network without the mode followed by the operators -- eager, and from a
    graph captured at the first write and replayed for the later ones"""
    from denoising_diffusion_deep_fake_amd import _lib
    net, untouched = _lit().model_a, _lit("untouched").model_a
    frames = correlated_frames(600 + B, 3 * B, *RAW_HW)[0]
    raws = [torch.from_numpy(frames[i * B:(i + 1) * B]).cuda() for i in range(3)]
    want = _reference(untouched, raws, color)
    assert torch.equal(want[0][1][0], want[0][0][0]), "the first frame of the first write passes through"
    assert B == 1 or not torch.equal(want[0][1][1:], want[0][0][1:]), "its later frames follow it"
    for it in (1, 2):
        assert not torch.equal(want[it][1][:, :, 64:], want[it][0][:, :, 64:]), (it, "the filter changes the fake")
        assert torch.equal(want[it][1][:, :, :64], want[it][0][:, :, :64]), (it, "and not the real half")
    raw = torch.empty_like(raws[0])
    pair_buf = torch.empty((B, 64, 128, 3), dtype=torch.uint8, device="cuda")
    full_buf = torch.empty_like(raw)
    kw = dict(temporal=0.75)
    for graph in (False, True):
        net.reset_frame_temporal()
        for it in range(3):          # the pair entry
            raw.copy_(raws[it])
            pair_buf.fill_(7)
            net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=graph, out=pair_buf, **kw)
            assert torch.equal(pair_buf, want[it][1]), (graph, it, "pair entry")
        net.reset_frame_temporal()
        for it in range(3):          # the full-frame entry
            raw.copy_(raws[it])
            pair_buf.fill_(7)
            full_buf.fill_(7)
            net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=graph, out=full_buf, pair_out=pair_buf, color_match=color, **kw)
            assert torch.equal(pair_buf, want[it][1]), (graph, it, "full entry, pair")
            assert torch.equal(full_buf, want[it][2]), (graph, it, "full entry, full")
    eng = net._engine(B, 64, 64, raw.device)
    s, t = _lib.C.c_float(), _lib.C.c_int()
    assert _lib.lib().d3f_unet_frame_temporal(eng.h, _lib.C.byref(s), _lib.C.byref(t)) == 0 and (s.value, t.value) == (0.75, 8)
    # after a reset the next call starts with a first frame again: the unfiltered bytes
    net.reset_frame_temporal()
    assert torch.equal(net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False, **kw)[0], want[2][0][0]), "after a reset"
    # other values start a new sequence too, and so does coming back to the old ones
    assert torch.equal(net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False, temporal=(0.5, 12))[0], want[2][0][0])
    assert torch.equal(net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=False, **kw)[0], want[2][0][0])
    assert not torch.equal(net.predict_frames_u8(raws[1], SIZE, MEAN, STD, graph=False, **kw)[0], want[1][0][0]), "a second frame"
    # mode off on the network that had it: the untouched network's bytes, eager and from a graph
    plain_full = untouched.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=False, color_match=color)
    for graph in (False, True, True):
        pair_buf.fill_(3)
        full_buf.fill_(3)
        net.predict_frames_full_u8(raw, SIZE, MEAN, STD, graph=graph, out=full_buf, pair_out=pair_buf, color_match=color)
        assert torch.equal(pair_buf, want[2][0]) and torch.equal(full_buf, plain_full), (graph, "mode off, full entry")
        pair_buf.fill_(3)
        net.predict_frames_u8(raw, SIZE, MEAN, STD, graph=graph, out=pair_buf, temporal=None)
        assert torch.equal(pair_buf, want[2][0]), (graph, "mode off, pair entry")
    if B == 1 and color:   # a single frame, in place
        net.reset_frame_temporal()
        for it in range(2):
            work = raws[it][0].clone()
            ret = net.predict_frames_full_u8(work, SIZE, MEAN, STD, graph=False, out=work, color_match=color, **kw)
            assert ret.data_ptr() == work.data_ptr() and torch.equal(work, want[it][2][0]), it
    with pytest.raises(ValueError, match="temporal"):
        net.predict_frames_u8(raw, SIZE, MEAN, STD, temporal=1.0)


@pytest.mark.parametrize("output", ["pair", "full"])
def test_render_fake_video_with_the_temporal_filter(output):
    """RenderFakeVideo(temporal=0.75) over 5 host frames, 2 at a time: each frame that reaches the sink equals the per-batch
    calls on a freshly reset network; from the second frame on it differs from the unfiltered render (the first frame of a
    video has no predecessor and passes through); a second render on the same module starts from a reset state and
    reproduces the first"""
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    lit = _lit()
    lit.hparams.mean_a, lit.hparams.std_a = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    lit.hparams.mean_b, lit.hparams.std_b = [0.45, 0.4, 0.55], [0.6, 0.5, 0.4]
    frames = list(correlated_frames(610, 5, 100, 180)[0])
    batches = [frames[0:2], frames[2:4], [frames[4], frames[4]]]
    order = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    model, mean, std = lit.model_a, lit.hparams.mean_b, lit.hparams.std_b
    extra = dict(output="full", color_match="meanstd") if output == "full" else {}

    def render(**kw):
        got = []
        RenderFakeVideo("clip.mp4", None, "a", "96", "64", batch_frames=2, frames=iter(frames), sink=got.append, model=lit,
                        **extra, **kw)
        return got

    got = render(temporal=0.75)
    shape = (100, 180, 3) if output == "full" else (64, 192, 3)
    assert len(got) == 5 and all(f.shape == shape and f.dtype == np.uint8 for f in got)
    unfiltered = render()
    model.reset_frame_temporal()
    want = []
    for b in batches:
        dev = torch.from_numpy(np.stack(b)).cuda()
        if output == "full":
            want.append(model.predict_frames_full_u8(dev, (64, 96), mean, std, graph=False, color_match="meanstd",
                                                     temporal=0.75).cpu().numpy())
        else:
            want.append(model.predict_frames_u8(dev, (64, 96), mean, std, graph=False, temporal=0.75).cpu().numpy())
    for i, (k, j) in enumerate(order):
        assert np.array_equal(got[i], want[k][j]), i
        assert np.array_equal(got[i], unfiltered[i]) == (i == 0), i
    again = render(temporal=0.75)
    assert all(np.array_equal(a, g) for a, g in zip(again, got))
