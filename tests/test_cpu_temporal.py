"""CPU: the temporal filter without a device -- the restatement's properties on temporally correlated frames (so that no device
test can pass on an identity filter), its independence of how a sequence is cut into calls, the coefficient smoothing's cut
and first-frame rules, the host-side refusals of both operators and of the handle's setting (refused before any device call:
the dummy pointers are never dereferenced), the render tool's flags, the Python-side refusals and the header / binding
tables."""
import ctypes as C

import numpy as np
import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib, ops
from temporal_restatement import (CUT_LEVELS, STRENGTH, THRESHOLD, CoefState, FilterState, bits, color_coef_smooth,
                                  correlated_frames, gate, sad3x3, temporal_filter, thirds)

NEW_SYMBOLS = ("d3f_temporal_filter_u8", "d3f_color_coef_smooth", "d3f_temporal_flag_set", "d3f_unet_set_frame_temporal",
               "d3f_unet_frame_temporal", "d3f_unet_frame_temporal_reset")
SHAPES = [(8, 8), (37, 53), (64, 64)]


@pytest.mark.parametrize("H, W", SHAPES)
def test_restatement_on_correlated_frames_is_no_identity(H, W):
    """seed 500, B = 5, the defaults: each regime of the gate (k == 0, 0 < k < s, k == s) holds a tenth of the pixels of
    frames 1..4 or more; the first frame passes through; the interior of the moving third comes through byte for byte; the
    static third's standard deviation along time at least halves"""
    real, fake = correlated_frames(500, 5, H, W)
    s = np.float32(STRENGTH)
    k = np.stack([gate(real[b], real[b - 1], STRENGTH, THRESHOLD) for b in range(1, 5)])
    shares = [(k == 0).mean(), ((k > 0) & (k < s)).mean(), (k == s).mean()]
    print("shares", shares)
    assert min(shares) >= 0.1, shares
    state = FilterState(H, W)
    out = temporal_filter(real, fake, state)
    assert np.array_equal(out[0], fake[0])
    a, b = thirds(W)
    assert np.array_equal(out[:, :, b + 1:], fake[:, :, b + 1:])
    assert not np.array_equal(out[1:, :, :a], fake[1:, :, :a])
    before = fake[:, :, :a].astype(np.float64).std(axis=0).mean()
    after = out[:, :, :a].astype(np.float64).std(axis=0).mean()
    print("static third, std along time", before, after)
    assert after <= 0.5 * before
    assert state.valid and np.array_equal(state.real, real[4]) and state.fake.dtype == np.float32


def test_restatement_sad_and_gate_by_hand():
    r0 = np.zeros((3, 4, 3), dtype=np.uint8)
    r1 = r0.copy()
    r1[0, 0] = (1, 2, 3)       # a corner: the replicated border counts it four times for (0, 0)
    sad = sad3x3(r1, r0)
    assert sad[0, 0] == 24 and sad[0, 1] == 12 and sad[1, 1] == 6 and sad[2, 3] == 0 and sad[0, 2] == 0
    assert sad3x3(np.full((2, 2, 3), 255, np.uint8), np.zeros((2, 2, 3), np.uint8)).max() == 6885
    k = gate(r1, r0, 0.75, 1)   # T = 27
    assert k.dtype == np.float32
    assert k[0, 0] == np.float32(0.75) * (np.float32(3) / np.float32(27)) and k[2, 3] == np.float32(0.75)
    assert gate(r1, r0, 0.75, 8)[1, 1] == np.float32(0.75) * (np.float32(210) / np.float32(216))


def test_restatement_k_zero_keeps_the_byte_and_the_state_is_unrounded():
    real = np.zeros((2, 1, 1, 3), dtype=np.uint8)
    fake = np.array([[[[10, 200, 0]]], [[[13, 100, 255]]]], dtype=np.uint8)
    state = FilterState(1, 1)
    out = temporal_filter(real, fake, state, 0.75, 8)
    # S = f + 0.75 * (S_prev - f): 13 + 0.75 * -3 = 10.75, 100 + 75 = 175, 255 - 191.25 = 63.75
    assert state.fake.reshape(-1).tolist() == [10.75, 175.0, 63.75] and out[1].reshape(-1).tolist() == [11, 175, 64]
    real[1] = 255               # everything moved: the fake's bytes pass, and the state holds them
    state = FilterState(1, 1)
    out = temporal_filter(real, fake, state, 0.75, 8)
    assert np.array_equal(out, fake) and state.fake.reshape(-1).tolist() == [13.0, 100.0, 255.0]


@pytest.mark.parametrize("H, W", SHAPES)
def test_restatement_does_not_depend_on_how_the_sequence_is_cut_into_calls(H, W):
    real, fake = correlated_frames(501, 5, H, W)
    whole = FilterState(H, W)
    want = temporal_filter(real, fake, whole)
    for cuts in ((2, 3), (1, 1, 1, 1, 1)):
        state, at, got = FilterState(H, W), 0, []
        for n in cuts:
            got.append(temporal_filter(real[at:at + n], fake[at:at + n], state))
            at += n
        assert np.array_equal(np.concatenate(got), want), cuts
        assert np.array_equal(bits(state.fake), bits(whole.fake)) and np.array_equal(state.real, whole.real), cuts


def _coef_case(seed, B, n, cut_at=None):
    rng = np.random.default_rng(seed)
    coef = np.stack([rng.uniform(0.5, 2.0, size=(B, 3)), rng.uniform(-40, 40, size=(B, 3))], axis=2).astype(np.float32)
    mean = 100 + rng.integers(-3, 4, size=(B, 3))
    if cut_at is not None:
        mean[cut_at:, 1] += CUT_LEVELS + 4
    sums = np.zeros((B, 3, 2), dtype=np.uint64)
    sums[:, :, 0] = (mean * n).astype(np.uint64)
    sums[:, :, 1] = 12345
    return coef, sums


def test_restatement_coefficient_smoothing_cut_first_frame_and_strength_zero():
    n = 64 * 64
    coef, sums = _coef_case(510, 8, n, cut_at=4)
    state = CoefState()          # invalid, its buffers NaN and -1: not read
    out = color_coef_smooth(coef, sums, n, state)
    assert np.array_equal(bits(out[0]), bits(coef[0])) and np.array_equal(bits(out[4]), bits(coef[4]))   # first frame, cut
    for b in (1, 2, 3, 5, 6, 7):
        want = coef[b] + np.float32(STRENGTH) * (out[b - 1] - coef[b])
        assert np.array_equal(bits(out[b]), bits(want)) and not np.array_equal(out[b], coef[b]), b
    assert np.isfinite(out).all() and state.valid and np.array_equal(bits(state.coef), bits(out[7]))
    assert state.sums.tolist() == [int(v) for v in sums[7, :, 0]]
    # exactly 16 levels is no cut, one more unit of the sum is
    edge = sums[:2].copy()
    edge[1, :, 0] = edge[0, :, 0]
    edge[1, 2, 0] += np.uint64(CUT_LEVELS * n)
    assert not np.array_equal(color_coef_smooth(coef[:2], edge, n, CoefState())[1], coef[1])
    edge[1, 2, 0] += np.uint64(1)
    assert np.array_equal(color_coef_smooth(coef[:2], edge, n, CoefState())[1], coef[1])
    # strength 0 gives c' back; chunked 3 + 5 equals 8
    assert np.array_equal(color_coef_smooth(coef, sums, n, CoefState(), strength=0.0), coef)
    state = CoefState()
    parts = [color_coef_smooth(coef[:3], sums[:3], n, state), color_coef_smooth(coef[3:], sums[3:], n, state)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(out))


def test_operator_entry_points_refuse_bad_arguments():
    """both operators check everything on the host before a launch"""
    lib = _lib.lib()
    real, fake, sf, sr, sv = 0x100000, 0x100000 + 192, 0x900000, 0xA00000, 0xB00000
    H, W = 32, 64
    img = ((H - 1) * 384 + 192)     # bytes from a half's first pixel to its last, B = 1

    def filt(real=real, rs=384, fake=fake, fs=384, B=1, H=H, W=W, sf=sf, sr=sr, sv=sv, s=0.75, thr=8):
        return lib.d3f_temporal_filter_u8(real, rs, fake, fs, B, H, W, sf, sr, sv, s, thr, None)

    for kw, word in ((dict(real=None), b"null"), (dict(fake=None), b"null"), (dict(sf=None), b"null"), (dict(sr=None), b"null"),
                     (dict(sv=None), b"null"), (dict(B=-1), b"65535"), (dict(B=65536), b"65535"), (dict(H=0), b"size"),
                     (dict(W=-2), b"size"), (dict(W=16385, rs=6 * 16385, fs=6 * 16385), b"size"),
                     (dict(s=1.0), b"strength"), (dict(s=-0.25), b"strength"), (dict(s=float("nan")), b"strength"),
                     (dict(s=float("inf")), b"strength"), (dict(thr=0), b"threshold"), (dict(thr=256), b"threshold"),
                     (dict(rs=191), b"stride"), (dict(fs=191), b"stride"), (dict(rs=0), b"stride"),
                     (dict(sf=sf + 2), b"aligned"), (dict(sv=sv + 1), b"aligned"),
                     (dict(fake=real), b"real and fake overlap"), (dict(fake=real + 191), b"real and fake overlap"),
                     (dict(fake=real + 193), b"real and fake overlap"), (dict(fake=real + 384 + 100), b"real and fake overlap"),
                     (dict(fake=real + 192, fs=388), b"real and fake overlap"),
                     (dict(rs=192, fs=192, fake=real + 192), b"real and fake overlap"),
                     (dict(sr=real + 10), b"state buffer overlaps"), (dict(sr=fake + img - 1), b"state buffer overlaps"),
                     (dict(sr=real - 3 * H * W + 1), b"state buffer overlaps"),
                     (dict(sf=real + 64), b"state buffer overlaps"), (dict(sf=real - 12 * H * W + 4), b"state buffer overlaps"),
                     (dict(sv=real + 8), b"state buffer overlaps"), (dict(sv=fake + img - 4), b"state buffer overlaps"),
                     (dict(sr=sf), b"state buffers overlap"), (dict(sr=sf + 12 * H * W - 1), b"state buffers overlap"),
                     (dict(sv=sf + 12 * H * W - 4), b"state buffers overlap"), (dict(sv=sr), b"state buffers overlap"),
                     (dict(B=2, sr=fake + img + H * 384 - 1), b"state buffer overlaps")):
        assert filt(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert filt(B=0) == 0                                       # nothing to do, nothing launched, nothing touched
    assert filt(B=0, fake=real + 384 + 192) == 0                # (the pair layout one row on is as good)

    co, su, sc, ss, fl = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000

    def smooth(co=co, su=su, B=1, n=4096, s=0.75, sc=sc, ss=ss, fl=fl):
        return lib.d3f_color_coef_smooth(co, su, B, n, s, sc, ss, fl, None)

    for kw, word in ((dict(co=None), b"null"), (dict(su=None), b"null"), (dict(sc=None), b"null"), (dict(ss=None), b"null"),
                     (dict(fl=None), b"null"), (dict(B=-1), b"65535"), (dict(B=65536), b"65535"), (dict(n=0), b"pixels"),
                     (dict(n=(1 << 22) + 1), b"pixels"), (dict(s=1.0), b"strength"), (dict(s=-0.5), b"strength"),
                     (dict(s=float("nan")), b"strength")):
        assert smooth(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert smooth(B=0) == 0
    assert lib.d3f_temporal_flag_set(None, 0, None) != 0 and b"null" in lib.d3f_last_error()


def test_engine_setting_refusals_and_default():
    """d3f_unet_set_frame_temporal: off (strength 0, threshold 8) is the default; a pair handle and values outside their
    ranges are refused and leave the setting alone; switching off a handle that never had the mode on allocates nothing and
    succeeds without a device, and so does a reset"""
    lib = _lib.lib()
    pair, single = C.c_void_p(), C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, 2, 2, C.byref(pair)))
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, C.byref(single)))

    def setting(h):
        s, t = C.c_float(-1), C.c_int(-1)
        assert lib.d3f_unet_frame_temporal(h, C.byref(s), C.byref(t)) == 0
        return s.value, t.value

    try:
        assert setting(single) == (0.0, 8)
        assert lib.d3f_unet_frame_temporal(None, None, None) != 0 and b"null handle" in lib.d3f_last_error()
        assert lib.d3f_unet_frame_temporal(single, None, None) == 0
        assert lib.d3f_unet_set_frame_temporal(None, 0.5, 8) != 0 and b"null handle" in lib.d3f_last_error()
        for s in (1.0, 1.5, -0.1, float("nan"), float("inf")):
            assert lib.d3f_unet_set_frame_temporal(single, s, 8) != 0
            assert b"strength" in lib.d3f_last_error(), lib.d3f_last_error()
        for t in (0, -1, 256):
            assert lib.d3f_unet_set_frame_temporal(single, 0.5, t) != 0
            assert b"threshold" in lib.d3f_last_error(), lib.d3f_last_error()
        assert lib.d3f_unet_set_frame_temporal(pair, 0.5, 8) != 0 and b"pair" in lib.d3f_last_error()
        assert lib.d3f_unet_frame_temporal_reset(pair, None) != 0 and b"pair" in lib.d3f_last_error()
        assert lib.d3f_unet_frame_temporal_reset(None, None) != 0
        assert setting(single) == (0.0, 8)
        assert lib.d3f_unet_set_frame_temporal(single, 0.0, 8) == 0
        assert lib.d3f_unet_set_frame_temporal(single, 0.0, 12) == 0       # still off; the threshold is kept
        assert setting(single) == (0.0, 12)
        assert lib.d3f_unet_frame_temporal_reset(single, None) == 0        # never on: nothing to forget
    finally:
        for h in (pair, single):
            lib.d3f_unet_destroy(h)


def test_python_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet
    assert (_lib.TEMPORAL_STRENGTH, _lib.TEMPORAL_THRESHOLD) == (STRENGTH, THRESHOLD)
    assert _lib.temporal_setting(None) == (0.0, 8) and _lib.temporal_setting(0.75) == (0.75, 8)
    assert _lib.temporal_setting((0.5, 12)) == (0.5, 12) and _lib.temporal_setting(0.5, 20) == (0.5, 20)
    assert _lib.temporal_setting(0.1) == (float(np.float32(0.1)), 8)       # the float32 the handle will hold
    for bad in (1.0, 1.5, -0.1, float("nan"), 0.99999999, "0.5", True, (0.5,), (0.5, 8, 1), (0.5, 0), (0.5, 256), (0.5, 8.0),
                ("a", 8)):
        with pytest.raises(ValueError, match="temporal"):
            _lib.temporal_setting(bad)
    frame = torch.zeros((90, 160, 3), dtype=torch.uint8)
    net = Unet("resnet18", None, 3, 3, None).eval()
    for call in (net.predict_frames_u8, net.predict_frames_full_u8):
        with pytest.raises(ValueError, match="temporal"):      # before the device is asked for
            call(frame, (64, 64), [0.5] * 3, [0.5] * 3, temporal=1.0)
        with pytest.raises(D3FError):                          # a good setting gets as far as the missing device
            call(frame, (64, 64), [0.5] * 3, [0.5] * 3, temporal=(0.5, 12))
    net.reset_frame_temporal()                                 # no plan yet: nothing to do
    with pytest.raises(D3FError):
        ops.TemporalState(8, 8, "cpu")
    with pytest.raises(ValueError):
        ops.TemporalState(0, 8)
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    state = object.__new__(ops.TemporalState)                  # (a state without its device buffers)
    state.H, state.W = 8, 8
    for kw in (dict(real=img.float()), dict(fake=img[:1]), dict(real=img[..., :2], fake=img[..., :2]),
               dict(real=torch.zeros((2, 8, 8, 4), dtype=torch.uint8)[..., :3], fake=img),   # pixels that are not packed
               dict(strength=1.0), dict(strength=-0.5), dict(strength=float("nan")), dict(strength="0.5"),
               dict(threshold=0), dict(threshold=256), dict(threshold=8.0), dict(state=None)):
        args = dict(real=img, fake=img.clone(), state=state)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.temporal_filter_u8(**args)
    other = object.__new__(ops.TemporalState)
    other.H, other.W = 8, 9
    with pytest.raises(ValueError, match="TemporalState"):
        ops.temporal_filter_u8(img, img.clone(), other)
    with pytest.raises(D3FError):                              # host tensors: no CPU fallback
        ops.temporal_filter_u8(img, img.clone(), state)
    coef, sums = torch.zeros((2, 3, 2)), torch.zeros((2, 3, 2), dtype=torch.uint64)
    for kw in (dict(coef=coef.double()), dict(sums_to=sums[:1]), dict(sums_to=sums.to(torch.int64)), dict(strength=1.0),
               dict(state=None), dict(coef=torch.zeros((2, 3, 4))[..., ::2])):
        args = dict(coef=coef, sums_to=sums, n=64, state=state)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.color_coef_smooth(**args)
    with pytest.raises(D3FError):
        ops.color_coef_smooth(coef, sums, 64, state)


def test_render_tool_temporal_options():
    import d3f.script_tools.put_video_through_fake_model as render
    base = ["in.mp4", "last.ckpt", "a", "448", "448"]
    a = render.parse_command_line_arguments(base)
    assert a.temporal is None and a.temporal_threshold is None
    a = render.parse_command_line_arguments(base + ["--temporal"])                       # a bare flag: the default strength
    assert a.temporal == STRENGTH and a.temporal_threshold is None
    a = render.parse_command_line_arguments(base + ["--temporal", "0.5", "--temporal-threshold", "12"])
    assert a.temporal == 0.5 and a.temporal_threshold == 12
    a = render.parse_command_line_arguments(base + ["--output", "full", "--color-match", "meanstd", "--temporal"])
    assert a.output == "full" and a.temporal == STRENGTH                                 # either output
    for argv in (base + ["--temporal", "1.0"], base + ["--temporal", "-0.5"], base + ["--temporal", "much"],
                 base + ["--temporal-threshold", "12"], base + ["--temporal", "--temporal-threshold", "0"],
                 base + ["--temporal", "--temporal-threshold", "256"], base + ["--temporal", "--temporal-threshold", "8.5"]):
        with pytest.raises(SystemExit):
            render.parse_command_line_arguments(argv)
    for kw in (dict(temporal=1.0), dict(temporal="0.75"), dict(temporal=0.5, temporal_threshold=0),
               dict(temporal_threshold=8)):
        with pytest.raises(ValueError, match="temporal"):
            render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), **kw)

    class Model:   # an empty source renders nothing; the filter's state is reset once, before the first batch
        resets = []

        def reset_frame_temporal(self, which):
            self.resets.append(which)

    got = []
    for output in ("pair", "full"):
        r = render.RenderFakeVideo("clip.mp4", None, "b", 64, 64, frames=[], sink=got.append, model=Model(), output=output,
                                   temporal=0.5, temporal_threshold=12)
        assert r.temporal == (0.5, 12)
    assert got == [] and Model.resets == ["b", "b"]
    r = render.RenderFakeVideo("clip.mp4", None, "b", 64, 64, frames=[], sink=got.append, model=object())
    assert r.temporal is None                                  # off: the model is not asked for anything


def test_header_and_binding_carry_the_new_symbols():
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.lib(), name), name
    text = _lib.HEADER_PATH.read_text()
    for word in ("D3F_TEMPORAL_STRENGTH 0.75f", "D3F_TEMPORAL_THRESHOLD 8", "D3F_TEMPORAL_CUT_LEVELS 16"):
        assert "#define " + word in text, word
    assert CUT_LEVELS == 16
