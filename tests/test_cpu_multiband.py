"""CPU: the multiband paste's restatement checks itself (tests/multiband_restatement.py), and the host-side pieces of the
feature that need no device: the default levels, the blend mode's validation, the tool's parser and RenderFakeVideo's
argument errors."""
import numpy as np
import pytest

import multiband_restatement as mb

SIZES = [(37, 29), (8, 8), (5, 64), (33, 17)]  # (ch, cw)


def _case(ch, cw, seed):
    """a random patch, a frame 7 rows and 9 columns larger than the box, the box at (5, 3), and V of the float64 restatement"""
    rng = np.random.default_rng(seed)
    patch = rng.integers(0, 256, (24, 20, 3), dtype=np.uint8)
    frame = rng.integers(0, 256, (ch + 7, cw + 9, 3), dtype=np.uint8)
    box = (5, 3, cw, ch)
    return patch, frame, box, mb.target_bytes_f64(patch, box)


@pytest.mark.parametrize("ch, cw", SIZES)
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_feather_zero_returns_the_target_bytes(ch, cw, levels):
    """F == 0: every mask is the identity and each level adds back the very expansion it subtracted, so E == D exactly"""
    if min(ch, cw) < (1 << levels):
        with pytest.raises(ValueError):
            mb.multiband_E(np.zeros((ch, cw, 3), np.int64), 0, levels)
        return
    patch, frame, box, V = _case(ch, cw, 11 * ch + cw)
    x1, y1 = box[:2]
    D = V.astype(np.int64) - frame[y1:y1 + ch, x1:x1 + cw]
    assert np.array_equal(mb.multiband_E(D, 0, levels), D)
    out = mb.paste_multiband(V, frame, box, 0, levels)
    assert np.array_equal(out[y1:y1 + ch, x1:x1 + cw], V)


@pytest.mark.parametrize("ch, cw", SIZES)
def test_zero_difference_returns_the_frame_and_the_outside_is_untouched(ch, cw):
    patch, frame, box, V = _case(ch, cw, 5 * ch + cw)
    x1, y1 = box[:2]
    levels = 2
    same = frame[y1:y1 + ch, x1:x1 + cw].copy()
    for feather in (0, 3, 9):
        assert np.array_equal(mb.paste_multiband(same, frame, box, feather, levels), frame)
        out = mb.paste_multiband(V, frame, box, feather, levels)
        outside = np.ones(frame.shape[:2], bool)
        outside[y1:y1 + ch, x1:x1 + cw] = False
        assert np.array_equal(out[outside], frame[outside])
        if feather:
            assert not np.array_equal(out[y1:y1 + ch, x1:x1 + cw], V), "a ramp moves bytes"


def test_the_ramp_fades_low_frequencies_wider_than_high_ones():
    """a constant difference (all low frequency) keeps fading far from the edge; a checkerboard (all high frequency) is whole
    a few pixels in"""
    ch = cw = 64
    feather, levels = 16, 3
    flat = mb.multiband_E(np.full((ch, cw), 128, np.int64), feather, levels)
    assert flat[32, 32] == 128 and 0 < flat[32, 6] < 128
    ii, jj = np.indices((ch, cw))
    board = np.where((ii + jj) & 1, 100, -100).astype(np.int64)
    E = mb.multiband_E(board, feather, levels)
    # (the clamped border leaves a trace of the board in the coarse levels near the edge: a level or two of the 100)
    assert np.abs(E[4:-4, 4:-4] - board[4:-4, 4:-4]).max() <= 2 and flat[32, 6] < 100
    assert np.array_equal(E[28:-28, 28:-28], board[28:-28, 28:-28])


def test_level_sizes_and_band_width():
    assert mb.level_sizes(37, 3) == [37, 19, 10, 5] and mb.level_sizes(8, 3) == [8, 4, 2, 1]
    assert [mb.band_F(f, 3) for f in (0, 1, 8, 9, 12)] == [0, 1, 1, 2, 2]
    x = np.arange(-40, 41, dtype=np.int64).reshape(9, 9)
    assert np.array_equal(mb.band_mask(x, 0), x)
    # F = 1, den = 4, x = -5: corner M = 1: floor(-6 / 8) = -1; edge M = 2: floor(-16 / 8) = -2; interior M = 4: -5
    m = mb.band_mask(np.full((5, 5), -5, np.int64), 1)
    assert m[0, 0] == -1 and m[0, 2] == -2 and m[2, 2] == -5


def test_default_levels():
    from denoising_diffusion_deep_fake_amd import ops
    assert [ops.multiband_levels(f) for f in (0, 3, 4, 16, 67)] == [1, 1, 1, 3, 5]
    assert ops.multiband_levels(10 ** 6) == 5


def test_blend_mode_validation():
    from denoising_diffusion_deep_fake_amd import _lib
    assert _lib.blend_mode(None) == _lib.blend_mode("feather") == _lib.BLEND_FEATHER == 0
    assert _lib.blend_mode("multiband") == _lib.BLEND_MULTIBAND == 1
    for bad in ("laplacian", "Multiband", 1, True, ["multiband"], b"multiband"):
        with pytest.raises(ValueError, match="blend"):
            _lib.blend_mode(bad)
    assert _lib.blend_levels(1) == 1 and _lib.blend_levels(6) == 6
    for bad in (0, 7, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="levels"):
            _lib.blend_levels(bad)


def test_header_and_binding_agree_on_the_constants():
    import re
    from denoising_diffusion_deep_fake_amd import _lib
    text = _lib.HEADER_PATH.read_text()
    defines = dict(re.findall(r"#define (D3F_(?:BLEND_\w+|MULTIBAND_MAX_LEVELS)) (\d+)", text))
    assert defines == {"D3F_BLEND_FEATHER": str(_lib.BLEND_FEATHER), "D3F_BLEND_MULTIBAND": str(_lib.BLEND_MULTIBAND),
                       "D3F_MULTIBAND_MAX_LEVELS": str(_lib.MULTIBAND_MAX_LEVELS)}
    for name in ("d3f_paste_multiband_u8", "d3f_paste_multiband_color_u8", "d3f_paste_multiband_boxes_u8",
                 "d3f_paste_multiband_color_boxes_u8", "d3f_paste_multiband_workspace_bytes", "d3f_unet_set_frame_blend",
                 "d3f_unet_frame_blend"):
        assert name in _lib.PROTOTYPES and re.search(rf"\b{name}\(", text), name


def test_render_tool_blend_options():
    import d3f.script_tools.put_video_through_fake_model as render
    base = ["in.mp4", "last.ckpt", "a", "448", "448"]
    a = render.parse_command_line_arguments(base)
    assert a.blend is None and a.blend_levels is None
    a = render.parse_command_line_arguments(base + ["--output", "full", "--blend", "multiband"])
    assert a.blend == "multiband" and a.blend_levels is None
    a = render.parse_command_line_arguments(base + ["--output", "full", "--blend", "multiband", "--blend-levels", "4"])
    assert a.blend == "multiband" and a.blend_levels == 4
    assert render.parse_command_line_arguments(base + ["--blend", "feather"]).blend == "feather"
    for argv in (base + ["--blend", "multiband"],                                  # without --output full
                 base + ["--output", "pair", "--blend", "multiband"],
                 base + ["--output", "full", "--blend-levels", "3"],              # without --blend multiband
                 base + ["--output", "full", "--blend", "feather", "--blend-levels", "3"],
                 base + ["--output", "full", "--blend", "multiband", "--blend-levels", "0"],   # outside 1..6
                 base + ["--output", "full", "--blend", "multiband", "--blend-levels", "7"],
                 base + ["--output", "full", "--blend", "pyramid"]):
        with pytest.raises(SystemExit):
            render.parse_command_line_arguments(argv)


def test_render_fake_video_blend_argument_errors_need_no_device():
    import d3f.script_tools.put_video_through_fake_model as render

    def make(**kw):
        return render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), **kw)

    with pytest.raises(ValueError, match="blend"):
        make(output="pair", blend="multiband")
    with pytest.raises(ValueError, match="blend"):
        make(blend="multiband")
    for bad in ("pyramid", 1, ["multiband"]):
        with pytest.raises(ValueError, match="blend"):
            make(output="full", blend=bad)
    with pytest.raises(ValueError, match="blend_levels"):
        make(output="full", blend_levels=3)
    with pytest.raises(ValueError, match="blend_levels"):
        make(output="full", blend="feather", blend_levels=3)
    for bad in (0, 7, 2.5, True, "3"):
        with pytest.raises(ValueError, match="blend_levels"):
            make(output="full", blend="multiband", blend_levels=bad)
    # an empty source in full mode renders nothing and touches no model
    got = []
    render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=got.append, model=object(), output="full",
                           blend="multiband", blend_levels=2)
    assert got == []
    # a track whose box is below 2 ** levels on a side is refused before the first batch reaches the model
    frames = [np.zeros((96, 160, 3), np.uint8)] * 2
    with pytest.raises(ValueError, match="short side"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=frames, sink=got.append, model=object(), output="full",
                               blend="multiband", blend_levels=6, track=[(60, 40, 20, 20), (62, 40, 20, 20)],
                               track_margin=1.0)
    assert got == []
