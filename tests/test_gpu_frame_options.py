"""GPU: the three options of the fused raw-frame entries together -- antialiased resize, colour match, temporal filter.  Every
combination of them, eager and replayed from a graph, gives byte for byte the composition of the operators on the plain
`predict_u8` of a network that never has an option set; and a walk through the combinations that changes one option per step
never replays a graph captured under another setting.  Set up as tests/test_gpu_temporal.py: 96 x 160 raw frames, whose
centre crop shrinks 1.5 times to the 64 x 64 network, B = 2."""
import pytest
import torch

from temporal_restatement import correlated_frames

pytestmark = pytest.mark.gpu

HP_FAKE = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet34",
               noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
               std_b=[0.5] * 3, synthetic=True, image_size=64, synthetic_length=4, ema_beta=0.9999,
               ema_update_every=1, augment=False)
SIZE, RAW_HW, BOX = (64, 64), (96, 160), (32, 0, 96, 96)
MEAN, STD = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
B, WRITES, STRENGTH, THRESHOLD = 2, 3, 0.75, 8
OPTIONS = [(aa, color, temporal) for aa in (False, True) for color in (None, "meanstd") for temporal in (None, STRENGTH)]
# one option changes per step, the last step included: back to everything off
GRAY_WALK = [OPTIONS[i] for i in (0b000, 0b001, 0b011, 0b010, 0b110, 0b111, 0b101, 0b100, 0b000)]

_lits, _raws, _wants = {}, [], {}


def _lit(which="first"):
    """as tests/test_gpu_temporal.py sets its module up: non-trivial running statistics, the same weights every time; two
    modules of equal weights are kept, so that one of them never has an option set"""
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
    """three successive writes of B temporally correlated raw frames, made once"""
    if not _raws:
        frames = correlated_frames(700, WRITES * B, *RAW_HW)[0]
        _raws.extend(torch.from_numpy(frames[i * B:(i + 1) * B]).cuda() for i in range(WRITES))
    return _raws


def _reference(antialias, color, temporal):
    """per write: (pair before the filter, pair, full) from the operators and the plain `predict_u8` of the network that never
    has an option set, the filter's state held here; computed once per combination and left unchanged"""
    key = (antialias, color, temporal)
    if key not in _wants:
        from denoising_diffusion_deep_fake_amd import ops
        untouched = _lit("untouched").model_a
        feather = ops.default_feather(*BOX[2:])
        state = ops.TemporalState(*SIZE)
        n = SIZE[0] * SIZE[1]
        out = []
        for raw in _writes():
            real = ops.crop_resize_cubic_u8(raw, SIZE, BOX, antialias=antialias)
            fake = untouched.predict_u8(real, MEAN, STD, graph=False)
            plain = torch.cat([real, fake], dim=2)
            if temporal:
                ops.temporal_filter_u8(real, fake, state, temporal, THRESHOLD)
            if color:
                s_to, s_from = ops.channel_sums_u8(real), ops.channel_sums_u8(fake)
                coef = ops.color_match_coef(s_from, s_to, n)
                if temporal:
                    ops.color_coef_smooth(coef, s_to, n, state, temporal)
                full = ops.paste_resize_cubic_u8(fake, raw, BOX, feather, color=coef)
            else:
                full = ops.paste_resize_cubic_u8(fake, raw, BOX, feather)
            out.append((plain, torch.cat([real, fake], dim=2), full))
        _wants[key] = out
    return _wants[key]


class _Buffers:
    """one input buffer and the two output buffers, the same ones for every call: what a captured graph bakes in"""

    def __init__(self):
        self.raw = torch.empty_like(_writes()[0])
        self.pair = torch.empty((B, SIZE[0], 2 * SIZE[1], 3), dtype=torch.uint8, device="cuda")
        self.full = torch.empty_like(self.raw)

    def check_both_entries(self, net, want, antialias, color, temporal, graph, writes, what):
        """a fresh sequence of `writes` writes through the pair entry, then one through the full-frame entry"""
        for entry in ("pair", "full"):
            net.reset_frame_temporal()
            for it in range(writes):
                self.raw.copy_(_writes()[it])
                self.pair.fill_(7)
                self.full.fill_(7)
                if entry == "pair":
                    net.predict_frames_u8(self.raw, SIZE, MEAN, STD, graph=graph, out=self.pair, antialias=antialias,
                                          temporal=temporal)
                else:
                    net.predict_frames_full_u8(self.raw, SIZE, MEAN, STD, graph=graph, out=self.full, pair_out=self.pair,
                                               antialias=antialias, color_match=color, temporal=temporal)
                    assert torch.equal(self.full, want[it][2]), (what, graph, it, "full entry, full")
                assert torch.equal(self.pair, want[it][1]), (what, graph, it, entry + " entry, pair")


@pytest.mark.parametrize("antialias, color, temporal", OPTIONS,
                         ids=[f"{'aa' if a else 'cubic'}-{c or 'plain'}-{'temporal' if t else 'still'}" for a, c, t in OPTIONS])
def test_every_combination_is_the_composition_of_the_ops(antialias, color, temporal):
    """three successive writes into one input buffer through both entries, eager and then from a graph into the same buffers;
    and each option that is on moves the bytes, against the combination that differs in that option alone"""
    want = _reference(antialias, color, temporal)
    if antialias:
        other = _reference(False, color, temporal)
        for it in range(WRITES):
            assert not torch.equal(want[it][1][:, :, :64], other[it][1][:, :, :64]), (it, "antialias moves the real half")
    if temporal:
        assert torch.equal(want[0][1][0], want[0][0][0]), "the first frame of the first write passes through"
        for it in range(1, WRITES):
            assert not torch.equal(want[it][1][:, :, 64:], want[it][0][:, :, 64:]), (it, "the filter changes the fake")
            assert torch.equal(want[it][1][:, :, :64], want[it][0][:, :, :64]), (it, "and not the real half")
    else:
        assert all(torch.equal(w[1], w[0]) for w in want)
    if color:
        other = _reference(antialias, None, temporal)
        for it in range(WRITES):
            assert torch.equal(want[it][1], other[it][1]), (it, "the colour match leaves the pair alone")
            assert not torch.equal(want[it][2], other[it][2]), (it, "and moves the pasted frame")
    net, bufs = _lit().model_a, _Buffers()
    for graph in (False, True):
        bufs.check_both_entries(net, want, antialias, color, temporal, graph, WRITES, "combination")


def test_one_option_changes_per_step_with_graphs_on():
    """one network, one set of buffers, graph=True throughout: the eight combinations in Gray-code order and back to all
    off.  Each step's bytes are those of the combination run eagerly (the test above holds them to the same reference), so
    a graph kept from the step before, which differs in one option, would show"""
    net, bufs = _lit().model_a, _Buffers()
    for step, (antialias, color, temporal) in enumerate(GRAY_WALK):
        want = _reference(antialias, color, temporal)
        bufs.check_both_entries(net, want, antialias, color, temporal, True, 2, ("step", step))
