"""GPU: the image-grid kernel byte for byte against its torch restatement (tests/image_grid_restatement.py), and the
three trainers writing the reference's tags through it without changing what they train."""
import numpy as np
import pytest
import torch

from image_grid_restatement import image_grid_u8 as restated_grid

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xA5


def boundary_values():
    """every value at which the byte changes, 2k/255 - 1 for k = 0..255, with both float32 neighbours of each; +-1 (among
    them), the middle of every byte's interval, values beyond +-1, +-inf, NaN, zeros and a few ordinary values"""
    k = torch.arange(256, dtype=torch.float64)
    edges = (2 * k / 255 - 1).float()
    up = torch.nextafter(edges, torch.full_like(edges, 2.0))
    down = torch.nextafter(edges, torch.full_like(edges, -2.0))
    special = torch.tensor([1.0, -1.0, 1.5, -1.5, 37.0, -1e30, 3e38, float("inf"), -float("inf"), float("nan"), 0.0, -0.0,
                            1e-40, 0.25, -0.3333])
    middles = ((2 * k[:255] + 1) / 255 - 1).float()  # (k + 0.5) / 255 after scaling: byte k, far from any boundary
    return torch.cat([edges, up, down, middles, special])


def batch_of(shape, seed):
    """a batch holding the boundary values: all of them, in shuffled places, when it is large enough; a draw otherwise"""
    g = torch.Generator().manual_seed(seed)
    vals = boundary_values()
    n = int(np.prod(shape))
    x = vals[torch.randint(0, len(vals), (n,), generator=g)]
    if n >= len(vals):
        x[torch.randperm(n, generator=g)[:len(vals)]] = vals
    return x.reshape(shape).contiguous()


def grid_in_guarded_buffer(ops, batches, misalign, **kw):
    """ops.image_grid_u8 into the middle of a poisoned buffer, `misalign` bytes past a 64-byte boundary: the grids, and
    whether the guard bytes on both sides are untouched"""
    xs = [batches] if isinstance(batches, torch.Tensor) else list(batches)
    B, _, H, W = xs[0].shape
    images = min(B, kw.get("max_images", 9))
    GH, GW = ops.image_grid_shape(images, kw.get("nrow", 3), kw.get("padding", 2), (H, W))
    nbytes = len(xs) * GH * GW * 3
    buf = torch.full((GUARD + misalign + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 64 == 0
    out = buf[GUARD + misalign:GUARD + misalign + nbytes].view(len(xs), GH, GW, 3)
    got = ops.image_grid_u8(batches, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu()
    intact = bool((host[:GUARD + misalign] == POISON).all()) and bool((host[GUARD + misalign + nbytes:] == POISON).all())
    return got.cpu(), intact


# B x C x H x W: a full 3 x 3 grid; a blank last cell; xmaps < nrow; a single image (no border); a row length that is no
# multiple of 4 bytes with unaligned plane starts (35 floats per plane); one channel, odd width; 14 images capped at 9
SHAPES = [(9, 3, 32, 40), (8, 3, 32, 40), (2, 3, 32, 40), (1, 3, 32, 40), (3, 3, 5, 7), (4, 1, 16, 33), (14, 3, 32, 40)]


@pytest.mark.parametrize("padding", [0, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement(shape, padding):
    from denoising_diffusion_deep_fake_amd import ops
    x = batch_of(shape, seed=sum(shape) + padding)
    want = restated_grid(x, 3, padding)
    if shape[0] == 8 and padding:
        assert bool((want[-1, -1] == 127).all()) and bool((want[-(shape[2] // 2) - padding, -(shape[3] // 2)] == 127).all())
    misalign = (shape[0] + padding) % 4  # the output's start takes every residue over the cases
    got, intact = grid_in_guarded_buffer(ops, x.cuda(), misalign, padding=padding)
    assert got.shape == (1,) + tuple(want.shape) and got.dtype == torch.uint8
    assert torch.equal(got[0], want)
    assert intact, "bytes outside the output were written"


def test_blank_cell_and_padding_are_mid_grey_and_every_byte_value_occurs():
    from denoising_diffusion_deep_fake_amd import ops
    x = batch_of((8, 3, 32, 40), seed=1)
    got = ops.image_grid_u8(x.cuda()).cpu()[0]
    assert got.shape == (104, 128, 3)
    assert bool((got[70:, 86:] == 127).all())        # the ninth cell and its borders
    assert bool((got[:2] == 127).all()) and bool((got[:, :2] == 127).all())
    assert len(torch.unique(got)) == 256            # the boundary values reach every byte
    assert torch.equal(got, restated_grid(x))


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_four_batches_in_one_call_equal_four_single_calls(misalign):
    from denoising_diffusion_deep_fake_amd import ops
    xs = [batch_of((3, 3, 5, 7) if misalign % 2 else (9, 3, 32, 40), seed=20 + i) for i in range(4)]
    dev = [x.cuda() for x in xs]
    got, intact = grid_in_guarded_buffer(ops, dev, misalign)
    assert intact and got.shape[0] == 4
    for i in range(4):
        assert torch.equal(got[i], ops.image_grid_u8(dev[i]).cpu()[0]), i
        assert torch.equal(got[i], restated_grid(xs[i])), i


def test_eight_batches_other_arguments_and_a_non_contiguous_input():
    from denoising_diffusion_deep_fake_amd import _lib, ops
    xs = [batch_of((5, 3, 9, 11), seed=40 + i) for i in range(8)]
    kw = dict(nrow=2, padding=1, pad_value=1.0, scale=1.0, shift=0.0, max_images=5)
    got, intact = grid_in_guarded_buffer(ops, [x.cuda() for x in xs], 1, **kw)
    assert intact and got.shape == (8, 31, 25, 3)
    for i in range(8):
        assert torch.equal(got[i], restated_grid(xs[i], **kw)), i
    assert bool((got[:, 0] == 255).all()) and bool((got[:, 21:, 13:] == 255).all())  # pad_value 1 -> 255; the blank cell
    with pytest.raises(_lib.D3FError):
        ops.image_grid_u8([x.cuda() for x in xs] + [xs[0].cuda()])  # nine batches
    # a non-contiguous view (every other column of a wider batch, channels-last memory) goes through the wrapper
    wide = batch_of((4, 3, 12, 26), seed=50)
    view = wide.cuda()[:, :, :, ::2]
    assert not view.is_contiguous()
    assert torch.equal(ops.image_grid_u8(view).cpu()[0], restated_grid(wide[:, :, :, ::2]))
    cl = batch_of((4, 3, 12, 13), seed=51).cuda().contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert torch.equal(ops.image_grid_u8(cl).cpu()[0], restated_grid(cl.cpu()))


# ---- trainers ---------------------------------------------------------------------------------------------------------
HP = dict(encoder_name="resnet18", batch_size=3, image_size=64, synthetic=True, synthetic_length=6, num_workers=0,
          learning_rate=0.01, cosine_scheduler_max_epoch=10, max_epochs=1, augment=False,
          image_logging=True, image_logging_every_n_steps=1)
HP_FAKE = dict(HP, mode="denoise", adam_b1=0.5, adam_b2=0.999, noise_exponential_sampling_lambda=3, mean_a=[0.5] * 3,
               std_a=[0.5] * 3, mean_b=[0.5] * 3, std_b=[0.5] * 3, ema_beta=0.9999, ema_update_every=1)
HP_DENOISER = dict(HP, noise_exponential_sampling_lambda=5, mean=[128] * 3, std=[128] * 3)


def fit(cls, hp, root, sink=None, prepare=None):
    """two batches of Trainer.fit on fixed seeds"""
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    torch.manual_seed(21)
    lit = cls(**hp)
    if sink is not None:
        lit.image_grid_sink = sink
    if prepare is not None:
        prepare(lit)
    torch.manual_seed(22)
    tr = Trainer(max_epochs=1, log_every_n_steps=1, default_root_dir=root, enable_checkpointing=False,
                 limit_train_batches=2).fit(lit)
    return lit, tr


def written(tr):
    from PIL import Image
    root = tr.log_dir / "images"
    out = {}
    for path in sorted(root.rglob("*.png")):
        with Image.open(path) as im:
            out[path.relative_to(root).as_posix()] = (im.size, im.mode)
    return out


def count_launches(monkeypatch):
    from denoising_diffusion_deep_fake_amd import ops
    calls = []
    kernel = ops.image_grid_u8

    def counted(batches, *a, **kw):
        calls.append(len(batches))
        return kernel(batches, *a, **kw)

    monkeypatch.setattr(ops, "image_grid_u8", counted)
    return calls


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "sequential"])
def test_deep_fake_denoise_mode_writes_its_four_tags_per_step(tmp_path, monkeypatch, fused):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    calls = count_launches(monkeypatch)
    lit, tr = fit(LitModule, dict(HP_FAKE, **({} if fused else {"pair_fused": False})), tmp_path)
    assert tr.global_step == 4
    want = {f"{tag}/{name}/step_{step:08d}.png": ((200, 68), "RGB")
            for tag in ("denoise_1_model_input", "denoise_2_model_prediction") for name in "ab" for step in (0, 2)}
    assert written(tr) == want
    # the fused route logs a batch's four tags with ONE kernel call, the sequential loop two per optimizer step
    assert calls == ([4, 4] if fused else [2, 2, 2, 2])
    assert (tr.log_dir / "metrics.csv").exists()


def test_swap_mode_writes_its_eight_tags(tmp_path, monkeypatch):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    calls = count_launches(monkeypatch)
    lit, tr = fit(LitModule, dict(HP_FAKE, mode="swap"), tmp_path)
    tags = [f"swap_1_real/{n}" for n in "ab"] + [f"swap_2_fake/{n}_to_fake" for n in "ab"] + \
           [f"swap_3_model_input/{n}" for n in "ab"] + [f"swap_4_model_prediction/{n}" for n in "ab"]
    assert written(tr) == {f"{tag}/step_{step:08d}.png": ((200, 68), "RGB") for tag in tags for step in (0, 2)}
    assert calls == [4, 4, 4, 4]  # four tags per optimizer step, one launch each


def test_denoiser_and_balance_write_their_three_tags(tmp_path, monkeypatch):
    from denoising_diffusion_deep_fake_amd.balance_training_images.lit_module import LitModule as Balance
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule as Denoiser
    calls = count_launches(monkeypatch)
    want = {f"{tag}/step_{step:08d}.png": ((200, 68), "RGB")
            for tag in ("image", "image_noisy", "image_prediction") for step in (0, 1)}
    lit, tr = fit(Denoiser, HP_DENOISER, tmp_path / "denoiser")
    assert written(tr) == want and calls == [3, 3]
    hp = dict(HP, ratio_of_noise=0.3, number_of_classes=4, mean=[128] * 3, std=[128] * 3)
    lit, tr = fit(Balance, hp, tmp_path / "balance")
    assert written(tr) == want and calls == [3, 3, 3, 3]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "sequential"])
def test_model_input_grid_is_the_restatement_of_the_blended_batch(tmp_path, fused):
    """the tensor blend_random_amount_of_noise_with_each_sample returns is what the network is fed: its grid, as the
    sink receives it, is the restatement of that tensor byte for byte -- for both domains, at both steps, in order"""
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    blended, got = [], []

    def record(lit):
        blend = lit.blend_random_amount_of_noise_with_each_sample

        def recording(batch, stream=0):
            out = blend(batch, stream)
            blended.append(("ab"[stream], out.detach().clone()))
            return out

        lit.blend_random_amount_of_noise_with_each_sample = recording

    lit, tr = fit(LitModule, dict(HP_FAKE, **({} if fused else {"pair_fused": False})), tmp_path,
                  sink=lambda tag, step, array: got.append((tag, step, array)), prepare=record)
    assert [name for name, _ in blended] == ["a", "b", "a", "b"]
    assert [(t, s) for t, s, _ in got] == [(f"{tag}/{name}", step) for step in (0, 2) for name in "ab"
                                           for tag in ("denoise_1_model_input", "denoise_2_model_prediction")]
    inputs = [(t, a) for t, _, a in got if t.startswith("denoise_1_model_input/")]
    for (tag, array), (name, tensor) in zip(inputs, blended):
        assert tag.endswith("/" + name) and array.shape == (68, 200, 3) and array.dtype == np.uint8
        assert np.array_equal(array, restated_grid(tensor).numpy()), tag
    predictions = [a for t, _, a in got if t.startswith("denoise_2_model_prediction/")]
    assert all(a.shape == (68, 200, 3) and (a[:2] == 127).all() and len(np.unique(a[2:66, 2:66])) > 8 for a in predictions)
    assert not (tr.log_dir / "images").exists()  # the sink replaces the file writer


def same(a, b):
    """equality of nested state: tensors bit for bit"""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_image_logging_changes_nothing_that_is_trained(tmp_path):
    """the same two-batch fit with and without image_logging, on the same seeds: equal parameters, optimizer moments,
    BatchNorm statistics and logged losses"""
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    runs = []
    for on in (True, False):
        hp = dict(HP_FAKE)
        if not on:
            del hp["image_logging"], hp["image_logging_every_n_steps"]
        lit, tr = fit(LitModule, hp, tmp_path / f"on{int(on)}")
        rows = (tr.log_dir / "metrics.csv").read_text()
        runs.append(({k: v.detach().cpu() for k, v in lit.state_dict().items()},
                     [o.state_dict() for o in tr.optimizers], rows, (tr.log_dir / "images").exists()))
    (sd_on, opt_on, rows_on, images_on), (sd_off, opt_off, rows_off, images_off) = runs
    assert images_on and not images_off
    assert sd_on.keys() == sd_off.keys() and all(torch.equal(sd_on[k], sd_off[k]) for k in sd_on)
    assert rows_on == rows_off and "loss_denoise/train_a" in rows_on and len(rows_on.strip().splitlines()) == 2
    assert same(opt_on, opt_off)
