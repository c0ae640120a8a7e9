"""GPU: held-out validation on the device -- the per-image scores of csrc/quality.hip against float64 with derived bounds
(tests/quality_restatement.py) and in the cases where the result is exact, the index form of the fixed-ratio noise blend
against the existing one and the numpy restatement of the draws, and the validation loop of the two trainers end to end."""
import numpy as np
import pytest
import torch

import quality_restatement as qr
import rng_restatement as rs
import test_gpu_helper_kernels as hk

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, OFFSET = 0x5EED, (1 << 24) | 2
# (1, 11, 11): one valid SSIM position; (2, 42, 42): 32 x 32 outputs fill exactly one output tile, the second tile row and
# column own the input rows and columns 32..41 and have no output; (3, 43, 75): ragged both ways; (5, 64, 96): scattered
SHAPES = [(1, 11, 11), (2, 42, 42), (3, 43, 75), (5, 64, 96)]
SCATTER_INDEX = [7, -1, 2, 9, 0]  # into N = 9: a permutation's worth of columns, one index below and one above the buffer


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from denoising_diffusion_deep_fake_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cases():
    """inputs (with pixels outside the range, so that mse and mse01 differ) and the float64 reference, made once"""
    out = {}
    for B, H, W in SHAPES:
        p, t = hk.loss_inputs(B, H, W, H)
        out[(B, H, W)] = (p, t, qr.quality_reference(p.double(), t.double()))
    return out


# ---- the operator against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_quality_per_image_against_float64(ops, cases, B, H, W):
    p, t, ref = cases[(B, H, W)]
    if B != 5:
        got = ops.quality_per_image(p.to(DEV), t.to(DEV)).cpu()
        assert got.shape == (4, B)
    else:
        index = torch.tensor(SCATTER_INDEX, device=DEV)
        buf = torch.full((4, 9), float("nan"), device=DEV)
        assert ops.quality_per_image(p.to(DEV), t.to(DEV), index=index, out=buf).data_ptr() == buf.data_ptr()
        buf = buf.cpu()
        named = [i for i in SCATTER_INDEX if 0 <= i < 9]
        untouched = [c for c in range(9) if c not in named]
        assert bool(torch.isnan(buf[:, untouched]).all()) and not bool(torch.isnan(buf[:, named]).any())
        # the two images whose index lies outside the buffer were not written: the others, in the batch's order
        keep = [b for b, i in enumerate(SCATTER_INDEX) if 0 <= i < 9]
        got = buf[:, named]
        ref = {row: qr.E(v.val[keep], v.err[keep]) for row, v in ref.items()}
    assert float((ref["mse"].val - ref["mse01"].val * 4).abs().max()) > 1e-4  # the planted pixels tell mse from 4 mse01
    qr.hold_rows(f"{B}x3x{H}x{W}", got, ref)
    # loss is formed from the fp32 mse and ssim as written: bit for bit
    assert torch.equal(got[3], (got[0] + (1.0 - got[1])) / 2.0)


def test_batch_means_agree_with_the_training_criterion(ops, cases):
    """mean over the batch of rows mse and ssim against d3f_mse_ssim_loss's out[1] and out[2] (all images have one size, so
    the batch mean is the mean of the image means), within the sum of the two derived bounds"""
    for (B, H, W), (p, t, ref) in cases.items():
        got = ops.quality_per_image(p.to(DEV), t.to(DEV)).cpu().double()
        out, _ = ops.mse_ssim_loss(p.to(DEV), t.to(DEV))
        out = out.cpu().double()
        _, mse, ssim, _ = hk.loss_reference(p.double().view(-1, H, W), t.double().view(-1, H, W))
        for row, i, whole in (("mse", 0, mse), ("ssim", 1, ssim)):
            d, bound = abs(float(got[i].mean() - out[i + 1])), float(ref[row].err.mean() + whole.err)
            print(f"{B}x3x{H}x{W} {row}: |batch mean - criterion| {d:.3e}, bound {bound:.3e}")
            assert d <= bound * (1 + 1e-3), (row, d, bound)


# ---- exact cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_prediction_equal_to_target_is_exact(ops, cases, B, H, W):
    """x = y: every product and sum of the map is the same on both sides, so each quotient is 1 and every sum of ones exact"""
    t = cases[(B, H, W)][1].to(DEV)
    got = ops.quality_per_image(t.clone(), t).cpu()
    assert bool((got[0] == 0).all()) and bool((got[1] == 1.0).all()) and bool((got[3] == 0).all())
    assert bool(torch.isposinf(got[2]).all())


def test_empty_batch_launches_nothing(ops):
    z = torch.zeros(0, 3, 32, 32, device=DEV)
    buf = torch.full((4, 3), float("nan"), device=DEV)
    assert ops.quality_per_image(z, z, index=torch.zeros(0, dtype=torch.int64, device=DEV), out=buf) is buf
    assert bool(torch.isnan(buf).all())
    assert ops.quality_per_image(z, z, N=2).shape == (4, 2)


def test_repeat_and_batch_position_do_not_change_the_bits(ops, cases):
    p, t, _ = cases[(5, 64, 96)]
    p, t = p.to(DEV), t.to(DEV)
    first, second = ops.quality_per_image(p, t), ops.quality_per_image(p, t)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    for i in range(5):  # image i alone (B = 1) against its column in the batch of 5
        alone = ops.quality_per_image(p[i:i + 1], t[i:i + 1])
        assert torch.equal(alone.view(torch.int32)[:, 0], first.view(torch.int32)[:, i]), i
    back = ops.quality_per_image(p.flip(0), t.flip(0))  # ... and in another place of another batch
    assert torch.equal(back.flip(1).view(torch.int32), first.view(torch.int32))


# ---- the index form of the noise blend ---------------------------------------------------------------------------------
def test_index_blend_equals_the_fixed_blend_at_arange(ops):
    from denoising_diffusion_deep_fake_amd.dataset import synthetic_face_crops
    for shape in ((5, 3, 64, 64), (2, 3, 40, 36)):
        x = synthetic_face_crops(shape[0], shape[2:], seed=3, device=DEV)
        ratios = torch.linspace(0.05, 0.95, shape[0], device=DEV)
        index = torch.arange(shape[0], device=DEV)
        for r in (ratios, 0.2):
            got = ops.noise_blend_fixed_index_rng(x, SEED, OFFSET, r, index)
            assert torch.equal(got.view(torch.int32), ops.noise_blend_fixed_rng(x, SEED, OFFSET, r).view(torch.int32))
        assert torch.equal(ops.noise_blend_fixed_index_rng(x, SEED, OFFSET, 0.2, list(range(shape[0]))), got)  # host index


def test_index_blend_draws_by_the_index_not_the_place(ops):
    from denoising_diffusion_deep_fake_amd.dataset import synthetic_face_crops
    index = [4, 0, 2]
    x5 = synthetic_face_crops(5, 64, seed=4, device=DEV)
    whole = ops.noise_blend_fixed_rng(x5, SEED, OFFSET, 0.5)
    got = ops.noise_blend_fixed_index_rng(x5[index].contiguous(), SEED, OFFSET, 0.5, torch.tensor(index, device=DEV))
    assert torch.equal(got.view(torch.int32), whole[index].view(torch.int32))
    # the draws themselves: x = 0 at ratio 1 leaves 0 * 0 + 1 * z = z exactly; against the float64 Box-Muller of the same
    # words, with the bound tests/test_gpu_rng.py states (16 * 2^-24 * max(1, R))
    big = [4, 0, 2, (1 << 32) - 1]
    z = ops.noise_blend_fixed_index_rng(torch.zeros(4, 3, 16, 16, device=DEV), SEED, OFFSET, 1.0, torch.tensor(big, device=DEV))
    z64, r64 = rs.normals64(SEED, OFFSET, 4, 3 * 16 * 16, images=big)
    err = np.abs(z.cpu().numpy().reshape(4, -1).astype(np.float64) - z64)
    assert (err <= 16 * 2.0 ** -24 * np.maximum(1.0, r64)).all(), float(err.max())
    # an index the counter cannot hold: refused where the host sees it, NaN for that image where it does not
    with pytest.raises(ValueError, match="outside"):
        ops.noise_blend_fixed_index_rng(x5[:2], SEED, OFFSET, 0.5, [1, 1 << 32])
    bad = ops.noise_blend_fixed_index_rng(x5[:3].contiguous(), SEED, OFFSET, 0.5, torch.tensor([1, 1 << 32, -1], device=DEV))
    assert bool(torch.isnan(bad[1:]).all())
    assert torch.equal(bad[0], ops.noise_blend_fixed_index_rng(x5[:1].contiguous(), SEED, OFFSET, 0.5, [1])[0])


# ---- end to end: Trainer.fit with a held-out set ---------------------------------------------------------------------
RATIOS = [0.1, 0.4]
HP_DENOISER = dict(batch_size=4, learning_rate=0.002, max_epochs=2, cosine_scheduler_max_epoch=4, num_workers=0,
                   encoder_name="resnet18", noise_exponential_sampling_lambda=5, mean=[128, 128, 128], std=[128, 128, 128],
                   synthetic=True, image_size=64, augment=True, synthetic_length=8)
HP_FAKE = dict(mode="denoise", batch_size=4, learning_rate=0.002, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet18", noise_exponential_sampling_lambda=3,
               mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3, std_b=[0.5] * 3, synthetic=True, image_size=64,
               synthetic_length=8, ema_beta=0.9999, ema_update_every=1, augment=True)
VAL = dict(val_synthetic_length=6, val_noise_ratios=RATIOS)  # batches of 4 + 2
SUFFIXES = ["", "_r0.1", "_r0.4"]


def fit(cls, hp, root, epochs):
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    torch.manual_seed(31)
    lit = cls(**dict(hp, default_root_dir=str(root)))
    torch.manual_seed(32)
    tr = Trainer(max_epochs=epochs, log_every_n_steps=1, default_root_dir=root).fit(lit)
    torch.cuda.synchronize()
    return lit, tr


def metric_rows(tr):
    rows = []
    for line in (tr.log_dir / "metrics.csv").read_text().splitlines():
        step, _, rest = line.partition(",")
        rows.append((int(step), {k: float(v) for k, v in (kv.split("=") for kv in rest.split(";"))}))
    return rows


def trained_state(lit):
    return {k: v.detach().clone() for k, v in lit.state_dict().items()}


@pytest.fixture(scope="module")
def denoiser_fit(tmp_path_factory):
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
    root = tmp_path_factory.mktemp("denoiser_val")
    report = root / "reports" / "val.tsv"
    return fit(LitModule, dict(HP_DENOISER, **VAL, val_report_path=str(report)), root, 2) + (report,)


def test_fit_logs_every_validation_key_and_keeps_the_best_epoch(denoiser_fit):
    lit, tr, report = denoiser_fit
    keys = {f"val/{m}{s}" for m in ("loss", "mse", "ssim", "psnr") for s in SUFFIXES} | {"val/psnr_inf"}
    rows = [(step, row) for step, row in metric_rows(tr) if any(k.startswith("val/") for k in row)]
    # two steps an epoch, a training row per step: the validation of epoch 0 gets its own row at step 2, rides along in the
    # training rows of steps 3 and 4, and the validation of epoch 1 gets its own row at step 4
    assert [step for step, _ in rows] == [2, 3, 4, 4]
    per_epoch = {}
    for step, row in rows:
        assert keys <= set(row), keys - set(row)
        assert all(np.isfinite(row[k]) for k in keys), row
        assert row["val/psnr_inf"] == 0 and 0 < row["val/ssim"] <= 1 and row["val/mse"] > 0
        per_epoch[step] = row["val/loss"]  # the last row of a step holds that epoch's validation
    assert not bool(torch.isnan(lit._val["flat"]).any())
    best = torch.load(tr.log_dir / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=False)
    assert best["epoch"] == (0 if per_epoch[2] <= per_epoch[4] else 1)
    assert best["hyper_parameters"]["val_noise_ratios"] == RATIOS
    assert len(list((tr.log_dir / "checkpoints").glob("epoch=*.ckpt"))) == 1  # the per-epoch checkpoint goes on as before
    lines = report.read_text().splitlines()
    assert len(lines) == 6 * len(RATIOS) and lines[0].startswith("synthetic/0\t0.1\t") and all(len(l.split("\t")) == 6 for l in lines)


def test_validation_repeats_and_equals_the_public_ops(denoiser_fit, ops):
    lit, tr, _ = denoiser_fit
    device = lit.device
    tr._run_validation(lit, device)
    first = lit._val["flat"].clone()
    state = (torch.random.get_rng_state(), torch.cuda.get_rng_state())
    tr._run_validation(lit, device)
    assert torch.equal(first.view(torch.int32), lit._val["flat"].view(torch.int32))  # no training step between: same bits
    assert torch.equal(torch.random.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert lit.training
    from denoising_diffusion_deep_fake_amd import rng
    seed = rng.module_stream(lit)[0]
    want = torch.full((len(RATIOS), 4, 6), float("nan"), device=device)
    lit.eval()
    with torch.no_grad():
        for batch in lit.val_dataloader():
            image, index = batch["image"].to(device), batch["index"].to(device)
            for k, ratio in enumerate(RATIOS):
                noisy = ops.noise_blend_fixed_index_rng(image, seed, rng.pack_offset(k, 0, 2), ratio, index)
                ops.quality_per_image(lit.model(noisy), image, -1.0, 1.0, index=index, out=want[k])
        # an image meets the same noise at any batch size: all six at once
        whole = torch.stack([lit.validation_datasets()[""][i]["image"] for i in range(6)]).to(device)
        at_once = ops.noise_blend_fixed_index_rng(whole, seed, rng.pack_offset(1, 0, 2), RATIOS[1], torch.arange(6, device=device))
        assert torch.equal(at_once[4:], ops.noise_blend_fixed_index_rng(whole[4:].contiguous(), seed, rng.pack_offset(1, 0, 2),
                                                                      RATIOS[1], torch.tensor([4, 5], device=device)))
    lit.train()
    assert torch.equal(want.view(torch.int32).reshape(-1), first.view(torch.int32))


def test_validation_changes_nothing_that_is_trained(denoiser_fit, tmp_path):
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
    lit_on = denoiser_fit[0]
    lit_off, tr_off = fit(LitModule, HP_DENOISER, tmp_path, 2)
    assert lit_off.val_dataloader() is None and not (tr_off.log_dir / "checkpoints" / "best.ckpt").exists()
    assert not any(k.startswith("val") for _, row in metric_rows(tr_off) for k in row)
    on, off = trained_state(lit_on), trained_state(lit_off)
    assert on.keys() == off.keys() and any("running_mean" in k for k in on)
    assert all(torch.equal(on[k], off[k]) for k in on), [k for k in on if not torch.equal(on[k], off[k])][:5]
    assert torch.equal(lit_on.model.flat_params, lit_off.model.flat_params)


def test_deep_fake_validation_scores_both_domains_and_changes_nothing(tmp_path):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    lit_on, tr_on = fit(LitModule, dict(HP_FAKE, **VAL), tmp_path / "on", 2)  # (a second epoch trains after a validation)
    lit_off, _ = fit(LitModule, HP_FAKE, tmp_path / "off", 2)
    row = [row for _, row in metric_rows(tr_on) if "val/loss" in row][-1]
    for prefix in ("val_a", "val_b", "val"):
        for m in ("loss", "mse", "ssim", "psnr"):
            for s in SUFFIXES if prefix != "val" else [""]:
                assert np.isfinite(row[f"{prefix}/{m}{s}"]), (prefix, m, s)
    assert row["val/loss"] == pytest.approx((row["val_a/loss"] + row["val_b/loss"]) / 2, rel=1e-5)
    assert row["val_a/loss"] != row["val_b/loss"] and not bool(torch.isnan(lit_on._val["flat"]).any())
    assert (tr_on.log_dir / "checkpoints" / "best.ckpt").exists() and (tr_on.log_dir / "checkpoints" / "last.ckpt").exists()
    assert lit_on._pair is not None  # training went on taking the fused two-network route
    on, off = trained_state(lit_on), trained_state(lit_off)
    assert on.keys() == off.keys() and all(torch.equal(on[k], off[k]) for k in on)
