"""Host side of held-out validation (no GPU): the new C entries are declared, bound and exported and refuse on the host, the
derived bounds of the per-image scores admit a plain torch fp32 evaluation, the two LitModules refuse what validation
cannot be combined with, the held-out loader keeps the list's order, ModelCheckpoint understands `monitor`, and the report
file and the shipped configs have the stated form."""
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import quality_restatement as qr
import test_gpu_helper_kernels as hk
from denoising_diffusion_deep_fake_amd import _lib, ops
from denoising_diffusion_deep_fake_amd.helpers import validation

PACKAGE = Path(_lib.__file__).resolve().parent
ENTRIES = ("d3f_quality_per_image_workspace_bytes", "d3f_quality_per_image_scatter", "d3f_noise_blend_fixed_index_rng")
HP_DENOISER = dict(batch_size=4, learning_rate=0.02, max_epochs=2, cosine_scheduler_max_epoch=2, num_workers=0,
                   encoder_name="resnet18", noise_exponential_sampling_lambda=5, mean=[128, 128, 128], std=[128, 128, 128],
                   synthetic=True, image_size=64, augment=False, synthetic_length=8)
HP_FAKE = dict(mode="denoise", batch_size=4, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
               cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet18", noise_exponential_sampling_lambda=3,
               mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3, std_b=[0.5] * 3, synthetic=True, image_size=64,
               synthetic_length=4, ema_beta=0.9999, ema_update_every=1, augment=False)
SHAPES = [(1, 11, 11), (2, 42, 42), (3, 43, 75), (5, 64, 96)]  # tests/test_gpu_quality.py: the shapes the kernel is held at


def denoiser(**kw):
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
    return LitModule(**dict(HP_DENOISER, **kw))


def deep_fake(**kw):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    return LitModule(**dict(HP_FAKE, **kw))


# ---- the C entries ---------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    declared = _lib.header_symbols()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in declared and name in _lib.PROTOTYPES
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert callable(ops.quality_per_image) and callable(ops.noise_blend_fixed_index_rng)
    header = _lib.HEADER_PATH.read_text()
    assert "structural_similarity_loss.py:14-26" in header.split("d3f_quality_per_image_workspace_bytes")[0][-2500:]
    assert "quality.hip" in (PACKAGE / "csrc" / "Makefile").read_text()
    assert "index[b]" in (PACKAGE / "csrc" / "philox.h").read_text()
    # three sums per tile, tiles(W) x tiles(H) x 3B tiles
    assert lib.d3f_quality_per_image_workspace_bytes(16, 256, 256) >= 16 * 3 * 8 * 8 * 3 * 4
    assert lib.d3f_quality_per_image_workspace_bytes(1, 42, 42) >= 3 * 2 * 2 * 3 * 4


def test_refusals_happen_before_any_device_call():
    """the dummy pointers are never dereferenced: every call below returns on the host"""
    lib = _lib.lib()
    d = C.c_void_p(0x1000)

    def quality(pred=d, target=d, lo=-1.0, hi=1.0, metrics=d, N=9, ws=d, B=5, H=32, W=32):
        return lib.d3f_quality_per_image_scatter(pred, target, lo, hi, None, metrics, N, ws, B, H, W, None)

    assert quality(B=0) == 0  # nothing to do
    for kw, word in ((dict(pred=None), b"null"), (dict(target=None), b"null"), (dict(metrics=None), b"null"),
                     (dict(ws=None), b"null"), (dict(H=10), b"11x11"), (dict(W=10), b"11x11"), (dict(lo=1.0), b"range"),
                     (dict(lo=2.0, hi=1.0), b"range"), (dict(N=0), b"N = 0"), (dict(N=-3), b"N = -3"),
                     (dict(B=21846), b"21845")):
        assert quality(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert lib.d3f_noise_blend_fixed_index_rng(d, 1, 2, d, d, d, 0, 192, None) == 0  # B == 0
    for args in ((None, 1, 2, d, d, d), (d, 1, 2, None, d, d), (d, 1, 2, d, None, d), (d, 1, 2, d, d, None)):
        assert lib.d3f_noise_blend_fixed_index_rng(*args, 2, 192, None) != 0 and b"null" in lib.d3f_last_error()
    assert lib.d3f_noise_blend_fixed_index_rng(d, 1, 2, d, d, C.c_void_p(0x2000), 2, 6, None) != 0
    assert b"multiple of 4" in lib.d3f_last_error()
    # the python surface refuses the same on host tensors, before it asks for a device
    x = torch.zeros(2, 3, 32, 32)
    for args, kw in (((x[:, :, :10], x[:, :, :10]), {}), ((x, x), dict(lo=1.0, hi=1.0)), ((x, x), dict(N=0)),
                     ((x, x[:1]), {}), ((x, x), dict(index=torch.zeros(3, dtype=torch.int64)))):
        with pytest.raises(ValueError):
            ops.quality_per_image(*args, **kw)
    for index in ([0, 1 << 32], [-1, 0], torch.tensor([0, 1 << 40])):
        with pytest.raises(ValueError, match="outside"):
            ops.noise_blend_fixed_index_rng(x, 1, 2, 0.5, index)


# ---- the bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_quality_bounds_admit_torch_fp32(B, H, W):
    """a plain torch fp32 evaluation (conv2d's and mean's own summation orders, torch's fp32 log10) stays inside the bounds
    the kernel is held to, at every shape: the bounds are neither vacuous nor out of an honest evaluation's reach"""
    p, t = hk.loss_inputs(B, H, W, H)
    ref = qr.quality_reference(p.double(), t.double())
    qr.hold_rows(f"torch fp32 {B}x3x{H}x{W}", qr.quality_torch_fp32(p, t), ref)
    # not vacuous: no bound is wider than 1e-3 of its value (the widest is the SSIM of the single 11 x 11 window, where
    # E[x^2] - mu^2 cancels most digits); a missing tap or a wrong constant moves a value by more than that
    for row in qr.ROWS:
        assert bool((ref[row].err < 1e-3 * ref[row].val.abs()).all()), row
    # and the float64 values are the criterion's: the batch means against the float64 reference of the training loss
    _, mse, ssim, _ = hk.loss_reference(p.double().view(-1, H, W), t.double().view(-1, H, W))
    assert abs(float(ref["mse"].val.mean() - mse.val)) < 1e-12 and abs(float(ref["ssim"].val.mean() - ssim.val)) < 1e-12


# ---- the LitModules --------------------------------------------------------------------------------------------------
def test_validation_is_off_without_its_keys():
    for lit in (denoiser(), deep_fake()):
        assert lit.val_dataloader() is None and not lit.validation_on()
        assert not any(k.startswith("val_") for k in lit.hparams)
    from denoising_diffusion_deep_fake_amd.trainer import ModelCheckpoint
    assert denoiser().configure_callbacks() == []
    assert not any(c.filename == "best" for c in deep_fake().configure_callbacks() if isinstance(c, ModelCheckpoint))


def test_refusals_at_construction(monkeypatch, tmp_path):
    for ratios in ([], [0.0], [1.0], [0.2, -0.1], [0.5, "x"], [0.1] * 17, 0.3, "0.3", [True]):
        with pytest.raises(ValueError, match="val_noise_ratios"):
            denoiser(val_noise_ratios=ratios)  # refused whether or not a held-out set is named
        with pytest.raises(ValueError, match="val_noise_ratios"):
            deep_fake(val_synthetic_length=6, val_noise_ratios=ratios)
    assert denoiser(val_synthetic_length=6)._val["ratios"] == (0.05, 0.2, 0.5)
    assert denoiser(val_synthetic_length=6, val_noise_ratios=[0.1] * 16)._val["ratios"] == (0.1,) * 16
    with pytest.raises(ValueError, match="graph_step"):
        denoiser(val_synthetic_length=6, graph_step=True)
    with pytest.raises(ValueError, match="val_synthetic_length"):
        denoiser(val_synthetic_length=6, synthetic=False, input_image_list_path=str(tmp_path / "images.txt"))
    with pytest.raises(ValueError, match="val_synthetic_length"):
        denoiser(val_synthetic_length=0)
    with pytest.raises(ValueError, match="val_data_path_b"):
        deep_fake(val_data_path_a=str(tmp_path / "a.txt"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="val_synthetic_length.*world size"):
        denoiser(val_synthetic_length=6)
    with pytest.raises(ValueError, match="val_image_list_path.*world size"):
        denoiser(val_image_list_path=str(tmp_path / "images.txt"))
    with pytest.raises(ValueError, match="val_data_path_a.*world size"):
        deep_fake(val_data_path_a=str(tmp_path / "a.txt"), val_data_path_b=str(tmp_path / "b.txt"))
    denoiser(), deep_fake()  # without the keys nothing is refused
    monkeypatch.setenv("WORLD_SIZE", "1")
    lit = denoiser(val_synthetic_length=6, val_noise_ratios=[0.1, 0.4], val_report_path="r.tsv")
    assert lit.hparams.val_noise_ratios == [0.1, 0.4] and lit.hparams.val_report_path == "r.tsv"  # saved with the checkpoint


def _write_images(folder, n, size=16):
    from PIL import Image
    folder.mkdir(parents=True, exist_ok=True)
    g = np.random.default_rng(0)
    names = [f"sub/im_{9 - i}.png" for i in range(n)]  # not in sorted order: the list's order is the loader's
    (folder / "sub").mkdir(exist_ok=True)
    for name in names:
        Image.fromarray(g.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(folder / name)
    (folder / "images.txt").write_text("".join(name + "\n" for name in names))
    return folder / "images.txt", names


def test_val_dataloader_keeps_the_lists_order(tmp_path):
    path, names = _write_images(tmp_path / "held_out", 6)
    for uint8 in (False, True):
        lit = denoiser(val_image_list_path=str(path), uint8_batches=uint8)
        loader = lit.val_dataloader()
        state = torch.random.get_rng_state()
        passes = [list(loader), list(loader)]
        assert torch.equal(torch.random.get_rng_state(), state)  # iterating draws nothing from torch's generator
        assert [b["index"].tolist() for b in passes[0]] == [[0, 1, 2, 3], [4, 5]]  # the ragged last batch is kept
        for a, b in zip(*passes):
            assert torch.equal(a["index"], b["index"]) and torch.equal(a["image"], b["image"])
        assert passes[0][0]["image"].dtype == (torch.uint8 if uint8 else torch.float32)
        assert lit.validation_image_names("") == names
        first = passes[0][0]["image"][0]
        direct = lit.validation_datasets()[""][0]["image"]
        assert torch.equal(first, direct)
    lit = deep_fake(val_synthetic_length=3, batch_size=2)
    batches = list(lit.val_dataloader())
    assert [(b["domain"], b["index"].tolist()) for b in batches] == [("a", [0, 1]), ("a", [2]), ("b", [0, 1]), ("b", [2])]
    assert len(lit.val_dataloader()) == 4
    # the held-out synthetic images are not the training ones, and the two domains' differ
    train = lit.train_dataloader()
    seeds = {lit.validation_datasets()[d].seed for d in "ab"} | {train[d].dataset.seed for d in "ab"}
    assert len(seeds) == 4 and min(lit.validation_datasets()[d].seed for d in "ab") > max(
        train[d].dataset.seed + len(train[d].dataset) for d in "ab")


# ---- epoch end on the host -------------------------------------------------------------------------------------------
def test_summary_and_report_format():
    nan, inf = float("nan"), float("inf")
    ratios = (0.05, 0.5)
    scores = np.full((2, 4, 3), nan)
    scores[0, :, 0] = (0.25, 0.5, 10.0, 0.375)
    scores[0, :, 2] = (0.75, 1.0, inf, 0.125)     # a perfect PSNR: left out of the mean, counted
    scores[1, :, 0] = (0.5, 0.25, 20.0, 0.625)    # image 1 was never scored; image 2 only at the first ratio
    s = validation.summarise(scores, ratios, "val")
    assert s["val/mse"] == 0.5 and s["val/ssim"] == pytest.approx(1.75 / 3) and s["val/loss"] == 0.375
    assert s["val/psnr"] == 15.0 and s["val/psnr_inf"] == 1.0
    assert s["val/mse_r0.05"] == 0.5 and s["val/mse_r0.5"] == 0.5 and s["val/psnr_r0.05"] == 10.0 and s["val/psnr_r0.5"] == 20.0
    assert set(s) == {f"val/{m}{r}" for m in ("mse", "ssim", "psnr", "loss") for r in ("", "_r0.05", "_r0.5")} | {"val/psnr_inf"}
    lines = validation.report_lines(["a/x.png", "b.png", "c.png"], scores, ratios)
    assert lines == ["a/x.png\t0.05\t0.25\t0.5\t10\t0.375", "a/x.png\t0.5\t0.5\t0.25\t20\t0.625", "c.png\t0.05\t0.75\t1\tinf\t0.125"]
    for line in lines:
        rel, ratio, *values = line.split("\t")
        assert len(values) == 4 and float(ratio) in ratios and all(float(v) == float(v) for v in values)


# ---- ModelCheckpoint(monitor=...) ------------------------------------------------------------------------------------
class FakeTrainer:
    def __init__(self, root):
        self.global_rank, self.current_epoch, self.global_step, self.log_dir, self.saved = 0, 0, 0, Path(root), []

    def save_checkpoint(self, path):
        self.saved.append((Path(path).name, self.current_epoch))


def run_epochs(checkpoint, values, key, tmp_path):
    trainer, module = FakeTrainer(tmp_path), SimpleNamespace(_logged={})
    for epoch, value in enumerate(values):
        trainer.current_epoch, trainer.global_step = epoch, 10 * (epoch + 1)
        if value is not None:
            module._logged[key] = value
        checkpoint.on_train_epoch_end(trainer, module)
    return [epoch for _, epoch in trainer.saved]


def test_model_checkpoint_monitor(tmp_path):
    from denoising_diffusion_deep_fake_amd.trainer import ModelCheckpoint
    best = lambda mode="min": ModelCheckpoint(filename="best", monitor="val/loss", mode=mode)  # noqa: E731
    assert run_epochs(best(), [0.5, 0.4, 0.45, 0.3, float("nan"), 0.31], "val/loss", tmp_path) == [0, 1, 3]
    assert run_epochs(best("max"), [0.5, 0.4, 0.6, 0.55], "val/loss", tmp_path) == [0, 2]
    assert run_epochs(best(), [torch.tensor(0.5), torch.tensor(0.6), torch.tensor(0.2)], "val/loss", tmp_path) == [0, 2]
    # the reference's monitor="epoch", mode="max", monitor=None, and a monitor nothing has logged: every epoch, as before
    assert run_epochs(ModelCheckpoint(save_top_k=8, monitor="epoch", mode="max"), [0.0, 1.0, 2.0], "epoch", tmp_path) == [0, 1, 2]
    assert run_epochs(ModelCheckpoint(), [0.5, 0.6, 0.7], "val/loss", tmp_path) == [0, 1, 2]
    assert run_epochs(best(), [None, None], "val/loss", tmp_path) == [0, 1]
    with pytest.raises(ValueError, match="mode"):
        ModelCheckpoint(monitor="val/loss", mode="smallest")
    assert "resume" in ModelCheckpoint.__doc__
    lit = denoiser(val_synthetic_length=6)
    kinds = [(c.filename, c.monitor, c.mode) for c in lit.configure_callbacks()]
    assert kinds == [(None, None, "min"), ("best", "val/loss", "min")]
    assert ("best", "val/loss", "min") in [(c.filename, getattr(c, "monitor", None), getattr(c, "mode", None))
                                            for c in deep_fake(val_synthetic_length=6).configure_callbacks()
                                            if isinstance(c, ModelCheckpoint)]


def test_trainer_passes_over_a_module_without_a_held_out_set():
    """_run_validation with val_dataloader() None: no eval / train flip, no step, no row"""
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    calls = []
    module = SimpleNamespace(val_dataloader=lambda: None, validation_step=lambda *a: calls.append("step"),
                             eval=lambda: calls.append("eval"), train=lambda: calls.append("train"), _logged={},
                             validation_logs_metrics_row=True)
    trainer = Trainer(enable_checkpointing=False)
    trainer._run_validation(module, "cpu")
    assert calls == [] and trainer._metric_rows == []
    module.val_dataloader = lambda: [{"x": 1}, {"x": 2}]
    module.validation_epoch_end = lambda outputs: module._logged.update({"val/loss": 0.25})
    trainer.global_step = 7
    trainer._run_validation(module, "cpu")
    assert calls == ["eval", "step", "step", "train"] and trainer._metric_rows == [(7, {"val/loss": 0.25})]


# ---- the shipped configs and documents -------------------------------------------------------------------------------
def test_shipped_configs_keep_validation_off_and_document_it():
    for rel, keys in (("train_denoiser/denoiser_config.yml", ("val_image_list_path",)),
                      ("train_deep_fake/denoise_config.yml", ("val_data_path_a", "val_data_path_b")),
                      ("train_deep_fake/swap_config.yml", ("val_data_path_a", "val_data_path_b"))):
        text = (PACKAGE / rel).read_text()
        config = yaml.safe_load(text)
        assert not any(k.startswith("val_") for k in config), rel
        for key in keys + ("val_noise_ratios", "val_report_path"):
            assert f"# {key}:" in text, (rel, key)
    root = PACKAGE.parent
    assert "Validation" in (root / "DESIGN.md").read_text() and "val_image_list_path" in (root / "INTEGRATION.md").read_text()
