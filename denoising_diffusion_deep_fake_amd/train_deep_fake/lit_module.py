"""`d3f.train_deep_fake.lit_module.LitModule` on the HIP hot path.

Mirrors d3f/train_deep_fake/lit_module.py:30-300: two U-Nets (`model_a`, `model_b`), two Adam
optimisers alternated by `optimizer_idx`, `mode: "denoise"` (noisy real -> real) or `mode: "swap"`
(EMA teacher of the OTHER domain renders a fake, the student denoises the noised fake back to the
real image), and the single-frame inference entry `predict_fake`.  Same hyper-parameter keys as
denoise_config.yml / swap_config.yml; extra optional keys: `synthetic`, `image_size`, `precision`, `augment`,
`pair_fused` (denoise mode: the two nets' optimizer steps of a batch as ONE set of kernel launches -- UnetPair; default on,
`false` = Lightning's one-after-the-other loop) and `pair_plan` (the sequential loop on the pair's kernel choices: the
bit-identical reference of the fused step).

Augmentation: the reference's `A.ShiftScaleRotate(shift_limit=0.2, scale_limit=0.1, rotate_limit=15, border_mode=0,
p=0.7)` after `A.Normalize` (lit_module.py:99-111) runs on the GPU here -- per-sample Bernoulli(0.7), the same
parameter ranges drawn with torch RNG, one HIP warp kernel (ops.affine_warp, K17) with a zero border in normalised
units -- inside `training_step`, before the noise blend, so that 8 GPUs are not fed by 8 CPU warps.
`augment: false` switches it off (benchmarks, parity tests).

`device_rng: true` (off by default; optional `rng_seed`): the noise, y and augmentation draws come from the counter-based
generator inside the kernels that consume them (rng.py, csrc/philox.h) -- a function of (seed, global_step, rank, domain:
stream 0 for a, 1 for b), so the fused two-network step equals the sequential loop whatever the order of the draws and a
resumed run continues the interrupted one.

`device_dataset: true` (off by default; optional `device_dataset_max_fraction`; not with `synthetic`): each domain's image
list is decoded once into a uint8 pool on the device (dataset/device_pool.py), the loaders yield indices and `domain_images`
gathers, normalises and augments a domain's batch in one launch -- the values of the `uint8_batches` path, bit for bit.

`balanced_sampling: true` (absent: off; not with `synthetic`): `data_path_a` and `data_path_b` are `--output_list`s of
`d3f balance`; in each domain every difficulty class that has an image is drawn with equal probability, then every image of
it, with replacement, N draws an epoch (dataset/balanced.py).  A BalancedSampler per domain on the host; with `device_dataset`
and `device_rng` the launch that assembles a domain's batch draws its indices too (ops.pool_batch_balanced_rng).

`val_data_path_a` and `val_data_path_b` (or `val_synthetic_length` with `synthetic`; absent: off; not with a world size above
1): held-out lists scored after every epoch at the fixed noise ratios `val_noise_ratios` -- model a on domain a, model b on
domain b, in both modes: per-image MSE, SSIM, PSNR and criterion value on the device, `val_a/...`, `val_b/...` and their mean
`val/...` in metrics.csv, `best.ckpt` by `val/loss`, optionally a per-image report (`val_report_path`).
helpers/validation.py states the contract.

Reference quirks kept on purpose: the dataloaders receive `mean_x` as BOTH
mean and std (lit_module.py:75-76); `predict_fake("a")` uses model_a with B's mean/std (:253-257);
de-normalisation truncates with `.int()` BEFORE clamping (:293-294).
"""
import math
import zlib
from datetime import timedelta

import numpy as np
import torch
import torch.nn as nn
import torch.optim.lr_scheduler as schedulers
from torch.utils.data import DataLoader

from .. import ops, rng
from ..dataset import balanced, device_pool
from ..dataset.device_pool import DeviceImagePool
from ..dataset.image_dataset import ImageDataset, NormalizeToTensor, SyntheticFaceDataset, ToUint8Tensor
from ..helpers import ImageLoggingMixin, ValidationMixin
from ..lightning import LightningModule
from ..loss_functions import MseStructuralSimilarityLoss
from ..optim import EMA, FusedAdam
from ..trainer import LearningRateMonitor, ModelCheckpoint
from ..unet import Unet, UnetPair


class ShiftScaleRotate(nn.Module):
    """albumentations.ShiftScaleRotate(shift_limit, scale_limit, rotate_limit, border_mode=0, p) on a normalised
    NCHW batch on the HIP device: with probability p per sample, rotate by U(-rotate, rotate) degrees and scale by
    U(1 - scale, 1 + scale) about the image centre, then shift by U(-shift, shift) x (width, height); bilinear,
    constant-zero border; the other samples pass through untouched."""

    def __init__(self, shift_limit=0.2, scale_limit=0.1, rotate_limit=15.0, p=0.7):
        super().__init__()
        self.shift_limit, self.scale_limit, self.rotate_limit, self.p = shift_limit, scale_limit, rotate_limit, p

    @staticmethod
    def theta(angle_deg, scale, dx, dy, height, width):
        """[B, 2, 3] affine_grid matrices (output -> input, normalised coordinates, align_corners=False) of
        cv2.warpAffine(img, M) with M = getRotationMatrix2D(centre, angle, scale) + (dx * width, dy * height):
        about the centre x - c = (W / 2) u, so  in - c = R(-angle) / scale * ((out - c) - shift)."""
        a = angle_deg * (math.pi / 180.0)
        cos, sin = torch.cos(a) / scale, torch.sin(a) / scale
        a11, a12, a21, a22 = cos, -sin * (height / width), sin * (width / height), cos
        t1 = -2.0 * (a11 * dx + a12 * dy)
        t2 = -2.0 * (a21 * dx + a22 * dy)
        return torch.stack([torch.stack([a11, a12, t1], 1), torch.stack([a21, a22, t2], 1)], 1)

    def draw(self, B, device):
        u = lambda lim: (torch.rand(B, device=device) * 2 - 1) * lim  # noqa: E731
        return {"apply": torch.rand(B, device=device) < self.p, "angle": u(self.rotate_limit),
                "scale": 1.0 + u(self.scale_limit), "dx": u(self.shift_limit), "dy": u(self.shift_limit)}

    KIND = "shift_scale_rotate"

    def rng_params(self):
        """the `params` of ops.affine_warp_rng / ops.pool_batch_rng"""
        return (self.shift_limit, self.scale_limit, self.rotate_limit, self.p)

    @torch.no_grad()
    def draw_theta(self, B, height, width, device, draws=None):
        """the torch draws of one batch, in their order -> (theta [B, 2, 3], apply [B] bool)"""
        d = self.draw(B, device) if draws is None else draws
        return self.theta(d["angle"], d["scale"], d["dx"], d["dy"], height, width), d["apply"]

    @torch.no_grad()
    def forward(self, x, draws=None, seed_offset=None):
        if seed_offset is not None:  # device_rng: (seed, offset) -- draws, theta, warp and pass-through in one kernel
            return ops.affine_warp_rng(x, seed_offset[0], seed_offset[1], self.KIND, self.rng_params())
        th, apply = self.draw_theta(x.shape[0], x.shape[2], x.shape[3], x.device, draws)
        warped = ops.affine_warp(x, th)
        return torch.where(apply.reshape(-1, 1, 1, 1), warped, x)


class LitModule(ValidationMixin, ImageLoggingMixin, LightningModule):
    # (domain, the key of its held-out list, RNG stream)
    VALIDATION_DOMAINS = (("a", "val_data_path_a", 2), ("b", "val_data_path_b", 3))

    def __init__(self, **kwargs):
        super().__init__()
        self.save_hyperparameters()
        device_pool.check_hparams(self.hparams, self.hparams.get("data_path_a"), self.hparams.get("data_path_b"))
        self.__dict__["_pools"] = {}  # device_dataset: the DeviceImagePool of domain "a" / "b", made by train_dataloader()
        balanced.check_hparams(self.hparams, self.hparams.get("data_path_a"), self.hparams.get("data_path_b"))
        self.__dict__["_balance_tables"] = {}  # balanced_sampling on the device: each pool's table, made with the pool
        self.setup_image_logging()  # image_logging_scheduler (:44); None unless `image_logging: true`
        self.setup_validation()     # held-out validation; off unless `val_...` lists are named (helpers/validation.py)
        self.augmentation = self.create_gpu_augmentation()
        self.model_a = self.create_model_instance()
        self.model_b = self.create_model_instance()
        if self.hparams.get("pair_plan", False):
            self.model_a.set_plan_nets(2)
            self.model_b.set_plan_nets(2)
        self.__dict__["_pair"] = None  # UnetPair(model_a, model_b), made on first use (not a sub-module: no state of its own)
        self.ema_model_a = self.create_ema_model(self.model_a)
        self.ema_model_b = self.create_ema_model(self.model_b)
        self.criterion = MseStructuralSimilarityLoss(-1.0, 1.0)

    def create_model_instance(self):
        p = self.hparams
        return Unet(
            encoder_name=p["encoder_name"],
            encoder_weights=None,
            in_channels=3,
            classes=3,
            activation=p.get("activation"),  # optional hparam (smp's names); saved with the checkpoint's hparams
            compute_dtype=p.get("precision", "f32"),
        )

    def create_ema_model(self, model):
        p = self.hparams
        if p.mode == "swap":
            return EMA(
                model,
                beta=p.ema_beta,
                update_every=p.ema_update_every,
                include_online_model=False,
            )
        return None

    def train_dataloader(self):
        p = self.hparams
        dataloader_a = self.create_dataloader(p.get("data_path_a"), p.mean_a, p.mean_a, domain="a")
        dataloader_b = self.create_dataloader(p.get("data_path_b"), p.mean_b, p.mean_b, domain="b")
        return {"a": dataloader_a, "b": dataloader_b}

    def create_dataloader(self, path, mean, std, domain=""):
        p = self.hparams
        if device_pool.check_hparams(p, path):  # the list decoded once into device memory, batches of indices
            if domain not in self._pools:
                self._pools[domain] = DeviceImagePool.from_hparams(p, path, self.device)
            pool, sampler = self._pools[domain], None
            if self.balanced_on_device():  # the launch draws: the loader gives the epoch its length and nothing else
                self._balance_tables[domain] = pool.balance_table()
            elif p.get("balanced_sampling", False):
                sampler = self.balanced_sampler(pool.classes, domain)
            return pool.loader(p.batch_size, shuffle=True, pin_memory=p.get("pin_memory", True), sampler=sampler)
        if p.get("synthetic", False) or path is None:
            # a stable, per-domain seed (str hashes are randomised per process; two None paths must still differ)
            seed = 1234 + zlib.crc32(f"{domain}:{path}".encode()) % 1000
            dataset = SyntheticFaceDataset(p.get("synthetic_length", 8 * p.batch_size), p.get("image_size", 256), seed=seed)
        else:
            dataset = ImageDataset(path, transform=self.create_augmentation_sequence(mean, std))
        workers = p.get("num_workers", 0)
        # shuffle=True and the ragged last batch kept, as the reference (lit_module.py:90-95); workers are SPAWNED:
        # forking a process that has initialised HIP is not safe
        extra = dict(multiprocessing_context="spawn", persistent_workers=True,
                     prefetch_factor=p.get("prefetch_factor", 2)) if workers > 0 else {}
        # pin_memory: the trainer's `.to(device, non_blocking=True)` is only asynchronous from page-locked memory
        order = dict(shuffle=True)
        if p.get("balanced_sampling", False):
            order = dict(sampler=self.balanced_sampler(dataset.image_class_list, domain))
        return DataLoader(dataset=dataset, batch_size=p.batch_size, num_workers=workers,
                          pin_memory=bool(p.get("pin_memory", True)) and torch.cuda.is_available(), **order, **extra)

    def balanced_on_device(self):
        """`balanced_sampling` where a domain's launch draws the indices: the pools with the device generator"""
        p = self.hparams
        return bool(p.get("balanced_sampling", False) and p.get("device_dataset", False) and p.get("device_rng", False))

    def balanced_sampler(self, classes, domain):
        """the host path's sampler of one domain (stream 0 for a, 1 for b); its seed is the device generator's (`rng_seed`,
        else the trainer's base seed, which a checkpoint carries), asked for when an epoch's draws are made"""
        if classes is None:
            raise ValueError("balanced_sampling: true needs the difficulty class of every image (the --output_list of "
                             "`d3f balance`)")
        return balanced.BalancedSampler(classes, seed=lambda: rng.module_stream(self)[0], stream="ab".index(domain))

    def create_augmentation_sequence(self, mean, std):
        # host half of the reference's A.Compose: Normalize + ToTensorV2; its ShiftScaleRotate(p=0.7) runs on the
        # GPU inside training_step (create_gpu_augmentation)
        # uint8_batches: true -- the workers hand over the decoded HWC uint8 image and Normalize + ToTensorV2 run on the
        # device too (ops.u8rgb_normalise, bit-identical): 4x fewer bytes through worker IPC and PCIe
        return ToUint8Tensor() if self.hparams.get("uint8_batches", False) else NormalizeToTensor(mean, std)

    def create_gpu_augmentation(self):
        if not self.hparams.get("augment", True):
            return None
        return ShiftScaleRotate(shift_limit=0.2, scale_limit=0.1, rotate_limit=15, p=0.7)

    def configure_optimizers(self):
        p = self.hparams
        b1, b2 = p.adam_b1, p.adam_b2
        tail = bool(p.get("optimizer_overlap_tail", False))  # FusedAdam docstring: part of the update inside backward
        optimizer_a = FusedAdam(self.model_a.parameters(), lr=p.learning_rate, betas=(b1, b2), module=self.model_a,
                                overlap_tail=tail)
        optimizer_b = FusedAdam(self.model_b.parameters(), lr=p.learning_rate, betas=(b1, b2), module=self.model_b,
                                overlap_tail=tail)
        scheduler_a = schedulers.CosineAnnealingLR(optimizer_a, T_max=p.cosine_scheduler_max_epoch)
        scheduler_b = schedulers.CosineAnnealingLR(optimizer_b, T_max=p.cosine_scheduler_max_epoch)
        return [optimizer_a, optimizer_b], [scheduler_a, scheduler_b]

    def optimizer_streams(self, device):
        """one HIP stream per optimizer when the two optimizer steps of a batch are independent of each other -- denoise
        mode: net a learns domain a, net b learns domain b, nothing is shared (d3f/train_deep_fake/lit_module.py:142-181)
        -- so that the trainer can overlap them (trainer.optimizer_steps).  Swap mode couples them through the EMA
        teachers (each step updates and runs the OTHER net's teacher, :183-206): sequential, None.
        OPT-IN (`concurrent_optimizers: true`): bit-identical to the sequential loop (tests/test_gpu_training.py) but
        measured 50 % SLOWER on MI355X / ROCm 7.0 (10.4 -> 15.5 ms per combined batch at bs 8 x 2, 256x256: four
        streams of MFMA-bound work -- two chains, two weight-gradient streams -- serve each other worse than two; the
        third-stream experiments of round 2 pointed the same way, profiles/README.md)."""
        if self.hparams.mode != "denoise" or not self.hparams.get("concurrent_optimizers", False):
            return None
        if self.__dict__.get("_opt_streams") is None:
            self.__dict__["_opt_streams"] = [torch.cuda.Stream(device=device) for _ in range(2)]
        return self.__dict__["_opt_streams"]

    def configure_callbacks(self):
        return [
            LearningRateMonitor(logging_interval="step"),
            ModelCheckpoint(save_top_k=8, monitor="epoch", mode="max", train_time_interval=timedelta(hours=2)),
            ModelCheckpoint(filename="last", save_on_train_epoch_end=True),
        ] + self.validation_callbacks()  # validation on: the best epoch's checkpoint by val/loss

    # ---- held-out validation (helpers/validation.py) -----------------------------------------------------------------
    def validation_model(self, domain):
        return self.model_a if domain == "a" else self.model_b

    def validation_transform(self, domain):
        mean = self.hparams[f"mean_{domain}"]
        return self.create_augmentation_sequence(mean, mean)  # the mean as std too, like train_dataloader

    @torch.no_grad()
    def validation_images(self, batch, domain):
        x, mean = batch["image"], self.hparams[f"mean_{domain}"]
        return ops.u8rgb_normalise(x, mean, mean) if x.dtype == torch.uint8 else x

    def training_step(self, batch, batch_idx, optimizer_idx):
        # the reference augments in the dataset; each image of a combined batch is consumed by exactly one of the two
        # optimiser steps (a by 0, b by 1), so preparing the half a step uses is the same thing
        if optimizer_idx == 0:
            batch_a = self.domain_images(batch, "a")
            self.update_image_logging_schedule()  # once per batch (:148)
            loss = self.training_step_for_one_model("a", batch_a, self.model_a, self.ema_model_b)
        if optimizer_idx == 1:
            batch_b = self.domain_images(batch, "b")
            loss = self.training_step_for_one_model("b", batch_b, self.model_b, self.ema_model_a)
        self.log("epoch", float(self.current_epoch))
        return loss

    @torch.no_grad()
    def domain_images(self, batch, key):
        """domain `key`'s part of a combined batch -> the normalised, augmented float batch its step trains on.  A
        `device_dataset` part carries `index` only: gather from the domain's pool, normalise and augment in ONE launch (the
        draws inside it under `device_rng`, otherwise ShiftScaleRotate's torch draws in their order, then the launch with
        their theta and apply).  Under `balanced_sampling` with `device_rng` the launch draws the images as well and `index` only
        says how many.  The mean is passed as std too, like train_dataloader / the reference :75-76."""
        p = self.hparams
        part, mean, stream, aug = batch[key], p[f"mean_{key}"], "ab".index(key), self.augmentation
        if "image" not in part:
            pool, index = self._pools[key], part["index"]
            if key in self._balance_tables:  # balanced_sampling: the indices are drawn inside the launch
                kind, params = (aug.KIND, aug.rng_params()) if aug is not None else ("none", None)
                return pool.batch_balanced_rng(self._balance_tables[key], index.shape[0], mean, mean,
                                               *rng.module_stream(self, stream), kind, params)[0]
            if aug is None:
                return pool.batch(index, mean, mean)
            if p.get("device_rng", False):
                return pool.batch_rng(index, mean, mean, *rng.module_stream(self, stream), aug.KIND, aug.rng_params())
            theta, apply = aug.draw_theta(index.shape[0], *pool.geometry, index.device)
            return pool.batch(index, mean, mean, theta=theta, apply=apply)
        x = part["image"]
        if x.dtype == torch.uint8:  # a `uint8_batches: true` loader
            x = ops.u8rgb_normalise(x, mean, mean)
        if aug is not None:
            x = self.augment(x, stream)
        return x

    def augment(self, x, stream):
        if self.hparams.get("device_rng", False):
            return self.augmentation(x, seed_offset=rng.module_stream(self, stream))
        return self.augmentation(x)

    # ---- the two optimizer steps of a denoise-mode batch as one set of launches ------------------------------------
    def pair_fused_active(self, batch=None, optimizers=None):
        """In `mode: "denoise"` optimizer 0 trains model_a on batch a and optimizer 1 trains model_b on batch b, nothing
        shared (d3f/train_deep_fake/lit_module.py:142-181): the trainer may run both steps as ONE forward / backward of a
        UnetPair (trainer.optimizer_steps).  Not in swap mode (each step updates and runs the OTHER net's EMA teacher,
        :183-206), not with `pair_fused: false`, not for a ragged batch pair, synchronised BatchNorm statistics or
        optimisers other than the two FusedAdam of configure_optimizers."""
        p = self.hparams
        if p.mode != "denoise" or p.get("pair_fused", None) is False or p.get("concurrent_optimizers", False):
            return False
        if optimizers is not None:
            if len(optimizers) != 2 or not all(isinstance(o, FusedAdam) for o in optimizers) or \
                    optimizers[0].module is not self.model_a or optimizers[1].module is not self.model_b:
                return False
        if batch is not None and "image" not in batch["a"]:  # device_dataset: equal B and equal pool geometry
            a, b = batch["a"]["index"], batch["b"]["index"]
            if a.shape != b.shape or a.device.type != "cuda" or self._pools["a"].geometry != self._pools["b"].geometry:
                return False
        elif batch is not None:
            a, b = batch["a"]["image"], batch["b"]["image"]
            if a.shape != b.shape or a.dtype != b.dtype or a.device.type != "cuda":
                return False
        if not (self.model_a.training and self.model_b.training):
            return False
        return not (self.model_a._rt.get("bn_sync") or self.model_b._rt.get("bn_sync"))

    def training_step_pair(self, batch, batch_idx):
        """training_step(batch, batch_idx, 0) and training_step(batch, batch_idx, 1) of a denoise-mode batch as one pass:
        the same preparation and the same random draws in the same order (a's augmentation and noise, then b's; with
        `device_rng` the same streams 0 / 1, whatever the order), ONE
        forward of UnetPair(model_a, model_b), the two losses.  Returns (loss_a, loss_b); the caller runs ONE backward,
        torch.autograd.backward([loss_a, loss_b]), then both optimizer steps."""
        self.update_image_logging_schedule()
        reals, noisy = [], []
        for stream, key in enumerate("ab"):
            x = self.domain_images(batch, key)
            with torch.no_grad():
                noisy.append(self.blend_random_amount_of_noise_with_each_sample(x, stream))
            reals.append(x)
        predictions = self._unet_pair()(noisy[0], noisy[1])
        losses = []
        for name, prediction, real, noisy_real in zip("ab", predictions, reals, noisy):
            loss = self.criterion(prediction, real)
            self.log_batch_as_image_grid(f"denoise_1_model_input/{name}", noisy_real)
            self.log_batch_as_image_grid(f"denoise_2_model_prediction/{name}", prediction)
            self.log(f"loss_denoise/train_{name}", loss)
            losses.append(loss)
        self.emit_image_grids()  # the four tags of the sequential loop, one launch
        self.log("epoch", float(self.current_epoch))
        return tuple(losses)

    def _unet_pair(self):
        """UnetPair(model_a, model_b), made on first use and made anew once either module was replaced (loading into a new
        module, say): a pair bound to the old modules would go on stepping them"""
        pair = self._pair
        if pair is None or pair.nets[0] is not self.model_a or pair.nets[1] is not self.model_b:
            pair = self.__dict__["_pair"] = UnetPair(self.model_a, self.model_b)
        return pair

    def training_step_for_one_model(self, name, real, real_model, fake_model):
        p = self.hparams
        if p.mode == "denoise":
            return self.training_denoise_step_for_one_model(name, real, real_model)
        elif p.mode == "swap":
            return self.training_swap_step_for_one_model(name, real, real_model, fake_model)
        raise ValueError(f"unknown mode {p.mode!r}")

    def training_denoise_step_for_one_model(self, name, real, real_model):
        with torch.no_grad():
            noisy_real = self.blend_random_amount_of_noise_with_each_sample(real, "ab".index(name))
        real_prediction = real_model(noisy_real)
        loss = self.criterion(real_prediction, real)
        self.log_batch_as_image_grid(f"denoise_1_model_input/{name}", noisy_real)
        self.log_batch_as_image_grid(f"denoise_2_model_prediction/{name}", real_prediction)
        self.emit_image_grids()
        self.log(f"loss_denoise/train_{name}", loss)
        return loss

    def training_swap_step_for_one_model(self, name, real, real_model, fake_model):
        fake_model.update()
        with torch.no_grad():
            fake = fake_model(real)  # train-mode BatchNorm: the EMA wrapper is a registered sub-module
            swap_diff = nn.functional.mse_loss(real, fake)
            noisy_fake = self.blend_random_amount_of_noise_with_each_sample(fake, "ab".index(name))
        real_prediction = real_model(noisy_fake)
        loss = self.criterion(real_prediction, real)
        self.log_batch_as_image_grid(f"swap_1_real/{name}", real)
        self.log_batch_as_image_grid(f"swap_2_fake/{name}_to_fake", fake)
        self.log_batch_as_image_grid(f"swap_3_model_input/{name}", noisy_fake)
        self.log_batch_as_image_grid(f"swap_4_model_prediction/{name}", real_prediction)
        self.emit_image_grids()
        self.log(f"swap_difference/{name}", swap_diff)
        self.log(f"loss_swap/train_{name}", loss)
        return loss

    @torch.no_grad()
    def blend_random_amount_of_noise_with_each_sample(self, batch, stream=0):
        """stream: the domain whose step this is (0: a, 1: b) -- names the draws of `device_rng`, otherwise unused"""
        p = self.hparams
        if p.get("device_rng", False):  # K12 as one kernel: the draws are a function of (seed, step, rank, domain)
            seed, offset = rng.module_stream(self, stream)
            return ops.noise_blend_rng(batch, seed, offset, p.noise_exponential_sampling_lambda)
        noise = torch.randn_like(batch)  # reference RNG order: randn_like first, then rand
        y = torch.rand(size=(batch.shape[0], 1, 1, 1), device=batch.device)
        return ops.noise_blend(batch, noise, y.reshape(-1), p.noise_exponential_sampling_lambda)

    # ---- single-frame inference (script_tools/put_video_through_fake_model.py:117) ----------------
    def predict_fake(self, real_bgr, model_a_or_b):
        p = self.hparams
        if model_a_or_b == "a":
            return self.predict_fake_for_single_frame(real_bgr, self.model_a, p.mean_b, p.std_b)
        if model_a_or_b == "b":
            return self.predict_fake_for_single_frame(real_bgr, self.model_b, p.mean_a, p.std_a)

    @torch.no_grad()
    def predict_fake_for_single_frame(self, real_bgr, model, mean, std):
        if not model.training and hasattr(model, "predict_u8"):
            # eval mode (script_tools/put_video_through_fake_model.py:49-52 calls .eval()): one C call with the
            # uint8 <-> normalised-tensor conversions fused in.  hipGraph replay (hparam `inference_graph`) is
            # available but off by default: at B=1 the ~100 kernels are GPU-bound (1.24 ms eager vs 1.31 ms
            # replayed at 448x448, profiles/README.md), the host stays ahead of the device either way.
            key = (tuple(real_bgr.shape), id(model))
            bufs = self._frame_buffers.get(key) if hasattr(self, "_frame_buffers") else None
            if bufs is None:
                if not hasattr(self, "_frame_buffers"):
                    self._frame_buffers = {}
                bufs = (torch.empty(real_bgr.shape, dtype=torch.uint8, device=self.device),
                        torch.empty((1,) + tuple(real_bgr.shape), dtype=torch.uint8, device=self.device))
                self._frame_buffers[key] = bufs
            bufs[0].copy_(torch.from_numpy(np.ascontiguousarray(real_bgr)))
            out = model.predict_u8(bufs[0], mean, std, graph=bool(self.hparams.get("inference_graph", False)),
                                   out=bufs[1])
            return out.cpu().numpy()
        mean = torch.tensor(mean, device=self.device, dtype=torch.float32)
        std = torch.tensor(std, device=self.device, dtype=torch.float32)
        input_tensor = self.cv2_to_tensor_normalised(real_bgr, mean, std)
        output_tensor = model(input_tensor)
        return self.tensor_cv2_to_denormalised(output_tensor, mean, std)

    # ---- raw frames to real|fake frames (script_tools/put_video_through_fake_model.py:111-119, 68) ----
    @torch.no_grad()
    def predict_fake_frames(self, raw_bgr_batch, model_a_or_b, width, height, antialias=False, temporal=None, boxes=None,
                            angles=None):
        """host frames [B, h, w, 3] (uint8 BGR, any size) -> host real|fake frames [B, height, 2 * width, 3]: centre crop,
        bicubic resize, `predict_fake` and the side-by-side concatenate of the reference's frame loop in one device call
        (`Unet.predict_frames_u8`).  Mean / std as in `predict_fake`: a model is fed the other domain's statistics.
        Pinned and device staging buffers are kept per shape, so a frame loop allocates nothing after its first batch.
        antialias=True: the antialiased bicubic resize (`ops.crop_resize_cubic_u8(..., antialias=True)`) -- prepare the
        training images the same way.  temporal: None, a strength or (strength, threshold), as `Unet.predict_frames_u8`: the
        fake half filtered against flicker; successive calls are then consecutive in time (`reset_frame_temporal` starts a
        new sequence).  boxes: None (the centre crop), one box or a box per frame [B][4], as `Unet.predict_frames_u8`.
        angles: None, or B angles in degrees next to a box per frame: the boxes turned about their centres."""
        model, mean, std, raw = self._frame_path_inputs(raw_bgr_batch, model_a_or_b, "predict_fake_frames")
        width, height = int(width), int(height)
        key = (raw.shape, id(model), width, height)
        if not hasattr(self, "_frames_buffers"):
            self._frames_buffers = {}
        bufs = self._frames_buffers.get(key)
        if bufs is None:
            pair = (raw.shape[0], height, 2 * width, 3)
            bufs = (torch.empty(raw.shape, dtype=torch.uint8).pin_memory(),
                    torch.empty(raw.shape, dtype=torch.uint8, device=self.device),
                    torch.empty(pair, dtype=torch.uint8, device=self.device),
                    torch.empty(pair, dtype=torch.uint8).pin_memory())
            self._frames_buffers[key] = bufs
        host_in, dev_in, dev_out, host_out = bufs
        host_in.copy_(torch.from_numpy(raw))
        dev_in.copy_(host_in, non_blocking=True)
        model.predict_frames_u8(dev_in, (height, width), mean, std, graph=bool(self.hparams.get("inference_graph", False)),
                                out=dev_out, antialias=antialias, temporal=temporal, boxes=boxes, angles=angles)
        host_out.copy_(dev_out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return host_out.numpy().copy()

    def reset_frame_temporal(self, model_a_or_b):
        """the next frame of `predict_fake_frames` / `predict_fake_frames_full` with `temporal=` on this model is a first
        frame again (`Unet.reset_frame_temporal`)"""
        if model_a_or_b not in ("a", "b"):
            raise ValueError("model_a_or_b is 'a' or 'b'")
        (self.model_a if model_a_or_b == "a" else self.model_b).reset_frame_temporal()

    def _frame_path_inputs(self, raw_bgr_batch, model_a_or_b, who):
        """what a raw-frame entry needs before it touches the device: the model with the OTHER domain's mean / std (as
        `predict_fake`), in eval mode, and the frames as one contiguous uint8 [B, h, w, 3] array"""
        p = self.hparams
        if model_a_or_b == "a":
            model, mean, std = self.model_a, p.mean_b, p.std_b
        elif model_a_or_b == "b":
            model, mean, std = self.model_b, p.mean_a, p.std_a
        else:
            raise ValueError("model_a_or_b is 'a' or 'b'")
        if model.training:
            raise RuntimeError(f"{who} is the eval-mode frame path: call .eval() first")
        raw = np.ascontiguousarray(raw_bgr_batch)
        if raw.dtype != np.uint8 or raw.ndim != 4 or raw.shape[-1] != 3:
            raise ValueError(f"{who} expects uint8 frames [B, h, w, 3] in BGR order")
        return model, mean, std, raw

    def _staging(self, cache, key, shape):
        """a pinned host buffer and a device buffer of `shape`, kept in the dict `cache` under `key`"""
        bufs = cache.get(key)
        if bufs is None:
            bufs = cache[key] = (torch.empty(shape, dtype=torch.uint8).pin_memory(),
                                 torch.empty(shape, dtype=torch.uint8, device=self.device))
        return bufs

    @torch.no_grad()
    def predict_fake_frames_full(self, raw_bgr_batch, model_a_or_b, width, height, feather=None, with_pair=False,
                                 antialias=False, color_match=None, temporal=None, boxes=None, blend=None,
                                 blend_levels=None, angles=None):
        """host frames [B, h, w, 3] (uint8 BGR, any size) -> host frames of the same shape with the centre-crop box replaced
        by the fake, resized back to the box and blended in over `feather` source pixels (None: `ops.default_feather`):
        the swapped video at the source's size, in one device call (`Unet.predict_frames_full_u8`).  with_pair: returns
        (full, pair), pair being what `predict_fake_frames` returns.  Models and statistics as `predict_fake_frames`;
        pinned and device staging is kept per shape in a cache of its own.  antialias: as `predict_fake_frames` (the
        crop-to-network resize only).  color_match: None / "none" / "meanstd", as `Unet.predict_frames_full_u8`: the fake's
        colour statistics matched to the crop it replaces before the paste; the pair is the same either way.  temporal: as
        `predict_fake_frames`; the pair then holds the filtered fake, and with color_match the coefficients are smoothed.
        boxes: as `predict_fake_frames`; every frame's fake goes back into its own box (`Unet.predict_frames_full_u8`).
        blend, blend_levels: as `Unet.predict_frames_full_u8` -- "multiband" fades each frequency band over its own ramp.
        angles: as `predict_fake_frames`; every frame's fake goes back into its own rotated rectangle."""
        model, mean, std, raw = self._frame_path_inputs(raw_bgr_batch, model_a_or_b, "predict_fake_frames_full")
        width, height = int(width), int(height)
        if not hasattr(self, "_frames_full_buffers"):
            self._frames_full_buffers = {}
        cache, key = self._frames_full_buffers, (raw.shape, id(model), width, height)
        host_in, dev_in = self._staging(cache, key + ("in",), raw.shape)
        host_full, dev_full = self._staging(cache, key + ("full",), raw.shape)
        host_pair, dev_pair = self._staging(cache, key + ("pair",), (raw.shape[0], height, 2 * width, 3))
        host_in.copy_(torch.from_numpy(raw))
        dev_in.copy_(host_in, non_blocking=True)
        model.predict_frames_full_u8(dev_in, (height, width), mean, std, feather=feather,
                                     graph=bool(self.hparams.get("inference_graph", False)), out=dev_full,
                                     pair_out=dev_pair, antialias=antialias, color_match=color_match,
                                     temporal=temporal, boxes=boxes, blend=blend, blend_levels=blend_levels, angles=angles)
        host_full.copy_(dev_full, non_blocking=True)
        if with_pair:
            host_pair.copy_(dev_pair, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if with_pair:
            return host_full.numpy().copy(), host_pair.numpy().copy()
        return host_full.numpy().copy()

    def cv2_to_tensor_normalised(self, image_bgr, mean, std):
        image_rgb = np.ascontiguousarray(image_bgr[:, :, ::-1])  # cv2.COLOR_BGR2RGB
        tensor = torch.from_numpy(image_rgb).float().to(self.device)
        tensor = tensor.permute(2, 0, 1)  # hwc to chw
        tensor = tensor - mean.reshape(3, 1, 1) * 255
        tensor = tensor / (std.reshape(3, 1, 1) * 255)
        return tensor.unsqueeze(0).contiguous()

    def tensor_cv2_to_denormalised(self, tensor, mean, std):
        tensor = tensor.squeeze(0)
        tensor = tensor * (std.reshape(3, 1, 1) * 255)
        tensor = tensor + mean.reshape(3, 1, 1) * 255
        tensor = tensor.permute(1, 2, 0)  # chw to hwc
        tensor = tensor.int()
        tensor = tensor.clamp(0, 255)
        image_rgb = tensor.cpu().numpy().astype(np.uint8)
        return np.ascontiguousarray(image_rgb[:, :, ::-1])  # cv2.COLOR_RGB2BGR
