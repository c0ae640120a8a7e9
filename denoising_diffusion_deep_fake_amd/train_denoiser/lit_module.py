"""`d3f.train_denoiser.lit_module.LitModule` on the HIP hot path.

Mirrors d3f/train_denoiser/lit_module.py:28-153 -- same hyper-parameter keys
(denoiser_config.yml), same method names, same training_step data flow:
    image -> (affine augmentation) -> blend noise -> self.model(image_noisy) -> criterion(pred, image)
with the U-Net, the loss, the noise blend and the optimiser running as HIP kernels.
Differences, all outside the parity-checked arithmetic:
  * the reference's dataloader transform is bit-rotted (nn.Sequential(T.Normalize) called with
    image=...); this module uses the train_deep_fake convention (Normalize + ToTensor) so the
    command actually runs; `synthetic: true` swaps in the synthetic face-crop dataset;
  * kornia's RandomAffine is replaced by the same parameter ranges drawn with torch RNG and one HIP warp
    kernel (ops.affine_warp = affine_grid + grid_sample(bilinear, zeros), parity-tested against torch on CPU);
    the random draws themselves are not part of the numerics contract; off in benchmarks (`augment: false`);
  * `image_logging: true` (absent: off; not together with `graph_step`): the `image` / `image_noisy` /
    `image_prediction` grids of :121-123 as PNG files (helpers/image_grid_logger.py), one HIP kernel per logging step;
  * `device_rng: true` (off by default; optional `rng_seed`): the noise, y and augmentation draws come from the
    counter-based generator inside the kernels that consume them (rng.py, csrc/philox.h) -- a function of (seed,
    global_step, rank), so a resumed run continues the interrupted one.  Not together with `graph_step`.
  * `device_dataset: true` (off by default; optional `device_dataset_max_fraction`; not with `synthetic`): the image list is
    decoded once into a uint8 pool on the device (dataset/device_pool.py), the loader yields indices and `step_images`
    gathers, normalises and augments the batch in one launch -- the values of the `uint8_batches` path, bit for bit.
  * `balanced_sampling: true` (absent: off; not with `synthetic`): `input_image_list_path` is the `--output_list` of
    `d3f balance`; every difficulty class that has an image is drawn with equal probability, then every image of it, with
    replacement, N draws an epoch (dataset/balanced.py).  A BalancedSampler on the host; with `device_dataset` and
    `device_rng` the launch that assembles the batch draws the indices too (ops.pool_batch_balanced_rng).
  * `val_image_list_path` (or `val_synthetic_length` with `synthetic`; absent: off; not with `graph_step` or a world size
    above 1): a held-out list scored after every epoch at the fixed noise ratios `val_noise_ratios` -- per-image MSE, SSIM,
    PSNR and criterion value on the device, `val/...` keys in metrics.csv, `best.ckpt` by `val/loss`, optionally a per-image
    report (`val_report_path`).  helpers/validation.py states the contract.
"""
import math

import torch
import torch.optim.lr_scheduler as schedulers
from torch.utils.data import DataLoader

from .. import ops, rng
from ..dataset import balanced, device_pool
from ..dataset.device_pool import DeviceImagePool
from ..dataset.image_dataset import ImageDataset, NormalizeToTensor, SyntheticFaceDataset, ToUint8Tensor
from ..helpers import ImageLoggingMixin, ValidationMixin
from ..lightning import LightningModule
from ..loss_functions import MseStructuralSimilarityLoss
from ..optim import FusedAdam
from ..unet import Unet


class RandomAffine(torch.nn.Module):
    """per-sample rotation U(-deg,deg), translation U(-t,t)*size, isotropic scale U(s0,s1); bilinear,
    zero padding (kornia RandomAffine(degrees=15, translate=[.2,.2], scale=[.8,1.2], p=1) stand-in)."""

    def __init__(self, degrees=15.0, translate=(0.2, 0.2), scale=(0.8, 1.2)):
        super().__init__()
        self.degrees, self.translate, self.scale = degrees, translate, scale

    KIND = "random_affine"

    def rng_params(self):
        """the `params` of ops.affine_warp_rng / ops.pool_batch_rng"""
        return (self.degrees, self.translate[0], self.translate[1], self.scale[0], self.scale[1])

    def forward(self, x, seed_offset=None):
        if seed_offset is not None:  # device_rng: (seed, offset) -- the draws and theta happen inside the warp kernel
            return ops.affine_warp_rng(x, seed_offset[0], seed_offset[1], self.KIND, self.rng_params())
        return ops.affine_warp(x, self.draw_theta(x.shape[0], x.device))  # K17: affine_grid + grid_sample in one HIP kernel

    def draw_theta(self, B, dev):
        """the torch draws of one batch, in their order, and the [B, 2, 3] theta they give"""
        ang = (torch.rand(B, device=dev) * 2 - 1) * math.radians(self.degrees)
        sc = torch.rand(B, device=dev) * (self.scale[1] - self.scale[0]) + self.scale[0]
        tx = (torch.rand(B, device=dev) * 2 - 1) * self.translate[0] * 2
        ty = (torch.rand(B, device=dev) * 2 - 1) * self.translate[1] * 2
        cos, sin = torch.cos(ang) / sc, torch.sin(ang) / sc
        return torch.stack([torch.stack([cos, -sin, tx], 1), torch.stack([sin, cos, ty], 1)], 1)


class LitModule(ValidationMixin, ImageLoggingMixin, LightningModule):
    VALIDATION_DOMAINS = (("", "val_image_list_path", 2),)  # (domain, the key of its held-out list, RNG stream)

    def __init__(self, **kwargs):
        super().__init__()
        self.save_hyperparameters()
        device_pool.check_hparams(self.hparams, self.hparams.get("input_image_list_path"))
        self.__dict__["_pool"] = None  # device_dataset: the DeviceImagePool, made by train_dataloader()
        balanced.check_hparams(self.hparams, self.hparams.get("input_image_list_path"))  # refusals: now, on the host
        self.__dict__["_balance_table"] = None  # balanced_sampling on the device: the pool's table, made with the pool
        self.setup_image_logging()  # image_logging_scheduler; None unless `image_logging: true` (not with graph_step)
        self.setup_validation()     # held-out validation; off unless a `val_...` list is named (helpers/validation.py)
        self.model = self.create_model_instance()
        self.training_criterion = MseStructuralSimilarityLoss(-1.0, 1.0)
        self.shared_augmentation_sequence = self.create_shared_augmentation_sequence()
        # graph_step: true -- the whole optimiser step as one captured hipGraph (graph_step.py).  Lightning's MANUAL
        # optimisation contract: training_step does its own backward and optimiser step, the trainer only calls it.
        # Single GPU only.  Measured on ROCm 7.0 / MI355X (profiles/README.md, round 3): bit-identical and SLOWER than the
        # eager step (the replay of a graph spanning the engine's three streams costs ~30 us per node), so it is off
        # unless asked for.
        rng.refuse_graph_step(self.hparams)
        self.automatic_optimization = not self.hparams.get("graph_step", False)
        self.__dict__["_graph_step"] = None

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

    def create_shared_augmentation_sequence(self):
        return RandomAffine(degrees=15, translate=[0.2, 0.2], scale=[0.8, 1.2])

    def train_dataloader(self):
        p = self.hparams
        return self.create_dataloader(p.get("input_image_list_path"), p.get("mean"), p.get("std"))

    def create_dataloader(self, path, mean, std):
        p = self.hparams
        if device_pool.check_hparams(p, path):  # the list decoded once into device memory, batches of indices
            if self._pool is None:
                self.__dict__["_pool"] = DeviceImagePool.from_hparams(p, path, self.device)
            sampler = None
            if self.balanced_on_device():  # the launch draws: the loader gives the epoch its length and nothing else
                self.__dict__["_balance_table"] = self._pool.balance_table()
            elif p.get("balanced_sampling", False):
                sampler = self.balanced_sampler(self._pool.classes)
            return self._pool.loader(p.batch_size, shuffle=True, pin_memory=p.get("pin_memory", True), sampler=sampler)
        if p.get("synthetic", False) or path is None:
            dataset = SyntheticFaceDataset(p.get("synthetic_length", 64 * p.batch_size), p.get("image_size", 256))
        else:
            # config means/stds are in 0..255 units (denoiser_config.yml:10-11) -> [0,1] units here
            m, s = self.mean_std_unit()
            # uint8_batches: true -- the workers hand over the decoded HWC uint8 image, Normalize + ToTensor run on the
            # device in training_step (normalise_on_device; bit-identical, 4x fewer bytes through IPC and PCIe)
            dataset = ImageDataset(path, transform=ToUint8Tensor() if p.get("uint8_batches", False) else NormalizeToTensor(m, s))
        workers = p.get("num_workers", 0)
        # shuffle=True, ragged last batch kept (d3f/train_denoiser/lit_module.py:78-86); workers are SPAWNED: forking
        # a process that has initialised HIP is not safe
        extra = dict(multiprocessing_context="spawn", persistent_workers=True,
                     prefetch_factor=p.get("prefetch_factor", 2)) if workers > 0 else {}
        # pin_memory: the trainer's `.to(device, non_blocking=True)` is only asynchronous from page-locked memory
        order = dict(shuffle=True)
        if p.get("balanced_sampling", False):
            order = dict(sampler=self.balanced_sampler(dataset.image_class_list))
        return DataLoader(dataset=dataset, batch_size=p.batch_size, num_workers=workers,
                          pin_memory=bool(p.get("pin_memory", True)) and torch.cuda.is_available(), **order, **extra)

    # ---- held-out validation (helpers/validation.py) -----------------------------------------------------------------
    def validation_model(self, domain):
        return self.model

    def validation_transform(self, domain):
        m, s = self.mean_std_unit()
        return ToUint8Tensor() if self.hparams.get("uint8_batches", False) else NormalizeToTensor(m, s)

    @torch.no_grad()
    def validation_images(self, batch, domain):
        image = batch["image"]
        return self.normalise_on_device(image) if image.dtype == torch.uint8 else image

    def configure_callbacks(self):
        """nothing without validation (the Trainer then adds its checkpoint per epoch, as ever); with it that checkpoint
        and the best epoch's"""
        from ..trainer import ModelCheckpoint
        best = self.validation_callbacks()
        return [ModelCheckpoint()] + best if best else []

    def balanced_on_device(self):
        """`balanced_sampling` where the batch's launch draws the indices: the pool with the device generator"""
        p = self.hparams
        return bool(p.get("balanced_sampling", False) and p.get("device_dataset", False) and p.get("device_rng", False))

    def balanced_sampler(self, classes):
        """the host path's sampler; its seed is the device generator's (`rng_seed`, else the trainer's base seed, which a
        checkpoint carries), asked for when an epoch's draws are made"""
        if classes is None:
            raise ValueError("balanced_sampling: true needs the difficulty class of every image (the --output_list of "
                             "`d3f balance`)")
        return balanced.BalancedSampler(classes, seed=lambda: rng.module_stream(self)[0])

    def mean_std_unit(self):
        """config means / stds are in 0..255 units (denoiser_config.yml:10-11) -> [0, 1] units"""
        p = self.hparams
        mean, std = p.get("mean"), p.get("std")
        return ([v / 255.0 if max(mean) > 1 else v for v in mean], [v / 255.0 if max(std) > 1 else v for v in std])

    @torch.no_grad()
    def normalise_on_device(self, frames_u8):
        """[B, H, W, 3] uint8 RGB batch of a `uint8_batches: true` loader -> the normalised NCHW float batch the host
        transform would have produced (bit-identical)"""
        m, s = self.mean_std_unit()
        return ops.u8rgb_normalise(frames_u8, m, s)

    @torch.no_grad()
    def step_images(self, batch):
        """a loader's batch -> the normalised, augmented float batch the step trains on.  A `device_dataset` batch carries
        `index` only: gather from the pool, normalise and augment in ONE launch (the draws inside it under `device_rng`,
        otherwise RandomAffine's torch draws in their order, then the launch with their theta).  Under `balanced_sampling`
        with `device_rng` the launch draws the images as well and `index` only says how many."""
        p = self.hparams
        augment, aug = p.get("augment", True), self.shared_augmentation_sequence
        if "image" not in batch:
            index = batch["index"]
            m, s = self.mean_std_unit()
            if self._balance_table is not None:  # balanced_sampling: the indices are drawn inside the launch
                kind, params = (aug.KIND, aug.rng_params()) if augment else ("none", None)
                return self._pool.batch_balanced_rng(self._balance_table, index.shape[0], m, s, *rng.module_stream(self),
                                                     kind, params)[0]
            if not augment:
                return self._pool.batch(index, m, s)
            if p.get("device_rng", False):
                return self._pool.batch_rng(index, m, s, *rng.module_stream(self), aug.KIND, aug.rng_params())
            return self._pool.batch(index, m, s, theta=aug.draw_theta(index.shape[0], index.device))
        image = batch["image"]
        if image.dtype == torch.uint8:
            image = self.normalise_on_device(image)
        if augment:
            image = aug(image, rng.module_stream(self)) if p.get("device_rng", False) else aug(image)
        return image

    def configure_optimizers(self):
        p = self.hparams
        # optimizer_overlap_tail: true -- the update of layer3 / layer4 / decoder / head runs inside backward next to the
        # last gradient bucket (FusedAdam docstring: one step() per backward(); bit-identical values)
        optimizer = FusedAdam(self.model.parameters(), lr=p.learning_rate, module=self.model,
                              overlap_tail=bool(p.get("optimizer_overlap_tail", False)))
        scheduler = schedulers.CosineAnnealingLR(optimizer, T_max=p.cosine_scheduler_max_epoch)
        return [optimizer], [scheduler]

    def forward(self, image):
        return self.model(image)

    def training_step(self, batch, batch_idx):
        self.update_image_logging_schedule()
        image = self.step_images(batch)
        if not self.automatic_optimization:
            if self._graph_step is None:
                from ..graph_step import GraphTrainStep
                opt = self.optimizers()
                self.__dict__["_graph_step"] = GraphTrainStep(self.model, opt, self.hparams.noise_exponential_sampling_lambda,
                                                              self.training_criterion.input_min_value,
                                                              self.training_criterion.input_max_value)
            loss = self._graph_step(image)
            self.log("loss", loss)
            return loss
        image_noisy = self.blend_random_amount_of_noise_with_each_sample(image)
        image_prediction = self.model(image_noisy)
        loss = self.training_criterion(image_prediction, image)
        self.log_batch_as_image_grid("image", image)
        self.log_batch_as_image_grid("image_noisy", image_noisy)
        self.log_batch_as_image_grid("image_prediction", image_prediction)
        self.emit_image_grids()
        self.log("loss", loss)
        return loss

    @torch.no_grad()
    def blend_random_amount_of_noise_with_each_sample(self, batch):
        p = self.hparams
        if p.get("device_rng", False):  # K12 as one kernel: the step's draws are a function of (seed, step, rank)
            seed, offset = rng.module_stream(self)
            return ops.noise_blend_rng(batch, seed, offset, p.noise_exponential_sampling_lambda)
        # RNG call order of the reference: randn_like(batch) first, then rand(B,1,1,1)
        noise = torch.randn_like(batch)
        y = torch.rand(size=(batch.shape[0], 1, 1, 1), device=batch.device)
        return ops.noise_blend(batch, noise, y.reshape(-1), p.noise_exponential_sampling_lambda)

    def sample_random_number_from_exponential_distribution(self, batch_size, lam):
        y = torch.rand(size=(batch_size, 1, 1, 1), device=self.device)
        zeros = torch.zeros(batch_size, 4, device=self.device)
        _, r = ops.noise_blend(zeros, zeros, y.reshape(-1), lam, return_r=True)
        return r.reshape(batch_size, 1, 1, 1)
