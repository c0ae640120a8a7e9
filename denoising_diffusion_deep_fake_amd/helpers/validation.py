"""Held-out validation of the two trainers (`train_denoiser`, `train_deep_fake`): per-image MSE, SSIM, PSNR and criterion
value of the eval-mode prediction at a few FIXED noise ratios, scored on the device.

The training loss is measured on augmented images at a random noise level per image, so two of its values are not
comparable.  Here every held-out image meets the same noise every epoch: the normals come from the counter-based
generator (csrc/philox.h) with the image's index in the held-out dataset as the counter's image word
(ops.noise_blend_fixed_index_rng), whatever `device_rng` says, so torch's generators are never advanced and the batch size
does not matter.  The scores (ops.quality_per_image, csrc/quality.hip) are scattered into one [K ratios][4][N images]
device buffer per domain at the batch's `index`; a validation step neither copies nor waits.  validation_epoch_end makes
ONE device-to-host copy and takes float64 means on the host.

Hyper-parameters (all optional; absent = off, and then no launch, loader, file or log key differs; saved with the
checkpoint like every other key):
  val_image_list_path                the held-out list of train_denoiser
  val_data_path_a, val_data_path_b   the held-out lists of train_deep_fake (both or neither)
  val_synthetic_length: n            with `synthetic: true`: a SyntheticFaceDataset of n images per domain whose seeds are
                                     disjoint from the training set's
  val_noise_ratios                   default [0.05, 0.2, 0.5]; 1 to 16 entries, each in (0, 1)
  val_report_path                    "<relative path>\\t<ratio>\\t<mse>\\t<ssim>\\t<psnr>\\t<loss>" per image and ratio,
                                     rewritten every epoch
Refused at construction (ValueError naming the key): a world size above 1 (sharded validation is not built) and
`graph_step: true`.

Logged at the end of every epoch (`<p>` = "val" for the denoiser, "val_a" / "val_b" for the deep-fake trainer's domains):
  <p>/loss, <p>/mse, <p>/ssim, <p>/psnr      means over the scored images and the ratios; an infinite PSNR (a perfect
                                             prediction) is left out of the PSNR mean and counted in <p>/psnr_inf
  <p>/loss_r<ratio> (and mse, ssim, psnr)    the same per ratio, <ratio> formatted with %g
The deep-fake trainer scores model a on domain a and model b on domain b, in both modes, one network after the other (the
pair entry is not used), and logs val/loss, val/mse, val/ssim, val/psnr as the means of the two domains' values and
val/psnr_inf as their sum.  With validation on, configure_callbacks adds ModelCheckpoint(filename="best",
monitor="val/loss", mode="min").

RNG streams (rng.py): offset = pack_offset(k, 0, stream), k the ratio's position, stream 2 for the denoiser / domain a and 3
for domain b; the seed is the module's (`rng_seed`, else the trainer's base seed).
"""
import math
import os
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import distributed, ops, rng
from ..dataset.image_dataset import ImageDataset, SyntheticFaceDataset

DEFAULT_NOISE_RATIOS = (0.05, 0.2, 0.5)
MAX_NOISE_RATIOS = 16
METRICS = ops.QUALITY_ROWS  # ("mse", "ssim", "psnr", "loss"): the rows of the score buffer
SYNTHETIC_SEED_BASE = 1 << 30  # held-out synthetic images: seeds from here (+ stream << 20); the training sets' start near 1234


def check_noise_ratios(ratios):
    """`val_noise_ratios` as a tuple of floats, or ValueError"""
    if ratios is None:
        return DEFAULT_NOISE_RATIOS
    if isinstance(ratios, (str, bytes)) or not hasattr(ratios, "__iter__"):
        raise ValueError(f"val_noise_ratios must be a list of numbers in (0, 1), not {ratios!r}")
    ratios = list(ratios)
    if not 1 <= len(ratios) <= MAX_NOISE_RATIOS:
        raise ValueError(f"val_noise_ratios holds {len(ratios)} entries: 1 to {MAX_NOISE_RATIOS} are allowed")
    for r in ratios:
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0.0 < float(r) < 1.0:
            raise ValueError(f"val_noise_ratios: every entry must be a number in (0, 1), not {r!r}")
    return tuple(float(r) for r in ratios)


def summarise(scores, ratios, prefix):
    """scores: [K, 4, N] (rows METRICS; NaN in row `mse` = not scored) -> {key: float}, float64 means over the scored
    entries.  An infinite PSNR is left out of the PSNR means; `<prefix>/psnr_inf` counts them (all ratios)."""
    scores = np.asarray(scores, dtype=np.float64)
    scored = ~np.isnan(scores[:, 0, :])
    out = {}

    def mean(values):
        return float(values.mean()) if values.size else float("nan")

    for m, name in enumerate(METRICS):
        rows = scores[:, m, :]
        keep = scored & np.isfinite(rows) if name == "psnr" else scored
        out[f"{prefix}/{name}"] = mean(rows[keep])
        for k, ratio in enumerate(ratios):
            out[f"{prefix}/{name}_r{ratio:g}"] = mean(rows[k][keep[k]])
    out[f"{prefix}/psnr_inf"] = float((scored & np.isinf(scores[:, METRICS.index("psnr"), :])).sum())
    return out


def report_lines(names, scores, ratios):
    """the lines of `val_report_path` for one domain: every scored image at every ratio, in the dataset's order"""
    scores = np.asarray(scores, dtype=np.float64)
    lines = []
    for n, name in enumerate(names):
        for k, ratio in enumerate(ratios):
            mse, ssim, psnr, loss = scores[k, :, n]
            if not math.isnan(mse):
                lines.append(f"{name}\t{ratio:g}\t{mse:.9g}\t{ssim:.9g}\t{psnr:.9g}\t{loss:.9g}")
    return lines


class DomainBatches:
    """the held-out loaders of several domains, one after the other; every batch says which `domain` it belongs to"""

    def __init__(self, loaders):
        self.loaders = loaders

    def __len__(self):
        return sum(len(loader) for loader in self.loaders.values())

    def __iter__(self):
        for domain, loader in self.loaders.items():
            for batch in loader:
                yield dict(batch, domain=domain)


class ValidationMixin:
    """The validation surface train_denoiser.LitModule and train_deep_fake.LitModule share.  The module names its domains
    in VALIDATION_DOMAINS -- (domain, hyper-parameter holding its list, RNG stream) -- calls setup_validation() in
    __init__, and provides validation_model(domain), validation_transform(domain) (the host transform of a held-out
    ImageDataset) and validation_images(batch, domain) (a loader's batch -> the normalised float batch)."""

    VALIDATION_DOMAINS = ()
    validation_logs_metrics_row = True  # the Trainer appends a metrics row after a validation that logged something

    # ---- construction ----------------------------------------------------------------------------------------------
    def setup_validation(self):
        p = self.hparams
        ratios = check_noise_ratios(p.get("val_noise_ratios"))
        path_keys = [key for _, key, _ in self.VALIDATION_DOMAINS]
        given = [key for key in path_keys if p.get(key) is not None]
        synthetic = p.get("val_synthetic_length") is not None
        if given and len(given) != len(path_keys):
            missing = [key for key in path_keys if key not in given]
            raise ValueError(f"{given[0]} is set and {missing[0]} is not: the held-out lists come together")
        if synthetic:
            if not p.get("synthetic", False):
                raise ValueError("val_synthetic_length validates on synthetic images: it needs synthetic: true")
            if isinstance(p["val_synthetic_length"], bool) or not isinstance(p["val_synthetic_length"], int) or \
                    p["val_synthetic_length"] < 1:
                raise ValueError(f"val_synthetic_length must be a positive integer, not {p['val_synthetic_length']!r}")
            if given:
                raise ValueError(f"val_synthetic_length and {given[0]} both name a held-out set: choose one")
        on = bool(given) or synthetic
        key = given[0] if given else "val_synthetic_length"
        if on and distributed.env_world()[0] > 1:
            raise ValueError(f"{key}: held-out validation scores the whole list in one process: it cannot be combined with a "
                             f"world size above 1 (WORLD_SIZE={distributed.env_world()[0]}); sharded validation is not built")
        if on and p.get("graph_step", False):
            raise ValueError(f"{key}: held-out validation cannot be combined with graph_step: true: the captured whole-step "
                             f"entry (d3f_unet_train_step) leaves no eval-mode forward to score")
        self.__dict__["_val"] = dict(on=on, ratios=ratios, datasets=None, flat=None, buffers=None)

    def validation_on(self):
        return self._val["on"]

    def validation_callbacks(self):
        """what configure_callbacks adds when validation is on: the checkpoint of the best epoch so far"""
        from ..trainer import ModelCheckpoint
        return [ModelCheckpoint(filename="best", monitor="val/loss", mode="min")] if self.validation_on() else []

    # ---- data ------------------------------------------------------------------------------------------------------
    def validation_datasets(self):
        """{domain: dataset}, made once: the held-out ImageDataset, or the synthetic one"""
        state, p = self._val, self.hparams
        if state["datasets"] is None:
            datasets = {}
            for domain, key, stream in self.VALIDATION_DOMAINS:
                if p.get("val_synthetic_length") is not None:
                    datasets[domain] = SyntheticFaceDataset(int(p["val_synthetic_length"]), p.get("image_size", 256),
                                                            seed=SYNTHETIC_SEED_BASE + (stream << 20))
                else:
                    datasets[domain] = ImageDataset(p[key], transform=self.validation_transform(domain))
            state["datasets"] = datasets
        return state["datasets"]

    def val_dataloader(self):
        """None without validation keys.  Otherwise the host loader over the held-out set in the list's order (no shuffle,
        no augmentation, the ragged last batch kept; `uint8_batches` and `num_workers` as the training loader, workers
        spawned), for several domains one after the other.  The loaders own a generator, so that making their iterators
        draws nothing from torch's global one."""
        if not self.validation_on():
            return None
        p = self.hparams
        workers = p.get("num_workers", 0)
        extra = dict(multiprocessing_context="spawn", persistent_workers=False,
                     prefetch_factor=p.get("prefetch_factor", 2)) if workers > 0 else {}
        loaders = {}
        for domain, dataset in self.validation_datasets().items():
            loaders[domain] = DataLoader(dataset=dataset, batch_size=p.batch_size, shuffle=False, drop_last=False,
                                         num_workers=workers, generator=torch.Generator().manual_seed(0),
                                         pin_memory=bool(p.get("pin_memory", True)) and torch.cuda.is_available(), **extra)
        return loaders[""] if list(loaders) == [""] else DomainBatches(loaders)

    def validation_image_names(self, domain):
        dataset = self.validation_datasets()[domain]
        if isinstance(dataset, ImageDataset):
            root = dataset.image_list_path.parent
            return [os.path.relpath(path, root) for path in dataset.image_path_list]
        return [f"synthetic{'_' + domain if domain else ''}/{i}" for i in range(len(dataset))]

    # ---- scoring ---------------------------------------------------------------------------------------------------
    def validation_buffers(self, device, reset=False):
        """{domain: [K, 4, N] f32 view} of ONE flat device buffer (so that the epoch's end copies once); reset: all NaN"""
        state = self._val
        if state["flat"] is None or state["flat"].device != device:
            K = len(state["ratios"])
            sizes = {domain: K * 4 * len(ds) for domain, ds in self.validation_datasets().items()}
            flat = torch.full((sum(sizes.values()),), float("nan"), dtype=torch.float32, device=device)
            buffers, start = {}, 0
            for domain, size in sizes.items():
                buffers[domain] = flat[start:start + size].view(K, 4, -1)
                start += size
            state["flat"], state["buffers"] = flat, buffers
        elif reset:
            state["flat"].fill_(float("nan"))
        return state["buffers"]

    def validation_stream(self, domain):
        return next(stream for d, _, stream in self.VALIDATION_DOMAINS if d == domain)

    def validation_range(self):
        return -1.0, 1.0  # MseStructuralSimilarityLoss(-1.0, 1.0) of both trainers

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        domain = batch.get("domain", self.VALIDATION_DOMAINS[0][0])
        image = self.validation_images(batch, domain)
        index = torch.as_tensor(batch["index"]).to(device=image.device, dtype=torch.int64)
        scores = self.validation_buffers(image.device, reset=batch_idx == 0)[domain]
        model, stream = self.validation_model(domain), self.validation_stream(domain)
        seed = rng.module_stream(self)[0]
        lo, hi = self.validation_range()
        for k, ratio in enumerate(self._val["ratios"]):
            noisy = ops.noise_blend_fixed_index_rng(image, seed, rng.pack_offset(k, 0, stream), ratio, index)
            ops.quality_per_image(model(noisy), image, lo, hi, index=index, out=scores[k])

    def validation_epoch_end(self, outputs=None):
        state = self._val
        if state["flat"] is None:
            raise RuntimeError("validation_epoch_end before any validation_step")
        host = state["flat"].cpu().numpy()  # the epoch's one device-to-host copy (and its one wait)
        ratios, logged, lines, start = state["ratios"], {}, [], 0
        per_domain = []
        for domain, dataset in self.validation_datasets().items():
            size = len(ratios) * 4 * len(dataset)
            scores = host[start:start + size].reshape(len(ratios), 4, len(dataset))
            start += size
            prefix = f"val_{domain}" if domain else "val"
            summary = summarise(scores, ratios, prefix)
            logged.update(summary)
            per_domain.append((prefix, summary))
            if self.hparams.get("val_report_path"):
                lines += report_lines(self.validation_image_names(domain), scores, ratios)
        if [prefix for prefix, _ in per_domain] != ["val"]:  # several domains: val/... is the mean of theirs
            for name in METRICS:
                logged[f"val/{name}"] = float(np.mean([s[f"{prefix}/{name}"] for prefix, s in per_domain]))
            logged["val/psnr_inf"] = float(sum(s[f"{prefix}/psnr_inf"] for prefix, s in per_domain))
        for key, value in logged.items():
            self.log(key, value)
        if self.hparams.get("val_report_path"):
            path = Path(self.hparams["val_report_path"])
            path.parent.mkdir(parents=True, exist_ok=True)
            tmp = path.with_name(path.name + ".tmp")
            tmp.write_text("".join(line + "\n" for line in lines))
            os.replace(tmp, path)
        return logged
