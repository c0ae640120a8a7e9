"""balance_training_images LitModule (d3f/balance_training_images/lit_module.py:28-193) on the HIP path.

Trains the same U-Net to denoise at ONE fixed noise ratio, then scores every image by its per-image L1
reconstruction error and bins the scores into `number_of_classes` difficulty classes:

    training_step   : image -> blend_fixed_amount_of_noise -> model -> (MSE + 1 - SSIM) / 2      (:88-107)
    validation_step : same blend, eval-mode forward, compute_difficulty_loss = mean |pred - image| per image (:123-142)
    validation_epoch_end : concatenate, compute_difficulty_index_for_each_loss (min-max, clamp, bin) (:144-193)

Device work is HIP: ops.noise_blend_fixed, the Unet engine, the fused loss, ops.l1_per_image, ops.image_grid_u8 (the
`image` / `image_noisy` / `image_prediction` grids of :102-104, written as PNG files: helpers/image_grid_logger.py).
Differences from the reference, on purpose: the matplotlib histogram figure of validation_epoch_end (:151-155) is
produced only with `device_scoring: true` (below), as a chart without text; the reference accepts `--output_list` but
never writes it (dead option) -- here the classes ARE written, one "<relative image path>\\t<class>" line per image, when
`output_image_list_path` is set.
`device_rng: true` (off by default; optional `rng_seed`): the noise is drawn inside the blend kernel by the counter-based
generator (rng.py, csrc/philox.h), a function of (seed, global_step or validation batch index, rank).
`device_scoring: true` (off by default; one process only): the scoring epoch stays on the device.  validation_step writes
its batch's scores into ONE [len(val dataset)] buffer at the batch's `index` (ops.l1_per_image_scatter; NaN = not scored)
and neither copies nor waits; validation_epoch_end runs ops.difficulty_classes and ops.difficulty_histogram_u8 on the
buffer, copies their results out once and logs `difficulty_class_max_count`, the 10 counts of axes.hist as
`difficulty_class_histogram/bin_<k>` and the chart as <log_dir>/images/difficulty_class_histogram/step_<global_step>.png
(helpers/image_grid_logger.py).  Where every score is equal (or one image was scored) the classes are 0; the host path
inherits the reference's NaN -> INT64_MIN there and fails in bincount.
`device_dataset: true` (off by default; optional `device_dataset_max_fraction`; not with `synthetic`): the image list is
decoded once into a uint8 pool on the device (dataset/device_pool.py) that the training and the scoring loader share; both
yield indices and `step_images` gathers and normalises a batch in one launch -- the host transform's values, bit for bit.
"""
import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import distributed, ops, rng
from ..dataset import device_pool
from ..dataset.device_pool import DeviceImagePool
from ..dataset.image_dataset import ImageDataset, NormalizeToTensor, SyntheticFaceDataset
from ..helpers import ImageLoggingMixin
from ..lightning import LightningModule
from ..loss_functions import MseStructuralSimilarityLoss
from ..optim import FusedAdam
from ..unet import Unet


class LitModule(ImageLoggingMixin, LightningModule):
    def __init__(self, **kwargs):
        super().__init__()
        self.save_hyperparameters()
        device_pool.check_hparams(self.hparams, self._data_path())
        self.__dict__["_pool"] = None  # device_dataset: the DeviceImagePool both loaders draw from
        self.setup_image_logging()  # image_logging_scheduler; None unless `image_logging: true`
        self.model = self.create_model_instance()
        self.training_criterion = MseStructuralSimilarityLoss(-1.0, 1.0)
        self.difficulty_index = None  # filled by validation_epoch_end: (image index [N], class [N])
        if self.hparams.get("device_scoring", False) and distributed.env_world()[0] > 1:
            raise ValueError("device_scoring: true scores the whole image list in one process: it cannot be combined with "
                             f"a world size above 1 (WORLD_SIZE={distributed.env_world()[0]}); sharded scoring is not built")
        self.__dict__["_val_dataset_length"] = None  # recorded by val_dataloader()
        self.__dict__["_score_buffer"] = None        # device_scoring: [len(val dataset)] f32, NaN = not scored

    def create_model_instance(self):
        p = self.hparams
        return Unet(encoder_name=p["encoder_name"], encoder_weights=None, in_channels=3, classes=3, activation=p.get("activation"),
                    compute_dtype=p.get("precision", "f32"))

    def _data_path(self):
        p = self.hparams
        return p.get("input_image_list_path") or p.get("data_path")

    def train_dataloader(self):
        p = self.hparams
        return self.create_dataloader(self._data_path(), p.mean, p.std, shuffle=True)

    def val_dataloader(self):
        p = self.hparams
        loader = self.create_dataloader(self._data_path(), p.mean, p.std, shuffle=True)  # the reference shuffles here too
        self.__dict__["_val_dataset_length"] = len(loader.dataset)
        return loader

    def mean_std_unit(self, mean, std):
        """config means / stds in 0..255 units -> [0, 1] units"""
        return [v / 255.0 if max(mean) > 1 else v for v in mean], [v / 255.0 if max(std) > 1 else v for v in std]

    def create_dataloader(self, path, mean, std, shuffle=True):
        p = self.hparams
        if device_pool.check_hparams(p, path):  # the list decoded once into device memory, batches of indices
            if self._pool is None:
                self.__dict__["_pool"] = DeviceImagePool.from_hparams(p, path, self.device)
            return self._pool.loader(p.batch_size, shuffle=shuffle, pin_memory=False)
        if p.get("synthetic", False) or path is None:
            dataset = SyntheticFaceDataset(p.get("synthetic_length", 4 * p.batch_size), p.get("image_size", 256))
        else:
            m, s = self.mean_std_unit(mean, std)
            dataset = ImageDataset(path, transform=NormalizeToTensor(m, s))
        workers = p.get("num_workers", 0)
        extra = dict(multiprocessing_context="spawn", persistent_workers=True) if workers > 0 else {}  # never fork after HIP init
        return DataLoader(dataset=dataset, batch_size=p.batch_size, num_workers=workers, shuffle=shuffle, **extra)

    def configure_optimizers(self):
        p = self.hparams
        return FusedAdam(self.model.parameters(), lr=p.learning_rate, module=self.model)

    @torch.no_grad()
    def step_images(self, batch):
        """a loader's batch -> the normalised float batch.  A `device_dataset` batch carries `index` only: gather from the
        pool and normalise in one launch."""
        if "image" in batch:
            return batch["image"]
        p = self.hparams
        return self._pool.batch(batch["index"], *self.mean_std_unit(p.mean, p.std))

    def training_step(self, batch, batch_idx):
        self.update_image_logging_schedule()
        image = self.step_images(batch)
        image_noisy = self.blend_fixed_amount_of_noise_with_each_sample(image)
        image_prediction = self.model(image_noisy)
        loss = self.training_criterion(image_prediction, image)
        self.log_batch_as_image_grid("image", image)
        self.log_batch_as_image_grid("image_noisy", image_noisy)
        self.log_batch_as_image_grid("image_prediction", image_prediction)
        self.emit_image_grids()
        self.log("loss", loss)
        return loss

    @torch.no_grad()
    def blend_fixed_amount_of_noise_with_each_sample(self, batch, step=None):
        if self.hparams.get("device_rng", False):  # the normals are drawn inside the blend kernel (rng.py, csrc/philox.h)
            seed, offset = rng.module_stream(self, 0, step)
            return ops.noise_blend_fixed_rng(batch, seed, offset, float(self.hparams.ratio_of_noise))
        noise = torch.randn_like(batch)
        return ops.noise_blend_fixed(batch, noise, float(self.hparams.ratio_of_noise))

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        image = self.step_images(batch)
        image_index = batch["index"]
        # (device_rng: validation has no optimiser step to count -- the batch index names the draws)
        image_noisy = self.blend_fixed_amount_of_noise_with_each_sample(image, step=batch_idx)
        image_prediction = self.model(image_noisy)
        if self.hparams.get("device_scoring", False):
            # no copy, no wait: the scores land in the epoch's buffer at the images' indices
            image_index = torch.as_tensor(image_index).to(device=image.device, dtype=torch.int64)  # (it is there already)
            ops.l1_per_image_scatter(image_prediction, image, image_index,
                                     self.score_buffer(image.device, reset=batch_idx == 0))
            return {"scored": int(image.shape[0])}
        difficulty_loss = self.compute_difficulty_loss(image_prediction, image)
        return {"index": torch.as_tensor(image_index).cpu(), "loss": difficulty_loss.cpu()}

    def score_buffer(self, device, reset=False):
        """device_scoring: the [len(val dataset)] score buffer of the current scoring epoch; reset: every entry NaN"""
        if self._val_dataset_length is None:
            self.val_dataloader()
        buffer = self._score_buffer
        if buffer is None or buffer.numel() != self._val_dataset_length or buffer.device != device:
            buffer = torch.empty(self._val_dataset_length, dtype=torch.float32, device=device)
            self.__dict__["_score_buffer"] = buffer
            reset = True
        if reset:
            buffer.fill_(float("nan"))
        return buffer

    def compute_difficulty_loss(self, predicted, target):
        return ops.l1_per_image(predicted, target)

    def validation_epoch_end(self, validation_step_output_list):
        if self.hparams.get("device_scoring", False):
            return self.device_scoring_epoch_end()
        tensors = self.concat_validation_output(validation_step_output_list)
        image_index, difficulty_loss = tensors["index"], tensors["loss"]
        difficulty_index = self.compute_difficulty_index_for_each_loss(difficulty_loss)
        self.difficulty_index = (image_index, difficulty_index)
        counts = torch.bincount(difficulty_index, minlength=int(self.hparams.number_of_classes))
        self.log("difficulty_class_max_count", counts.max().float())
        out_path = self.hparams.get("output_image_list_path")
        if out_path:
            self.write_output_list(out_path, image_index, difficulty_index)
        return difficulty_index

    HISTOGRAM_BINS, HISTOGRAM_SIZE = 10, (480, 640)  # matplotlib's defaults: axes.hist(x), plt.subplots(1, 1)

    def device_scoring_epoch_end(self):
        """the epilogue of a device_scoring epoch: classes, counts, histogram and chart in five launches on the score buffer,
        ONE copy to the host (all results live in one byte buffer), then the host-side logging"""
        scores = self._score_buffer
        if scores is None:
            raise RuntimeError("device_scoring: validation_epoch_end before any validation_step")
        N, nc, bins, (H, W) = scores.numel(), int(self.hparams.number_of_classes), self.HISTOGRAM_BINS, self.HISTOGRAM_SIZE
        layout, total = {}, 0
        for name, dtype, shape in (("classes", torch.int64, (N,)), ("range", torch.float64, (2,)),
                                   ("counts", torch.int32, (nc,)), ("bin_counts", torch.int32, (bins,)),
                                   ("minmax", torch.float32, (2,)), ("chart", torch.uint8, (H, W, 3))):
            size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            layout[name] = (total, size, dtype, shape)
            total += (size + 15) // 16 * 16
        packed = torch.empty(total, dtype=torch.uint8, device=scores.device)
        view = {k: packed[o:o + n].view(dt).view(shape) for k, (o, n, dt, shape) in layout.items()}
        ops.difficulty_classes(scores, nc, out=(view["classes"], view["counts"], view["minmax"]))
        ops.difficulty_histogram_u8(view["classes"], bins, (H, W), out=(view["bin_counts"], view["range"], view["chart"]))
        host = packed.cpu()  # the epoch's one device-to-host copy
        host = {k: host[o:o + n].view(dt).view(shape) for k, (o, n, dt, shape) in layout.items()}
        image_index = torch.nonzero(host["classes"] >= 0).reshape(-1)  # the scored images, ascending
        difficulty_index = host["classes"][image_index].clone()
        self.difficulty_index = (image_index, difficulty_index)
        self.log("difficulty_class_max_count", host["counts"].max().float())
        for k in range(bins):
            self.log(f"difficulty_class_histogram/bin_{k}", float(host["bin_counts"][k]))
        out_path = self.hparams.get("output_image_list_path")
        if out_path:
            self.write_output_list(out_path, image_index, difficulty_index)
        logger = self.image_grid_logger()  # rank 0 writes; `sink` / `experiment` as for the image grids
        if logger.log_dir is not None or logger.sink is not None:  # (a module driven by hand without either: no chart)
            logger.enqueue(["difficulty_class_histogram"], self.global_step, host["chart"].numpy()[None])
            logger.drain()
        return difficulty_index

    def write_output_list(self, out_path, image_index, difficulty_index):
        names = None
        path = self._data_path()
        if path and not self.hparams.get("synthetic", False):
            with open(path) as f:
                names = [line.strip() for line in f if line.strip()]
        order = torch.argsort(image_index)
        with open(out_path, "w") as f:
            for i in order.tolist():
                idx = int(image_index[i])
                name = names[idx] if names is not None and idx < len(names) else str(idx)
                f.write(f"{name}\t{int(difficulty_index[i])}\n")

    def concat_validation_output(self, validation_step_output_list):
        keys = validation_step_output_list[0].keys()
        return {k: torch.concat([o[k].reshape(-1) for o in validation_step_output_list]) for k in keys}

    def compute_difficulty_index_for_each_loss(self, loss):
        # host arithmetic on the gathered [N] vector, operation for operation as the reference (:181-193)
        p = self.hparams
        loss_min = loss.min()
        loss_max = loss.max()
        loss_normalised = (loss - loss_min) / (loss_max - loss_min)
        loss_normalised = loss_normalised.clamp(0, 0.99999)
        return (loss_normalised * p.number_of_classes).long()
