"""`log_batch_as_image_grid` of the three LitModules (d3f/train_deep_fake/lit_module.py:235-249,
d3f/train_denoiser/lit_module.py:157-171, d3f/balance_training_images/lit_module.py:197-211) without TensorBoard: the
grid the reference hands to `add_image` is built on the device as the uint8 HWC image TensorBoard would have stored
(ops.image_grid_u8: make_grid, * 0.5 + 0.5, clamp, * 255 truncated) and lands as a PNG next to metrics.csv,

    <log_dir>/images/<tag>/step_<global_step:08d>.png        ("/" in a tag is a directory, as TensorBoard groups tags)

The step path does not wait for the device: all tags of one call site go through ONE kernel launch, the result is copied
into page-locked host memory with non_blocking=True, an event is recorded and (tags, step, buffer, event) is queued.  The
queue is drained -- wait for the event, then write -- at the start of the next logging step, when the Trainer flushes its
metrics, and at the end of fit.
"""
from pathlib import Path

import numpy as np
import torch

from .logging_scheduler import LoggingScheduler

MAX_TAGS_PER_LAUNCH = 8  # d3f_image_grid_u8


class ImageGridLogger:
    """log(): the device half (rank 0 only); enqueue() / drain(): the host half, usable with host arrays alone.

    sink: a callable (tag, step, ndarray [GH, GW, 3] uint8) that replaces the PNG writer.  experiment: an object with
    TensorBoard's `add_image`; called as add_image(tag, array, step, dataformats="HWC") after the writer."""

    def __init__(self, log_dir=None, rank=0, sink=None, experiment=None, nrow=3, padding=2, max_images=9):
        self.log_dir = None if log_dir is None else Path(log_dir)
        self.rank, self.sink = int(rank), sink
        self.experiment = experiment if hasattr(experiment, "add_image") else None
        self.nrow, self.padding, self.max_images = nrow, padding, max_images
        self._queue = []  # (tags, step, host grids [n, GH, GW, 3], event or None, pooled)
        self._pool = {}   # shape -> page-locked host buffers not in the queue

    # ---- step path -------------------------------------------------------------------------------------------------
    def log(self, pairs, step):
        """pairs: (tag, NCHW batch on the HIP device) of one call site.  Grids of EARLIER steps are drained first."""
        pairs = list(pairs)
        if self.rank != 0 or not pairs:
            return
        from .. import ops
        self.drain(before_step=step)
        start = 0
        while start < len(pairs):  # runs of one shape, at most 8 tags each: one launch per run
            stop = start + 1
            while stop < len(pairs) and stop - start < MAX_TAGS_PER_LAUNCH and \
                    pairs[stop][1].shape == pairs[start][1].shape:
                stop += 1
            run = pairs[start:stop]
            grids = ops.image_grid_u8([b for _, b in run], nrow=self.nrow, padding=self.padding,
                                      max_images=self.max_images)
            free = self._pool.setdefault(tuple(grids.shape), [])
            host = free.pop() if free else torch.empty(grids.shape, dtype=torch.uint8).pin_memory()
            host.copy_(grids, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            self._queue.append(([t for t, _ in run], int(step), host, event, True))
            start = stop

    # ---- host half -------------------------------------------------------------------------------------------------
    def enqueue(self, tags, step, grids, event=None):
        """queue finished grids [n, GH, GW, 3] (uint8 ndarray or host tensor), one per tag; event: what to wait for"""
        if self.rank != 0:
            return
        tags = list(tags)
        if len(tags) != len(grids):
            raise ValueError(f"{len(tags)} tags for {len(grids)} grids")
        self._queue.append((tags, int(step), grids, event, False))

    def drain(self, before_step=None):
        """write what is queued, in the order it was queued; before_step: only the grids of earlier steps"""
        keep = []
        for entry in self._queue:
            tags, step, grids, event, pooled = entry
            if before_step is not None and step >= before_step:
                keep.append(entry)
                continue
            if event is not None:
                event.synchronize()
            arrays = grids.numpy() if isinstance(grids, torch.Tensor) else np.asarray(grids)
            for tag, array in zip(tags, arrays):
                self.write(tag, step, array)
            if pooled:
                self._pool[tuple(grids.shape)].append(grids)
        self._queue = keep

    def path(self, tag, step):
        return self.log_dir.joinpath("images", *[part for part in tag.split("/") if part], f"step_{int(step):08d}.png")

    def write(self, tag, step, array):
        if self.sink is not None:
            self.sink(tag, step, np.array(array, dtype=np.uint8))  # a copy: the host buffer is used again
        else:
            if self.log_dir is None:
                raise RuntimeError("ImageGridLogger needs a log_dir or a sink")
            from PIL import Image
            path = self.path(tag, step)
            path.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(np.ascontiguousarray(array, dtype=np.uint8)).save(path)
        if self.experiment is not None:
            self.experiment.add_image(tag, np.array(array, dtype=np.uint8), step, dataformats="HWC")


class ImageLoggingMixin:
    """The image-logging surface the LitModules share.  hparams: `image_logging` (absent: off -- nothing below does any
    work), `image_logging_every_n_steps` (global_step % n == 0 in place of the clock).  A training step calls
    update_image_logging_schedule() once per batch, log_batch_as_image_grid(tag, batch) where the reference does, and
    emit_image_grids() once all tags of the call site are named: they leave as one kernel launch.
    `image_grid_sink` (attribute): a callable (tag, step, ndarray) in place of the PNG files."""

    def setup_image_logging(self):
        p = self.hparams
        on = bool(p.get("image_logging", False))
        if on and p.get("graph_step", False):
            raise ValueError("image_logging: true cannot be combined with graph_step: true: the captured whole-step "
                             "entry (d3f_unet_train_step) exposes no tensors to log")
        self.image_logging_scheduler = LoggingScheduler(p.get("image_logging_every_n_steps")) if on else None
        self.image_grid_sink = None
        self.__dict__["_grid_pending"] = []
        self.__dict__["_grid_logger"] = None

    def update_image_logging_schedule(self):
        if self.image_logging_scheduler is not None:
            self.image_logging_scheduler.update_with_step_number(self.global_step)

    def log_batch_as_image_grid(self, tag, batch, first_batch_only=False):
        scheduler = self.image_logging_scheduler
        if scheduler is not None and scheduler.should_we_log_this_step():
            self._grid_pending.append((tag, batch))  # 3 x 3 grid of the first 9 images, built in emit_image_grids

    def emit_image_grids(self):
        if self._grid_pending:
            pending = list(self._grid_pending)
            self._grid_pending.clear()
            self.image_grid_logger().log(pending, self.global_step)

    def image_grid_logger(self):
        """the logger of the current fit (a new Trainer.fit has a new log_dir), made on first use"""
        trainer = self.trainer
        log_dir = getattr(trainer, "log_dir", None)
        logger = self._grid_logger
        if logger is None or logger.log_dir != (None if log_dir is None else Path(log_dir)) or \
                logger.sink is not self.image_grid_sink:
            if logger is not None:
                logger.drain()
            logger = self.__dict__["_grid_logger"] = ImageGridLogger(
                log_dir=log_dir, rank=getattr(trainer, "global_rank", 0), sink=self.image_grid_sink,
                experiment=getattr(getattr(trainer, "logger", None), "experiment", None))
        return logger

    def drain_image_grids(self):
        if self._grid_logger is not None:
            self._grid_logger.drain()
