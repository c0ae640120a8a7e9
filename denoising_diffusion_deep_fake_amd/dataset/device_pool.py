"""Device-resident image dataset (hyper-parameter `device_dataset: true`).

A training set here is the frames of one video, a few thousand 448x448 crops, trained over for hundreds of epochs -- and
decoded again by the host loader in every one of them.  `DeviceImagePool` decodes the image list ONCE into a
`[N, H, W, 3]` uint8 tensor in device memory (10 000 frames at 448x448 are 6 GB of the MI355X's 288 GB); after that a batch
is its indices: the loader yields `{"index": int64 [B]}` and the LitModule's step turns them into the normalised, augmented
float batch with one kernel launch (ops.pool_batch / ops.pool_batch_rng).  No image byte crosses PCIe in steady state and
loader workers run only while the pool is filled.  With `balanced_sampling` and `device_rng` the launch draws the indices too
(ops.pool_batch_balanced_rng, from `balance_table`): the loader then only counts the epoch's batches.

The loader is an ordinary DataLoader over an index-only dataset, so everything the trainer does to a loader --
`shard_loader`, the per-epoch generator of `_set_epoch` (and with it the replay of a mid-epoch resume), `CombinedLoader`,
`limit_*_batches` -- works unchanged and visits the images in the order the host loader would for the same seed and epoch.
Under data parallelism every rank holds the WHOLE pool: the distributed sampler deals a fresh shard of the list to each rank
every epoch, so a rank needs every image sooner or later.
"""
import torch
from torch.utils.data import DataLoader, Dataset

from . import balanced
from .image_dataset import ImageDataset, ToUint8Tensor


def check_hparams(hparams, *paths):
    """`device_dataset: true` needs real image lists: refuse it together with `synthetic` or without a list"""
    if not hparams.get("device_dataset", False):
        return False
    if hparams.get("synthetic", False):
        raise ValueError("device_dataset: true keeps the images of an image list on the device: it cannot be combined "
                         "with synthetic: true")
    if any(path is None for path in paths):
        raise ValueError("device_dataset: true needs an image list (none of the image list paths may be missing)")
    return True


class IndexDataset(Dataset):
    """the index half of ImageDataset's items: `[i] -> {"index": i}`"""

    def __init__(self, length):
        self.length = int(length)

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        return {"index": index}


class IndexCollate:
    """items -> {"index": int64 [B]}, every index checked against [0, N) on the host, where the sampler made it (the
    kernel would answer one outside with an all-NaN image)"""

    def __init__(self, length):
        self.length = int(length)

    def __call__(self, items):
        index = [int(item["index"]) for item in items]
        bad = [i for i in index if not 0 <= i < self.length]
        if bad:
            raise IndexError(f"device dataset: index {bad[0]} outside the pool's [0, {self.length})")
        return {"index": torch.tensor(index, dtype=torch.int64)}


def _list_collate(items):
    """the fill loader's collate: the decoded images as they are (images of unequal size must reach the check, not
    torch.stack)"""
    return [(int(item["index"]), item["image"]) for item in items]


class DeviceImagePool:
    CHUNK = 64  # images per staging buffer and copy while the pool is filled

    def __init__(self, images, paths=None, classes=None):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError("DeviceImagePool holds uint8 images [N, H, W, 3] (RGB)")
        self.images = images.contiguous()
        self.paths = paths
        self.classes = classes  # the list's difficulty classes (ImageDataset.image_class_list), or None

    def __len__(self):
        return self.images.shape[0]

    @property
    def geometry(self):
        """(H, W) of every image"""
        return tuple(self.images.shape[1:3])

    @classmethod
    def from_list(cls, path, device, num_workers=0, max_fraction=0.5):
        """decode the image list `path` once into a pool on `device`: ImageDataset(path, ToUint8Tensor()) read in order
        through spawned workers, staged in pinned memory, copied in chunks"""
        device = torch.device(device)
        dataset = ImageDataset(path, ToUint8Tensor())
        N = len(dataset)
        if N == 0:
            raise ValueError(f"device dataset: the image list {path} is empty")
        first = dataset[0]["image"]
        H, W = int(first.shape[0]), int(first.shape[1])
        asked = N * H * W * 3
        free = int(torch.cuda.mem_get_info(device)[0])
        if asked > float(max_fraction) * free:
            raise ValueError(f"device dataset: the pool of {path} ({N} images of {H}x{W}) asks for {asked} bytes, more than "
                             f"{max_fraction} of the {free} bytes free on {device}; raise device_dataset_max_fraction or "
                             f"train from files")
        pool = torch.empty((N, H, W, 3), dtype=torch.uint8, device=device)
        on_gpu = device.type == "cuda"
        chunk = min(cls.CHUNK, N)
        staging = [torch.empty((chunk, H, W, 3), dtype=torch.uint8, pin_memory=on_gpu) for _ in range(2)]
        copied = [None, None]  # the event behind the last copy out of each staging buffer
        extra = dict(multiprocessing_context="spawn", prefetch_factor=2) if num_workers > 0 else {}  # never fork after HIP init
        # (a generator of its own: a loader's iterator takes its base seed from `generator`, by default the global one --
        # filling the pool must leave the global generator where a run from files has it, or every later shuffle differs)
        loader = DataLoader(dataset, batch_size=chunk, shuffle=False, num_workers=num_workers, collate_fn=_list_collate,
                            generator=torch.Generator().manual_seed(0), **extra)
        for k, items in enumerate(loader):
            buf = staging[k % 2]
            if copied[k % 2] is not None:
                copied[k % 2].synchronize()
            for j, (i, image) in enumerate(items):
                if tuple(image.shape) != (H, W, 3):
                    raise ValueError(f"device dataset: {dataset.image_path_list[i]} is {image.shape[0]}x{image.shape[1]}, "
                                     f"the first image {dataset.image_path_list[0]} is {H}x{W}; a pool holds images of one "
                                     f"size")
                buf[j].copy_(image)
            i0 = items[0][0]
            pool[i0:i0 + len(items)].copy_(buf[:len(items)], non_blocking=True)
            if on_gpu:
                copied[k % 2] = torch.cuda.Event()
                copied[k % 2].record()
        if on_gpu:
            torch.cuda.current_stream(device).synchronize()
        return cls(pool, paths=dataset.image_path_list, classes=dataset.image_class_list)

    @classmethod
    def from_hparams(cls, hparams, path, device):
        return cls.from_list(path, device, num_workers=hparams.get("num_workers", 0),
                             max_fraction=hparams.get("device_dataset_max_fraction", 0.5))

    def loader(self, batch_size, shuffle=True, pin_memory=True, sampler=None):
        """index batches in the order the host loader visits the images: RandomSampler / SequentialSampler (or `sampler`,
        a BalancedSampler say), ragged last batch kept, no workers (there is nothing to decode)"""
        N = len(self)
        order = dict(shuffle=shuffle) if sampler is None else dict(sampler=sampler)
        return DataLoader(IndexDataset(N), batch_size=batch_size, num_workers=0, collate_fn=IndexCollate(N),
                          pin_memory=bool(pin_memory) and torch.cuda.is_available(), **order)

    def balance_table(self, classes=None, index=None):
        """the table the balanced launch draws from, in device memory next to the pool: `members`, the listed images sorted
        by (class, index), and `class_start`, the offsets of the classes that have an image (balanced.balance_table, built on
        the host once).  classes: default the classes of the list the pool was filled from; index: the image each entry
        means when the classes cover only part of the pool."""
        classes = self.classes if classes is None else classes
        if classes is None:
            raise ValueError("device dataset: the pool's image list carries no difficulty classes")
        members, class_start = balanced.balance_table(classes, len(self), index)
        return balanced.BalanceTable(members.to(self.images.device), class_start.to(self.images.device))

    # ---- a batch part {"index": int64 [B] on the device} -> the float batch, one launch ---------------------------------
    def batch(self, index, mean, std, theta=None, apply=None):
        from .. import ops
        return ops.pool_batch(self.images, index, mean, std, theta, apply)

    def batch_rng(self, index, mean, std, seed, offset, kind, params):
        from .. import ops
        return ops.pool_batch_rng(self.images, index, mean, std, seed, offset, kind, params)

    def batch_balanced_rng(self, table, B, mean, std, seed, offset, kind, params=None):
        """(batch, index): B images drawn from `table` inside the launch that gathers, normalises and augments them"""
        from .. import ops
        return ops.pool_batch_balanced_rng(self.images, table.members, table.class_start, B, mean, std, seed, offset, kind,
                                           params)
