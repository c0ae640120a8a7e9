"""Balanced sampling (hyper-parameter `balanced_sampling: true`): train from the difficulty classes `d3f balance` writes.

The reference's balance command exists "to assign difficulty class to each image for balanced sampling" and stops there; the
sampling is this project's.  A draw picks one of the classes that have an image, each with equal probability, then one of that
class's images, each with equal probability -- with replacement; an epoch is N draws, N the number of listed images, so the
steps per epoch and the learning-rate schedule are those of the plain run.

Two forms of the same distribution:
  * `BalancedSampler`, a torch sampler for any host loader (and for the device pool's index loader without `device_rng`);
  * the balance table (`balance_table`) that ops.pool_batch_balanced_rng draws from inside the launch that assembles the batch
    (`device_dataset` with `device_rng`; csrc/philox.h has the draw).
"""
import torch
from torch.utils.data import Sampler

from .image_dataset import ImageDataset


def check_hparams(hparams, *paths):
    """`balanced_sampling: true` needs image lists with classes: refuse it together with `synthetic`, without a list or with a
    list that `d3f balance` did not write.  Returns None when off, else each list's classes (one int per image).  Host only:
    the lists are read, no image is."""
    if not hparams.get("balanced_sampling", False):
        return None
    if hparams.get("synthetic", False):
        raise ValueError("balanced_sampling: true draws from the difficulty classes of an image list: it cannot be combined "
                         "with synthetic: true")
    if any(path is None for path in paths):
        raise ValueError("balanced_sampling: true needs an image list with classes (none of the image list paths may be "
                         "missing)")
    classes = []
    for path in paths:
        found = ImageDataset(path).image_class_list
        if found is None:
            raise ValueError(f"balanced_sampling: true needs the difficulty class of every image, and the image list {path} "
                             f"has none: train from the --output_list of `d3f balance` (lines '<path>\\t<class>')")
        classes.append(found)
    return classes


def balance_table(classes, N=None, index=None):
    """(members [M] int64, class_start [Kn + 1] int64) on the host: `members` the listed images sorted by (class, index),
    `class_start` the offsets into it of the Kn classes that have an image -- empty classes are squeezed out, so a draw never
    meets one.  classes: the class of every listed image; index: which image of a pool of N each entry means (default: entry
    i is image i; N defaults to the number of entries)."""
    classes = torch.as_tensor(classes, dtype=torch.int64).reshape(-1)
    M = classes.numel()
    if M == 0:
        raise ValueError("balanced sampling: the class list is empty (no class has an image)")
    if M >= 1 << 31:
        raise ValueError(f"balanced sampling: {M} listed images, the draw addresses fewer than 2**31")
    index = torch.arange(M, dtype=torch.int64) if index is None else torch.as_tensor(index, dtype=torch.int64).reshape(-1)
    if index.numel() != M:
        raise ValueError(f"balanced sampling: {M} classes for {index.numel()} images")
    N = M if N is None else int(N)
    outside = (index < 0) | (index >= N)
    if bool(outside.any()):
        raise ValueError(f"balanced sampling: member {int(index[outside][0])} outside the pool's [0, {N})")
    if bool((classes < 0).any()):
        raise ValueError(f"balanced sampling: a difficulty class below 0 ({int(classes.min())})")
    order = torch.argsort(index, stable=True)
    order = order[torch.argsort(classes[order], stable=True)]  # by class, ties by index
    _, counts = torch.unique_consecutive(classes[order], return_counts=True)
    class_start = torch.zeros(counts.numel() + 1, dtype=torch.int64)
    class_start[1:] = torch.cumsum(counts, 0)
    return index[order].contiguous(), class_start


class BalanceTable:
    """a balance table next to the pool it indexes, on the pool's device"""

    def __init__(self, members, class_start):
        self.members, self.class_start = members, class_start

    @property
    def Kn(self):
        return self.class_start.shape[0] - 1

    def __len__(self):
        return self.members.shape[0]


class BalancedSampler(Sampler):
    """N = len(classes) draws per epoch, each a class (among those with an image) and then one of its images, from a
    torch.Generator seeded from (seed, epoch, rank, stream): `set_epoch` (trainer._set_epoch calls it) moves to the next
    epoch's draws and a resumed run replays the interrupted epoch.  seed: an int, or a callable that gives one when the
    epoch's draws are made (a LitModule learns its trainer's base seed only after train_dataloader()).  stream tells the
    loaders of one run apart (train_deep_fake's two domains)."""

    def __init__(self, classes, seed=0, num_samples=None, rank=0, stream=0):
        self.classes = [int(c) for c in classes]
        self.members, self.class_start = balance_table(self.classes)
        self.seed, self.rank, self.stream, self.epoch = seed, int(rank), int(stream), 0
        self.num_samples = len(self.classes) if num_samples is None else int(num_samples)

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def for_rank(self, world_size, rank, seed=None):
        """this sampler for one rank of `world_size`: ceil(N / world) draws per epoch from the rank's own stream (draws with
        replacement need no sharding of the list)"""
        n = -(-len(self.classes) // int(world_size))
        return BalancedSampler(self.classes, self.seed if seed is None else seed, num_samples=n, rank=rank,
                               stream=self.stream)

    def generator(self):
        seed = int(self.seed() if callable(self.seed) else self.seed)
        mixed = (seed * 0x9E3779B97F4A7C15 + (self.epoch << 24 | self.rank << 8 | self.stream)) % (1 << 63)
        return torch.Generator().manual_seed(mixed)

    def draw(self, n):
        """n draws of the current epoch's stream: int64 [n]"""
        g = self.generator()
        start = self.class_start
        j = torch.randint(start.numel() - 1, (n,), generator=g)
        count = start[j + 1] - start[j]
        m = (torch.rand(n, dtype=torch.float64, generator=g) * count).long()
        return self.members[start[j] + torch.minimum(m, count - 1)]

    def __iter__(self):
        return iter(self.draw(self.num_samples).tolist())
