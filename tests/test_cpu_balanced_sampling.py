"""Balanced sampling (`balanced_sampling: true`), the host half: the class list `d3f balance` writes as an input list, the
balance table, BalancedSampler and its sharding, and every refusal that happens before a device call.  No test here needs a
GPU."""
import ctypes as C
from pathlib import Path

import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib
from denoising_diffusion_deep_fake_amd.dataset import BalancedSampler, ImageDataset, balanced
from denoising_diffusion_deep_fake_amd.dataset.device_pool import DeviceImagePool

ROOT = Path(__file__).resolve().parent.parent
SIZES = [1, 5, 0, 17, 40]                     # images per class; class 2 is empty
CLASSES = [k for k, n in enumerate(SIZES) for _ in range(n)]


def _write(path, lines):
    path.write_text("".join(line + "\n" for line in lines))
    return path


# ---- the class list as input ----------------------------------------------------------------------------------------------
def test_a_plain_list_is_read_as_before(tmp_path):
    path = _write(tmp_path / "images.txt", ["a/0.png", "", "  a/1 1.png  ", "b/2.png"])
    dataset = ImageDataset(path)
    assert dataset.image_path_list == [tmp_path / "a/0.png", tmp_path / "a/1 1.png", tmp_path / "b/2.png"]
    assert dataset.image_class_list is None and len(dataset) == 3


def test_a_class_list_gives_paths_and_classes(tmp_path):
    path = _write(tmp_path / "classes.txt", ["a/0.png\t3", "a/1.png\t0", "", "odd\tname.png\t12", "b/2.png\t3"])
    dataset = ImageDataset(path)
    assert dataset.image_path_list == [tmp_path / "a/0.png", tmp_path / "a/1.png", tmp_path / "odd\tname.png",
                                       tmp_path / "b/2.png"]
    assert dataset.image_class_list == [3, 0, 12, 3]


def test_a_tab_without_a_trailing_integer_is_part_of_the_path(tmp_path):
    names = ["odd\tname.png", "odd\t-1", "odd\t1.5", "odd\t1e3", "odd\t", "odd\t0x10"]
    dataset = ImageDataset(_write(tmp_path / "images.txt", names))
    assert dataset.image_class_list is None
    assert dataset.image_path_list == [tmp_path / name.strip() for name in names]


def test_a_mixed_list_is_refused_and_names_the_first_offending_line(tmp_path):
    path = _write(tmp_path / "mixed.txt", ["a/0.png\t3", "a/1.png\t0", "a/2.png", "a/3.png\t1"])
    with pytest.raises(ValueError, match=r"mixed\.txt: line 3 \('a/2\.png'\) has no difficulty class"):
        ImageDataset(path)
    path = _write(tmp_path / "mixed2.txt", ["a/0.png", "", "a/1.png\t7"])
    with pytest.raises(ValueError, match=r"mixed2\.txt: line 3 \('a/1\.png\\t7'\) has a difficulty class"):
        ImageDataset(path)


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_balance_table_squeezes_empty_classes_out():
    """classes [3, 0, 3, 9, 0] of number_of_classes 10: three classes have an image"""
    members, class_start = balanced.balance_table([3, 0, 3, 9, 0])
    assert members.dtype == class_start.dtype == torch.int64
    assert members.tolist() == [1, 4, 0, 2, 3] and class_start.tolist() == [0, 2, 4, 5]
    pool = DeviceImagePool(torch.zeros(5, 2, 2, 3, dtype=torch.uint8), classes=[3, 0, 3, 9, 0])
    table = pool.balance_table()
    assert table.Kn == 3 and len(table) == 5
    assert table.members.tolist() == [1, 4, 0, 2, 3] and table.class_start.tolist() == [0, 2, 4, 5]


def test_balance_table_of_a_single_class_and_of_part_of_a_pool():
    members, class_start = balanced.balance_table([7, 7, 7, 7])
    assert members.tolist() == [0, 1, 2, 3] and class_start.tolist() == [0, 4]
    # 9 of 23 images, listed out of order: sorted by (class, index)
    index = [22, 3, 17, 0, 8, 11, 5, 20, 1]
    classes = [2, 0, 2, 5, 0, 2, 5, 0, 2]
    pool = DeviceImagePool(torch.zeros(23, 2, 2, 3, dtype=torch.uint8))
    table = pool.balance_table(classes, index)
    assert table.members.tolist() == [3, 8, 20, 1, 11, 17, 22, 0, 5] and table.class_start.tolist() == [0, 3, 7, 9]
    assert table.Kn == 3


def test_balance_table_refusals():
    pool = DeviceImagePool(torch.zeros(5, 2, 2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="empty"):
        balanced.balance_table([])
    with pytest.raises(ValueError, match="empty"):
        pool.balance_table([])
    with pytest.raises(ValueError, match="no difficulty classes"):
        pool.balance_table()
    with pytest.raises(ValueError, match=r"member 5 outside the pool's \[0, 5\)"):
        pool.balance_table([0, 1], [4, 5])
    with pytest.raises(ValueError, match=r"member -1 outside"):
        pool.balance_table([0, 1], [-1, 2])
    with pytest.raises(ValueError, match=r"member 5 outside"):
        pool.balance_table([0] * 6)          # a class list longer than the pool
    with pytest.raises(ValueError, match="2 classes for 3 images"):
        pool.balance_table([0, 1], [1, 2, 3])


# ---- the sampler ----------------------------------------------------------------------------------------------------------
def test_sampler_is_a_function_of_seed_epoch_and_rank():
    a, b = BalancedSampler(CLASSES, 5), BalancedSampler(CLASSES, 5)
    assert isinstance(a, torch.utils.data.Sampler) and len(a) == len(CLASSES) == 63
    first = list(a)
    assert len(first) == 63 and all(0 <= i < 63 for i in first)
    assert first == list(a) == list(b)
    assert first != list(BalancedSampler(CLASSES, 6))
    a.set_epoch(1)
    assert list(a) != first
    b.set_epoch(1)
    assert list(a) == list(b)
    a.set_epoch(0)
    assert list(a) == first                   # a resumed run replays the epoch
    assert list(BalancedSampler(CLASSES, lambda: 5)) == first     # the seed may be asked for late
    assert list(BalancedSampler(CLASSES, 5, stream=1)) != first
    ranks = [a.for_rank(2, r, 5) for r in (0, 1)]
    assert [len(s) for s in ranks] == [32, 32] and [len(list(s)) for s in ranks] == [32, 32]
    assert list(ranks[0]) != list(ranks[1]) and list(ranks[0]) == list(a.for_rank(2, 0, 5))
    assert len(BalancedSampler(CLASSES, 5).for_rank(4, 3, 5)) == 16


def test_sampler_draws_every_class_equally_often():
    """16 384 draws over four non-empty classes: 4096 each, standard deviation sqrt(16384 * 1/4 * 3/4) = 55.4; the bound is
    five of them.  Within the class of 40 every image is expected 102.4 times (sd 10.1): 103 +- 51."""
    sampler = BalancedSampler(CLASSES, 1234)
    draws = sampler.draw(16384)
    assert draws.dtype == torch.int64 and draws.shape == (16384,)
    per_class = torch.bincount(torch.tensor(CLASSES)[draws], minlength=5).tolist()
    print("class counts", per_class)
    assert per_class[2] == 0
    for k in (0, 1, 3, 4):
        assert abs(per_class[k] - 4096) <= 277, per_class
    per_image = torch.bincount(draws, minlength=63)[23:]
    print("members of the class of 40", per_image.min().item(), per_image.max().item())
    assert per_image.numel() == 40 and bool(((per_image - 103).abs() <= 51).all())


def test_shard_loader_rebuilds_a_balanced_loader_through_for_rank():
    from torch.utils.data import DataLoader, WeightedRandomSampler
    from denoising_diffusion_deep_fake_amd.trainer import _set_epoch, shard_loader
    pool = DeviceImagePool(torch.zeros(63, 2, 2, 3, dtype=torch.uint8), classes=CLASSES)
    loader = pool.loader(4, sampler=BalancedSampler(CLASSES, 9))
    assert len(loader) == 16 and shard_loader(loader, 1, 0, 9) is loader
    seen = []
    for rank in (0, 1):
        mine = shard_loader(loader, 2, rank, 77)
        assert isinstance(mine.sampler, BalancedSampler) and mine.sampler is not loader.sampler
        assert mine.sampler.rank == rank and mine.sampler.seed == 77 and len(mine.sampler) == 32 and len(mine) == 8
        assert mine.batch_size == 4 and mine.collate_fn is loader.collate_fn
        _set_epoch(mine, 3, 77)
        assert mine.sampler.epoch == 3
        batches = [b["index"].tolist() for b in mine]
        assert len(batches) == 8 and all(len(b) == 4 for b in batches)
        assert batches == [b["index"].tolist() for b in mine]
        seen.append(batches)
    assert seen[0] != seen[1]
    weighted = DataLoader(pool.loader(4).dataset, batch_size=4, sampler=WeightedRandomSampler([1.0] * 63, 63))
    with pytest.raises(TypeError, match="WeightedRandomSampler"):
        shard_loader(weighted, 2, 0, 77)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_modules_refuse_balanced_sampling_without_classes_or_with_synthetic(tmp_path):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule as Fake
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule as Denoiser
    plain = str(_write(tmp_path / "images.txt", [f"{i}.png" for i in range(4)]))
    classes = str(_write(tmp_path / "classes.txt", [f"{i}.png\t{i % 2}" for i in range(4)]))
    common = dict(batch_size=4, learning_rate=0.01, encoder_name="resnet18", num_workers=0, balanced_sampling=True)
    fake = dict(common, mode="denoise")
    with pytest.raises(ValueError, match=r"images\.txt\s+has none"):
        Denoiser(**dict(common, input_image_list_path=plain))
    with pytest.raises(ValueError, match=r"images\.txt\s+has none"):
        Fake(**dict(fake, data_path_a=plain, data_path_b=classes))
    with pytest.raises(ValueError, match=r"images\.txt\s+has none"):
        Fake(**dict(fake, data_path_a=classes, data_path_b=plain))
    with pytest.raises(ValueError, match="image list"):
        Denoiser(**common)
    with pytest.raises(ValueError, match="image list"):
        Fake(**dict(fake, data_path_a=classes))
    for device_dataset in (False, True):
        with pytest.raises(ValueError, match="synthetic"):
            Denoiser(**dict(common, input_image_list_path=classes, synthetic=True, device_dataset=device_dataset))
        with pytest.raises(ValueError, match="synthetic"):
            Fake(**dict(fake, data_path_a=classes, data_path_b=classes, synthetic=True, device_dataset=device_dataset))
    # with classes both construct, on the host and for the device path, without a device call
    for extra in ({}, dict(device_dataset=True, device_rng=True)):
        lit = Denoiser(**dict(common, input_image_list_path=classes, **extra))
        assert lit.balanced_on_device() is bool(extra) and lit._balance_table is None
        lit = Fake(**dict(fake, data_path_a=classes, data_path_b=classes, **extra))
        assert lit.balanced_on_device() is bool(extra) and lit._balance_tables == {}
    # absent or false: nothing is asked of the list
    assert not Denoiser(**dict(common, balanced_sampling=False, input_image_list_path=plain)).balanced_on_device()


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """every refusal happens on the host: the dummy device pointers are never dereferenced"""
    lib = _lib.lib()
    names = {"d3f_pool_batch_balanced_rng", "d3f_balanced_index_draw"}
    assert names <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES) and all(hasattr(lib, n) for n in names)
    d = C.c_void_p(0x1000)
    f3 = C.c_float * 3
    good = dict(pool=d, N=5, members=d, class_start=d, Kn=3, out=d, index_out=d, B=4, H=8, W=10, mean=f3(0.4, 0.5, 0.6),
                std=f3(0.2, 0.3, 0.4), kind=1, params=(C.c_float * 5)(0.2, 0.1, 15.0, 0.7, 0.0))

    def batch(**kw):
        a = dict(good, **kw)
        return lib.d3f_pool_batch_balanced_rng(a["pool"], a["N"], a["members"], a["class_start"], a["Kn"], a["out"],
                                               a["index_out"], a["B"], a["H"], a["W"], a["mean"], a["std"], 0x5EED, 3,
                                               a["kind"], a["params"], None)

    def draw(**kw):
        a = dict(good, **kw)
        return lib.d3f_balanced_index_draw(a["members"], a["class_start"], a["Kn"], 0x5EED, 3, a["index_out"], a["B"], None)

    shared = ((dict(members=None), b"members is null"), (dict(class_start=None), b"class_start is null"),
              (dict(index_out=None), b"index_out is null"), (dict(Kn=0), b"Kn 0 < 1"), (dict(Kn=-2), b"Kn -2 < 1"),
              (dict(B=65536), b"B 65536 above 65535"), (dict(B=-1), b"B -1 < 0"))
    only_batch = ((dict(pool=None), b"pool is null"), (dict(out=None), b"out is null"), (dict(mean=None), b"mean is null"),
                  (dict(std=None), b"std is null"), (dict(N=0), b"N 0 < 1"), (dict(H=0), b"H 0"), (dict(W=-1), b"W -1"),
                  (dict(std=f3(0.2, 0.0, 0.4)), b"zero std"), (dict(H=32768, W=21846), b"2^31"),
                  (dict(params=None), b"params is null"), (dict(kind=2), b"kind"), (dict(kind=-2), b"kind"))
    for name, call, cases in ((b"pool_batch_balanced_rng:", batch, shared + only_batch), (b"balanced_index_draw:", draw, shared)):
        for kw, word in cases:
            assert call(**kw) != 0, (name, kw)
            message = lib.d3f_last_error()
            if kw.keys() & {"params", "kind"}:
                assert word in message, (name, kw, message)   # (the augmentation's own check words these)
            else:
                assert message.startswith(name) and word in message, (name, kw, message)
    # B == 0 launches nothing; without an augmentation no params are needed
    assert batch(B=0, index_out=None, out=None) == 0 and draw(B=0, index_out=None) == 0
    assert batch(B=0, kind=_lib.AUGMENT_NONE, params=None) == 0
    assert batch(B=0, H=32768, W=21845) == 0


def test_shipped_configs_leave_balanced_sampling_off():
    import yaml
    configs = sorted((ROOT / "denoising_diffusion_deep_fake_amd").rglob("*.yml"))
    assert len(configs) >= 4
    mentioned = 0
    for config in configs:
        assert not (yaml.safe_load(config.read_text()) or {}).get("balanced_sampling", False), config
        mentioned += "balanced_sampling" in config.read_text()
    assert mentioned >= 3                     # the trainers' configs show the line, commented out
