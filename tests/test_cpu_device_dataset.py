"""Device dataset (`device_dataset: true`), the host half: the C ABI's refusals, the index loader, the pool's refusals and
the shipped configs.  No test here needs a GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib
from denoising_diffusion_deep_fake_amd.dataset import device_pool
from denoising_diffusion_deep_fake_amd.dataset.device_pool import DeviceImagePool

ROOT = Path(__file__).resolve().parent.parent


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """every refusal happens on the host: the dummy device pointers are never dereferenced"""
    lib = _lib.lib()
    assert hasattr(lib, "d3f_pool_batch") and hasattr(lib, "d3f_pool_batch_rng")
    assert {"d3f_pool_batch", "d3f_pool_batch_rng"} <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES)
    d = C.c_void_p(0x1000)
    f3 = C.c_float * 3
    good = dict(pool=d, N=5, index=d, out=d, B=4, H=8, W=10, mean=f3(0.4, 0.5, 0.6), std=f3(0.2, 0.3, 0.4))
    ssr = (C.c_float * 5)(0.2, 0.1, 15.0, 0.7, 0.0)
    affine = (C.c_float * 5)(15.0, 0.2, 0.2, 0.8, 1.2)

    def plain(theta=None, apply=None, **kw):
        a = dict(good, **kw)
        return lib.d3f_pool_batch(a["pool"], a["N"], a["index"], a["out"], a["B"], a["H"], a["W"], a["mean"], a["std"], theta,
                                  apply, None)

    def rng(kind=1, params=ssr, **kw):
        a = dict(good, **kw)
        return lib.d3f_pool_batch_rng(a["pool"], a["N"], a["index"], a["out"], a["B"], a["H"], a["W"], a["mean"], a["std"],
                                      0x5EED, 3, kind, params, None)

    shared = ((dict(pool=None), b"pool"), (dict(index=None), b"index"), (dict(out=None), b"out"), (dict(mean=None), b"mean"),
              (dict(std=None), b"std"), (dict(N=0), b"N "), (dict(N=-4), b"N "), (dict(B=-1), b"B "), (dict(H=0), b"H "),
              (dict(W=0), b"W "), (dict(H=-2), b"H "), (dict(std=f3(0.2, 0.0, 0.4)), b"zero std"),
              (dict(std=f3(0.0, 0.3, 0.4)), b"zero std"), (dict(std=f3(0.2, 0.3, 0.0)), b"zero std"),
              (dict(H=32768, W=21846), b"2^31"),     # 32768 x 21846 x 3 = 2^31 + 65536 bytes
              (dict(H=46341, W=46341), b"2^31"))     # H x W itself passes 2^31
    for name, call in ((b"pool_batch:", plain), (b"pool_batch_rng:", rng)):
        for kw, word in shared:
            assert call(**kw) != 0, (name, kw)
            message = lib.d3f_last_error()
            assert message.startswith(name) and word in message, (name, kw, message)
    assert plain(apply=d) != 0 and b"apply without theta" in lib.d3f_last_error()
    for kw, word in ((dict(params=None), b"params"), (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"),
                     (dict(kind=0, params=(C.c_float * 5)(15.0, 0.2, 0.2, 0.0, 1.2)), b"scale range"),
                     (dict(kind=0, params=(C.c_float * 5)(15.0, 0.2, 0.2, 1.2, 0.8)), b"scale range"),
                     (dict(kind=1, params=(C.c_float * 5)(0.2, 1.0, 15.0, 0.7, 0.0)), b"scale_limit")):
        assert rng(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    # the largest image allowed passes the host checks of the shape (B = 0: nothing is launched)
    assert plain(B=0, H=32768, W=21845) == 0 and rng(B=0, kind=0, params=affine) == 0


class _Images(torch.utils.data.Dataset):
    """the host loader's dataset shape: items {"image", "index"}"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {"image": torch.full((2,), float(i)), "index": i}


def test_pool_loader_yields_the_host_loaders_index_batches():
    from torch.utils.data import DataLoader
    from denoising_diffusion_deep_fake_amd.trainer import CombinedLoader, _set_epoch, shard_loader
    N, bs, seed = 11, 4, 1234
    pool = DeviceImagePool(torch.zeros(N, 2, 2, 3, dtype=torch.uint8))
    assert len(pool) == N and pool.geometry == (2, 2)

    def batches(loader, epoch):
        _set_epoch(loader, epoch, seed)
        return [b["index"].tolist() for b in loader]

    for shuffle in (True, False):
        host = DataLoader(_Images(N), batch_size=bs, shuffle=shuffle)
        mine = pool.loader(bs, shuffle=shuffle)
        assert mine.num_workers == 0 and len(mine) == len(host) == 3
        for epoch in (0, 1, 5):
            got, want = batches(mine, epoch), batches(host, epoch)
            assert got == want and len(got[-1]) == 3 and sorted(sum(got, [])) == list(range(N))
            assert all(b["index"].dtype == torch.int64 and set(b) == {"index"} for b in mine)
        if shuffle:
            assert batches(mine, 0) != batches(mine, 1)
        for rank in (0, 1):
            host_r, mine_r = shard_loader(host, 2, rank, seed), shard_loader(mine, 2, rank, seed)
            for epoch in (0, 3):
                got = batches(mine_r, epoch)
                assert got == batches(host_r, epoch) and sum(len(b) for b in got) == 6
    # two domains in a CombinedLoader: each loader its own generator, as for the host loaders
    both = lambda make: CombinedLoader({"a": make(), "b": make()})  # noqa: E731
    combined, combined_host = both(lambda: pool.loader(bs)), both(lambda: DataLoader(_Images(N), batch_size=bs, shuffle=True))
    _set_epoch(combined, 2, seed)
    _set_epoch(combined_host, 2, seed)
    for got, want in zip(combined, combined_host):
        assert all(got[k]["index"].tolist() == want[k]["index"].tolist() for k in "ab")
    # an index the sampler cannot have made
    collate = pool.loader(bs).collate_fn
    assert collate([{"index": 0}, {"index": N - 1}])["index"].tolist() == [0, N - 1]
    for bad in (-1, N, N + 7):
        with pytest.raises(IndexError, match=str(bad)):
            collate([{"index": 0}, {"index": bad}])


def _image_list(root, sizes, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    (root / "images").mkdir(parents=True)
    images = []
    for i, (h, w) in enumerate(sizes):
        images.append(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        Image.fromarray(images[-1]).save(root / "images" / f"{i}.png")
    (root / "images.txt").write_text("".join(f"images/{i}.png\n" for i in range(len(sizes))))
    return root / "images.txt", images


def test_pool_refuses_unequal_images_and_a_pool_over_the_memory_fraction(tmp_path, monkeypatch):
    """the pool is filled into host memory (device "cpu") with torch.cuda.mem_get_info stood in for: no GPU needed"""
    free = [1 << 20]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (free[0], 1 << 30))
    path, images = _image_list(tmp_path / "ok", [(5, 7)] * 5)
    monkeypatch.setattr(DeviceImagePool, "CHUNK", 2)   # three copies, the last one short
    torch.manual_seed(3)
    before = torch.get_rng_state()
    pool = DeviceImagePool.from_list(path, "cpu")
    assert pool.images.shape == (5, 5, 7, 3) and np.array_equal(pool.images.numpy(), np.stack(images))
    assert torch.equal(torch.get_rng_state(), before)   # the fill draws nothing from the global generator
    # 5 x 105 = 525 bytes asked: allowed at half of 1050 bytes free, refused at half of 1049
    free[0] = 1050
    DeviceImagePool.from_list(path, "cpu")
    free[0] = 1049
    with pytest.raises(ValueError, match=r"525 bytes.*1049 bytes free"):
        DeviceImagePool.from_list(path, "cpu")
    DeviceImagePool.from_list(path, "cpu", max_fraction=0.9)
    hp = {"device_dataset_max_fraction": 0.9, "num_workers": 0}
    assert len(DeviceImagePool.from_hparams(hp, path, "cpu")) == 5
    with pytest.raises(ValueError, match="525 bytes"):
        DeviceImagePool.from_hparams({}, path, "cpu")
    free[0] = 1 << 20
    path, _ = _image_list(tmp_path / "unequal", [(5, 7), (5, 7), (5, 7), (7, 5), (5, 7)])
    with pytest.raises(ValueError, match=r"images/3\.png is 7x5.*images/0\.png is 5x7"):
        DeviceImagePool.from_list(path, "cpu")


def test_device_dataset_needs_an_image_list(tmp_path):
    from denoising_diffusion_deep_fake_amd.balance_training_images.lit_module import LitModule as Balance
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule as Fake
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule as Denoiser
    common = dict(batch_size=4, learning_rate=0.01, encoder_name="resnet18", num_workers=0, device_dataset=True)
    lists = {Denoiser: dict(input_image_list_path="images.txt"), Balance: dict(input_image_list_path="images.txt"),
             Fake: dict(data_path_a="a.txt", data_path_b="b.txt", mode="denoise")}
    for cls, paths in lists.items():
        with pytest.raises(ValueError, match="synthetic"):
            cls(**dict(common, synthetic=True, **paths))
        with pytest.raises(ValueError, match="image list"):
            cls(**dict(common, **{k: v for k, v in paths.items() if k == "mode"}))
    with pytest.raises(ValueError, match="image list"):
        Fake(**dict(common, mode="denoise", data_path_a="a.txt"))
    assert device_pool.check_hparams({"device_dataset": True}, "images.txt") is True
    assert device_pool.check_hparams({}, None) is False and device_pool.check_hparams({"device_dataset": False}, None) is False


def test_shipped_configs_do_not_turn_the_device_dataset_on():
    configs = sorted((ROOT / "denoising_diffusion_deep_fake_amd").rglob("*.yml"))
    assert len(configs) >= 4
    for config in configs:
        assert "device_dataset" not in config.read_text(), config
