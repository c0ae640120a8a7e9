"""Balanced sampling (`balanced_sampling: true`) on the MI355X: the index draw against its numpy restatement, the fused launch
against the entries it extends, the two trainers on the device path, and `d3f balance` -> `d3f denoise` end to end.

The reference has no sampler, so the oracle of the draw is restated here from the contract (csrc/philox.h, include/d3f_hip.h):
integers only, hence exact.  The images are compared with torch.equal against ops.pool_batch / ops.pool_batch_rng of the
restated indices, which tests/test_gpu_device_dataset.py ties to the unfused launches.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rng_restatement as rs

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SSR = (0.2, 0.1, 15.0, 0.7)                 # ShiftScaleRotate(shift_limit, scale_limit, rotate_limit, p)
RA = (15.0, 0.2, 0.2, 0.8, 1.2)             # RandomAffine(degrees, translate_x, translate_y, scale_lo, scale_hi)
KINDS = (("none", None), ("shift_scale_rotate", SSR), ("random_affine", RA))
SIZES = [1, 5, 0, 17, 40]                   # images per class; class 2 is empty
STREAMS = ((0x5EED, 0), (1234, 7 << 24 | 3 << 8 | 1), (0xDEADBEEFCAFEF00D, (1 << 39) + (5 << 24) + 1))   # (seed, offset)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from denoising_diffusion_deep_fake_amd import ops as o
    return o


def _tables():
    """name -> (members, class_start, N) on the host"""
    from denoising_diffusion_deep_fake_amd.dataset.balanced import balance_table
    five = [k for k, n in enumerate(SIZES) for _ in range(n)]
    return {"five classes, one empty": balance_table(five) + (63,),
            "one class": balance_table([4] * 11) + (11,),
            "9 of 23 images": balance_table([2, 0, 2, 5, 0, 2, 5, 0, 2], 23, [22, 3, 17, 0, 8, 11, 5, 20, 1]) + (23,)}


def restated_index(members, class_start, seed, offset, B):
    """the draw of include/d3f_hip.h in numpy: words 1 and 2 of block 0xFFFFFFFD of image b, two multiply-highs"""
    members, class_start = np.asarray(members, dtype=np.int64), np.asarray(class_start, dtype=np.int64)
    x = rs.block(seed, offset, np.arange(B), rs.G_APPLY)
    Kn = len(class_start) - 1
    j = ((x[1].astype(np.uint64) * np.uint64(Kn)) >> np.uint64(32)).astype(np.int64)
    cnt = class_start[j + 1] - class_start[j]
    m = ((x[2].astype(np.uint64) * cnt.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    return members[class_start[j] + m]


def _pool(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g).cuda()


# ---- the draw -------------------------------------------------------------------------------------------------------------
def test_index_draw_equals_the_restatement(ops):
    assert STREAMS[2][1] > 1 << 32
    for name, (members, class_start, N) in _tables().items():
        m, c = members.cuda(), class_start.cuda()
        for seed, offset in STREAMS:
            got = ops.balanced_index_draw(m, c, seed, offset, 37)
            assert got.dtype == torch.int64 and got.shape == (37,) and got.is_cuda
            want = restated_index(members.numpy(), class_start.numpy(), seed, offset, 37)
            assert np.array_equal(got.cpu().numpy(), want), (name, seed, offset)
            assert set(want.tolist()) <= set(members.tolist())
        assert ops.balanced_index_draw(m, c, 1, 2, 0).shape == (0,)
        draws = [ops.balanced_index_draw(m, c, s, o, 37).tolist() for s, o in STREAMS]
        assert draws[0] != draws[1] != draws[2]
    m, c, _ = _tables()["one class"]
    with pytest.raises(ValueError):
        ops.balanced_index_draw(m.cuda(), c.cuda().int(), 1, 2, 4)
    with pytest.raises(ValueError):
        ops.balanced_index_draw(m.cuda(), c[:1].cuda(), 1, 2, 4)


def test_device_draws_every_class_and_every_member_equally_often(ops):
    """256 steps of 64 draws = 16 384 over four non-empty classes: 4096 each, standard deviation sqrt(16384 * 1/4 * 3/4) =
    55.4, the bound five of them; a member of the class of 40 is expected 102.4 times (sd 10.1): 103 +- 51"""
    members, class_start, _ = _tables()["five classes, one empty"]
    m, c = members.cuda(), class_start.cuda()
    draws = torch.cat([ops.balanced_index_draw(m, c, 1234, step << 24, 64) for step in range(256)]).cpu()
    restated = np.concatenate([restated_index(members.numpy(), class_start.numpy(), 1234, step << 24, 64)
                               for step in range(256)])
    assert np.array_equal(draws.numpy(), restated)
    per_image = torch.bincount(draws, minlength=63)
    per_class = [int(per_image[a:b].sum()) for a, b in ((0, 1), (1, 6), (6, 23), (23, 63))]
    print("class counts", per_class, "members of the class of 40", int(per_image[23:].min()), int(per_image[23:].max()))
    assert sum(per_class) == 16384
    assert all(abs(n - 4096) <= 277 for n in per_class), per_class
    assert bool(((per_image[23:] - 103).abs() <= 51).all()), per_image[23:].tolist()


# ---- the fused launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (8, 8), (64, 64)])
def test_fused_launch_is_pool_batch_rng_of_the_drawn_index(ops, shape):
    """5x7: the byte path; 8x8: the dword path; 64x64: 16 workgroups per image, which all draw the same index, hand it over
    through LDS, and of which one writes index_out"""
    N = 23
    pool = _pool(N, *shape, seed=1)
    classes = [0] * 3 + [4] * 12 + [9] * 8
    from denoising_diffusion_deep_fake_amd.dataset.device_pool import DeviceImagePool
    table = DeviceImagePool(pool).balance_table(classes)
    assert table.Kn == 3 and table.members.is_cuda
    for B in (1, 9):
        for kind, params in KINDS:
            for seed, offset in STREAMS[:2]:
                batch, index = ops.pool_batch_balanced_rng(pool, table.members, table.class_start, B, MEAN, STD, seed, offset,
                                                           kind, params)
                assert batch.shape == (B, 3) + shape and batch.dtype == torch.float32
                assert index.shape == (B,) and index.dtype == torch.int64
                assert torch.equal(index, ops.balanced_index_draw(table.members, table.class_start, seed, offset, B))
                want = restated_index(table.members.cpu().numpy(), table.class_start.cpu().numpy(), seed, offset, B)
                assert np.array_equal(index.cpu().numpy(), want)
                if kind == "none":
                    ref = ops.pool_batch(pool, index, MEAN, STD)
                else:
                    ref = ops.pool_batch_rng(pool, index, MEAN, STD, seed, offset, kind, params)
                assert torch.equal(batch, ref), (B, kind, seed, offset)
                assert not torch.isnan(batch).any()
    # the augmentation did something, and the pool's own wrapper is the same launch
    plain, index = ops.pool_batch_balanced_rng(pool, table.members, table.class_start, 9, MEAN, STD, 5, 0, "none")
    warped, index2 = DeviceImagePool(pool).batch_balanced_rng(table, 9, MEAN, STD, 5, 0, "random_affine", RA)
    assert torch.equal(index, index2) and not torch.equal(plain, warped)
    empty, none = ops.pool_batch_balanced_rng(pool, table.members, table.class_start, 0, MEAN, STD, 5, 0, "none")
    assert empty.shape == (0, 3) + shape and none.shape == (0,)
    with pytest.raises(ValueError):
        ops.pool_batch_balanced_rng(pool, table.members, table.class_start, 2, MEAN, STD, 5, 0, "shear", RA)


def test_a_table_over_part_of_the_pool_draws_only_its_members(ops):
    members, class_start, N = _tables()["9 of 23 images"]
    pool = _pool(N, 8, 10, seed=2)
    batch, index = ops.pool_batch_balanced_rng(pool, members.cuda(), class_start.cuda(), 64, MEAN, STD, 77, 1 << 24, "none")
    assert set(index.tolist()) <= set(members.tolist()) and len(set(index.tolist())) > 5
    assert torch.equal(batch, ops.u8rgb_normalise(pool[index], MEAN, STD))


# ---- the trainers ---------------------------------------------------------------------------------------------------------
HP_DENOISER = dict(batch_size=6, learning_rate=0.02, max_epochs=1, cosine_scheduler_max_epoch=2, num_workers=0,
                   encoder_name="resnet18", noise_exponential_sampling_lambda=5, mean=[120, 128, 136], std=[60, 64, 68],
                   augment=True, device_dataset=True, device_rng=True, balanced_sampling=True)
HP_FAKE = dict(batch_size=6, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1, cosine_scheduler_max_epoch=50,
               num_workers=0, encoder_name="resnet18", noise_exponential_sampling_lambda=3, mean_a=[0.45, 0.5, 0.55],
               std_a=[0.5] * 3, mean_b=[0.55, 0.5, 0.45], std_b=[0.5] * 3, ema_beta=0.9999, ema_update_every=1, augment=True,
               mode="denoise", device_dataset=True, device_rng=True, balanced_sampling=True)
CLASSES = {"a": [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 3, 3], "b": [5] + [2] * 11}


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    """two lists of 12 JPEG images of 64x64, plain (`a`, `b`) and with classes written by hand (`a_classes`, `b_classes`)"""
    from PIL import Image
    root = tmp_path_factory.mktemp("lists")
    rng = np.random.default_rng(7)
    paths = {}
    for domain in "ab":
        (root / domain).mkdir()
        for i in range(12):
            low = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1).astype(np.int16)
            image = np.clip(low + rng.integers(-20, 21, size=(64, 64, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(image).save(root / domain / f"{i}.jpg", quality=90)
        (root / f"{domain}.txt").write_text("".join(f"{domain}/{i}.jpg\n" for i in range(12)))
        (root / f"{domain}_classes.txt").write_text("".join(f"{domain}/{i}.jpg\t{c}\n" for i, c in enumerate(CLASSES[domain])))
        paths[domain], paths[f"{domain}_classes"] = str(root / f"{domain}.txt"), str(root / f"{domain}_classes.txt")
    return paths


def _module_case(name, lists, **extra):
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule as Fake
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule as Denoiser
    if name == "train_denoiser":
        return Denoiser, dict(HP_DENOISER, input_image_list_path=lists["a_classes"], **extra)
    return Fake, dict(HP_FAKE, data_path_a=lists["a_classes"], data_path_b=lists["b_classes"],
                      pair_fused=name.endswith("pair fused"), **extra)


def _count(n):
    """what the pool's loader yields in this mode matters for its length only"""
    return {"index": torch.zeros(n, dtype=torch.int64, device="cuda")}


def test_step_images_are_the_restated_draws_of_the_step(ops, lists, monkeypatch):
    """train_denoiser: step_images at global_step 0 and 1, at batch sizes 6 and 2 (a ragged last batch) = the pool's images
    at the restated indices, normalised and warped by the step's own augmentation draws; with `balanced_sampling` absent the
    module takes today's path and launches no balanced kernel"""
    from denoising_diffusion_deep_fake_amd import rng
    cls, hp = _module_case("train_denoiser", lists, rng_seed=5)
    trainer = SimpleNamespace(global_step=0, global_rank=0, _base_seed=77, current_epoch=0, logger=None, optimizers=[])
    torch.manual_seed(0)
    lit = cls(**hp).cuda().train()
    lit.__dict__["trainer"] = trainer
    loader = lit.train_dataloader()
    assert len(loader) == 2 and lit._balance_table.Kn == 3 and lit._pool.classes == CLASSES["a"]
    table, aug = lit._balance_table, lit.shared_augmentation_sequence
    m, s = lit.mean_std_unit()
    seen = []
    for step, B in ((0, 6), (1, 6), (1, 2)):
        trainer.global_step = step
        seed, offset = rng.module_stream(lit)
        assert seed == 5 and offset == step << 24
        got = lit.step_images(_count(B))
        index = restated_index(table.members.cpu().numpy(), table.class_start.cpu().numpy(), seed, offset, B)
        x = ops.u8rgb_normalise(lit._pool.images[torch.from_numpy(index).cuda()], m, s)
        assert torch.equal(got, ops.affine_warp_rng(x, seed, offset, aug.KIND, aug.rng_params())), (step, B)
        seen.append(index.tolist())
    assert seen[0] != seen[1] and seen[2] == seen[1][:2]      # a function of (step, image), not of the batch size
    lit.hparams["augment"] = False
    assert torch.equal(lit.step_images(_count(2)), x)
    # balanced_sampling absent: the index batch is used, through the existing entry
    lit = cls(**{k: v for k, v in hp.items() if k != "balanced_sampling"}).cuda().train()
    lit.__dict__["trainer"] = trainer
    lit.train_dataloader()
    assert lit._balance_table is None

    def refuse(*args, **kwargs):
        raise AssertionError("the balanced launch without balanced_sampling")

    monkeypatch.setattr(ops, "pool_batch_balanced_rng", refuse)
    index = torch.tensor([11, 0, 3, 3], dtype=torch.int64, device="cuda")
    want = ops.pool_batch_rng(lit._pool.images, index, m, s, *rng.module_stream(lit), aug.KIND, aug.rng_params())
    assert torch.equal(lit.step_images({"index": index}), want)


@pytest.mark.parametrize("name", ["train_deep_fake pair fused", "train_deep_fake loop"])
def test_domain_images_are_the_restated_draws_of_each_domain(ops, lists, name):
    """train_deep_fake in denoise mode: each domain draws from its own classes on its own stream (0 / 1); the fused
    two-network step and the loop both run on these batches without a device-to-host copy or a wait"""
    from denoising_diffusion_deep_fake_amd import rng
    cls, hp = _module_case(name, lists, rng_seed=9)
    trainer = SimpleNamespace(global_step=1, global_rank=0, _base_seed=77, current_epoch=0, logger=None, optimizers=[])
    torch.manual_seed(0)
    lit = cls(**hp).cuda().train()
    lit.__dict__["trainer"] = trainer
    loaders = lit.train_dataloader()
    assert len(loaders["a"]) == len(loaders["b"]) == 2
    assert lit._balance_tables["a"].Kn == 3 and lit._balance_tables["b"].Kn == 2
    batch = {"a": _count(6), "b": _count(6)}
    drawn = {}
    for stream, key in enumerate("ab"):
        seed, offset = rng.module_stream(lit, stream)
        assert offset == 1 << 24 | stream
        table, mean = lit._balance_tables[key], hp[f"mean_{key}"]
        index = restated_index(table.members.cpu().numpy(), table.class_start.cpu().numpy(), seed, offset, 6)
        x = ops.u8rgb_normalise(lit._pools[key].images[torch.from_numpy(index).cuda()], mean, mean)
        want = ops.affine_warp_rng(x, seed, offset, lit.augmentation.KIND, lit.augmentation.rng_params())
        assert torch.equal(lit.domain_images(batch, key), want), key
        drawn[key] = index.tolist()
    assert drawn["a"] != drawn["b"]
    if name.endswith("pair fused"):
        assert lit.pair_fused_active(batch)
        steps = [lambda: lit.training_step_pair(batch, 0)[0]]
    else:
        assert not lit.pair_fused_active(batch)
        steps = [lambda: lit.training_step(batch, 0, 0), lambda: lit.training_step(batch, 0, 1)]
    for step in steps:
        step()                                # (first use: engines are built, workspaces allocated)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [step() for step in steps]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(loss) for loss in losses)


def _fit(cls, hp, root, **trainer_kw):
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    torch.manual_seed(11)
    lit = cls(**dict(hp, default_root_dir=str(root)))
    torch.manual_seed(12)
    kw = dict(max_epochs=1, log_every_n_steps=1, default_root_dir=root, enable_checkpointing=False, flush_every=100)
    tr = Trainer(**dict(kw, **trainer_kw)).fit(lit)
    torch.cuda.synchronize()
    return lit, tr


@pytest.mark.parametrize("name", ["train_denoiser", "train_deep_fake pair fused", "train_deep_fake loop"])
def test_resumed_balanced_run_continues_the_interrupted_one(lists, tmp_path, name):
    """one epoch = two batches of 6.  Stopped after the first by max_steps, checkpointed, resumed in a process state with
    another torch seed: the second batch is drawn and trained on as in the uninterrupted run, bit for bit"""
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    cls, hp = _module_case(name, lists)
    per_batch = 1 if name == "train_denoiser" else 2       # optimiser steps
    lit, tr = _fit(cls, hp, tmp_path / "straight")
    assert tr.global_step == 2 * per_batch
    straight = {k: v.detach().clone() for k, v in lit.state_dict().items()}
    lit, tr = _fit(cls, hp, tmp_path / "stopped", max_steps=per_batch)
    assert tr.global_step == per_batch and tr._batches_done == 1
    stopped = {k: v.detach().clone() for k, v in lit.state_dict().items()}
    assert any(not torch.equal(stopped[k], straight[k]) for k in straight)
    tr.save_checkpoint(tmp_path / "mid.ckpt")
    torch.manual_seed(12345)
    lit = cls.load_from_checkpoint(tmp_path / "mid.ckpt")
    assert lit.hparams["balanced_sampling"] is True
    tr = Trainer(max_epochs=1, default_root_dir=tmp_path / "resumed", enable_checkpointing=False).fit(
        lit, ckpt_path=tmp_path / "mid.ckpt")
    torch.cuda.synchronize()
    assert tr.global_step == 2 * per_batch
    resumed = lit.state_dict()
    assert resumed.keys() == straight.keys()
    for k in straight:
        assert torch.equal(resumed[k], straight[k]), k


def test_host_sampler_feeds_the_pool_without_device_rng(lists, tmp_path):
    """`device_dataset` without `device_rng`: the pool's loader carries a BalancedSampler and the existing launch gathers
    what it drew"""
    from denoising_diffusion_deep_fake_amd.dataset import BalancedSampler
    cls, hp = _module_case("train_denoiser", lists, rng_seed=5)
    lit = cls(**dict(hp, device_rng=False)).cuda().train()
    loader = lit.train_dataloader()
    assert isinstance(loader.sampler, BalancedSampler) and lit._balance_table is None and len(loader) == 2
    batches = [b["index"] for b in loader]
    assert [len(b) for b in batches] == [6, 6] and torch.cat(batches).tolist() == list(loader.sampler)
    lit.hparams["augment"] = False
    m, s = lit.mean_std_unit()
    index = batches[0].cuda()
    assert torch.equal(lit.step_images({"index": index}), lit._pool.batch(index, m, s))


# ---- d3f balance -> d3f denoise -------------------------------------------------------------------------------------------
def test_balance_output_list_trains_the_denoiser(lists, tmp_path):
    import yaml
    from click.testing import CliRunner
    from denoising_diffusion_deep_fake_amd.dataset import ImageDataset
    from denoising_diffusion_deep_fake_amd.main import cli
    out_list = str(ImageDataset(lists["a"]).image_list_path.parent / "a_from_balance.txt")   # next to the list it comes from
    common = dict(batch_size=4, learning_rate=0.01, max_epochs=1, num_workers=0, encoder_name="resnet18",
                  mean=[120, 128, 136], std=[60, 64, 68], device_dataset=True, device_rng=True, rng_seed=3)
    balance = dict(common, ratio_of_noise=0.7, number_of_classes=4, device_scoring=True,
                   default_root_dir=str(tmp_path / "balance"))
    denoise = dict(common, cosine_scheduler_max_epoch=2, noise_exponential_sampling_lambda=5, augment=True,
                   balanced_sampling=True, default_root_dir=str(tmp_path / "denoise"))
    (tmp_path / "balance.yml").write_text(yaml.safe_dump(balance))
    (tmp_path / "denoise.yml").write_text(yaml.safe_dump(denoise))
    runner = CliRunner()
    result = runner.invoke(cli, ["balance", "--config", str(tmp_path / "balance.yml"), "--input_list", lists["a"],
                                 "--output_list", out_list], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    written = ImageDataset(out_list)
    assert written.image_path_list == ImageDataset(lists["a"]).image_path_list
    assert len(written.image_class_list) == 12 and set(written.image_class_list) <= set(range(4))
    result = runner.invoke(cli, ["denoise", "--config", str(tmp_path / "denoise.yml"), "--input_list", out_list,
                                 "--max_steps", "1"], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    assert list((tmp_path / "denoise").rglob("metrics.csv"))
