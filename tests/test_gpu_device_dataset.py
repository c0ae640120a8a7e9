"""Device dataset (`device_dataset: true`) on the MI355X: ops.pool_batch / ops.pool_batch_rng against the launches they fuse,
and the three LitModules trained from a pool against the same run from files.

Every comparison is torch.equal: the fused kernel instantiates the sampling and theta functions of the warp kernels and the
normalisation of u8rgb_to_nchw_kernel (csrc/pointwise.h), with contraction off -- the same fp32 operations in the same order.
"""
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # asymmetric: a swapped channel shows
SEED = 0x5EED
SSR = (0.2, 0.1, 15.0, 0.7)                 # ShiftScaleRotate(shift_limit, scale_limit, rotate_limit, p)
RA = (15.0, 0.2, 0.2, 0.8, 1.2)             # RandomAffine(degrees, translate_x, translate_y, scale_lo, scale_hi)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from denoising_diffusion_deep_fake_amd import ops as o
    return o


def _pool(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g).cuda()


def _index(values):
    return torch.tensor(values, dtype=torch.int64, device="cuda")


# ---- operator level -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (8, 10), (32, 32)])
def test_plain_form_is_the_normalise_of_the_gathered_images(ops, shape):
    """5x7: the image bytes (105) are no multiple of 4, so image bases are unaligned; 8x10: the row bytes (30) are not;
    32x32: several workgroups per image and the dword path"""
    pool = _pool(5, *shape, seed=1)
    index = _index([4, 0, 4, 2])            # unsorted, with a repeat
    got = ops.pool_batch(pool, index, MEAN, STD)
    want = ops.u8rgb_normalise(pool[index], MEAN, STD)
    assert got.shape == (4, 3) + shape and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert not torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    empty = ops.pool_batch(pool, _index([]), MEAN, STD)
    assert empty.shape == (0, 3) + shape
    assert ops.pool_batch_rng(pool, _index([]), MEAN, STD, SEED, 0, "random_affine", RA).shape == (0, 3) + shape
    with pytest.raises(ValueError):
        ops.pool_batch(pool, index.int(), MEAN, STD)
    with pytest.raises(ValueError):
        ops.pool_batch(pool, index, MEAN, STD, apply=torch.ones(4, dtype=torch.bool, device="cuda"))


@pytest.mark.parametrize("shape", [(8, 10), (32, 48)])
def test_theta_form_is_where_apply_warp_plain(ops, shape):
    pool = _pool(5, *shape, seed=2)
    index = _index([4, 0, 4, 2])
    x = ops.u8rgb_normalise(pool[index], MEAN, STD)
    a, s = math.radians(25.0), 1.0 / 0.9
    thetas = {"identity": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
              "rotation with scale": [[s * math.cos(a), -s * math.sin(a), 0.1], [s * math.sin(a), s * math.cos(a), -0.05]],
              "out of frame": [[1.0, 0.0, 5.0], [0.0, 1.0, 0.0]]}
    applies = {"all": [1, 1, 1, 1], "none": [0, 0, 0, 0], "mixed": [1, 0, 0, 1], "null": None}
    for name, t in thetas.items():
        theta = torch.tensor([t] * 4, dtype=torch.float32, device="cuda")
        theta[1] *= 0.97                      # (the images of a batch do not share a theta)
        warped = ops.affine_warp(x, theta)
        if name == "out of frame":
            assert not warped.any()           # every tap outside the frame: zeros
        else:
            assert not torch.equal(warped, x)
        for how, apply in applies.items():
            if apply is None:
                got, want = ops.pool_batch(pool, index, MEAN, STD, theta=theta), warped
            else:
                apply = torch.tensor(apply, dtype=torch.bool, device="cuda")
                got = ops.pool_batch(pool, index, MEAN, STD, theta=theta, apply=apply)
                want = torch.where(apply.reshape(-1, 1, 1, 1), warped, x)
                assert torch.equal(ops.pool_batch(pool, index, MEAN, STD, theta=theta, apply=apply.to(torch.uint8)), want)
            assert torch.equal(got, want), (name, how)
    # one batch with a theta of each kind
    theta = torch.tensor([thetas["identity"], thetas["rotation with scale"], thetas["out of frame"],
                          thetas["rotation with scale"]], dtype=torch.float32, device="cuda")
    assert torch.equal(ops.pool_batch(pool, index, MEAN, STD, theta=theta), ops.affine_warp(x, theta))


def test_rng_form_is_affine_warp_rng_of_the_plain_batch(ops):
    B, H, W = 64, 32, 48
    pool = _pool(9, H, W, seed=3)
    index = torch.randint(0, 9, (B,), generator=torch.Generator().manual_seed(4)).cuda()
    x = ops.u8rgb_normalise(pool[index], MEAN, STD)
    for kind, params, offset in (("random_affine", RA, 0), ("shift_scale_rotate", SSR, 0), ("shift_scale_rotate", SSR, 7 << 24)):
        _, apply = ops.affine_theta_draw(SEED, offset, kind, params, B, H, W)
        if kind == "shift_scale_rotate":      # p = 0.7: both branches of the kernel run
            assert apply.any() and not apply.all()
        else:
            assert apply.all()
        got = ops.pool_batch_rng(pool, index, MEAN, STD, SEED, offset, kind, params)
        assert torch.equal(got, ops.affine_warp_rng(x, SEED, offset, kind, params)), (kind, offset)
        passed = ~apply
        assert torch.equal(got[passed], x[passed]) and not torch.equal(got[apply], x[apply])


def test_image_bases_are_64_bit(ops):
    """5 462 images of 512x512x3 are 4.295e9 bytes, just over 2^32: image 2 730 straddles 2^31, 2 731 lies behind it,
    5 461 (the last) straddles 2^32.  The pool is allocated and not filled; only the gathered images get bytes."""
    if torch.cuda.mem_get_info()[0] < 8e9:
        pytest.skip("needs 8 GB of free device memory")
    N, H, W = 5462, 512, 512
    assert N * H * W * 3 > 1 << 32 and 2730 * H * W * 3 < 1 << 31 < 2731 * H * W * 3 and 5461 * H * W * 3 < 1 << 32
    pool = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    picks = [0, 2730, 2731, 5461, 5460]
    g = torch.Generator().manual_seed(5)
    for i in picks:
        pool[i] = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).cuda()
    got = ops.pool_batch(pool, _index(picks), MEAN, STD)
    for k, i in enumerate(picks):
        assert torch.equal(got[k:k + 1], ops.u8rgb_normalise(pool[i:i + 1], MEAN, STD)), i
    assert len({got[k].sum().item() for k in range(len(picks))}) == len(picks)   # five different images
    theta = torch.tensor([[[0.9, 0.1, 0.05], [-0.1, 0.9, 0.0]]] * 5, dtype=torch.float32, device="cuda")
    assert torch.equal(ops.pool_batch(pool, _index(picks), MEAN, STD, theta=theta), ops.affine_warp(got, theta))
    del pool, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(5, 7), (32, 32)])
def test_an_index_outside_the_pool_gives_a_nan_image_and_leaves_the_neighbours(ops, shape):
    pool = _pool(5, *shape, seed=6)
    index = _index([4, -1, 0, 5, 2])
    want = ops.u8rgb_normalise(pool[_index([4, 0, 0, 0, 2])], MEAN, STD)
    theta = torch.tensor([[[0.9, 0.1, 0.05], [-0.1, 0.9, 0.0]]] * 5, dtype=torch.float32, device="cuda")
    for got, ref in ((ops.pool_batch(pool, index, MEAN, STD), want),
                     (ops.pool_batch(pool, index, MEAN, STD, theta=theta), ops.affine_warp(want, theta)),
                     (ops.pool_batch_rng(pool, index, MEAN, STD, SEED, 0, "random_affine", RA),
                      ops.affine_warp_rng(want, SEED, 0, "random_affine", RA))):
        assert torch.isnan(got[1]).all() and torch.isnan(got[3]).all()
        for k in (0, 2, 4):
            assert torch.equal(got[k], ref[k]), k


# ---- module level ---------------------------------------------------------------------------------------------------------
HP_DENOISER = dict(batch_size=4, learning_rate=0.02, max_epochs=1, cosine_scheduler_max_epoch=2, num_workers=0,
                   encoder_name="resnet18", noise_exponential_sampling_lambda=5, mean=[120, 128, 136], std=[60, 64, 68],
                   augment=True, uint8_batches=True)
HP_FAKE = dict(batch_size=4, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1, cosine_scheduler_max_epoch=50,
               num_workers=0, encoder_name="resnet18", noise_exponential_sampling_lambda=3, mean_a=[0.45, 0.5, 0.55],
               std_a=[0.5] * 3, mean_b=[0.55, 0.5, 0.45], std_b=[0.5] * 3, ema_beta=0.9999, ema_update_every=1, augment=True,
               uint8_batches=True)
HP_BALANCE = dict(batch_size=4, learning_rate=0.01, max_epochs=1, num_workers=0, encoder_name="resnet18", ratio_of_noise=0.7,
                  number_of_classes=4, mean=[120, 128, 136], std=[60, 64, 68])


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    """two image lists of 6 lossless 64x64 images each: at batch 4 the last batch is ragged"""
    from PIL import Image
    root = tmp_path_factory.mktemp("lists")
    rng = np.random.default_rng(7)
    paths = {}
    for domain in "ab":
        (root / domain).mkdir()
        for i in range(6):
            low = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1).astype(np.int16)
            image = np.clip(low + rng.integers(-20, 21, size=(64, 64, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(image).save(root / domain / f"{i}.png")
        (root / f"{domain}.txt").write_text("".join(f"{domain}/{i}.png\n" for i in range(6)))
        paths[domain] = str(root / f"{domain}.txt")
    return paths


def _module_case(name, lists):
    from denoising_diffusion_deep_fake_amd.balance_training_images.lit_module import LitModule as Balance
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule as Fake
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule as Denoiser
    if name == "train_denoiser":
        return Denoiser, dict(HP_DENOISER, input_image_list_path=lists["a"])
    if name == "balance_training_images":
        return Balance, dict(HP_BALANCE, input_image_list_path=lists["a"])
    return Fake, dict(HP_FAKE, mode=name.split()[-1], data_path_a=lists["a"], data_path_b=lists["b"])


def _fit(cls, hp, root, **trainer_kw):
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    torch.manual_seed(11)
    lit = cls(**dict(hp, default_root_dir=str(root)))
    torch.manual_seed(12)
    kw = dict(max_epochs=1, log_every_n_steps=1, default_root_dir=root, enable_checkpointing=False, flush_every=100)
    tr = Trainer(**dict(kw, **trainer_kw)).fit(lit)
    torch.cuda.synchronize()
    return lit, tr


@pytest.mark.parametrize("device_rng", [False, True])
@pytest.mark.parametrize("name", ["train_denoiser", "train_deep_fake denoise", "train_deep_fake swap",
                                  "balance_training_images"])
def test_fit_from_the_pool_equals_fit_from_files(name, device_rng, lists, tmp_path):
    """one epoch of Trainer.fit (two batches, the second ragged) with `device_dataset: true` against the same run from
    files (`uint8_batches: true` where the module has it, the default loader for balance): every logged value and the final
    state_dict equal; for balance the difficulty classes too.  "train_deep_fake denoise" takes the fused two-network route."""
    cls, hp = _module_case(name, lists)
    hp = dict(hp, device_rng=device_rng, rng_seed=5)
    results = []
    for pool in (False, True):
        lit, tr = _fit(cls, dict(hp, device_dataset=True) if pool else hp, tmp_path / f"pool{int(pool)}")
        assert tr.global_step == (4 if "deep_fake" in name else 2)
        rows = (tr.log_dir / "metrics.csv").read_text().splitlines()
        assert len(rows) == 2 and all(re.search(r"loss[^=]*=[-+0-9.e]+", row) for row in rows)
        state = {k: v.detach().clone() for k, v in lit.state_dict().items()}
        results.append((rows, state, getattr(lit, "difficulty_index", None)))
        if pool:
            pools = [lit._pool] if hasattr(lit, "_pool") else [lit._pools["a"], lit._pools["b"]]
            assert all(p.images.shape == (6, 64, 64, 3) and p.images.is_cuda for p in pools)
            assert not any(k.startswith("_pool") for k in state)
        if name == "train_deep_fake denoise":
            assert lit._pair is not None      # the fused two-network route ran
    (rows_f, state_f, classes_f), (rows_p, state_p, classes_p) = results
    assert rows_p == rows_f
    assert state_p.keys() == state_f.keys()
    for k in state_f:
        assert torch.equal(state_p[k], state_f[k]), k
    if name == "balance_training_images":
        assert classes_f is not None and len(classes_f[0]) == 6
        assert torch.equal(classes_p[0], classes_f[0]) and torch.equal(classes_p[1], classes_f[1])


def test_pool_path_of_training_step_does_not_synchronise(lists):
    """`device_rng: true`: between the index batch and the loss nothing copies to the host or waits"""
    trainer = SimpleNamespace(global_step=3, global_rank=0, _base_seed=77, current_epoch=0, logger=None, optimizers=[])
    for name in ("train_denoiser", "train_deep_fake denoise", "train_deep_fake swap", "balance_training_images"):
        cls, hp = _module_case(name, lists)
        torch.manual_seed(0)
        lit = cls(**dict(hp, device_dataset=True, device_rng=True)).cuda().train()
        lit.__dict__["trainer"] = trainer
        lit.train_dataloader()
        part = lambda values: {"index": _index(values)}  # noqa: E731
        if "deep_fake" in name:
            batch = {"a": part([5, 0, 3, 3]), "b": part([1, 2, 4, 0])}
            steps = [lambda: lit.training_step(batch, 0, 0), lambda: lit.training_step(batch, 0, 1)]
            if name.endswith("denoise"):
                assert lit.pair_fused_active(batch)
                steps.append(lambda: lit.training_step_pair(batch, 0)[0])
            else:
                assert not lit.pair_fused_active(batch)
        else:
            batch = part([5, 0, 3, 3])
            steps = [lambda: lit.training_step(batch, 0)]
        for step in steps:
            step()                            # (first use: engines are built, workspaces allocated)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = [step() for step in steps]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(torch.isfinite(loss) for loss in losses), name


def test_resumed_pool_run_continues_the_interrupted_one(lists, tmp_path):
    """train_denoiser from the pool under `device_rng: true`: stopped after batch 1 by max_steps, checkpointed, resumed in a
    process state with another torch seed -- the second batch is the one the uninterrupted run trained on"""
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    cls, hp = _module_case("train_denoiser", lists)
    hp = dict(hp, device_dataset=True, device_rng=True)
    lit, tr = _fit(cls, hp, tmp_path / "straight")
    assert tr.global_step == 2
    straight = {k: v.detach().clone() for k, v in lit.state_dict().items()}
    lit, tr = _fit(cls, hp, tmp_path / "stopped", max_steps=1)
    assert tr.global_step == 1 and tr._batches_done == 1
    tr.save_checkpoint(tmp_path / "mid.ckpt")
    torch.manual_seed(12345)
    lit = cls.load_from_checkpoint(tmp_path / "mid.ckpt")
    assert lit.hparams["device_dataset"] is True
    tr = Trainer(max_epochs=1, default_root_dir=tmp_path / "resumed", enable_checkpointing=False).fit(
        lit, ckpt_path=tmp_path / "mid.ckpt")
    torch.cuda.synchronize()
    assert tr.global_step == 2
    resumed = lit.state_dict()
    assert resumed.keys() == straight.keys()
    for k in straight:
        assert torch.equal(resumed[k], straight[k]), k
