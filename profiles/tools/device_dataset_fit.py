"""`device_dataset: true` end to end: Trainer.fit on the train_denoiser module at 256x256, bs 16, f32 and bf16, three ways in
one process --
    resident : the same step on one batch that already lies on the device (what `python bench.py` times)
    files    : `uint8_batches: true`, `num_workers: 8`, pinned -- the best path from files (profiles/README.md, round 5)
    pool     : `device_dataset: true` -- the list decoded once into a uint8 pool in HBM, batches of indices
-- with the pool's fill time, and the fused launch against the two launches it replaces (HIP events).

The image list (FILES JPEG files of SIZE x SIZE, written with PIL into a temporary directory) is the same for `files` and
`pool`; augmentation is on; `--device-rng on|off` (default on: the pool's batch is then ONE launch) applies to all three.
    python profiles/tools/device_dataset_fit.py [--steps 150] [--warmup 30] [--files 512] [--device-rng on]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import tempfile
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch
from denoising_diffusion_deep_fake_amd import _lib, ops
from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
from denoising_diffusion_deep_fake_amd.trainer import Callback, Trainer

SIZE, BATCH, SEED = 256, 16, 0x5EED
RA = (15.0, 0.2, 0.2, 0.8, 1.2)


def write_image_list(root, files):
    from PIL import Image
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "images"))
    names = []
    for i in range(files):  # smooth content + grain: JPEG files of a realistic size
        low = rng.integers(0, 256, size=(SIZE // 16, SIZE // 16, 3), dtype=np.uint8)
        image = np.asarray(Image.fromarray(low).resize((SIZE, SIZE), Image.BILINEAR)).astype(np.int16)
        image = np.clip(image + rng.integers(-12, 13, size=image.shape), 0, 255).astype(np.uint8)
        Image.fromarray(image).save(os.path.join(root, "images", f"{i}.jpg"), quality=90)
        names.append(f"images/{i}.jpg")
    with open(os.path.join(root, "images.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return os.path.join(root, "images.txt")


class Clock(Callback):
    def __init__(self, warmup, total):
        self.warmup, self.total, self.n, self.t0, self.t1 = warmup, total, 0, None, None

    def on_train_batch_end(self, trainer, module):
        self.n += 1
        if self.n == self.warmup:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()
        elif self.n == self.total:
            torch.cuda.synchronize()
            self.t1 = time.perf_counter()


def fit(way, dtype, path, args):
    """-> images/s through Trainer.fit, images/s of the same step on a resident batch, pool fill seconds (pool only)"""
    torch.manual_seed(0)
    hp = dict(batch_size=BATCH, learning_rate=0.02, max_epochs=10 ** 6, cosine_scheduler_max_epoch=10 ** 6, num_workers=8,
              encoder_name="resnet34", noise_exponential_sampling_lambda=5, mean=[128, 128, 128], std=[128, 128, 128],
              augment=True, precision=dtype, input_image_list_path=path, pin_memory=True,
              device_rng=args.device_rng == "on", **({"device_dataset": True} if way == "pool" else {"uint8_batches": True}))
    lit = LitModule(**hp).cuda()
    fill = None
    if way == "pool":
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lit.train_dataloader()  # fills the pool; Trainer.fit's own call finds it
        torch.cuda.synchronize()
        fill = time.perf_counter() - t0
    total = args.warmup + args.steps
    clock = Clock(args.warmup, total)
    with tempfile.TemporaryDirectory() as tmp:
        tr = Trainer(max_epochs=10 ** 6, max_steps=total, callbacks=[clock], enable_checkpointing=False, default_root_dir=tmp,
                     log_every_n_steps=50)
        tr.fit(lit)
    fit_rate = BATCH * args.steps / (clock.t1 - clock.t0)
    (opt,) = tr.optimizers
    x = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    batch = {"image": lit.normalise_on_device(x), "index": None}

    def step():
        opt.zero_grad(set_to_none=True)
        lit.training_step(batch, 0).backward()
        opt.step()
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    n = min(args.steps, 100)
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    resident_rate = BATCH * n / (time.perf_counter() - t0)
    del tr, lit, opt
    gc.collect()  # (the persistent loader workers end with their loader)
    return fit_rate, resident_rate, fill


def launch_timing():
    """the fused launch against u8rgb_normalise + affine_warp_rng on a contiguous uint8 batch (what the copy from the host
    leaves), 16x3x256x256, from a pool larger than the Infinity Cache; us per call, median of ROUNDS rounds"""
    N, ITERS, ROUNDS = 2048, 200, 7  # 2048 x 196 608 B = 403 MB
    pool = torch.randint(0, 256, (N, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(1)
    index = [torch.randperm(N, generator=g)[:BATCH].cuda() for _ in range(ITERS)]
    m, s = [0.5] * 3, [0.5] * 3

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ITERS):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ITERS * 1e3

    def contiguous(i):
        k = (i * BATCH) % (N - BATCH)
        return pool[k:k + BATCH]

    forms = {
        "plain: u8rgb_normalise": lambda i: ops.u8rgb_normalise(contiguous(i), m, s),
        "plain: pool_batch": lambda i: ops.pool_batch(pool, index[i], m, s),
        "rng: u8rgb_normalise + affine_warp_rng":
            lambda i: ops.affine_warp_rng(ops.u8rgb_normalise(contiguous(i), m, s), SEED, i << 24, "random_affine", RA),
        "rng: pool_batch_rng": lambda i: ops.pool_batch_rng(pool, index[i], m, s, SEED, i << 24, "random_affine", RA),
    }
    for fn in forms.values():
        for i in range(20):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    return {k: round(statistics.median(v), 2) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--device-rng", dest="device_rng", choices=("on", "off"), default="on")
    ap.add_argument("--dtypes", default="f32,bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}, "
          f"device_rng {args.device_rng}", flush=True)
    out = {"device_rng": args.device_rng, "steps": args.steps, "files": args.files, "fit": {}}
    with tempfile.TemporaryDirectory() as root:
        path = write_image_list(root, args.files)
        for dtype in args.dtypes.split(","):
            row = {}
            for way in ("files", "pool"):
                rate, resident, fill = fit(way, dtype, path, args)
                row[way] = {"fit_images_per_sec": round(rate, 1), "resident_images_per_sec": round(resident, 1),
                            "fit_over_resident": round(rate / resident, 4)}
                if fill is not None:
                    row[way]["pool_fill_seconds"] = round(fill, 2)
                print(f"{dtype:5s} {way:6s} fit {rate:8.1f} images/s   resident {resident:8.1f}   fit / resident "
                      f"{rate / resident:.3f}" + (f"   pool of {args.files} images filled in {fill:.2f} s" if fill else ""),
                      flush=True)
            out["fit"][dtype] = row
    out["launch_us"] = launch_timing()
    for k, v in out["launch_us"].items():
        print(f"{k:42s} {v:8.2f} us", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
