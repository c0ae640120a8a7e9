"""`balanced_sampling: true` on the device path: what the index draw inside the batch's launch costs.

    launch : ops.pool_batch_balanced_rng against ops.pool_batch_rng at 16x3x256x256 from a pool larger than the Infinity
             Cache (HIP events, us per call, median and spread of ROUNDS rounds).  `--parent-lib PATH` times pool_batch_rng
             of another build of the library (the parent commit's) in a child process of the same run.
    fit    : Trainer.fit on the train_denoiser module from the pool (`device_dataset` + `device_rng`, f32, bs 16, 256x256)
             with and without `balanced_sampling`, images/s.

    python profiles/tools/balanced_sampling_timing.py [--steps 100] [--warmup 20] [--files 512] [--parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from device_dataset_fit import BATCH, RA, SEED, SIZE, Clock, write_image_list
from denoising_diffusion_deep_fake_amd import _lib, ops
from denoising_diffusion_deep_fake_amd.dataset.balanced import balance_table

N, ITERS, ROUNDS = 2048, 200, 9  # 2048 x 196 608 B = 403 MB


def launch_timing(balanced):
    pool = torch.randint(0, 256, (N, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(1)
    index = [torch.randperm(N, generator=g)[:BATCH].cuda() for _ in range(ITERS)]
    m, s = [0.5] * 3, [0.5] * 3
    forms = {"pool_batch_rng": lambda i: ops.pool_batch_rng(pool, index[i], m, s, SEED, i << 24, "random_affine", RA)}
    if balanced:
        classes = torch.randint(0, 64, (N,), generator=g) ** 2 // 64  # 64 classes of unequal size
        members, class_start = (t.cuda() for t in balance_table(classes))
        forms["pool_batch_balanced_rng"] = lambda i: ops.pool_batch_balanced_rng(pool, members, class_start, BATCH, m, s, SEED,
                                                                                 i << 24, "random_affine", RA)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ITERS):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ITERS * 1e3

    for fn in forms.values():
        for i in range(20):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in times.items()}


def fit(path, balanced, args):
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    torch.manual_seed(0)
    hp = dict(batch_size=BATCH, learning_rate=0.02, max_epochs=10 ** 6, cosine_scheduler_max_epoch=10 ** 6, num_workers=8,
              encoder_name="resnet34", noise_exponential_sampling_lambda=5, mean=[128, 128, 128], std=[128, 128, 128],
              augment=True, precision="f32", input_image_list_path=path, pin_memory=True, device_rng=True,
              device_dataset=True, **({"balanced_sampling": True} if balanced else {}))
    lit = LitModule(**hp).cuda()
    total = args.warmup + args.steps
    clock = Clock(args.warmup, total)
    with tempfile.TemporaryDirectory() as tmp:
        Trainer(max_epochs=10 ** 6, max_steps=total, callbacks=[clock], enable_checkpointing=False, default_root_dir=tmp,
                log_every_n_steps=50).fit(lit)
    return BATCH * args.steps / (clock.t1 - clock.t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--parent-lib", dest="parent_lib", default=None)
    ap.add_argument("--launch-only", dest="launch_only", action="store_true", help="(the child of --parent-lib)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.launch_only:
        print(json.dumps(launch_timing(balanced=False)), flush=True)
        return
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}", flush=True)
    out = {"launch_us": launch_timing(balanced=True)}
    if args.parent_lib:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--launch-only"], check=True, text=True,
                               capture_output=True, timeout=300, env=dict(os.environ, D3F_LIB=os.path.abspath(args.parent_lib)))
        out["launch_us"]["pool_batch_rng (parent library)"] = json.loads(child.stdout.strip().splitlines()[-1])["pool_batch_rng"]
    for k, v in out["launch_us"].items():
        print(f"{k:34s} median {v['median_us']:7.2f} us   min {v['min_us']:7.2f}   max {v['max_us']:7.2f}", flush=True)
    with tempfile.TemporaryDirectory() as root:
        path = write_image_list(root, args.files)
        with open(path) as f:
            names = f.read().split()
        with open(os.path.join(root, "images_classes.txt"), "w") as f:  # ten classes of unequal size
            f.write("".join(f"{name}\t{(i % 100) ** 2 // 1000}\n" for i, name in enumerate(names)))
        out["fit_images_per_sec"] = {}
        for key, balanced in (("plain", False), ("balanced_sampling", True), ("plain again", False)):
            rate = fit(os.path.join(root, "images_classes.txt"), balanced, args)
            out["fit_images_per_sec"][key] = round(rate, 1)
            print(f"Trainer.fit {key:18s} {rate:8.1f} images/s", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
