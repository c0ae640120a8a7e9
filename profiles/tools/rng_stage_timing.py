"""The noise stage and the augmentation stage of a training step, torch-RNG path against device-RNG path (HIP events).

  noise  : randn_like + rand + d3f_noise_blend (`device_rng: false`)  vs  d3f_noise_blend_rng, at 16x3x256x256 and 8x3x256x256
  augment: ShiftScaleRotate's draws + theta + d3f_affine_warp + where vs  d3f_affine_warp_rng, at 8x3x256x256

Back-to-back enqueues of one stage on one stream, ITERS iterations after WARMUP, the two forms alternating in ROUNDS
rounds; the figure is the median round's time per call (device time when the launches keep the GPU busy, the host's
enqueue cost when they do not: what a step pays either way).
    python profiles/tools/rng_stage_timing.py
"""
import os
import statistics
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from denoising_diffusion_deep_fake_amd import _lib, ops
from denoising_diffusion_deep_fake_amd.dataset import synthetic_face_crops
from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import ShiftScaleRotate

WARMUP, ITERS, ROUNDS = 50, 200, 7
LAM, SEED = 5.0, 0x5EED


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(ITERS):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e3  # us per call


def compare(name, old, new):
    for i in range(WARMUP):
        old(i), new(i)
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(ROUNDS):
        t_old.append(timed(old))
        t_new.append(timed(new))
    a, b = statistics.median(t_old), statistics.median(t_new)
    print(f"{name:28s} torch RNG {a:8.1f} us (min {min(t_old):.1f}, max {max(t_old):.1f})   "
          f"device RNG {b:8.1f} us (min {min(t_new):.1f}, max {max(t_new):.1f})   x{a / b:.1f}")
    return a, b


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}")
    aug = ShiftScaleRotate(shift_limit=0.2, scale_limit=0.1, rotate_limit=15, p=0.7)
    for B in (16, 8):
        x = synthetic_face_crops(B, 256, seed=3, device="cuda")

        def noise_old(i):
            noise = torch.randn_like(x)
            y = torch.rand(size=(B, 1, 1, 1), device=x.device)
            return ops.noise_blend(x, noise, y.reshape(-1), LAM)

        compare(f"noise {B}x3x256x256", noise_old, lambda i: ops.noise_blend_rng(x, SEED, i << 24, LAM))
        if B == 8:
            compare(f"ShiftScaleRotate {B}x3x256x256", lambda i: aug(x), lambda i: aug(x, seed_offset=(SEED, i << 24)))


if __name__ == "__main__":
    main()
