"""Held-out validation: what the scores cost (HIP events, one process, every shape warmed up first).

    pair   : d3f_quality_per_image_scatter (quality_partial_kernel + quality_finalize_kernel) at 16x3x256x256, buffers
             allocated once, us per call
    route  : the only other way to the same numbers, one d3f_mse_ssim_loss call (ssim_fwd_kernel + ssim_mse_bwd_kernel +
             loss_finalize_kernel: the gradient comes along, and one value per batch instead of one per image)
             -- the two alternate within every round: median and spread of ROUNDS rounds of ITERS calls
    pass   : one validation pass of train_denoiser (resnet34, f32) over 96 held-out images at three ratios, batches of 16
             resident on the device (the host loader is not timed): 18 x (blend, eval-mode forward, scores) and the epoch's
             one copy and float64 means, ms per pass; and the same pass with the scores left out

    python profiles/tools/validation_cost.py
"""
import ctypes as C
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from denoising_diffusion_deep_fake_amd import _lib, ops
from denoising_diffusion_deep_fake_amd._lib import ptr, stream_ptr

B, SIZE, ITERS, ROUNDS, PASSES = 16, 256, 200, 9, 5


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def kernels():
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    target = torch.tanh(torch.randn(B, 3, SIZE, SIZE, generator=g)).cuda()
    pred = (target + 0.1 * torch.randn(B, 3, SIZE, SIZE, generator=g).cuda()).contiguous()
    metrics = torch.full((4, B), float("nan"), device="cuda")
    q_ws = torch.empty(L.d3f_quality_per_image_workspace_bytes(B, SIZE, SIZE), dtype=torch.uint8, device="cuda")
    l_ws = torch.empty(L.d3f_mse_ssim_loss_workspace_bytes(B, SIZE, SIZE), dtype=torch.uint8, device="cuda")
    out, grad = torch.empty(3, device="cuda"), torch.empty_like(pred)
    s = stream_ptr()
    forms = {
        "quality_per_image (partial + finalize)": lambda: _lib.check(L.d3f_quality_per_image_scatter(
            ptr(pred), ptr(target), -1.0, 1.0, None, ptr(metrics), B, ptr(q_ws), B, SIZE, SIZE, s)),
        "mse_ssim_loss (fwd + bwd + finalize)": lambda: _lib.check(L.d3f_mse_ssim_loss(
            ptr(pred), ptr(target), -1.0, 1.0, ptr(out), ptr(grad), ptr(l_ws), B, SIZE, SIZE, s)),
    }
    for fn in forms.values():
        events(fn, 50)
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(events(fn, ITERS) * 1e3)
    # the two routes give the same numbers: batch means of the per-image rows against the criterion's
    agree = {"mse": abs(float(metrics[0].double().mean()) - float(out[1])), "ssim": abs(float(metrics[1].double().mean()) - float(out[2]))}
    return {k: spread(v) for k, v in times.items()}, agree, (q_ws.numel(), l_ws.numel())


def validation_pass():
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
    torch.manual_seed(0)
    lit = LitModule(batch_size=B, learning_rate=0.02, max_epochs=1, cosine_scheduler_max_epoch=1, num_workers=0,
                    encoder_name="resnet34", noise_exponential_sampling_lambda=5, mean=[128] * 3, std=[128] * 3, synthetic=True,
                    image_size=SIZE, augment=False, precision="f32", val_synthetic_length=96).cuda().eval()
    batches = [{k: v.cuda() for k, v in b.items()} for b in lit.val_dataloader()]
    assert len(batches) == 6 and len(lit._val["ratios"]) == 3

    def whole():
        with torch.no_grad():
            for i, batch in enumerate(batches):
                lit.validation_step(batch, i)
        lit.validation_epoch_end([])

    real = ops.quality_per_image

    def timed(fn):
        fn()
        fn()
        return [events(fn, 1) for _ in range(PASSES)]

    with_scores = timed(whole)
    logged = {k: round(v, 5) for k, v in lit._logged.items() if k in ("val/loss", "val/mse", "val/ssim", "val/psnr")}
    ops.quality_per_image = lambda *a, **kw: kw["out"]  # the same pass with the scores left out
    try:
        without = timed(whole)
    finally:
        ops.quality_per_image = real
    return spread(with_scores, 3), spread(without, 3), logged


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}", flush=True)
    times, agree, ws = kernels()
    for k, v in times.items():
        print(f"{k:42s} median {v['median']:7.2f} us   min {v['min']:7.2f}   max {v['max']:7.2f}", flush=True)
    print(f"workspace bytes: quality {ws[0]}, criterion {ws[1]}; |batch mean - criterion|: mse {agree['mse']:.2e}, ssim {agree['ssim']:.2e}")
    on, off, logged = validation_pass()
    print(f"validation pass, 96 images x 3 ratios: median {on['median']:.3f} ms (min {on['min']:.3f}, max {on['max']:.3f}); "
          f"without the scores {off['median']:.3f} ms (min {off['min']:.3f}, max {off['max']:.3f}); {logged}", flush=True)
    print(json.dumps({"kernels_us": times, "pass_ms": on, "pass_without_scores_ms": off, "workspace_bytes": ws}), flush=True)


if __name__ == "__main__":
    main()
