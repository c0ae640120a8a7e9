"""The training image grid (ops.image_grid_u8, csrc/image_grid.hip) against its restatement with torch ops on the device
(HIP events, device resident), at the two shapes a logging step meets:

  4 tags x 9 x 3 x 256 x 256   : the fused denoise pair / one swap-mode optimizer step at the benchmark size
  1 tag  x 9 x 3 x 448 x 448   : one tag at the authors' size

  kernel       : ONE launch for all tags of the call
  torch ops    : per tag new_full + 9 slice copies (make_grid) + mul + add + clamp + nan_to_num + mul + to(uint8) +
                 permute().contiguous() -- what log_batch_as_image_grid costs when it is written with tensor ops

Back-to-back enqueues on one stream, ITERS iterations after WARMUP, the forms alternating in ROUNDS rounds; the figure is
the median round's time per call.  The device-to-host copy and the PNG encode are the same for both and not part of any
figure.  The two forms are compared byte for byte first.  One JSON line at the end.
    python profiles/tools/image_grid.py [--iters N]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from denoising_diffusion_deep_fake_amd import _lib, ops

CASES = {"4tags_9x3x256x256": (4, (9, 3, 256, 256)), "1tag_9x3x448x448": (1, (9, 3, 448, 448))}


def torch_grid_u8(batch, nrow=3, padding=2, pad_value=0.0, images=9):
    """make_grid(batch[:images], nrow, padding, pad_value) * 0.5 + 0.5, clamp, uint8 HWC -- tensor ops on the device"""
    x = batch[:images]
    k, _, H, W = x.shape
    xmaps = min(nrow, k)
    ymaps = -(-k // xmaps)
    h, w = H + padding, W + padding
    grid = x.new_full((3, h * ymaps + padding, w * xmaps + padding), pad_value)
    for i in range(k):
        r, c = divmod(i, xmaps)
        grid[:, r * h + padding:r * h + padding + H, c * w + padding:c * w + padding + W] = x[i]
    grid = (grid * 0.5 + 0.5).clamp(0, 1)
    grid = torch.nan_to_num(grid, nan=0.0)
    return (grid * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def compare(forms, warmup, iters, rounds):
    """forms: {name: callable}; returns {name: (median, min, max)} in us per call, the forms alternating"""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}")
    g = torch.Generator().manual_seed(1)
    result = {"digest": _lib.built_digest(), "iters": args.iters, "rounds": args.rounds, "us_per_call": {}, "GBps": {}}
    for name, (tags, shape) in CASES.items():
        batches = [(torch.randn(shape, generator=g) * 0.6).cuda() for _ in range(tags)]
        out = ops.image_grid_u8(batches)
        for i, b in enumerate(batches):
            assert torch.equal(out[i], torch_grid_u8(b)), f"{name}: kernel and torch ops differ on tag {i}"
        forms = {
            f"kernel_{name}": lambda: ops.image_grid_u8(batches, out=out),
            f"torch_ops_{name}": lambda: [torch_grid_u8(b) for b in batches],
        }
        moved = tags * 9 * 3 * shape[2] * shape[3] * 4 + out.numel()  # every input float once, every output byte once
        for form, (med, lo, hi) in compare(forms, args.warmup, args.iters, args.rounds).items():
            print(f"{form:36s} {med:9.1f} us per call (min {lo:.1f}, max {hi:.1f})")
            result["us_per_call"][form] = round(med, 1)
        result["GBps"][name] = round(moved / (result["us_per_call"][f"kernel_{name}"] * 1e-6) / 1e9, 1)
        result[f"torch_ops_over_kernel_{name}"] = round(
            result["us_per_call"][f"torch_ops_{name}"] / result["us_per_call"][f"kernel_{name}"], 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
