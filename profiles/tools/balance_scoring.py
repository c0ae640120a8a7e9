"""One scoring pass of balance_training_images both ways: the host path (a blocking copy per batch, host epilogue) and
`device_scoring: true` (scores scattered into one device buffer, one epilogue, one copy).

  list    : 96 synthetic images at 256 x 256, batch size 12 (8 batches), resnet34, fp32, device_rng (both passes blend the
            same noise, so the two class lists are compared first)
  a pass  : validation_step over the 8 device-resident batches, then validation_epoch_end (the class list and the chart go
            to a sink; no file is written)

Per pass two figures: the time between HIP events recorded around it (the device's view) and the wall time of the loop
between two device synchronisations (what the trainer waits).  WARMUP passes of each path, then ROUNDS rounds, the two
paths alternating; the figure is the median round.  The epilogue alone (d3f_difficulty_classes + d3f_difficulty_histogram_u8,
five launches) is timed with HIP events over --iters back-to-back calls.  One JSON line at the end.
    python profiles/tools/balance_scoring.py [--rounds N]
Kernel times of the epilogue come from a trace of the epilogue alone, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \\
        python profiles/tools/balance_scoring.py --epilogue-only --iters 50 --scores 1048576
"""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from denoising_diffusion_deep_fake_amd import _lib, ops
from denoising_diffusion_deep_fake_amd.balance_training_images.lit_module import LitModule

IMAGES, SIZE, BATCH = 96, 256, 12
HP = dict(batch_size=BATCH, learning_rate=0.01, max_epochs=1, num_workers=0, encoder_name="resnet34", ratio_of_noise=0.7,
          number_of_classes=10, mean=[128] * 3, std=[128] * 3, synthetic=True, synthetic_length=IMAGES, image_size=SIZE,
          device_rng=True, rng_seed=7)


def scoring_pass(lit, batches):
    """(ms between the events, ms of wall time) of one scoring pass"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    with torch.no_grad():
        lit.validation_epoch_end([lit.validation_step(b, i) for i, b in enumerate(batches)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--epilogue-only", action="store_true", help="skip the scoring passes (for a kernel trace)")
    ap.add_argument("--scores", type=int, nargs="+", default=[IMAGES, 1 << 20], help="score buffer sizes of the epilogue runs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, library digest {_lib.built_digest()}")
    result = {"digest": _lib.built_digest(), "images": IMAGES, "image_size": SIZE, "batch_size": BATCH, "rounds": args.rounds}
    if not args.epilogue_only:
        time_passes(args, result)
    time_epilogue(args, result)
    print(json.dumps(result))


def time_passes(args, result):
    torch.manual_seed(0)
    lit = LitModule(**HP).cuda().eval()
    lit.image_grid_sink = lambda tag, step, array: None
    dataset = lit.val_dataloader().dataset
    order = torch.randperm(IMAGES, generator=torch.Generator().manual_seed(1)).tolist()
    batches = [{"image": torch.stack([dataset[i]["image"] for i in order[s:s + BATCH]]).cuda(),
                "index": torch.tensor(order[s:s + BATCH]).cuda()} for s in range(0, IMAGES, BATCH)]

    def run(device_scoring):
        lit.hparams["device_scoring"] = device_scoring
        return scoring_pass(lit, batches)

    lists = {}
    for path in (False, True):
        for _ in range(args.warmup):
            run(path)
        index, classes = lit.difficulty_index
        lists[path] = classes[torch.argsort(index)]
    assert torch.equal(lists[False], lists[True]), "the two paths give different class lists"
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for path in (False, True):
            times[path].append(run(path))
    for path, name in ((False, "host_path"), (True, "device_scoring")):
        ev, wall = [t[0] for t in times[path]], [t[1] for t in times[path]]
        result[f"{name}_event_ms"] = round(statistics.median(ev), 3)
        result[f"{name}_wall_ms"] = round(statistics.median(wall), 3)
        print(f"{name:16s} events {statistics.median(ev):8.3f} ms (min {min(ev):.3f}, max {max(ev):.3f})   "
              f"wall {statistics.median(wall):8.3f} ms (min {min(wall):.3f}, max {max(wall):.3f})")


def time_epilogue(args, result):
    """the epilogue's five launches alone; by default on the score buffer of this list and on one of a million images"""
    for n in args.scores:
        scores = torch.rand(n, device="cuda")
        out_c = ops.difficulty_classes(scores, 10)
        out_h = ops.difficulty_histogram_u8(out_c[0])

        def epilogue():
            ops.difficulty_classes(scores, 10, out=out_c)
            ops.difficulty_histogram_u8(out_c[0], out=out_h)

        for _ in range(10):
            epilogue()
        rounds = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                epilogue()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / args.iters * 1e3)
        result[f"epilogue_us_n{n}"] = round(statistics.median(rounds), 1)
        print(f"epilogue, {n} scores: {statistics.median(rounds):.1f} us per call (min {min(rounds):.1f}, max {max(rounds):.1f})")


if __name__ == "__main__":
    main()
