"""Generate tests/golden/logging_scheduler.npz by running the REFERENCE's own LoggingScheduler.

Run once where a checkout of the reference is (no device needed):
    python tests/golden/make_golden_logging.py path/to/d3f/helpers/logging_scheduler.py

The file is loaded by path (it imports only `time`), its clock `get_current_time` is overridden, and about 400
(time, step) calls are driven through update_with_step_number / should_we_log_this_step: all four cadence bands (10 s
under 1 min, 1 min under 15 min, 10 min under 2 h, then 1 h), every fifth call repeating the previous step number (the
second optimizer of a batch).  Only data is written: the times, the step numbers and the decisions.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent


def schedule():
    """(time since construction, step number) of every call"""
    times = []
    t = 0.0
    for dt, count in ((1.5, 60), (7.0, 120), (95.0, 80), (610.0, 120)):  # up to 90 s, 15.5 min, 2 h 22 min, 22.7 h
        for _ in range(count):
            t += dt
            times.append(t)
    steps, step = [], -1
    for i in range(len(times)):
        if i % 5 != 4:
            step += 1
        steps.append(step)
    return np.array(times, dtype=np.float64), np.array(steps, dtype=np.int64)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = Path(sys.argv[1])
    spec = importlib.util.spec_from_file_location("reference_logging_scheduler", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)

    class Clocked(module.LoggingScheduler):
        now = 1000.0

        def get_current_time(self):
            return Clocked.now

    scheduler = Clocked()
    times, steps = schedule()
    decisions = []
    for t, step in zip(times, steps):
        Clocked.now = 1000.0 + float(t)
        scheduler.update_with_step_number(int(step))
        decisions.append(bool(scheduler.should_we_log_this_step()))
    decisions = np.array(decisions, dtype=np.bool_)
    np.savez(OUT / "logging_scheduler.npz", start=np.float64(1000.0), times=times, steps=steps, decisions=decisions)
    first = times[decisions.argmax()] if decisions.any() else None
    print(f"{len(times)} calls, {int(decisions.sum())} logging decisions, the first at {first} s")


if __name__ == "__main__":
    main()
