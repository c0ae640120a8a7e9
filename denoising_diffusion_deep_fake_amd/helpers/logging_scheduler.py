"""When a training run logs its image grids (d3f/helpers/logging_scheduler.py): by the wall clock, densely at the start
of a run and sparsely later --

    time since the start        at most one logging step per
    under 1 minute              10 seconds
    under 15 minutes            1 minute
    under 2 hours               10 minutes
    afterwards                  1 hour

The interval is compared (strictly) with the time since the last logging step, which starts at construction: nothing is
logged before the first interval has passed.  A step number seen again -- the second optimizer of a batch asks with the
number the first one asked with -- keeps the decision made for it.

`every_n_steps` (hparam `image_logging_every_n_steps`, no counterpart in the reference) replaces the clock by
`global_step % n == 0`: short runs and tests.
"""
import time

# (the run is younger than, seconds between logging steps); older than the last row: LATE_INTERVAL
CADENCE = ((60.0, 10.0), (15 * 60.0, 60.0), (2 * 3600.0, 600.0))
LATE_INTERVAL = 3600.0


class LoggingScheduler:
    def __init__(self, every_n_steps=None):
        if every_n_steps is not None and int(every_n_steps) < 1:
            raise ValueError(f"image_logging_every_n_steps must be at least 1, got {every_n_steps!r}")
        self.every_n_steps = None if every_n_steps is None else int(every_n_steps)
        now = self.get_current_time()
        self.start_time = now
        self.last_log_time = now
        self.last_step_number = None
        self.elapsed_time_since_start = 0.0
        self.elapsed_time_since_last_log = 0.0
        self.log_this_step = False

    def update_with_step_number(self, global_step_number):
        if not self.has_step_number_changed(global_step_number):
            return  # the decision made for this step number stands
        if self.every_n_steps is not None:
            self.log_this_step = global_step_number % self.every_n_steps == 0
            return
        self.log_this_step = self.has_enough_time_elapsed_since_last_log()
        if self.log_this_step:
            self.last_log_time = self.get_current_time()

    def should_we_log_this_step(self):
        return self.log_this_step

    def has_step_number_changed(self, global_step_number):
        changed = global_step_number != self.last_step_number
        self.last_step_number = global_step_number
        return changed

    def time_between_logs(self):
        for younger_than, interval in CADENCE:
            if self.elapsed_time_since_start < younger_than:
                return interval
        return LATE_INTERVAL

    def has_enough_time_elapsed_since_last_log(self):
        self.update_elapsed_times()
        return self.elapsed_time_since_last_log > self.time_between_logs()

    def update_elapsed_times(self):
        now = self.get_current_time()
        self.elapsed_time_since_start = now - self.start_time
        self.elapsed_time_since_last_log = now - self.last_log_time

    def get_current_time(self):
        """the clock; tests override it"""
        return time.time()
