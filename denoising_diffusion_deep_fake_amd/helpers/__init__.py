"""`d3f.helpers` (d3f/helpers/__init__.py): the image-logging cadence of the three LitModules and the device-side grid
logger behind their `log_batch_as_image_grid`.  (The reference's convert_pyplot_figure_to_image_tensor serves balance's
matplotlib histogram: with `device_scoring: true` the balance LitModule builds that figure's counts and a chart of them on
the device, ops.difficulty_histogram_u8, and hands the chart to ImageGridLogger.enqueue -- no pyplot figure is converted.)
validation.py: held-out validation of the two trainers (no counterpart in the reference, which never validates them)."""
from .image_grid_logger import ImageGridLogger, ImageLoggingMixin
from .logging_scheduler import LoggingScheduler
from .validation import ValidationMixin

__all__ = ["ImageGridLogger", "ImageLoggingMixin", "LoggingScheduler", "ValidationMixin"]
