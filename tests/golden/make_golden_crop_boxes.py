"""Generate tests/golden/crop_boxes.npz by running the REFERENCE's own crop_image_at_center.

Run once in the build container (needs /root/reference; never runs on the GPU box):
    python tests/golden/make_golden_crop_boxes.py

The two script tools import cv2 and tqdm at module level, which are not installed: both are replaced by inert mocks only
so that the modules import.  crop_image_at_center itself (d3f/script_tools/video_to_center_cropped_images.py:83-100 and,
the same lines, put_video_through_fake_model.py:121-138) touches neither: it is called unbound on an image whose pixels
hold their own coordinates, so the slice it returns names its box.  Only data is written: the (h, w, width, height)
cases and the (x1, y1, crop_width, crop_height) boxes.
"""
import importlib.util
import sys
from pathlib import Path
from types import SimpleNamespace
from unittest import mock

import numpy as np

REF = Path("/root/reference/d3f/script_tools")
OUT = Path(__file__).resolve().parent

# (h, w, width, height): crop on width, crop on height, no crop, non-integer scales both ways, enlarging, odd sizes
CASES = [
    (1080, 1920, 448, 448), (1920, 1080, 448, 448), (720, 1280, 256, 256), (1080, 1920, 256, 448), (1080, 1920, 448, 256),
    (90, 160, 64, 64), (48, 40, 64, 64), (67, 131, 96, 32), (64, 64, 64, 64), (100, 180, 96, 64), (700, 900, 32, 32),
    (480, 640, 448, 448), (481, 641, 448, 320), (1079, 1919, 447, 449), (333, 777, 100, 30), (777, 333, 30, 100),
    (50, 50, 640, 480), (7, 1000, 33, 3), (1000, 7, 3, 33), (2160, 3840, 1000, 563), (1080, 1920, 1920, 1080),
    (1080, 1920, 3, 7), (101, 103, 107, 109), (2, 3, 5, 7),
]


def load(name):
    for stub in ("cv2", "tqdm"):
        sys.modules.setdefault(stub, mock.MagicMock(name=stub))
    spec = importlib.util.spec_from_file_location("reference_" + name, REF / (name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    crop = load("video_to_center_cropped_images").VideoToImages.crop_image_at_center
    boxes = []
    for h, w, width, height in CASES:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        image = np.stack([yy, xx, yy], axis=2)
        out = crop(SimpleNamespace(image_width=width, image_height=height), image)
        ch, cw, _ = out.shape
        y1, x1 = (int(out[0, 0, 0]), int(out[0, 0, 1])) if out.size else (-1, -1)
        boxes.append((x1, y1, cw, ch))
    np.savez(OUT / "crop_boxes.npz", cases=np.array(CASES, dtype=np.int64), boxes=np.array(boxes, dtype=np.int64))
    for c, b in zip(CASES, boxes):
        print(c, "->", b)


if __name__ == "__main__":
    main()
