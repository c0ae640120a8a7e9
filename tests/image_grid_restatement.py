"""The training image grid restated with torch ops on the CPU (a helper, not a test): torchvision.utils.make_grid as
the reference calls it (d3f/train_deep_fake/lit_module.py:235-249), the reference's scaling of the whole grid, and
TensorBoard's uint8 conversion.

    make_grid(batch[:images], nrow, padding, pad_value):
        xmaps = min(nrow, images), ymaps = ceil(images / xmaps); cell (H + padding) x (W + padding);
        grid (ymaps * (H + padding) + padding) x (xmaps * (W + padding) + padding), filled with pad_value;
        image k at row (k // xmaps) * (H + padding) + padding, column (k % xmaps) * (W + padding) + padding;
        a single image is returned as it is; one channel is replicated to three
    g = (g * scale + shift).clamp(0, 1); NaN -> 0; (g * 255).to(uint8) (truncation); CHW -> HWC
"""
import math

import torch


def make_grid(batch, nrow=3, padding=2, pad_value=0.0):
    """[K, C, H, W] float32 (C = 1 or 3) -> [3, GH, GW]"""
    if batch.dim() != 4 or batch.shape[1] not in (1, 3):
        raise ValueError("make_grid restatement: [K, 1 or 3, H, W]")
    if batch.shape[1] == 1:
        batch = torch.cat((batch, batch, batch), 1)
    if batch.shape[0] == 1:
        return batch[0].clone()
    images = batch.shape[0]
    xmaps = min(nrow, images)
    ymaps = int(math.ceil(float(images) / xmaps))
    height, width = batch.shape[2] + padding, batch.shape[3] + padding
    grid = batch.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= images:
                break
            grid[:, y * height + padding:y * height + padding + height - padding,
                 x * width + padding:x * width + padding + width - padding] = batch[k]
            k += 1
    return grid


def image_grid_u8(batch, nrow=3, padding=2, pad_value=0.0, scale=0.5, shift=0.5, max_images=9):
    """[B, C, H, W] -> uint8 [GH, GW, 3]"""
    g = make_grid(batch.detach().cpu().float()[:max_images], nrow, padding, pad_value)
    g = (g * scale + shift).clamp(0, 1)
    g = torch.nan_to_num(g, nan=0.0)
    return (g * 255).to(torch.uint8).permute(1, 2, 0).contiguous()
