import torch


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def to_nhwc(x, cpad=None):
    """NCHW cpu tensor -> NHWC (channel-padded) tensor"""
    x = x.permute(0, 2, 3, 1).contiguous()
    if cpad is not None and cpad > x.shape[-1]:
        x = torch.nn.functional.pad(x, (0, cpad - x.shape[-1]))
    return x.contiguous()


def to_nchw(x, c=None):
    x = x.permute(0, 3, 1, 2)
    if c is not None:
        x = x[:, :c]
    return x.contiguous()


SENTINEL = -8192.0   # exact in fp32 and bf16


class Guarded:
    """a device buffer of n elements between two sentinel bands"""

    def __init__(self, n, guard, dtype, fill=SENTINEL, band=SENTINEL, device="cuda"):
        self.n, self.g, self.band = n, guard, band
        self.buf = torch.full((guard + n + guard,), band, dtype=dtype, device=device)
        self.t = self.buf[guard:guard + n]
        if fill != band:
            self.t.fill_(fill)

    def intact(self):
        front, back = self.buf[:self.g], self.buf[self.g + self.n:]
        if self.band != self.band:  # NaN bands
            return bool(torch.isnan(front).all() and torch.isnan(back).all())
        return bool((front == self.band).all() and (back == self.band).all())
