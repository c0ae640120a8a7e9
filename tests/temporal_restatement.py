"""The temporal filter restated in numpy (include/d3f_hip.h: d3f_temporal_filter_u8, d3f_color_coef_smooth): float32 where the
header says fp32 (every numpy operation on float32 arrays is one correctly rounded operation, the division included), int64
where it says integer.  The device tests compare bytes and the raw bits of the state with these, exactly.  Also the recipe
of temporally correlated test frames: independent random frames give sad >= T everywhere, and the filter is the identity."""
import numpy as np

STRENGTH, THRESHOLD, CUT_LEVELS = 0.75, 8, 16


class FilterState:
    """state_fake [H][W][3] float32, state_real [H][W][3] uint8, valid"""

    def __init__(self, H, W):
        self.fake = np.full((H, W, 3), np.nan, dtype=np.float32)  # (never read while invalid)
        self.real = np.full((H, W, 3), 0xA5, dtype=np.uint8)
        self.valid = False

    def copy(self):
        s = FilterState(*self.fake.shape[:2])
        s.fake, s.real, s.valid = self.fake.copy(), self.real.copy(), self.valid
        return s


def sad3x3(r, r_prev):
    """sum over the 3 x 3 surroundings (replicated border) and the 3 bytes of |r - r_prev|: int64 [H][W], 0..6885"""
    d = np.abs(r.astype(np.int64) - r_prev.astype(np.int64)).sum(axis=2)
    p = np.pad(d, 1, mode="edge")
    H, W = d.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def gate(r, r_prev, strength, threshold):
    """k [H][W] float32"""
    T = 27 * int(threshold)
    num = np.maximum(T - sad3x3(r, r_prev), 0).astype(np.float32)
    return np.float32(strength) * (num / np.float32(T))


def temporal_filter(real, fake, state, strength=STRENGTH, threshold=THRESHOLD):
    """real, fake [B][H][W][3] uint8 -> the filtered fake (a new array); state is advanced in place"""
    out = np.empty_like(fake)
    for b in range(real.shape[0]):
        f = fake[b].astype(np.float32)
        if state.valid:
            k = gate(real[b], state.real, strength, threshold)[:, :, None]
            d = state.fake - f
            p = k * d
            S = f + p
        else:
            S = f
        assert S.dtype == np.float32
        out[b] = np.clip(np.rint(S), 0, 255).astype(np.uint8)
        state.fake, state.real, state.valid = S.copy(), real[b].copy(), True
    return out


class CoefState:
    """state_coef [3][2] float32, state_sum [3] int64, valid"""

    def __init__(self):
        self.coef = np.full((3, 2), np.nan, dtype=np.float32)
        self.sums = np.full((3,), -1, dtype=np.int64)
        self.valid = False


def color_coef_smooth(coef, sums_to, n, state, strength=STRENGTH):
    """coef [B][3][2] float32, sums_to [B][3][2] (S, Q) integers -> the smoothed coefficients (a new array)"""
    out = np.array(coef, dtype=np.float32, copy=True)
    a = np.float32(strength)
    for b in range(out.shape[0]):
        S = np.array([int(sums_to[b][c][0]) for c in range(3)], dtype=np.int64)
        cut = not state.valid or bool((np.abs(S - state.sums) > CUT_LEVELS * int(n)).any())
        if not cut:
            d = state.coef - out[b]
            q = a * d
            out[b] = out[b] + q
            assert q.dtype == np.float32
        state.coef, state.sums, state.valid = out[b].copy(), S, True
    return out


def correlated_frames(seed, B, H, W):
    """(real, fake) [B][H][W][3] uint8: the real frames are one random base frame whose left third of the columns stays, whose
    middle third gets uniform integer noise in -6..6 per frame and whose right third is fresh random bytes per frame; the fake
    is one random base frame plus uniform noise in -20..20 per frame"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H, W, 3)).astype(np.int64)
    fbase = rng.integers(0, 256, size=(H, W, 3)).astype(np.int64)
    a, b = W // 3, 2 * W // 3
    real = np.empty((B, H, W, 3), dtype=np.uint8)
    fake = np.empty((B, H, W, 3), dtype=np.uint8)
    for t in range(B):
        r = base.copy()
        r[:, a:b] += rng.integers(-6, 7, size=(H, b - a, 3))
        r[:, b:] = rng.integers(0, 256, size=(H, W - b, 3))
        real[t] = np.clip(r, 0, 255).astype(np.uint8)
        fake[t] = np.clip(fbase + rng.integers(-20, 21, size=(H, W, 3)), 0, 255).astype(np.uint8)
    return real, fake


def thirds(W):
    return W // 3, 2 * W // 3


def bits(a):
    """the raw bits of a float32 array"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
