"""The template tracker's rotation search (include/d3f_hip.h: d3f_track_search_rot_u8; DESIGN.md section 4, "Template tracker:
rotation search") restated in numpy and Python integers, independent of the package: the table of rotations, the disc, the
rotation of a template, the search over (dA, dx, dy), the seed with an angle, the way back to the frame, what the tool
writes with --rotate, and the recipe of the frames the tests track through -- a smooth-textured patch that rolls.
Everything is exact integer arithmetic, so every comparison against the device is array_equal."""
import math

import numpy as np

from track_restatement import geometry, gray_decimate, seed  # noqa: F401  (the reduced image, the geometry and the seed are shared)
from track_scale_restatement import _smooth, bgr_at_stride  # noqa: F401  (the textures of the recipes)

STEP, MAX_DEGREES, MAX_INDEX, PENALTY = 200, 60, 64, 512


def table(step=STEP, max_degrees=MAX_DEGREES):
    """(amax, {a: (c16, s16)}) for the angle indices -amax..amax, index a the angle a * step hundredths of a degree"""
    amax = int(max_degrees * 100) // step
    assert step >= 1 and 0 <= amax <= MAX_INDEX and amax * step <= 18000
    out = {}
    for a in range(-amax, amax + 1):
        r = math.radians(a * step / 100.0)
        out[a] = (int(round(math.cos(r) * 65536.0)), int(round(math.sin(r) * 65536.0)))
    return amax, out


def disc_spans(tw0, th0):
    """[(lo, n)] per row: the samples (i, j) with u u + v v <= D D, u = 2 i + 1 - tw0, v = 2 j + 1 - th0, D = min(tw0, th0);
    an empty row is (0, 0)"""
    D = min(tw0, th0)
    spans = []
    for j in range(th0):
        v = 2 * j + 1 - th0
        inside = [i for i in range(tw0) if (2 * i + 1 - tw0) ** 2 + v * v <= D * D]
        assert inside == list(range(inside[0], inside[0] + len(inside))) if inside else True
        spans.append((inside[0], len(inside)) if inside else (0, 0))
    return spans


def disc_mask(tw0, th0):
    mask = np.zeros((th0, tw0), dtype=bool)
    for j, (lo, n) in enumerate(disc_spans(tw0, th0)):
        mask[j, lo:lo + n] = True
    return mask


def rot(A, c, s):
    """[th0, tw0] uint8 -> [th0, tw0] uint8, output sample (i, j) read from A at the position turned by (c, s) about the
    centre: bilinear, 6-bit weights, the taps clamped to the array; 0 outside the disc"""
    A = np.asarray(A).astype(np.int64)
    th0, tw0 = A.shape
    j, i = np.mgrid[0:th0, 0:tw0]
    u, v = 2 * i + 1 - tw0, 2 * j + 1 - th0
    X = c * u + s * v + (tw0 - 1) * 65536
    Y = -s * u + c * v + (th0 - 1) * 65536
    assert np.abs(X).max() < 1 << 31 and np.abs(Y).max() < 1 << 31
    x0, fx, y0, fy = X >> 17, (X >> 11) & 63, Y >> 17, (Y >> 11) & 63
    x1, y1 = np.clip(x0 + 1, 0, tw0 - 1), np.clip(y0 + 1, 0, th0 - 1)
    x0, y0 = np.clip(x0, 0, tw0 - 1), np.clip(y0, 0, th0 - 1)
    out = (A[y0, x0] * (64 - fy) * (64 - fx) + A[y0, x1] * (64 - fy) * fx + A[y1, x0] * fy * (64 - fx)
           + A[y1, x1] * fy * fx + 2048) >> 12
    return np.where(disc_mask(tw0, th0), out, 0).astype(np.uint8)


def seed_rot(gray_key, tx, ty, tw, th, angle=None, step=STEP, max_degrees=MAX_DEGREES):
    """(T0, pos, a0): the plain seed; with an angle in hundredths of a degree, a0 = round(angle / step) (halves away from
    zero) and the grey turned back by it on the disc, the samples outside the disc kept"""
    T0, pos = seed(gray_key, tx, ty, tw, th)
    if angle is None:
        return T0, pos, 0
    amax, tab = table(step, max_degrees)
    a0 = (2 * abs(angle) + step) // (2 * step) * (1 if angle >= 0 else -1)
    if abs(a0) > amax:
        raise ValueError("angle")
    c, s = tab[a0]
    return np.where(disc_mask(tw, th), rot(T0, c, -s), T0).astype(np.uint8), pos, a0


def search_frame(G, T0, pos, a, R, adapt, lost, steps=1, penalty=PENALTY, step=STEP, max_degrees=MAX_DEGREES):
    """one frame: -> (T0, pos, a, row) with row = (px, py, tw0, th0, ncost, found, a, cost), taken after the update.  Every
    candidate's key is a tuple of Python integers, in the order of the 64-bit key's fields, and the smallest is taken."""
    gh, gw = G.shape
    th0, tw0 = T0.shape
    amax, tab = table(step, max_degrees)
    mask = disc_mask(tw0, th0)
    n = int(mask.sum())
    G = G.astype(np.int64)
    best = None
    for dA in range(-steps, steps + 1):
        ac = a + dA
        if not -amax <= ac <= amax:
            continue
        T = rot(T0, *tab[ac]).astype(np.int16)
        dxs = [dx for dx in range(-R, R + 1) if 0 <= pos[0] + dx <= gw - tw0]
        for dy in range(-R, R + 1):
            y = pos[1] + dy
            if not 0 <= y <= gh - th0:
                continue
            strip = G[y:y + th0, pos[0] + dxs[0]:pos[0] + dxs[-1] + tw0]
            windows = np.lib.stride_tricks.sliding_window_view(strip.astype(np.int16), tw0, axis=1)
            costs = (np.abs(windows - T[:, None, :]) * mask[:, None, :]).sum(axis=(0, 2), dtype=np.int64)
            for dx, cost in zip(dxs, costs.tolist()):
                ncost = (cost << 12) // n
                key = (ncost + penalty * abs(dA), abs(dA), dA + 1, dx * dx + dy * dy, dy + R, dx + R)
                assert key[0] < 1 << 21 and key[3] < 1 << 14
                if best is None or key < best[0]:
                    best = (key, cost, ncost, ac, pos[0] + dx, y)
    _, cost, ncost, ac, x, y = best
    found = cost <= lost * n
    if found:
        a, pos = ac, (x, y)
        c, s = tab[a]
        W0 = rot(G[y:y + th0, x:x + tw0], c, -s).astype(np.int64)
        blend = (T0.astype(np.int64) * (8 - adapt) + W0 * adapt + 4) >> 3
        T0 = np.where(mask, blend, T0).astype(np.uint8)
    return T0, pos, a, (pos[0], pos[1], tw0, th0, ncost, int(found), a, cost)


def clamp_state(pos, a, gh, gw, tw0, th0, step=STEP, max_degrees=MAX_DEGREES):
    """the nearest valid state of a position and an angle index the host never saw"""
    amax = table(step, max_degrees)[0]
    return (min(max(pos[0], 0), gw - tw0), min(max(pos[1], 0), gh - th0)), min(max(a, -amax), amax)


def search(gray, T0, pos, a, R, adapt, lost, steps=1, penalty=PENALTY, step=STEP, max_degrees=MAX_DEGREES):
    """the frames of a call in order: -> (T0, pos, a, rows int32 [B, 8])"""
    rows = []
    for G in gray:
        T0, pos, a, row = search_frame(G, T0, pos, a, R, adapt, lost, steps, penalty, step, max_degrees)
        rows.append(row)
    return T0, pos, a, np.array(rows, dtype=np.int32).reshape(len(rows), 8)


def face_of_row(row, geo, step=STEP):
    """the row's box in frame pixels and its angle in hundredths of a degree (None: not found)"""
    s, _, _, _, _, ox, oy, fw, fh = geo
    px, py, _, _, _, found, a, _ = [int(v) for v in row]
    return (px * s + ox, py * s + oy, fw, fh, a * step) if found else None


def faces(rows, geo, step=STEP):
    return [face_of_row(row, geo, step) for row in rows]


def tool_track(frames, keys, key_angles=None, R=16, adapt=1, lost=16, side=48, penalty=PENALTY, step=STEP,
               max_degrees=MAX_DEGREES):
    """what script_tools/track_face_box.py --rotate writes for the frames [n, h, w, 3], keys {k: (x, y, w, h)} and
    key_angles {k: hundredths}: (x, y, w, h, hundredths) per frame, None before the first key and where the face is not
    found; at a key frame the key's clipped box and the angle of the seed's index"""
    track, state = [], None
    for k, frame in enumerate(frames):
        h, w = frame.shape[:2]
        if k in keys:
            geo = geometry(h, w, keys[k], side)
            s, tx, ty, tw, th = geo[:5]
            T0, pos, a = seed_rot(gray_decimate(frame, s), tx, ty, tw, th, (key_angles or {}).get(k), step, max_degrees)
            state = (geo, T0, pos, a)
            track.append((tx * s + geo[5], ty * s + geo[6], geo[7], geo[8], a * step))
        elif state is None:
            track.append(None)
        else:
            geo, T0, pos, a = state
            T0, pos, a, row = search_frame(gray_decimate(frame, geo[0]), T0, pos, a, R, adapt, lost, 1, penalty, step,
                                           max_degrees)
            state = (geo, T0, pos, a)
            track.append(face_of_row(row, geo, step))
    return track


def _sample(face, y, x):
    """the float texture `face` bilinearly at the positions (y, x), clamped to it"""
    h, w = face.shape
    y, x = np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)
    y0, x0 = np.minimum(y.astype(int), h - 2), np.minimum(x.astype(int), w - 2)
    fy, fx = y - y0, x - x0
    return ((face[y0, x0] * (1 - fx) + face[y0, x0 + 1] * fx) * (1 - fy)
            + (face[y0 + 1, x0] * (1 - fx) + face[y0 + 1, x0 + 1] * fx) * fy)


def turned_patch(g, face, x, y, pw, ph, degrees):
    """paste into the float image g the texture `face` (twice pw x ph samples) as a pw x ph patch whose un-rotated box has
    its corner at (x, y), turned clockwise on the screen (x right, y down) by `degrees` about the box's centre"""
    gh, gw = g.shape
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    Y, X = np.mgrid[0:gh, 0:gw].astype(np.float64)
    dx, dy = X - (x + (pw - 1) / 2), Y - (y + (ph - 1) / 2)
    lx, ly = c * dx + s * dy, -s * dx + c * dy
    inside = (np.abs(lx) <= pw / 2) & (np.abs(ly) <= ph / 2)
    fx, fy = (lx + pw / 2) * (face.shape[1] / pw) - 0.5, (ly + ph / 2) * (face.shape[0] / ph) - 0.5
    g[inside] = _sample(face, fy, fx)[inside]


def rolling_patch_frames(seed_, B, gh, gw, step, roll, patch=(48, 40), cell=6, absent=(), noise=6, start=0.0):
    """-> (gray [B, gh, gw] uint8, boxes): a static smooth-textured background; a smooth-textured patch of patch = (ph, pw)
    samples that is turned by start + roll * k degrees in frame k about its centre and whose un-rotated box moves by at most
    `step` samples per axis and frame, the turned patch kept inside the image; per-frame noise in -noise..noise; the patch
    left out of the frames listed in `absent`.  boxes[k] = (x, y, pw, ph, degrees)."""
    rng = np.random.default_rng(seed_)
    ph, pw = patch
    back = _smooth(rng, gh, gw, cell)
    face = _smooth(rng, 2 * ph, 2 * pw, 2 * cell)
    half = int(math.ceil(math.hypot(ph, pw) / 2)) + 1
    x = int(rng.integers(half - pw // 2, gw - half - pw // 2 + 1))
    y = int(rng.integers(half - ph // 2, gh - half - ph // 2 + 1))
    frames, boxes = [], []
    for k in range(B):
        if k > 0:
            x = int(np.clip(x + rng.integers(-step, step + 1), half - pw // 2, gw - half - pw // 2))
            y = int(np.clip(y + rng.integers(-step, step + 1), half - ph // 2, gh - half - ph // 2))
        g = back.copy()
        if k not in absent:
            turned_patch(g, face, x, y, pw, ph, start + roll * k)
        g = np.rint(g) + rng.integers(-noise, noise + 1, size=g.shape)
        frames.append(np.clip(g, 0, 255).astype(np.uint8))
        boxes.append((x, y, pw, ph, start + roll * k))
    return np.stack(frames), boxes
