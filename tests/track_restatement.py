"""The template tracker of include/d3f_hip.h ("Template tracker") restated in numpy integers and plain
Python, independent of the package: the reduced grey image, the geometry, the seed and the search, and the recipe of the
moving-patch frames the tests track through.  Everything is exact integer arithmetic, so every comparison against the
device is array_equal."""
import numpy as np


def gray_decimate(frames, s):
    """[B, h, w, 3] (or [h, w, 3]) uint8 BGR -> [B, h // s, w // s] uint8: (sum over the s x s block of B + 2 G + R) //
    (4 s s), partial blocks dropped"""
    x = np.asarray(frames)
    single = x.ndim == 3
    if single:
        x = x[None]
    B, h, w, _ = x.shape
    gh, gw = h // s, w // s
    v = x[:, :gh * s, :gw * s].astype(np.int64)
    p = v[..., 0] + 2 * v[..., 1] + v[..., 2]
    out = (p.reshape(B, gh, s, gw, s).sum(axis=(2, 4)) // (4 * s * s)).astype(np.uint8)
    return out[0] if single else out


def geometry(h, w, face, side=48):
    """(s, tx, ty, tw, th, ox, oy, fw, fh) of a face box marked in an h x w frame; ValueError as the issue lists them"""
    fx, fy, fw, fh = [int(v) for v in face]
    if not 1 <= side <= 64:
        raise ValueError("side")
    x0, y0, x1, y1 = max(fx, 0), max(fy, 0), min(fx + fw, w), min(fy + fh, h)
    if x1 <= x0 or y1 <= y0:
        raise ValueError("empty clip")
    fx, fy, fw, fh = x0, y0, x1 - x0, y1 - y0
    s = max(1, (max(fw, fh) + side - 1) // side)
    if s > 32:
        raise ValueError("stride")
    tx, ty = fx // s, fy // s
    tw, th = (fx + fw) // s - tx, (fy + fh) // s - ty
    if tw < 4 or th < 4:
        raise ValueError("template")
    return s, tx, ty, tw, th, fx - tx * s, fy - ty * s, fw, fh


def seed(gray_key, tx, ty, tw, th):
    """(T, pos): the template [th, tw] uint8 cut from the key frame's reduced grey image, and (tx, ty)"""
    return np.array(gray_key[ty:ty + th, tx:tx + tw], dtype=np.uint8), (int(tx), int(ty))


def search_frame(G, T, pos, R, adapt, lost):
    """one frame: -> (T, pos, row) with row = (pos.x, pos.y, cost, found), pos after the update.  Every candidate's key is
    formed as a Python integer and the smallest taken."""
    gh, gw = G.shape
    th, tw = T.shape
    G = G.astype(np.int64)
    Ti = T.astype(np.int64)
    best = None
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            x, y = pos[0] + dx, pos[1] + dy
            if not (0 <= x <= gw - tw and 0 <= y <= gh - th):
                continue
            cost = int(np.abs(G[y:y + th, x:x + tw] - Ti).sum())
            key = cost << 32 | (dx * dx + dy * dy) << 16 | (dy + R) << 8 | (dx + R)
            if best is None or key < best:
                best = key
    cost = best >> 32
    dx, dy = (best & 255) - R, ((best >> 8) & 255) - R
    found = cost <= lost * tw * th
    if found:
        pos = (pos[0] + dx, pos[1] + dy)
        W = G[pos[1]:pos[1] + th, pos[0]:pos[0] + tw]
        T = ((Ti * (8 - adapt) + W * adapt + 4) >> 3).astype(np.uint8)
    return T, pos, (pos[0], pos[1], cost, int(found))


def search(gray, T, pos, R, adapt, lost):
    """the frames of a call in order: -> (T, pos, rows int32 [B, 4])"""
    rows = []
    for G in gray:
        T, pos, row = search_frame(G, T, pos, R, adapt, lost)
        rows.append(row)
    return T, pos, np.array(rows, dtype=np.int32).reshape(len(rows), 4)


def faces(rows, geo):
    s, _, _, _, _, ox, oy, fw, fh = geo
    return [(int(px) * s + ox, int(py) * s + oy, fw, fh) if found else None for px, py, _, found in rows]


def tool_track(frames, keys, R=16, adapt=1, lost=16, side=48):
    """what script_tools/track_face_box.py writes for the frames [n, h, w, 3] and keys {k: (x, y, w, h)}: None before the first
    key and where the face is not found, the key's clipped box at a key frame, where the tracker is seeded anew"""
    track, state = [], None
    for k, frame in enumerate(frames):
        if k in keys:
            geo = geometry(frame.shape[0], frame.shape[1], keys[k], side)
            s, tx, ty, tw, th = geo[:5]
            T, pos = seed(gray_decimate(frame, s), tx, ty, tw, th)
            state = (geo, T, pos)
            track.append((tx * s + geo[5], ty * s + geo[6], geo[7], geo[8]))
        elif state is None:
            track.append(None)
        else:
            geo, T, pos = state
            T, pos, row = search_frame(gray_decimate(frame, geo[0]), T, pos, R, adapt, lost)
            state = (geo, T, pos)
            track.append(faces([row], geo)[0])
    return track


def moving_patch_frames(seed_, B, h, w, s, step, absent=(), patch=(24, 20)):
    """-> (frames [B, h, w, 3] uint8, positions): a static random-texture background; a random-texture patch of patch =
    (ph, pw) REDUCED pixels (s times that in the frame) whose top-left corner moves by at most `step` reduced pixels per
    axis and frame -- multiples of s in the frame, so the patch's reduced image moves by whole samples -- and stays inside
    the frame; per-frame noise in -6..6 on every byte; the patch left out of the frames listed in `absent` (its position
    still moves).  positions[k] = (x, y) of the patch in reduced pixels.  Texture in 40..215, so the noise never clips."""
    rng = np.random.default_rng(seed_)
    ph, pw = patch
    gh, gw = h // s, w // s
    # textures are drawn per reduced pixel and blown up, so that the reduced image keeps their contrast
    back = np.repeat(np.repeat(rng.integers(40, 216, size=(gh + 1, gw + 1, 3)), s, axis=0), s, axis=1)[:h, :w]
    face = np.repeat(np.repeat(rng.integers(40, 216, size=(ph, pw, 3)), s, axis=0), s, axis=1)
    x, y = int(rng.integers(0, gw - pw + 1)), int(rng.integers(0, gh - ph + 1))
    frames, positions = [], []
    for k in range(B):
        if k > 0:
            x = int(np.clip(x + rng.integers(-step, step + 1), 0, gw - pw))
            y = int(np.clip(y + rng.integers(-step, step + 1), 0, gh - ph))
        f = back.copy()
        if k not in absent:
            f[y * s:(y + ph) * s, x * s:(x + pw) * s] = face
        f = f + rng.integers(-6, 7, size=f.shape)
        frames.append(f.astype(np.uint8))
        positions.append((x, y))
    return np.stack(frames), positions
