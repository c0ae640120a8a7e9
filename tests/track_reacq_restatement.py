"""The template tracker's re-acquisition of include/d3f_hip.h ("Template tracker, re-acquisition")
restated in numpy integers and plain Python, independent of the package: the whole-frame search, the serial search that
takes a frame it does not find from there, the tool's loop with it, and the recipe of the teleporting patch.  The plain
step is tests/track_restatement.py's.  Everything is exact integer arithmetic, so every comparison against the device is
array_equal."""
import numpy as np

import track_restatement as tr

RELOST = 8


def global_key(G, K):
    """one frame: the smallest cost << 32 | y << 16 | x over every position of K [th, tw] in G [gh, gw], a Python integer"""
    gh, gw = G.shape
    th, tw = K.shape
    G = G.astype(np.int64)
    Ki = K.astype(np.int64)
    best = None
    for y in range(gh - th + 1):
        # a row of candidates at once: rows[j, x, i] = G[y + j, x + i]
        rows = np.lib.stride_tricks.sliding_window_view(G[y:y + th], tw, axis=1)
        costs = np.abs(rows - Ki[:, None, :]).sum(axis=(0, 2))
        for x, cost in enumerate(costs.tolist()):
            key = cost << 32 | y << 16 | x
            if best is None or key < best:
                best = key
    return best


def global_keys(gray, K):
    """[B, gh, gw] -> the B keys, Python integers"""
    return [global_key(G, K) for G in gray]


def decode(key):
    """key -> (cost, x, y)"""
    return key >> 32, key & 0xffff, (key >> 16) & 0xffff


def search_reacq_frame(G, T, K, pos, key, R, adapt, lost, relost=RELOST):
    """one frame: the plain step; a frame it does not find takes the position of `key`, this frame's whole-frame key, and
    K's bytes for the template when the key's cost is at most relost a sample -> (T, pos, row), found 2 in that row"""
    T, pos, row = tr.search_frame(G, T, pos, R, adapt, lost)
    if not row[3]:
        gcost, x, y = decode(key)
        if gcost <= relost * K.shape[0] * K.shape[1]:
            T, pos, row = K.copy(), (x, y), (x, y, gcost, 2)
    return T, pos, row


def search_reacq(gray, T, K, pos, R, adapt, lost, relost=RELOST, keys=None):
    """the frames of a call in order: -> (T, pos, rows int32 [B, 4])"""
    keys = global_keys(gray, K) if keys is None else keys
    rows = []
    for G, key in zip(gray, keys):
        T, pos, row = search_reacq_frame(G, T, K, pos, key, R, adapt, lost, relost)
        rows.append(row)
    return T, pos, np.array(rows, dtype=np.int32).reshape(len(rows), 4)


def tool_track(frames, keys, R=16, adapt=1, lost=16, relost=RELOST, side=48):
    """what script_tools/track_face_box.py --reacquire writes for the frames [n, h, w, 3] and keys {k: (x, y, w, h)} -> (the
    track, the flags): tests/track_restatement.py's loop, the key template the seed's and replaced at every key; a
    re-acquired frame is an ordinary box.  flags[k]: 1 found (a key frame too), 2 re-acquired, 0 written as `-`"""
    track, flags, state = [], [], None
    for k, frame in enumerate(frames):
        if k in keys:
            geo = tr.geometry(frame.shape[0], frame.shape[1], keys[k], side)
            s, tx, ty, tw, th = geo[:5]
            T, pos = tr.seed(tr.gray_decimate(frame, s), tx, ty, tw, th)
            state = (geo, T, T.copy(), pos)
            track.append((tx * s + geo[5], ty * s + geo[6], geo[7], geo[8]))
            flags.append(1)
        elif state is None:
            track.append(None)
            flags.append(0)
        else:
            geo, T, K, pos = state
            G = tr.gray_decimate(frame, geo[0])
            T, pos, row = search_reacq_frame(G, T, K, pos, global_key(G, K), R, adapt, lost, relost)
            state = (geo, T, K, pos)
            track.append(tr.faces([row], geo)[0])
            flags.append(row[3])
    return track, flags


# ---- the recipe: the teleporting patch ----
# 24 frames of 72 x 100 at stride 1, a patch of 24 x 20 (rows x columns); search 8, adapt 1, lost 16
FRAMES, H, W, PATCH, SEARCH, ADAPT, LOST = 24, 72, 100, (24, 20), 8, 1, 16
JUMPS, ABSENT = (6, 12, 18), (9, 10, 11)


def teleporting_patch_frames(seed_, B=FRAMES, h=H, w=W, patch=PATCH, step=2, jumps=JUMPS, absent=ABSENT, reach=2 * SEARCH,
                             noise=6):
    """-> (frames [B, h, w, 3] uint8, positions): tests/track_restatement.py's moving patch at stride 1 -- a static
    random-texture background, a random-texture patch whose corner moves by at most `step` per axis and frame inside the
    frame, noise in -noise..noise on every byte -- that TELEPORTS at the frames listed in `jumps` and is left out of the
    frames listed in `absent` (its position still moves).
    The jump rule: at a jump frame the new corner is drawn uniformly over the frame, again and again, until it lies more than
    `reach` samples on at least one axis from the corner in the last frame that SHOWED the patch -- so a tracker that stayed
    there cannot reach it with a search radius of up to `reach`, whether the frames between held the patch or not.
    positions[k] = (x, y) of the patch's corner in frame k.  Texture in 40..215, so the noise never clips."""
    rng = np.random.default_rng(seed_)
    ph, pw = patch
    back = rng.integers(40, 216, size=(h, w, 3))
    face = rng.integers(40, 216, size=(ph, pw, 3))
    x, y = int(rng.integers(0, w - pw + 1)), int(rng.integers(0, h - ph + 1))
    shown = (x, y)
    frames, positions = [], []
    for k in range(B):
        if k in jumps:
            while max(abs(x - shown[0]), abs(y - shown[1])) <= reach:
                x, y = int(rng.integers(0, w - pw + 1)), int(rng.integers(0, h - ph + 1))
        elif k > 0:
            x = int(np.clip(x + rng.integers(-step, step + 1), 0, w - pw))
            y = int(np.clip(y + rng.integers(-step, step + 1), 0, h - ph))
        f = back.copy()
        if k not in absent:
            f[y:y + ph, x:x + pw] = face
            shown = (x, y)
        f = f + rng.integers(-noise, noise + 1, size=f.shape)
        frames.append(f.astype(np.uint8))
        positions.append((x, y))
    return np.stack(frames), positions
