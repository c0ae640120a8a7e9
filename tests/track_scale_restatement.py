"""The template tracker's scale search (include/d3f_hip.h: d3f_track_search_scale_u8; DESIGN.md section 4, "Template tracker:
scale search") restated in numpy and Python integers, independent of the package: the level sizes, the resample, the
search over (dL, dx, dy), the way back to the frame, what the tool writes with --scale, and the recipe of the frames the
tests track through -- a smooth-textured patch whose size changes linearly.  Everything is exact integer arithmetic, so
every comparison against the device is array_equal."""
import numpy as np

from track_restatement import geometry, gray_decimate, seed  # noqa: F401  (the reduced image, the geometry and the seed are shared)

MIN_SIDE, MAX_SIDE, PENALTY = 4, 64, 512


def level_size(tw0, th0, L):
    """(tw(L), th(L)): level L0 = max(tw0, th0) is the seed's size, one level one sample on the longer side"""
    L0 = max(tw0, th0)
    return (tw0 * L + L0 // 2) // L0, (th0 * L + L0 // 2) // L0


def level_valid(tw0, th0, L, gh, gw):
    if L < 1:
        return False
    tw, th = level_size(tw0, th0, L)
    return MIN_SIDE <= tw <= MAX_SIDE and MIN_SIDE <= th <= MAX_SIDE and tw <= gw and th <= gh


def level_range(tw0, th0, gh, gw):
    """(the smallest, the largest) valid level; the sizes grow with L, so the levels between them are valid too"""
    valid = [L for L in range(1, MAX_SIDE + 1) if level_valid(tw0, th0, L, gh, gw)]
    return valid[0], valid[-1]


def axis_taps(n_in, n_out):
    """[(i0, i1, f)] per output index: bilinear at pixel centres, 6-bit weights"""
    taps = []
    for i in range(n_out):
        num, den = (2 * i + 1) * n_in - n_out, 2 * n_out
        if num < 0:
            i0, f = 0, 0
        else:
            i0 = num // den
            f = ((num - i0 * den) * 64) // den
        taps.append((min(i0, n_in - 1), min(i0 + 1, n_in - 1), f))
    return taps


def resample(A, h_out, w_out):
    """[h_in, w_in] uint8 -> [h_out, w_out] uint8"""
    A = np.asarray(A).astype(np.int64)
    ys, xs = axis_taps(A.shape[0], h_out), axis_taps(A.shape[1], w_out)
    out = np.empty((h_out, w_out), dtype=np.uint8)
    for j, (y0, y1, fy) in enumerate(ys):
        for i, (x0, x1, fx) in enumerate(xs):
            v = (A[y0, x0] * (64 - fy) * (64 - fx) + A[y0, x1] * (64 - fy) * fx + A[y1, x0] * fy * (64 - fx)
                 + A[y1, x1] * fy * fx + 2048) >> 12
            out[j, i] = v
    return out


def search_frame(G, T0, pos, L, R, adapt, lost, levels=1, penalty=PENALTY):
    """one frame: -> (T0, pos, L, row) with row = (px, py, tw(L), th(L), ncost, found, L, cost), taken after the update.
    Every candidate's key is a tuple of Python integers, in the order of the 64-bit key's fields, and the smallest is taken."""
    gh, gw = G.shape
    th0, tw0 = T0.shape
    G = G.astype(np.int64)
    tw, th = level_size(tw0, th0, L)
    best = None
    for dL in range(-levels, levels + 1):
        Lc = L + dL
        if not level_valid(tw0, th0, Lc, gh, gw):
            continue
        twc, thc = level_size(tw0, th0, Lc)
        T = resample(T0, thc, twc).astype(np.int64)
        ax = min(max(pos[0] + (tw - twc) // 2, 0), gw - twc)
        ay = min(max(pos[1] + (th - thc) // 2, 0), gh - thc)
        dxs = [dx for dx in range(-R, R + 1) if 0 <= ax + dx <= gw - twc]
        for dy in range(-R, R + 1):
            y = ay + dy
            if not 0 <= y <= gh - thc:
                continue
            # the costs of this row of candidates at once: [thc, len(dxs), twc] windows against T
            strip = G[y:y + thc, ax + dxs[0]:ax + dxs[-1] + twc]
            windows = np.lib.stride_tricks.sliding_window_view(strip.astype(np.int16), twc, axis=1)
            costs = np.abs(windows - T.astype(np.int16)[:, None, :]).sum(axis=(0, 2), dtype=np.int64)
            for dx, cost in zip(dxs, costs.tolist()):
                x = ax + dx
                ncost = (cost << 12) // (twc * thc)
                key = (ncost + penalty * abs(dL), abs(dL), dL + 1, dx * dx + dy * dy, dy + R, dx + R)
                assert key[0] < 1 << 21 and key[3] < 1 << 14
                if best is None or key < best[0]:
                    best = (key, cost, ncost, Lc, x, y, twc, thc)
    _, cost, ncost, Lc, x, y, twc, thc = best
    found = cost <= lost * twc * thc
    if found:
        L, pos, tw, th = Lc, (x, y), twc, thc
        W0 = resample(G[y:y + thc, x:x + twc], th0, tw0).astype(np.int64)
        T0 = ((T0.astype(np.int64) * (8 - adapt) + W0 * adapt + 4) >> 3).astype(np.uint8)
    return T0, pos, L, (pos[0], pos[1], tw, th, ncost, int(found), L, cost)


def search(gray, T0, pos, L, R, adapt, lost, levels=1, penalty=PENALTY):
    """the frames of a call in order: -> (T0, pos, L, rows int32 [B, 8])"""
    rows = []
    for G in gray:
        T0, pos, L, row = search_frame(G, T0, pos, L, R, adapt, lost, levels, penalty)
        rows.append(row)
    return T0, pos, L, np.array(rows, dtype=np.int32).reshape(len(rows), 8)


def face_of_row(row, geo, h, w):
    """the row's box in frame pixels (None: not found): the seed's face scaled by L / L0 about the reduced box's centre,
    then moved so that at least one pixel of it lies inside the h x w frame"""
    s, _, _, tw0, th0, ox, oy, fw, fh = geo
    px, py, tw, th, _, found, L, _ = [int(v) for v in row]
    if not found:
        return None
    L0 = max(tw0, th0)
    fw1, fh1 = (fw * L + L0 // 2) // L0, (fh * L + L0 // 2) // L0
    x = ((2 * px + tw) * s + 2 * ox + fw - tw0 * s - fw1) // 2
    y = ((2 * py + th) * s + 2 * oy + fh - th0 * s - fh1) // 2
    return min(max(x, 1 - fw1), w - 1), min(max(y, 1 - fh1), h - 1), fw1, fh1


def faces(rows, geo, h, w):
    return [face_of_row(row, geo, h, w) for row in rows]


def tool_track(frames, keys, R=16, adapt=1, lost=16, side=48, penalty=PENALTY):
    """what script_tools/track_face_box.py --scale writes for the frames [n, h, w, 3] and keys {k: (x, y, w, h)}: None
    before the first key and where the face is not found, the key's clipped box at a key frame, where the tracker is
    seeded anew and the level goes back to the new L0"""
    track, state = [], None
    for k, frame in enumerate(frames):
        h, w = frame.shape[:2]
        if k in keys:
            geo = geometry(h, w, keys[k], side)
            s, tx, ty, tw, th = geo[:5]
            T0, pos = seed(gray_decimate(frame, s), tx, ty, tw, th)
            state = (geo, T0, pos, max(tw, th))
            track.append((tx * s + geo[5], ty * s + geo[6], geo[7], geo[8]))
        elif state is None:
            track.append(None)
        else:
            geo, T0, pos, L = state
            T0, pos, L, row = search_frame(gray_decimate(frame, geo[0]), T0, pos, L, R, adapt, lost, 1, penalty)
            state = (geo, T0, pos, L)
            track.append(face_of_row(row, geo, h, w))
    return track


def _smooth(rng, h, w, cell):
    """a random texture in 40..215 of h x w samples: random cells `cell` samples apart, bilinearly enlarged, so that a resize
    keeps it (white noise does not survive one)"""
    ch, cw = h // cell + 2, w // cell + 2
    c = rng.integers(40, 216, size=(ch, cw)).astype(np.float64)
    y, x = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    top = c[y0][:, x0] * (1 - fx) + c[y0][:, x0 + 1] * fx
    bot = c[y0 + 1][:, x0] * (1 - fx) + c[y0 + 1][:, x0 + 1] * fx
    return top * (1 - fy) + bot * fy


def _render(face, ph, pw):
    """the float texture `face` bilinearly resized to ph x pw at pixel centres"""
    h, w = face.shape
    y = np.clip((np.arange(ph) + 0.5) * h / ph - 0.5, 0, h - 1)
    x = np.clip((np.arange(pw) + 0.5) * w / pw - 0.5, 0, w - 1)
    y0, x0 = np.minimum(y.astype(int), h - 2), np.minimum(x.astype(int), w - 2)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    top = face[y0][:, x0] * (1 - fx) + face[y0][:, x0 + 1] * fx
    bot = face[y0 + 1][:, x0] * (1 - fx) + face[y0 + 1][:, x0 + 1] * fx
    return top * (1 - fy) + bot * fy


def scaling_patch_frames(seed_, B, gh, gw, step, grow, patch=(48, 40), cell=6, absent=()):
    """-> (gray [B, gh, gw] uint8, boxes): a static smooth-textured background; a smooth-textured patch of patch = (ph, pw)
    samples in frame 0 whose sides change linearly to (1 + grow) times that in frame B - 1 (rounded to whole samples) and
    whose centre moves by at most `step` samples per axis and frame, the patch kept inside the image; per-frame noise in
    -6..6; the patch left out of the frames listed in `absent`.  boxes[k] = (x, y, pw_k, ph_k) in samples."""
    rng = np.random.default_rng(seed_)
    ph0, pw0 = patch
    back = _smooth(rng, gh, gw, cell)
    face = _smooth(rng, 2 * ph0, 2 * pw0, 2 * cell)
    big_h, big_w = max(ph0, int(round(ph0 * (1 + grow)))), max(pw0, int(round(pw0 * (1 + grow))))
    cx = int(rng.integers(big_w // 2 + 1, gw - big_w // 2 - 1))
    cy = int(rng.integers(big_h // 2 + 1, gh - big_h // 2 - 1))
    frames, boxes = [], []
    for k in range(B):
        f = 1 + grow * k / max(B - 1, 1)
        ph, pw = int(round(ph0 * f)), int(round(pw0 * f))
        if k > 0:
            cx = int(np.clip(cx + rng.integers(-step, step + 1), big_w // 2 + 1, gw - big_w // 2 - 1))
            cy = int(np.clip(cy + rng.integers(-step, step + 1), big_h // 2 + 1, gh - big_h // 2 - 1))
        x, y = cx - pw // 2, cy - ph // 2
        g = back.copy()
        if k not in absent:
            g[y:y + ph, x:x + pw] = _render(face, ph, pw)
        g = np.rint(g) + rng.integers(-6, 7, size=g.shape)
        frames.append(g.astype(np.uint8))
        boxes.append((x, y, pw, ph))
    return np.stack(frames), boxes


def bgr_at_stride(gray, s):
    """[B, gh, gw] uint8 -> frames [B, gh s, gw s, 3] uint8 whose reduced grey image at stride s is `gray`"""
    big = np.repeat(np.repeat(gray, s, axis=1), s, axis=2)
    return np.ascontiguousarray(np.repeat(big[..., None], 3, axis=3))
