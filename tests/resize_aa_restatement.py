"""The antialiased crop + bicubic resize contract restated in float64 numpy (csrc/resize.hip, include/d3f_hip.h:
d3f_crop_resize_cubic_aa_u8), independent of the library: Pillow's bicubic, which is also
torch.nn.functional.interpolate(mode="bicubic", antialias=True).  Windows and tap offsets are exact integers, as in the
kernel; the weights, their normalisation and the two passes are float64, which is what the fp32 kernel is measured
against."""
import numpy as np

A = -0.5


def keys_weight_aa(x):
    """Keys cubic convolution kernel, A = -0.5, for x >= 0; 0 from 2 on"""
    x = np.asarray(x, dtype=np.float64)
    inner = ((A + 2) * x - (A + 3)) * x * x + 1          # x < 1
    outer = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A    # 1 <= x < 2
    return np.where(x < 1, inner, np.where(x < 2, outer, 0.0))


def axis_windows_aa(n_in, n_out):
    """for every output index i of an axis n_in -> n_out: the first tap xmin [n_out] and the end xmax [n_out] of its
    window (taps xmin .. xmax - 1, truncated at the ends of the axis), and the offsets' divisor D.  Centre
    c = (2i + 1) n_in / (2 n_out); support 2 n_in / n_out when the axis shrinks (n_in >= n_out), else 2"""
    i = np.arange(n_out, dtype=np.int64)
    down = n_in >= n_out
    S = 4 * n_in if down else 4 * n_out
    D = 2 * n_in if down else 2 * n_out
    c2 = (2 * i + 1) * n_in
    xmin = np.maximum((c2 - S + n_out) // (2 * n_out), 0)      # floor division
    xmax = np.minimum((c2 + S + n_out) // (2 * n_out), n_in)
    return xmin, xmax, D


def axis_taps_aa(n_in, n_out):
    """-> xmin [n_out], count [n_out], w [n_out, max count]: the normalised weights of taps xmin + t, t < count; zero
    behind count.  Raw weight keys(|a|), a = ((2k + 1) n_out - (2i + 1) n_in) / D; divided by their sum"""
    xmin, xmax, D = axis_windows_aa(n_in, n_out)
    i = np.arange(n_out, dtype=np.int64)
    count = xmax - xmin
    k = xmin[:, None] + np.arange(int(count.max()), dtype=np.int64)[None, :]
    num = (2 * k + 1) * n_out - ((2 * i + 1) * n_in)[:, None]
    raw = np.where(k < xmax[:, None], keys_weight_aa(np.abs(num) / D), 0.0)
    return xmin, count, raw / raw.sum(axis=1, keepdims=True)


def axis_matrix_aa(n_in, n_out):
    """the axis as a dense [n_out, n_in] matrix of normalised weights"""
    xmin, count, w = axis_taps_aa(n_in, n_out)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        m[i, xmin[i]:xmin[i] + count[i]] = w[i, :count[i]]
    return m


def crop_resize_cubic_aa_f64(frame, box, size):
    """frame [h, w, c] uint8, box (x1, y1, cw, ch), size (H, W) -> float64 [H, W, c] before rounding: horizontal pass over
    the crop, then vertical pass"""
    x1, y1, cw, ch = box
    H, W = size
    crop = frame[y1:y1 + ch, x1:x1 + cw].astype(np.float64)
    horizontal = np.einsum("jk,rkc->rjc", axis_matrix_aa(cw, W), crop)       # [ch, W, c]
    return np.einsum("ir,rjc->ijc", axis_matrix_aa(ch, H), horizontal)       # [H, W, c]


def case_taps_aa(box, size):
    """-> (n_x, n_y, S): the most taps an output column / row of the case has, and S = the product over the two axes of
    max over the axis' output indices of sum |w| / |sum w| (how far a value can lie outside 0..255, and the factor by
    which rounding errors relative to the terms exceed errors relative to the result)"""
    _, _, cw, ch = box
    H, W = size
    n, s = [], 1.0
    for n_in, n_out in ((cw, W), (ch, H)):
        _, count, w = axis_taps_aa(n_in, n_out)
        n.append(int(count.max()))
        s *= float((np.abs(w).sum(axis=1) / np.abs(w.sum(axis=1))).max())
    return n[0], n[1], s
