"""The derived weight operands restated on the host, element by element: the Winograd filter transform, the plain forward
and data-gradient layouts, the up-fold layouts and the three bf16 planes of f32x3 -- written from the layout comments of
csrc/pointwise.hip (weight packing, "Up-sample folded into the weights") and csrc/conv_winograd.hip (winograd_pack_kernel).
tests/test_gpu_packed_operands.py compares the kernels' buffers with these bit for bit; tests/test_cpu_packed_operands.py
checks the restatement itself against torch's convolutions, which know nothing of the layouts.  Nothing here touches the
GPU.

Values.  fp32 throughout, in the kernels' own operation order:

    Winograd U       t[1] = 0.5f * ((g0 + g1) + g2), t[2] = 0.5f * ((g0 - g1) + g2) down the columns, the same along the
                     rows of t: two additions and one exact halving per stage
    up-fold sums     v = 0.f, then v += w[kh][kw] over the taps of the set, kh-major and kw-minor (the first addition to
                     zero is exact); bf16 storage rounds the sum once to nearest-even; f32x3 splits it
    f32x3            h = the top 16 bits of v, m = the top 16 bits of r1 = v - h, l = the top 16 bits of r2 = r1 - m (both
                     differences exact in fp32; r2 has at most 8 significant bits, so h + m + l == v)

Layouts (row-major, the last index fastest).  ve = 4 (fp32, f32x3) / 8 (bf16), k-tile = 32 / 64 elements:

    U      [pos = 4 i + j][c / 16][k][c % 16] = (G g G^T)[i][j] of g = w[k][c]
    wf     [CoutPad][Kpad]       wf[n][(kh * K + kw) * Cin + c] = w[n][c][kh][kw]
    wd     [CinRows][KpadD]      wd[c][slot * CoutD + n] = w[n][c][taps - 1 - f(slot)]; f(slot) = slot, except that the
                                 stride-2 layers whose data gradient runs as output-parity classes store f = 0, 2, 6, 8,
                                 1, 7, 3, 5, 4
    wfc    [4][CoutPad][Kc]      Kc = 4 C0 + 9 C1, class z = 2 py + px:
                                 wfc[z][n][(2 a + b) * C0 + c] = sum of w[n][c][kh][kw] over kh in S(py, a), kw in S(px, b),
                                 S(0, 0) = {0}, S(0, 1) = {1, 2}, S(1, 0) = {0, 1}, S(1, 1) = {2};
                                 wfc[z][n][4 C0 + (3 kh + kw) * C1 + c1] = w[n][C0 + c1][kh][kw]
    wd4    [C0Rows][16 CoutD]    wd4[c][(4 u + v) * CoutD + n] = sum over kh in T(u), kw in T(v),
                                 T(0) = {2}, T(1) = {1, 2}, T(2) = {0, 1}, T(3) = {0}
    wds    [C1Rows][K9]          wds[c1][f * CoutD + n] = w[n][C0 + c1][8 - f], K9 = 9 CoutD in whole k-tiles
    f32x3  three planes of bf16 bit patterns one plane-stride apart: wf / wd / wd4 / wds as a whole, wfc class by class
           ([z][plane][CoutPad][Kc]); the data-gradient buffer of a folded layer is [wd4 | wds] in every type

CoutPad, CinRows, C0Rows, C1Rows: multiples of 16; CoutD: Cout in whole vectors; everything outside the real filter is zero
(in all three planes).
"""
import torch

F32, BF16, F32X3 = 0, 1, 2

S_SETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}   # (output parity, tap of the 2 x 2 neighbourhood)
T_SETS = {0: (2,), 1: (1, 2), 2: (0, 1), 3: (0,)}
PARITY_SLOTS = (0, 2, 6, 8, 1, 7, 3, 5, 4)


def round_up(a, b):
    return (a + b - 1) // b * b


def geometry(dt, C0, C1, Cout, K):
    """the padded extents of csrc/conv_plan.hip (storage type of f32x3: fp32)"""
    ve, bke = (8, 64) if dt == BF16 else (4, 32)
    cin, coutd = C0 + C1, round_up(Cout, ve)
    return dict(ve=ve, bke=bke, Cin=cin, CoutPad=round_up(Cout, 16), CoutD=coutd, Kpad=round_up(K * K * cin, bke),
                KpadD=round_up(K * K * coutd, bke), CinRows=round_up(cin, 16), C0Rows=round_up(C0, 16),
                C1Rows=round_up(C1, 16), wsz=6 if dt == F32X3 else 2 if dt == BF16 else 4)


# ---- f32x3 ---------------------------------------------------------------------------------------------------------------
def _top16(v):
    """fp32 -> (the value of its top 16 bits, those bits as int16)"""
    b = v.contiguous().view(torch.int32)
    return (b & -65536).view(torch.float32), (b >> 16).to(torch.int16)


def split3(v):
    """fp32 tensor -> [3, ...] int16: the bf16 bit patterns of the h, m and l planes"""
    v = v.float()
    h, hb = _top16(v)
    r1 = v - h
    m, mb = _top16(r1)
    _, lb = _top16(r1 - m)
    return torch.stack([hb, mb, lb])


def plane_values(p):
    """int16 bf16 bit patterns -> float64 values"""
    return (p.to(torch.int32) << 16).view(torch.float32).double()


def bits_of(t):
    """bf16 / fp32 tensor -> its bit patterns (int16 / int32)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def stored_bits(v, dt):
    """fp32 layout -> the bits the pack kernels store: [1, ...] int32 (fp32), [1, ...] int16 (bf16, one rounding to
    nearest-even), [3, ...] int16 (f32x3)"""
    if dt == F32X3:
        return split3(v)
    return bits_of(v.float() if dt == F32 else v.float().bfloat16()).unsqueeze(0)


# ---- Winograd filter transform -------------------------------------------------------------------------------------------
def winograd_filter_fp32(w):
    """w [K, C, 3, 3] fp32 -> G g G^T [K, C, 4, 4] in winograd_pack_kernel's order of operations"""
    g = w.float()

    def stage(a0, a1, a2):
        return [a0, 0.5 * ((a0 + a1) + a2), 0.5 * ((a0 - a1) + a2), a2]
    t = torch.stack(stage(g[:, :, 0], g[:, :, 1], g[:, :, 2]), 2)          # [K, C, 4, 3]: down the columns
    return torch.stack(stage(t[..., 0], t[..., 1], t[..., 2]), 3)          # [K, C, 4, 4]: along the rows


def winograd_layout(u):
    """[K, C, 4, 4] -> U[pos][c / 16][k][c % 16]"""
    K, C = u.shape[:2]
    return u.reshape(K, C // 16, 16, 16).permute(3, 1, 0, 2).contiguous()


def winograd_unlayout(U):
    """U[pos][c / 16][k][c % 16] -> [K, C, 4, 4]"""
    _, chunks, K, _ = U.shape
    return U.permute(2, 1, 3, 0).reshape(K, chunks * 16, 4, 4)


# ---- plain layouts ---------------------------------------------------------------------------------------------------------
def plain_layouts(w, C0, Cout, K, stride, pad, dt):
    """w [Cout, CinReal, K, K] fp32 -> (wf [CoutPad, Kpad], wd [CinRows, KpadD]) fp32 values"""
    g = geometry(dt, C0, 0, Cout, K)
    cin_real, taps = w.shape[1], K * K
    wf = torch.zeros(g["CoutPad"], g["Kpad"])
    wd = torch.zeros(g["CinRows"], g["KpadD"])
    parity = stride == 2 and g["CoutD"] % g["bke"] == 0 and ((K == 3 and pad == 1) or (K == 1 and pad == 0))
    flipped = PARITY_SLOTS if parity and taps == 9 else tuple(range(taps))
    flat = w.float().reshape(Cout, cin_real, taps)
    for n in range(Cout):
        for tap in range(taps):
            wf[n, tap * C0:tap * C0 + cin_real] = flat[n, :, tap]
    for slot, f in enumerate(flipped):
        wd[:cin_real, slot * g["CoutD"]:slot * g["CoutD"] + Cout] = flat[:, :, taps - 1 - f].t()
    return wf, wd


# ---- up-fold layouts -------------------------------------------------------------------------------------------------------
def _set_sum(w9, khs, kws):
    """w9 [..., 3, 3] fp32: 0.f + the taps of the set, kh-major, kw-minor, one fp32 addition each"""
    v = torch.zeros(w9.shape[:-2])
    for kh in khs:
        for kw in kws:
            v = v + w9[..., kh, kw]
    return v


def upfold_layouts(w, C0, C1, Cout, dt):
    """w [Cout, C0 + C1, 3, 3] fp32 -> (wfc [4, CoutPad, Kc], wd4 [C0Rows, 16 CoutD], wds [C1Rows, K9] or None): the
    fp32 values before the storage type's rounding / split"""
    g = geometry(dt, C0, C1, Cout, 3)
    w = w.float()
    coutd, kc = g["CoutD"], 4 * C0 + 9 * C1
    wfc = torch.zeros(4, g["CoutPad"], kc)
    for py in range(2):
        for px in range(2):
            z = 2 * py + px
            for a in range(2):
                for b in range(2):
                    k0 = (2 * a + b) * C0
                    wfc[z, :Cout, k0:k0 + C0] = _set_sum(w[:, :C0], S_SETS[(py, a)], S_SETS[(px, b)])
            for tap in range(9):
                k0 = 4 * C0 + tap * C1
                wfc[z, :Cout, k0:k0 + C1] = w[:, C0:, tap // 3, tap % 3]
    wd4 = torch.zeros(g["C0Rows"], 16 * coutd)
    for u in range(4):
        for v in range(4):
            k0 = (4 * u + v) * coutd
            wd4[:C0, k0:k0 + Cout] = _set_sum(w[:, :C0], T_SETS[u], T_SETS[v]).t()
    wds = None
    if C1:
        wds = torch.zeros(g["C1Rows"], g["KpadD"])
        for f in range(9):
            wds[:C1, f * coutd:f * coutd + Cout] = w[:, C0:, (8 - f) // 3, (8 - f) % 3].t()
    return wfc, wd4, wds


def upfold_forward_bits(wfc, dt):
    """wfc fp32 values -> the forward buffer's bits, flat: [z][CoutPad][Kc], f32x3 [z][plane][CoutPad][Kc]"""
    if dt == F32X3:
        return torch.stack([split3(wfc[z]) for z in range(4)]).reshape(-1)
    return stored_bits(wfc, dt).reshape(-1)


def upfold_dgrad_bits(wd4, wds, dt):
    """the data-gradient buffer's bits, flat: [wd4 | wds], each with its planes in f32x3"""
    parts = [stored_bits(wd4, dt).reshape(-1)] + ([stored_bits(wds, dt).reshape(-1)] if wds is not None else [])
    return torch.cat(parts)
