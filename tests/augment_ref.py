"""NumPy float64 restatement of the augmentation pixel function (clip_lite_amd/augment.py, its docstring is the specification): the yardstick of
the kernels in csrc/augment_ops.hip and of the host-side tests. Written from the specification, not from the kernel source; shares no code with it."""
import numpy as np

X0, Y0, CW, CH, FLIP, JIT, FB, FC, FS, FH, ORD, NORM = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def axis_weights(o0, c, S, n):
    """[S][n] matrix of PIL's normalised triangle-filter coefficients for the box [o0, o0 + c) of an axis of n pixels."""
    W = np.zeros((S, n))
    scale = c / S
    support = max(scale, 1.0)
    for o in range(S):
        centre = o0 + (o + 0.5) * scale
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n)
        i = np.arange(lo, hi)
        wt = np.maximum(0.0, 1.0 - np.abs((i - centre + 0.5) / support))
        W[o, lo:hi] = wt / wt.sum()
    return W


def resample(canvas, row, S):
    """HWC uint8 canvas -> [S][S][3] float64 in [0, 255]: crop box, triangle resample, flip."""
    img = canvas.astype(np.float64)
    h, w = img.shape[:2]
    Wy, Wx = axis_weights(float(row[Y0]), float(row[CH]), S, h), axis_weights(float(row[X0]), float(row[CW]), S, w)
    out = np.einsum("yh,hwc,xw->yxc", Wy, img, Wx)
    return out[:, ::-1] if row[FLIP] != 0 else out


def gray(v):
    return 0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2]


def hue(v, fh):
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    maxc, minc = v.max(-1), v.min(-1)
    d = maxc - minc
    ok = d > 0
    dd, mm = np.where(ok, d, 1.0), np.where(ok, maxc, 1.0)
    s = dd / mm
    rc, gc, bc = (maxc - r) / dd, (maxc - g) / dd, (maxc - b) / dd
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = (h / 6.0 + fh) % 1.0
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.astype(int) % 6
    p, q, t = maxc * (1 - s), maxc * (1 - s * f), maxc * (1 - s * (1 - f))
    table = {0: (maxc, t, p), 1: (q, maxc, p), 2: (p, maxc, t), 3: (p, q, maxc), 4: (t, p, maxc), 5: (maxc, p, q)}
    out = v.copy()
    for k, rgb in table.items():
        sel = ok & (i == k)
        for c in range(3):
            out[..., c] = np.where(sel, rgb[c], out[..., c])
    return out


def jitter(v, row, stop_before_contrast=False):
    """The four colour ops in the row's order on [0, 255] values, clamped after each. Returns (values, mean gray in front of the contrast op)."""
    m = 0.0
    for k in range(4):
        op = int(row[ORD + k])
        if op == 0:
            v = v * float(row[FB])
        elif op == 1:
            m = gray(v).mean()
            if stop_before_contrast:
                return v, m
            v = m + float(row[FC]) * (v - m)
        elif op == 2:
            g = gray(v)[..., None]
            v = g + float(row[FS]) * (v - g)
        else:
            v = hue(v, float(row[FH]))
        v = np.clip(v, 0.0, 255.0)
    return v, m


def view(canvas, row, S):
    """[3][S][S] float64: the finished view of one plan row."""
    v = resample(canvas, row, S)
    if row[JIT] != 0:
        v, _ = jitter(v, row)
    v = v / 255.0
    if row[NORM] != 0:
        v = (v - MEAN) / STD
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def gray_mean(canvas, row, S):
    """The contrast mean of one view (0 with jitter off), as clite_augment_gray_mean defines it."""
    if row[JIT] == 0:
        return 0.0
    return float(jitter(resample(canvas, row, S), row, stop_before_contrast=True)[1])


def views(canvases, plan, S):
    return np.stack([view(c, r, S) for c, r in zip(canvases, plan)])
