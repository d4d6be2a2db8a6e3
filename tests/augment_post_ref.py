"""NumPy float64 restatement of steps 3b (gray) and 3c (blur) of the augmentation pixel function (clip_lite_amd/augment.py, its docstring is the
specification) on top of tests/augment_ref.py, which it imports and leaves as it is. Written from the specification, not from the kernel
source; shares no code with it."""
import numpy as np

import augment_ref as R

GRAY, BLUR, W0 = 0, 1, 2
WEIGHTS = {3: (0.5, 0.25, 0.0, 0.0), 5: (0.375, 0.25, 0.0625, 0.0), 7: (0.28125, 0.21875, 0.109375, 0.03125)}      # centre outward


def post_row(gray=0, k=0):
    """One post row: gray flag, blur flag, the weights of kernel size k (0: no blur), two reserved zeros."""
    q = np.zeros(8, np.float32)
    q[GRAY] = gray
    if k:
        q[BLUR] = 1
        q[W0:W0 + 4] = WEIGHTS[k]
    return q


def to_gray(v):
    """3b on [S][S][3] values"""
    g = R.gray(v)
    return np.stack([g, g, g], axis=-1)


def blur(v, w):
    """3c on [S][S][3] values: separable 7 taps w[|i|], border REFLECT_101, the horizontal pass then the vertical one"""
    taps = np.array([w[3], w[2], w[1], w[0], w[1], w[2], w[3]], np.float64)
    S = v.shape[0]
    p = np.pad(v, ((0, 0), (3, 3), (0, 0)), mode="reflect")
    hz = sum(taps[i] * p[:, i:i + S] for i in range(7))
    p = np.pad(hz, ((3, 3), (0, 0), (0, 0)), mode="reflect")
    return sum(taps[i] * p[i:i + S] for i in range(7))


def resample(canvas, row, S):
    """augment_ref.resample as two matrix products (the same weights, one axis at a time): the three-operand einsum there takes most of a
    minute for a 224 x 224 view of a 256 x 341 canvas"""
    img = canvas.astype(np.float64)
    h, w = img.shape[:2]
    Wy = R.axis_weights(float(row[R.Y0]), float(row[R.CH]), S, h)
    Wx = R.axis_weights(float(row[R.X0]), float(row[R.CW]), S, w)
    out = np.tensordot(Wx, np.tensordot(Wy, img, axes=(1, 0)), axes=(1, 1)).transpose(1, 0, 2)          # [y][x][c]
    return out[:, ::-1] if row[R.FLIP] != 0 else out


def view(canvas, row, post, S):
    """[3][S][S] float64: the finished view of one plan row and its post row."""
    v = resample(canvas, row, S)
    if row[R.JIT] != 0:
        v, _ = R.jitter(v, row)
    if post[GRAY] != 0:
        v = to_gray(v)
    if post[BLUR] != 0:
        v = blur(v, [float(x) for x in post[W0:W0 + 4]])
    v = v / 255.0
    if row[R.NORM] != 0:
        v = (v - R.MEAN) / R.STD
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def views(canvases, plan, post, S):
    return np.stack([view(c, r, q, S) for c, r, q in zip(canvases, plan, post)])
