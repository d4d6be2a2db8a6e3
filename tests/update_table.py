"""The hand-made item table and the bookkeeping that the shared checks of the update kernels (tests/lars_ref.py, tests/lamb_ref.py; the option
list and clip_setup also tests/test_gpu_optim_ops.py) are built on. Nothing here calls into clip_lite_amd."""
from collections import namedtuple

import numpy as np

import loss_ref as R

Tensor = namedtuple("Tensor", "start n adapted")          # a tensor's element range [start, start + n) of the flat buffers

SENT = 100.0
CHUNK = 8192                                   # the host's elements per item (optim/fused_sgd.py)
PAIRS = [(0.2, 1e-4), (1e-3, 0.0), (0.05, 5e-2)]          # (lr, wd) of tensor i: PAIRS[i % 3]
# (elements, norm slot or None = not adapted, special). One workgroup per item, a sweep is 256 threads x 4 elements: 4 -> thread 0 alone; 1028 ->
# thread 0 takes a second sweep; 8192 -> exactly one item; 8192 * 3 + 1020 -> four items, the last one ragged (255 threads); two not-adapted
# tensors between adapted ones (reserved = 0: they must never read norms); an adapted tensor with g = 0 and one with p = 0 (q = 1). The slots are
# deliberately not in table order, and slots 4 and 7 belong to no tensor.
TABLE = [(4, 5, None), (64, None, None), (1028, 0, None), (8192, 3, None), (1020, None, None), (8192 * 3 + 1020, 1, None), (260, 6, "g0"),
         (516, 2, "p0")]
N_SLOTS = 8
# (sync, cast given, clipping, pre-scale): every option in both states, not the full product
OPTIONS = [(False, True, "active", 0.25), (True, False, "inactive", 1.0), (True, True, "disabled", 0.25), (False, False, "disabled", 1.0),
           (True, True, "active", 1.0)]


def table(adapt=True):
    """rows, [Tensor], [slot or None], [index of each tensor's first item], arena length. Starts are multiples of 64; a gap of >= 64 sentinel
    elements precedes the first tensor and follows every tensor. adapt = False: the same table with every reserved word 0."""
    rows, tensors, slots, heads, start = [], [], [], [], 64
    for i, (n, slot, _) in enumerate(TABLE):
        lr, wd = PAIRS[i % 3]
        if not adapt:
            slot = None
        tensors.append(Tensor(start, n, slot is not None))
        slots.append(slot)
        heads.append(len(rows))
        for s in range(0, n, CHUNK):
            rows.append((start + s, min(CHUNK, n - s), lr, wd, 0 if slot is None else slot + 1))
        start = (start + n + 63) // 64 * 64 + 64
    return rows, tensors, slots, heads, start


def inside_of(tensors, n):
    """Which of the n arena elements lie in a tensor; the others hold SENT in every buffer."""
    inside = np.zeros(n, bool)
    for t in tensors:
        inside[t.start:t.start + t.n] = True
    return inside


def finish_problem(arrays, rows, n):
    """The buffers of a problem - `arrays` plus the bf16 copy, the partial pairs and the norm slots, sentinels in and behind all three - and the
    per-element lr and wd of the table."""
    bufs = dict(arrays, cast=R.to_bf16_bits(np.full(n, 3.0, np.float32)), partials=np.full(2 * len(rows) + 8, SENT, np.float32),
                norms=np.full(2 * N_SLOTS + 8, SENT, np.float32))
    lr, wd = np.zeros(n), np.zeros(n)
    for s, c, a, b, _ in rows:
        lr[s:s + c], wd[s:s + c] = np.float32(a), np.float32(b)
    return bufs, lr, wd


def clip_setup(clip, g, inside, gs):
    """(max_norm, sumsq value): clipping active (norm = 2 max_norm), inactive (norm = max_norm / 2), or disabled with NaN in sumsq."""
    ss = np.float32((g[inside].astype(np.float64) ** 2).sum())
    norm = float(np.sqrt(ss)) * gs
    return {"active": (norm / 2, ss), "inactive": (norm * 2, ss), "disabled": (0.0, np.float32("nan"))}[clip]


def note(measured, name, value):
    """The running maximum of what the checks print, by name, in the caller's `measured`."""
    measured[name] = max(measured.get(name, 0.0), float(value))
    return measured[name]


def kept(name, got, before, keep):
    assert R.same_bits(np.ascontiguousarray(got[keep]), np.ascontiguousarray(before[keep])), f"{name}: a kept element changed"


def check_norm_slots(tag, what, norms, pair, tensors, slots, launched, measured):
    """`norms` after a norms call over the tensors `launched` (indices): the launched slots against the float64 sums of squares of the two arrays
    `pair` = ((name, array), (name, array)), each within 1e-5 * max(1, sum of terms); every other slot untouched."""
    live = set()
    for i in launched:
        if slots[i] is None:
            continue
        live.add(slots[i])
        t = tensors[i]
        for k, (name, arr) in enumerate(pair):
            terms = np.asarray(arr[t.start:t.start + t.n], np.float64) ** 2
            den = max(1.0, terms.sum())
            err = abs(float(norms[2 * slots[i] + k]) - terms.sum()) / den
            print(f"{tag} {what} norms: tensor {i} ({t.n} elements) sum {name}^2: error / max(1, sum terms) = {err:.2e}, "
                  f"running max {note(measured, 'norms', err):.2e} (bound 1e-5)")
            assert err <= 1e-5, (what, i, name, err)
    dead = np.ones(len(norms), bool)
    for s in live:
        dead[2 * s:2 * s + 2] = False
    assert (norms[dead] == SENT).all(), f"{what}: a slot of a tensor outside the launched range (or behind the buffer) was written"
