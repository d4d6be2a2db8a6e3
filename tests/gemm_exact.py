"""Exact cases for the implicit-GEMM engine (csrc/gemm.hip, igemm*.h, gemm_wide.hip, gemm_group.hip, conv_patch.hip): the case tables, the case
builder and the checker that tests/test_gpu_gemm_edges.py (the real kernels) and tests/test_wavesim_gemm_edges.py (the wave-simulator build) share.
numpy only (nothing here touches a GPU or a kernel library); the two ways a case reaches a kernel are in tests/gemm_backends.py.

Why equality. Operands are small integers ([-4, 4]; ternary where column statistics are accumulated), so every product and every partial sum of a
case is an integer (a multiple of 1/2 or 1/4 where alpha = 0.5) far below 2^24: an f32 accumulator holds it exactly WHATEVER the summation order -
K tiles, split-K slices meeting through float atomics, the two K-groups of the 8-wave kernels, the three bf16 MFMAs of clite_set_f32_split (an
integer in [-4, 4] is its own bf16 `hi` part). The builder computes the largest magnitude any partial sum of the case can reach (sums of absolute
values, epilogue terms and statistics included) and asserts it is below 2^24 in units of the case's quantum; that holds for the reference alone. The
comparison with the float64 reference is then equality - nothing is measured, no tolerance exists. A bf16 store is compared with round-to-nearest-
even of the exact value.

Placement. Every operand is a view into the interior of a larger allocation filled with NaN: row strides with 8 (A) and 24 (B) slack columns (one
form: lda = 3 K, ldc = 2 N, as the BERT pooler's views), GUARD elements before it, a NaN row and GUARD elements after it - a load past K or past the
last row that reaches an MFMA poisons the output. Outputs have ldc = N + 8, one extra row and GUARD elements on both sides, all pre-filled with
7.0; the statistics accumulator has one replica more than the call is told about. After the call the WHOLE allocation is compared: the inside
equals the reference, everything else still holds its pre-fill. No element is excluded (the split-K workspace, which clite.h documents as left
dirty, is an operand: only its surroundings are compared).

Epilogue order (include/clite.h, igemm.h igemm_epilogue): v = alpha * acc + bias; preact <- v; v = relu(v); v *= relu'(dact_aux); v += residual;
out <- v; colsum += (sum, sum of squares) of the STORED values. ep.atomic: out += alpha * acc and nothing else."""
import zlib

import numpy as np

from simlib import bf16_round          # (numpy only: round-to-nearest-even; importing simlib builds nothing)

BF16, F32 = 0, 1
GUARD = 128          # elements of padding on each side of every view (a multiple of 8: the views stay 16-byte aligned)
PREFILL = 7.0        # what every output element holds before the call
WGRAD_PREFILL = 3.0  # the non-zero gradient a weight gradient accumulates onto
LIMIT = float(1 << 24)
ACT_RELU = 1
REPLICAS = 4


class Ref:
    """element `off` of the allocation `name`"""
    __slots__ = ("name", "off")

    def __init__(self, name, off=GUARD):
        self.name, self.off = name, off


# ---------------------------------------------------------------------------------------------------------------- epilogue forms
def _form(**kw):
    f = dict(out_f32=False, alpha=1.0, bias=False, relu=False, preact=False, dact=False, residual=False, atomic=False, colsum=None, replicas=REPLICAS,
             ws=False, ld2=False)
    f.update(kw)
    return f


FORMS = {
    "f32": _form(out_f32=True), "bf16": _form(),
    "alpha_half": _form(alpha=0.5), "alpha_half_f32": _form(alpha=0.5, out_f32=True), "alpha_m2": _form(alpha=-2.0, out_f32=True),
    "bias": _form(bias=True), "relu_preact": _form(bias=True, relu=True, preact=True), "dact": _form(dact=True, out_f32=True),
    "residual": _form(residual=True), "atomic": _form(atomic=True, out_f32=True), "atomic_m2": _form(atomic=True, out_f32=True, alpha=-2.0),
    "colsum": _form(colsum=0), "colsum_bias": _form(colsum=0, bias=True), "colsum_rows1": _form(colsum=1, out_f32=True, replicas=1),
    "ws": _form(ws=True), "ws_full": _form(ws=True, bias=True, relu=True, preact=True, residual=True, colsum=0), "ws_f32": _form(ws=True, out_f32=True, alpha=0.5),
    "ld2": _form(ld2=True), "ld2_f32": _form(ld2=True, out_f32=True, bias=True),
}


# ---------------------------------------------------------------------------------------------------------------- case tables
def G(op, dt, M, N, K, form, det=0, split=0):
    return dict(op=op, dt=dt, shape=(M, N, K), form=form, det=det, split=split)


def CV(op, dt, shape, form, slack=8, det=0, split=0):
    """shape = (N, H, W, C, K, R, stride, pad); slack: ldc minus the output's columns"""
    return dict(op=op, dt=dt, shape=tuple(shape), form=form, slack=slack, det=det, split=split)


def case_id(c):
    tags = [k + str(c[k]) for k in ("slack", "det", "split") if c.get(k) not in (None, 0, 8)]
    return "-".join([c["op"], "f32" if c["dt"] == F32 else "bf16", "x".join(map(str, c["shape"])), c["form"]] + tags)


# residues around every tile boundary of the engine: tiles of 64 / 128 / 256 rows and columns, K tiles of 32 and 64
MS = [1, 7, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257]
NS = [8, 56, 64, 72, 120, 128, 136, 248, 256, 264]
KS = [8, 24, 32, 40, 56, 64, 72, 120, 128, 136, 256, 264, 520]
TN_KS = KS + [1, 9, 129, 263]          # gemm_tn: K is unconstrained, M and N are multiples of 8
DENSE = ("gemm_nt", "gemm_nn", "gemm_tn")


def dense_shapes(op):
    """all M x N at K = 40 and K = 264, all K at two (M, N) just past the 128 and the 256 boundary. gemm_tn needs M % 8 == 0: its M runs over the N
    list, and the two (M, N) are (136, 136) and (264, 264)."""
    tn = op == "gemm_tn"
    ms = NS if tn else MS
    out = [(m, n, k) for k in (40, 264) for m in ms for n in NS]
    for mn in ((136, 136), (264, 264)) if tn else ((129, 136), (257, 264)):
        out += [mn + (k,) for k in (TN_KS if tn else KS) if k not in (40, 264)]
    return out


def long_k_shapes(op):
    """K = 2304 (72 / 36 K tiles) with 1 - 6 output tiles: the split factor reaches 8, so the grid is the 1-D one in which each XCD owns whole splits"""
    return [(136, 136, 2304), (72, 264, 2304)] if op == "gemm_tn" else [(129, 136, 2304), (65, 72, 2304)]


def subset_shapes(op):
    """about a dozen shapes that contain every residue of the lists above at least once: what the epilogue forms and the modes run on"""
    if op == "gemm_tn":
        return [(8, 8, 8), (56, 56, 24), (64, 64, 32), (72, 72, 40), (120, 120, 56), (128, 128, 64), (136, 136, 72), (248, 248, 120), (256, 256, 128), (264, 264, 136),
                (136, 8, 256), (264, 136, 264), (72, 264, 520), (8, 136, 1), (136, 72, 9), (264, 264, 129), (128, 56, 263)]
    return [(1, 8, 8), (7, 56, 24), (8, 64, 32), (63, 72, 40), (64, 120, 56), (65, 128, 64), (127, 136, 72), (128, 248, 120), (129, 256, 128), (255, 264, 136),
            (256, 136, 256), (257, 264, 264), (129, 72, 520)]


BF16_FORMS = ["alpha_half", "alpha_half_f32", "alpha_m2", "bias", "relu_preact", "dact", "residual", "atomic", "atomic_m2", "colsum", "colsum_bias", "colsum_rows1",
              "ld2", "ld2_f32"]
WS_FORMS = ["ws", "ws_full", "ws_f32"]          # clite_gemm_nt / _nn only
F32_FORMS = ["f32", "alpha_half", "relu_preact", "dact", "residual", "atomic", "colsum", "colsum_rows1", "ld2"]


def plain_cases(op, dt):
    """every shape with the plain f32 store and the plain bf16 store; F32 storage (which has one store) on the dozen, as it is and as split bf16"""
    if dt == F32:
        return [G(op, F32, *s, "f32", split=sp) for sp in (0, 1) for s in subset_shapes(op) + long_k_shapes(op)[:1]]
    shapes = dense_shapes(op)
    shapes += [s for s in subset_shapes(op) if s not in shapes]
    return [G(op, BF16, *s, f) for s in shapes for f in ("f32", "bf16")]


def form_cases(op, dt):
    if dt == F32:
        return [G(op, F32, *s, f, split=sp) for sp in (0, 1) for f in F32_FORMS[1:] for s in subset_shapes(op)]
    forms = BF16_FORMS + (WS_FORMS if op != "gemm_tn" else [])
    return [G(op, BF16, *s, f) for f in forms for s in subset_shapes(op)]


def long_k_cases(op, dt):
    forms = ["f32", "atomic"] if dt == F32 else ["f32", "bf16", "atomic", "atomic_m2"] + (["ws", "ws_full"] if op != "gemm_tn" else [])
    return [G(op, dt, *s, f) for f in forms for s in long_k_shapes(op)]


def deterministic_cases(dt):
    """clite_set_deterministic(1): unsplit K for the accumulating forms, the statistics from the stored tensor (colstats_det_kernel); the workspace is declined"""
    forms = ["atomic", "colsum", "colsum_rows1", "bias"] + (["colsum_bias", "ws_full"] if dt == BF16 else [])
    out = [G(op, dt, *s, f, det=1) for op in DENSE for f in forms if not (f.startswith("ws") and op == "gemm_tn") for s in subset_shapes(op)]
    out += [G(op, dt, *long_k_shapes(op)[0], "atomic", det=1) for op in DENSE]
    out += [CV("conv_fwd", dt, s, "colsum", det=1) for s in CONV_SHAPES[:6]] + [CV("conv_wgrad", dt, s, "wgrad", det=1) for s in CONV_SHAPES[:6]]
    return out


# (N, H, W, C, K, R, stride, pad). N H W and N Ho Wo land on 63 / 126 / 127 / 128 / 129; odd images (7 x 9, 5 x 5), a 1 x 1 output; C in and out of
# the K tiles of 32 and 64 (8, 40, 64, 72, 96, 136) and K on both sides of the 64- and 128-column tiles (8, 64, 72, 160). A window needs C % 32 == K % 32 == 0.
CONV_SHAPES = [
    (1, 7, 9, 8, 8, 1, 1, 0), (2, 8, 8, 40, 72, 1, 1, 0), (127, 1, 1, 40, 8, 1, 1, 0), (43, 1, 3, 136, 160, 1, 1, 0), (2, 7, 9, 64, 72, 1, 1, 0), (1, 5, 5, 136, 64, 1, 1, 0),
    (3, 1, 1, 72, 64, 1, 1, 0), (2, 7, 9, 72, 64, 1, 2, 0), (2, 8, 8, 64, 160, 1, 2, 0), (4, 8, 8, 136, 8, 1, 2, 0),
    (2, 8, 8, 64, 64, 3, 1, 1), (2, 7, 9, 64, 64, 3, 1, 1), (1, 5, 5, 64, 160, 3, 1, 1), (1, 5, 5, 96, 64, 3, 1, 1), (3, 1, 1, 64, 160, 3, 1, 1),
    (2, 7, 9, 64, 160, 3, 2, 1), (2, 8, 8, 64, 64, 3, 2, 1), (1, 6, 10, 128, 64, 3, 2, 1), (1, 3, 3, 32, 32, 3, 1, 0),
]
PATCH_SHAPES = [(2, 8, 8, 64, 64, 3, 1, 1), (2, 7, 9, 64, 64, 3, 1, 1), (3, 10, 12, 64, 64, 3, 1, 1)]          # conv_patch.hip takes them at ldc = 64 under the automatic policy


def conv_out_hw(s):
    N, H, W, Cc, K, R, st, pad = s
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1


def s2_ok(s):
    N, H, W, Cc, K, R, st, pad = s
    return R == 3 and st == 2 and pad == 1 and H % 2 == 0 and W % 2 == 0 and Cc % 64 == 0 and K % 64 == 0


def conv_cases(op, dt):
    split = (0, 1) if dt == F32 else (0,)
    out = []
    for sp in split:
        if op == "conv_fwd":
            out += [CV(op, dt, s, f, split=sp) for s in CONV_SHAPES for f in ("f32", "bf16", "colsum")]
            out += [CV(op, dt, s, f, slack=0, split=sp) for s in PATCH_SHAPES for f in ("bf16", "colsum")]
        elif op in ("conv_dgrad", "conv_dgrad_wt"):
            out += [CV(op, dt, s, f, split=sp) for s in CONV_SHAPES for f in ("f32", "bf16")]
            out += [CV(op, dt, s, "inplace", split=sp) for s in CONV_SHAPES if s[5] == 1 and s[6] == 2]
            out += [CV(op, dt, s, "bf16", slack=0, split=sp) for s in PATCH_SHAPES]
        elif op in ("conv_dgrad_s2", "conv_dgrad_s2_wt"):
            out += [CV(op, dt, s, f, split=sp) for s in CONV_SHAPES if s2_ok(s) for f in ("f32", "bf16")]
        elif op == "conv_wgrad":
            out += [CV(op, dt, s, "wgrad", split=sp) for s in CONV_SHAPES + PATCH_SHAPES[2:]]
    return out


CONV_OPS = ("conv_fwd", "conv_dgrad", "conv_dgrad_wt", "conv_dgrad_s2", "conv_dgrad_s2_wt", "conv_wgrad")

# The member list of test_gpu_igemm.py::test_grouped_weight_gradients_match_members with its channel counts, at reduced spatial sizes: the three conv
# tile families (<= 64 output channels, <= 64 (r, s, ci) columns, general) and the 8-wave 256 x 256 tile; one member keeps more than 256 K tiles of
# pixels (9 x 32 x 32), so its contraction is cut into K chunks that meet through float atomics; a small ragged member; the two BERT-shaped linear
# gradients over 136 / 129 tokens and two small ones, of which one has strided operands and a strided output.
GROUP_CONVS = [(2, 8, 8, 64, 64, 3, 1, 1), (2, 7, 9, 64, 256, 1, 1, 0), (3, 5, 5, 512, 128, 1, 1, 0), (1, 7, 7, 256, 256, 3, 1, 1), (2, 3, 3, 2048, 512, 1, 1, 0),
               (9, 32, 32, 64, 64, 1, 1, 0), (5, 5, 5, 32, 72, 1, 1, 0)]
GROUP_LINEARS = [(3072, 768, 136, 0), (768, 768, 129, 0), (72, 136, 129, 8), (264, 136, 300, 0)]          # (M, N, K, slack of every row stride)


def group_case(dt, det=0, convs=None, linears=None):
    convs, linears = tuple(GROUP_CONVS if convs is None else convs), tuple(GROUP_LINEARS if linears is None else linears)
    return dict(op="wgrad_group", dt=dt, shape=(len(convs), len(linears)), form="group", det=det, split=0, convs=convs, linears=linears)


def refusal_cases(dt):
    """shapes the API refuses (check_gemm, check_ep, check_conv in csrc/gemm.hip): a non-zero return code and no output byte changed"""
    r = lambda c, why: dict(c, refuse=why)
    return [r(G("gemm_nt", dt, 64, 132, 64, "bf16"), "N % 8"), r(G("gemm_nt", dt, 64, 136, 60, "bf16"), "K % 8"), r(G("gemm_nn", dt, 64, 136, 60, "f32"), "K % 8"),
            r(G("gemm_tn", dt, 60, 136, 64, "atomic"), "M % 8"), r(G("gemm_tn", dt, 64, 132, 64, "atomic"), "N % 8"),
            r(G("gemm_nt", dt, 64, 136, 64, "f32"), "lda < K"), r(G("gemm_nn", dt, 64, 136, 64, "f32"), "ldb < N"), r(G("gemm_tn", dt, 64, 136, 64, "f32"), "lda < M"),
            r(G("gemm_nt", dt, 64, 136, 64, "bf16"), "lda % 8"), r(G("gemm_nt", dt, 64, 136, 64, "bf16"), "ldc % 8"), r(G("gemm_nt", dt, 64, 136, 64, "bf16"), "atomic without out_f32"),
            r(G("gemm_nn", dt, 64, 136, 64, "bf16"), "M = 0"),
            r(CV("conv_fwd", dt, (2, 5, 5, 40, 64, 3, 1, 1), "f32"), "window with C % 32"), r(CV("conv_dgrad", dt, (2, 5, 5, 64, 72, 3, 1, 1), "f32"), "window with K % 32"),
            r(CV("conv_fwd", dt, (2, 5, 5, 36, 64, 1, 1, 0), "f32"), "C % 8"), r(CV("conv_fwd", dt, (2, 5, 5, 64, 64, 1, 1, 0), "f32"), "Ho"),
            r(CV("conv_wgrad", dt, (2, 5, 5, 64, 68, 1, 1, 0), "wgrad"), "K % 8"), r(CV("conv_dgrad_s2", dt, (2, 7, 8, 64, 64, 3, 2, 1), "f32"), "odd H")]


TABLES = {}          # name -> function(dt) -> cases: what one test function of tests/test_gpu_gemm_edges.py runs under one storage type
for _op in DENSE:
    TABLES[_op + "_plain"] = (lambda dt, op=_op: plain_cases(op, dt))
    TABLES[_op + "_forms"] = (lambda dt, op=_op: form_cases(op, dt))
    TABLES[_op + "_long_k"] = (lambda dt, op=_op: long_k_cases(op, dt))
for _op in CONV_OPS:
    TABLES[_op] = (lambda dt, op=_op: conv_cases(op, dt))
TABLES["deterministic"] = deterministic_cases
TABLES["grouped"] = lambda dt: [group_case(dt), group_case(dt, det=1)]


def full_table(dt):
    return [c for name in TABLES for c in TABLES[name](dt)]


# ---------------------------------------------------------------------------------------------------------------- builder
class Built:
    """One case laid out in memory. allocs: name -> (storage kind, float32 values | None in a dry build); calls: [(entry, [args])] with Ref / int /
    ("conv", 12 ints) / ("ep", dict) / ("items", [dict]) arguments; expect: name -> float32 values of the whole allocation after the calls;
    stats: name -> (replicas, columns, rows written) of a replicated statistics accumulator; dirty: name -> (first, last + 1) of a region whose
    contents are undefined afterwards; bound: the largest partial sum of the case in units of its quantum."""

    def __init__(self, case, dry):
        self.case, self.dry = case, dry
        self.allocs, self.calls, self.expect, self.stats, self.dirty, self.views = {}, [], {}, {}, {}, {}
        self.bound = 0.0
        self.rng = np.random.default_rng(zlib.crc32(repr(sorted((k, str(v)) for k, v in case.items())).encode()))

    def need(self, magnitude, quantum=1.0):
        """a partial sum of this magnitude, a multiple of `quantum`, must be exact in f32"""
        b = float(magnitude) / quantum
        self.bound = max(self.bound, b)
        assert b < LIMIT, "%s: a partial sum can reach %g x %g >= 2^24: equality would not be legitimate" % (case_id(self.case), b, quantum)

    def matrix(self, name, kind, rows, cols, ld, fill):
        """[rows][cols] at row stride ld, with one more row behind it, inside an allocation filled with `fill`; returns (Ref, the [rows][cols] view of
        the values | None)"""
        size = GUARD + (rows + 1) * ld + GUARD
        data = None if self.dry else np.full(size, fill, np.float32)
        self.allocs[name] = (kind, data, size)
        self.views[name] = (rows, cols, ld)
        return Ref(name), (None if self.dry else self.view(data, name))

    def view(self, data, name):
        rows, cols, ld = self.views[name]
        return data[GUARD:GUARD + rows * ld].reshape(rows, ld)[:, :cols]

    def ints(self, shape, lo, hi):
        return self.rng.integers(lo, hi + 1, size=shape).astype(np.float64)

    def operand(self, name, kind, values_shape, ld, lo, hi):
        rows, cols = values_shape
        ref, v = self.matrix(name, kind, rows, cols, ld, np.nan)
        vals = None
        if not self.dry:
            vals = self.ints((rows, cols), lo, hi)
            v[...] = vals
        return ref, vals

    def output(self, name, kind, rows, cols, ld):
        ref, _ = self.matrix(name, kind, rows, cols, ld, PREFILL)
        if not self.dry:
            self.expect[name] = self.allocs[name][1].copy()
        return ref

    def expected(self, name):
        return self.view(self.expect[name], name)


def _store(v, kind):
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "the exact value is not an f32"
    return bf16_round(v32) if kind == BF16 else v32


def _quantum(alpha):
    return 1.0 if float(alpha).is_integer() else 0.5


def _epilogue(b, f, dt, M, N, acc, mag, ldc, ep):
    """lays out the epilogue operands of form f for an [M][N] product `acc` (float64; mag = the same product of absolute values), fills `ep`, writes
    the expectations"""
    out_f32 = bool(f["out_f32"] or dt == F32)
    okind = F32 if out_f32 else BF16
    alpha, q = f["alpha"], _quantum(f["alpha"])
    ep.update(out=b.output("out", okind, M, N, ldc), ldc=ldc, out_f32=int(f["out_f32"]), atomic=int(f["atomic"]), alpha=alpha)
    if f["bias"]:
        ep["bias"], bias = b.operand("bias", F32, (1, N), N, -4, 4)
    if f["preact"]:
        ep["preact"] = b.output("preact", dt, M, N, ldc)
    if f["relu"]:
        ep["act"] = ACT_RELU
    if f["dact"]:
        ep["dact_aux"], aux = b.operand("aux", dt, (M, N), ldc, -2, 2)
        ep["dact"] = 1
    if f["residual"]:
        ep["residual"], res = b.operand("res", dt, (M, N), ldc, -4, 4)
    if f["colsum"] is not None:
        R = f["replicas"]
        size = GUARD + (R + 1) * 3 * N + GUARD
        b.allocs["stats"] = (F32, None if b.dry else np.full(size, PREFILL, np.float32), size)
        ep.update(colsum=Ref("stats"), colsum_replicas=R, colsum_stride=3 * N, colsum_rows=f["colsum"])
    if f["ws"]:
        size = GUARD + M * N + GUARD
        data = None
        if not b.dry:
            data = np.full(size, PREFILL, np.float32)
            data[GUARD:GUARD + M * N] = 0.0
        b.allocs["ws"] = (F32, data, size)
        ep["splitk_ws"] = Ref("ws")
    if b.dry:
        return
    b.need(mag.max())
    if f["atomic"]:
        b.need(PREFILL + abs(alpha) * mag.max(), q)
        b.expected("out")[...] = _store(PREFILL + alpha * acc, F32)
        return
    v = alpha * acc
    lim = abs(alpha) * mag.max()
    if f["bias"]:
        v = v + bias
        lim += 4
    if f["preact"]:
        b.expected("preact")[...] = _store(v, dt)
    if f["relu"]:
        v = np.maximum(v, 0.0)
    if f["dact"]:
        v = v * (aux > 0)
    if f["residual"]:
        v = v + res
        lim += 4
    b.need(lim, q)
    stored = _store(v, okind)
    b.expected("out")[...] = stored
    if f["colsum"] is not None:
        s = stored.astype(np.float64)
        rows = np.full((3, N), PREFILL * R)
        rows[0] += s.sum(0)
        b.need(PREFILL + np.abs(s).sum(0).max(), q)
        if f["colsum"] != 1:
            rows[1] += (s * s).sum(0)
            b.need(PREFILL + (s * s).sum(0).max(), q * q)
        b.stats["stats"] = (R, N, rows, 1 if f["colsum"] == 1 else 2)
        b.expect["stats"] = b.allocs["stats"][1].copy()          # (the replicas are folded before they are compared: check())
    if f["ws"]:
        b.expect["ws"] = b.allocs["ws"][1].copy()
        b.dirty["ws"] = (GUARD, GUARD + M * N)


def build_gemm(case, dry=False, refuse=None):
    b = Built(case, dry)
    op, dt, (M, N, K), f = case["op"], case["dt"], case["shape"], FORMS[case["form"]]
    lo, hi = (-1, 1) if f["colsum"] is not None else (-4, 4)
    sa, sb = (2 * K if op != "gemm_tn" else 2 * M, 24) if f["ld2"] else (8, 24)
    a_shape, b_shape = {"gemm_nt": ((M, K), (N, K)), "gemm_nn": ((M, K), (K, N)), "gemm_tn": ((K, M), (K, N))}[op]
    up8 = lambda n: (n + 7) // 8 * 8
    lda, ldb = up8(a_shape[1]) + sa, up8(b_shape[1]) + sb
    ldc = 2 * up8(N) if f["ld2"] else up8(N) + 8
    if refuse in ("lda < K", "lda < M"):
        lda = a_shape[1] - 8
    if refuse == "ldb < N":
        ldb = b_shape[1] - 8
    ra, A = b.operand("A", dt, a_shape, max(lda, a_shape[1]), lo, hi)
    rb, B = b.operand("B", dt, b_shape, max(ldb, b_shape[1]), lo, hi)
    acc = mag = None
    if not dry:
        prod = {"gemm_nt": lambda x, y: x @ y.T, "gemm_nn": lambda x, y: x @ y, "gemm_tn": lambda x, y: x.T @ y}[op]
        acc, mag = prod(A, B), prod(np.abs(A), np.abs(B))
    ep = {}
    _epilogue(b, f, dt, M, N, acc, mag, ldc, ep)
    if refuse == "lda % 8":
        lda += 4
    if refuse == "ldc % 8":
        ep["ldc"] -= 4
    if refuse == "atomic without out_f32":
        ep["atomic"] = 1
    if refuse == "M = 0":
        M = 0
    b.calls.append(("clite_" + op, [ra, lda, rb, ldb, M, N, K, dt, ("ep", ep)]))
    return b


def conv_ref(x, w, stride, pad):
    """direct float64 sums: x [N][H][W][C], w [K][R][S][C] -> [N][Ho][Wo][K]"""
    N, H, W, Cc = x.shape
    K, R, S, _ = w.shape
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, Cc))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((N, Ho, Wo, K))
    for r in range(R):
        for s in range(S):
            y += xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :] @ w[:, r, s, :].T
    return y


def conv_dgrad_ref(dy, w, xshape, stride, pad):
    N, H, W, Cc = xshape
    K, R, S, _ = w.shape
    _, Ho, Wo, _ = dy.shape
    dxp = np.zeros((N, max(H + 2 * pad, R + stride * (Ho - 1)), max(W + 2 * pad, S + stride * (Wo - 1)), Cc))
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :] += dy @ w[:, r, s, :]
    return dxp[:, pad:pad + H, pad:pad + W]


def conv_wgrad_ref(dy, x, wshape, stride, pad):
    N, H, W, Cc = x.shape
    K, R, S, _ = wshape
    _, Ho, Wo, _ = dy.shape
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, Cc))
    xp[:, pad:pad + H, pad:pad + W] = x
    dw = np.zeros(wshape)
    for r in range(R):
        for s in range(S):
            patch = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :]
            dw[:, r, s, :] = dy.reshape(-1, K).T @ patch.reshape(-1, Cc)
    return dw


def _tensor(b, name, kind, shape, lo, hi):
    """a contiguous tensor between NaN guards (the convolution entry points take no row strides)"""
    n = int(np.prod(shape))
    ref, vals = b.operand(name, kind, (1, n), n, lo, hi)
    return ref, (None if vals is None else vals.reshape(shape))


def _put(b, name, kind, shape, values):
    """a derived contiguous operand (a transposed or sliced weight; values is None in a dry build) between NaN guards"""
    n = int(np.prod(shape))
    ref, v = b.matrix(name, kind, 1, n, n, np.nan)
    if not b.dry:
        v[...] = values.reshape(1, n)
    return ref


def build_conv(case, dry=False, refuse=None):
    b = Built(case, dry)
    op, dt, s, form = case["op"], case["dt"], case["shape"], case["form"]
    N, H, W, Cc, K, R, st, pad = s
    Ho, Wo = conv_out_hw(s)
    cvt = [dt, N, H, W, Cc, K, R, R, st, pad, Ho + (1 if refuse == "Ho" else 0), Wo]
    tern = form == "colsum"
    lo, hi = (-1, 1) if tern else (-4, 4)
    rx, x = _tensor(b, "x", dt, (N, H, W, Cc), lo, hi)
    rdy, dy = _tensor(b, "dy", dt, (N, Ho, Wo, K), lo, hi)
    if op == "conv_wgrad":
        n = K * R * R * Cc
        rdw, v = b.matrix("dw", F32, 1, n, n, PREFILL)
        if not dry:
            v[...] = WGRAD_PREFILL
            b.expect["dw"] = b.allocs["dw"][1].copy()
            ref = conv_wgrad_ref(dy, x, (K, R, R, Cc), st, pad)
            b.need(WGRAD_PREFILL + conv_wgrad_ref(np.abs(dy), np.abs(x), (K, R, R, Cc), st, pad).max())
            b.expected("dw")[...] = _store(WGRAD_PREFILL + ref.reshape(1, n), F32)
        b.calls.append(("clite_conv_wgrad", [rdy, rx, ("conv", cvt), rdw]))
        return b
    rw, w = _tensor(b, "w", dt, (K, R, R, Cc), lo, hi)
    wt = "_wt" in op
    if op == "conv_fwd":
        f = FORMS[{"f32": "f32", "bf16": "bf16", "colsum": "colsum"}[form]]
        M, Ncol = N * Ho * Wo, K
        acc = mag = None
        if not dry:
            acc, mag = conv_ref(x, w, st, pad).reshape(M, K), conv_ref(np.abs(x), np.abs(w), st, pad).reshape(M, K)
        ep = {}
        _epilogue(b, f, dt, M, Ncol, acc, mag, Ncol + case["slack"], ep)
        b.calls.append(("clite_conv_fwd", [rx, rw, ("conv", cvt), ("ep", ep)]))
        return b
    M, Ncol = N * H * W, Cc
    ldc = Ncol + case["slack"]
    acc = mag = None
    if not dry:
        acc, mag = conv_dgrad_ref(dy, w, (N, H, W, Cc), st, pad).reshape(M, Cc), conv_dgrad_ref(np.abs(dy), np.abs(w), (N, H, W, Cc), st, pad).reshape(M, Cc)
    ep = {}
    if form == "inplace":
        # dx += dgrad in place (residual == out, in the call's dtype): a strided 1 x 1 shortcut takes the dense GEMM over the output pixels whose rows
        # are scattered (RowMap) - the pixels in between keep what they hold
        ro, v = b.matrix("out", dt, M, Ncol, ldc, PREFILL)
        ep.update(out=ro, ldc=ldc, out_f32=0, atomic=0, alpha=1.0, residual=ro)
        if not dry:
            r0 = b.ints((M, Ncol), -4, 4)
            v[...] = r0
            b.expect["out"] = b.allocs["out"][1].copy()
            b.need(mag.max() + 4)
            b.expected("out")[...] = _store(r0 + acc, dt)
    else:
        _epilogue(b, FORMS[form], dt, M, Ncol, acc, mag, ldc, ep)
    if op in ("conv_dgrad", "conv_dgrad_wt"):
        if wt:
            rw = _put(b, "wt", dt, (Cc, R, R, K), None if dry else np.ascontiguousarray(w.transpose(3, 1, 2, 0)))
        b.calls.append(("clite_" + op, [rdy, rw, ("conv", cvt), ("ep", ep)]))
        return b
    # the four input-parity classes of a 3 x 3 / stride 2 / pad 1 dgrad, each on its own taps; together they write every row once
    for ph in (0, 1):
        for pw in (0, 1):
            r0, s0 = (ph + 1) & 1, (pw + 1) & 1
            na, nb = (3 - r0 + 1) // 2, (3 - s0 + 1) // 2
            sub = None
            if not dry:
                sub = w[:, r0::2, s0::2, :]
                sub = np.ascontiguousarray(sub.transpose(3, 1, 2, 0) if wt else sub)
            rs = _put(b, "wsub%d%d" % (ph, pw), dt, (K, na, nb, Cc), sub)
            b.calls.append(("clite_conv_dgrad_s2class" + ("_wt" if wt else ""), [rdy, rs, ("conv", cvt), ph, pw, ("ep", dict(ep))]))
    return b


def build_group(case, dry=False):
    """every member of the grouped weight-gradient launch with its own operands and its own += target"""
    b = Built(case, dry)
    dt = case["dt"]
    items = []
    for i, s in enumerate(case["convs"]):
        N, H, W, Cc, K, R, st, pad = s
        Ho, Wo = conv_out_hw(s)
        rx, x = _tensor(b, "x%d" % i, dt, (N, H, W, Cc), -4, 4)
        rdy, dy = _tensor(b, "dy%d" % i, dt, (N, Ho, Wo, K), -4, 4)
        n = K * R * R * Cc
        name = "dw%d" % i
        rdw, v = b.matrix(name, F32, 1, n, n, PREFILL)
        if not dry:
            v[...] = WGRAD_PREFILL
            b.expect[name] = b.allocs[name][1].copy()
            b.need(WGRAD_PREFILL + conv_wgrad_ref(np.abs(dy), np.abs(x), (K, R, R, Cc), st, pad).max())
            b.expected(name)[...] = _store(WGRAD_PREFILL + conv_wgrad_ref(dy, x, (K, R, R, Cc), st, pad).reshape(1, n), F32)
        items.append(dict(kind=0, a=rdy, b=rx, out=rdw, cv=[dt, N, H, W, Cc, K, R, R, st, pad, Ho, Wo]))
    for i, (M, N, K, slack) in enumerate(case["linears"]):
        lda, ldb, ldc = M + slack, N + 3 * slack, N + slack
        ra, A = b.operand("A%d" % i, dt, (K, M), lda, -4, 4)
        rb, B = b.operand("B%d" % i, dt, (K, N), ldb, -4, 4)
        name = "lin%d" % i
        ro, v = b.matrix(name, F32, M, N, ldc, PREFILL)
        if not dry:
            v[...] = WGRAD_PREFILL
            b.expect[name] = b.allocs[name][1].copy()
            b.need(WGRAD_PREFILL + (np.abs(A).T @ np.abs(B)).max())
            b.expected(name)[...] = _store(WGRAD_PREFILL + A.T @ B, F32)
        items.append(dict(kind=1, a=ra, b=rb, out=ro, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc))
    b.calls.append(("clite_wgrad_group", [dt, ("items", items)]))
    return b


def build(case, dry=False):
    """dry: the layout and the calls only (no values, no reference): what a dry run of the launchers needs"""
    refuse = case.get("refuse")
    if case["op"] in DENSE:
        return build_gemm(case, dry, refuse)
    if case["op"] == "wgrad_group":
        return build_group(case, dry)
    return build_conv(case, dry, refuse)


# ---------------------------------------------------------------------------------------------------------------- checker
def _first_difference(b, name, got, want):
    bad = np.flatnonzero(~(got == want))
    i = int(bad[0])
    where = "element %d" % i
    if name in b.views:
        rows, cols, ld = b.views[name]
        r, c = divmod(i - GUARD, ld)
        where = "row %d col %d of the [%d][%d] view (row stride %d)" % (r, c, rows, cols, ld) if i >= GUARD else "guard element %d in front of the view" % i
    return "%s: %s differs in %d elements, first at %s: got %r, expected %r" % (case_id(b.case), name, bad.size, where, float(got[i]), float(want[i]))


def check(b, got):
    """got: name -> float32 values of the whole allocation after the calls. Equality of every element of every output allocation."""
    for name, want in b.expect.items():
        g = got[name]
        assert g.shape == want.shape and g.dtype == np.float32
        if name in b.stats:
            R, N, rows, written = b.stats[name]
            reps = g[GUARD:GUARD + (R + 1) * 3 * N].reshape(R + 1, 3, N).astype(np.float64)
            outside = g.copy()
            outside[GUARD:GUARD + R * 3 * N] = PREFILL
            assert np.array_equal(outside, want), _first_difference(b, name, outside, want)          # the guards and the replica the call was not told about
            folded = reps[:R].sum(0)
            assert np.array_equal(folded, rows), "%s: column statistics differ in %d elements (row, column) %s" % (
                case_id(b.case), int((folded != rows).sum()), np.argwhere(folded != rows)[:4].tolist())
            untouched = reps[:R, written:]
            assert np.array_equal(untouched, np.full_like(untouched, PREFILL)), "%s: a statistics row the call does not accumulate changed" % case_id(b.case)
            continue
        if name in b.dirty:
            lo, hi = b.dirty[name]
            g = g.copy()
            g[lo:hi] = want[lo:hi]
        assert np.array_equal(g, want), _first_difference(b, name, g, want)


def check_untouched(b, got):
    """after a refused call: every output allocation still holds what it held"""
    for name in b.expect:
        kind, data, _ = b.allocs[name]
        assert np.array_equal(got[name], data), "%s: the refused call changed %s" % (case_id(b.case), name)
