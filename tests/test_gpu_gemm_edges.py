"""The implicit-GEMM engine's tile edges on the GPU, bit for bit. Every case of tests/gemm_exact.py (integer operands: exact in f32 whatever the
summation order; NaN slack around every operand; 7.0 sentinels around every output) runs on the real kernels - the LDS-DMA ring, the MFMA layouts,
the hardware's out-of-range buffer reads - and the WHOLE of every output allocation must equal the float64 reference. There is no tolerance and no
excluded element in this file: gemm_exact.check compares with numpy.array_equal.

One test function per routine walks its shape table (a launch costs well under a millisecond), under each tile policy for bf16 storage and once
for f32 storage (plain and as split bf16: gemm_exact's tables carry the switches). tests/test_wavesim_gemm_edges.py runs a subset of the same table
on the simulator and pins which kernel families the table reaches; tests/test_gpu_igemm.py keeps the full-size shapes and the adjoint identities."""
import pytest

import gemm_exact as X
from gemm_exact import BF16, F32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from gemm_backends import HipBackend
    return HipBackend()


@pytest.fixture(autouse=True, params=[(0, BF16), (1, BF16), (2, BF16), (3, BF16), (4, BF16), (0, F32)], ids=["auto", "w128", "w256x128", "w256", "narrow", "f32"])
def tile_policy(request, gpu):
    """bf16 storage under the automatic tile choice and with each tile family forced (include/clite.h: clite_set_tile_policy); f32 storage, which
    ignores the policy, once. Yields the storage type whose table the test walks."""
    policy, dt = request.param
    gpu.set_tile_policy(policy)
    try:
        yield dt
    finally:
        gpu.set_tile_policy(0)


def walk(gpu, cases):
    """every case; all failures are reported together, each naming the routine, the shape (its residues name the edge) and the first wrong element"""
    assert cases
    failures = []
    for case in cases:
        b = X.build(case)
        rcs, got = gpu.run(b)          # (restores the deterministic and f32-split switches in a finally)
        try:
            assert not any(rcs), "%s: return codes %s" % (X.case_id(case), rcs)
            X.check(b, got)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d cases differ:\n%s" % (len(failures), len(cases), "\n".join(failures[:40]))


@pytest.mark.parametrize("op", X.DENSE)
def test_dense_plain_stores_at_every_residue(gpu, tile_policy, op):
    walk(gpu, X.TABLES[op + "_plain"](tile_policy))


@pytest.mark.parametrize("op", X.DENSE)
def test_dense_epilogue_forms(gpu, tile_policy, op):
    walk(gpu, X.TABLES[op + "_forms"](tile_policy))


@pytest.mark.parametrize("op", X.DENSE)
def test_dense_long_k_split_over_the_xcds(gpu, tile_policy, op):
    walk(gpu, X.TABLES[op + "_long_k"](tile_policy))


def test_deterministic_mode(gpu, tile_policy):
    walk(gpu, X.TABLES["deterministic"](tile_policy))


@pytest.mark.parametrize("op", X.CONV_OPS)
def test_convolutions(gpu, tile_policy, op):
    walk(gpu, X.TABLES[op](tile_policy))


def test_grouped_weight_gradients_against_float64(gpu, tile_policy):
    walk(gpu, X.TABLES["grouped"](tile_policy))


def test_refused_shapes_return_an_error_and_write_nothing(gpu, tile_policy):
    for case in X.refusal_cases(tile_policy):
        b = X.build(case)
        rcs, got = gpu.run(b)
        assert all(rc != 0 for rc in rcs), (case["refuse"], rcs)
        X.check_untouched(b, got)
