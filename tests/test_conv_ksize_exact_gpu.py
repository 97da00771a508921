"""GPU: the conv family at kernel sizes 3 and 1 -- forward, data gradient, filter gradient -- on exact integer data, one case per
route and cell of tests/conv_ksize_cases.py (tests/test_conv_ksize_cases_cpu.py proves every case exact in float32 and on its claimed
route on the CPU).  tests/test_conv_ksize_gpu.py holds the same kernels to a tolerance of about 1e-4 of the output scale; here every
comparison is array_equal against the float64 oracle, so one tap applied at a wrong border pixel, one K step dropped at a split-K
seam, a padding tap read as data, or a tapless phase that stores anything but zero moves an output by at least 1 and fails.

The harness is the one of tests/test_conv_exact_gpu.py, imported, not restated: guarded 16-byte-aligned views for every operand,
output, split-K scratch and slab buffer, NaN-filled outputs and workspaces exactly as long as their queries report, bit-unchanged
inputs, the recorded launch names equal to the restated ones (the gather-GEMM's tile, order and skipped padding taps through the
matrix-pipe flops of prof_records(with_exec=True), the filter-gradient modes through the slab count).  The kernel size travels as the
seventh element of the case shape.

Not here: tanh (inexact; tests/test_conv_ksize_gpu.py holds it to its tolerance at k = 3 and 1), the tuning-aid switches, the
2^29 / 2^31 guards, and the once-read switches of conv_cases.SWITCHED_ENV -- the generic families they expose at 5x5 are the ones
these tables reach directly, so no child process is needed."""
import pytest

import conv_cases as CC
import conv_ksize_cases as KC
import test_conv_exact_gpu as T

pytestmark = pytest.mark.gpu

ROUTE_IDS = [CC.case_id(c[0]) for c in KC.ROUTE_CASES]
WGRAD_IDS = [CC.case_id(c[0]) for c in KC.WGRAD_CASES]
FWD_CASES = [c[0] for c in KC.ROUTE_CASES if c[1] is not None]
DGRAD_CASES = [c[0] for c in KC.ROUTE_CASES if c[3] is not None]
ids = lambda tbl: [CC.case_id(c) for c in tbl]
way_ids = lambda tbl: [T.way_id(t) for t in tbl]


@pytest.mark.parametrize("shape", FWD_CASES, ids=ids(FWD_CASES))
def test_forward_exact_on_its_route(shape):
    T.check_route_exact(0, shape)


@pytest.mark.parametrize("shape", DGRAD_CASES, ids=ids(DGRAD_CASES))
def test_data_gradient_exact_on_its_route(shape):
    """The phases of a 1x1 stride-2 data gradient that have no tap are exact zeros of the reference, written over the NaN."""
    T.check_route_exact(1, shape)


@pytest.mark.parametrize("case", KC.WGRAD_CASES, ids=WGRAD_IDS)
def test_filter_gradient_exact_on_its_mode(case):
    T.check_filter_gradient_exact(case[0])


@pytest.mark.parametrize("bwd,shape", KC.EPI_CASES, ids=way_ids(KC.EPI_CASES))
def test_epilogues_exact(bwd, shape):
    T.check_epilogues_exact(bwd, shape)


@pytest.mark.parametrize("bwd,shape", KC.STATS_CASES, ids=way_ids(KC.STATS_CASES))
def test_statistics_epilogue_exact(bwd, shape):
    T.check_statistics_epilogue_exact(bwd, shape)


@pytest.mark.parametrize("bwd,shape", KC.ISOLATION_ROUTES, ids=way_ids(KC.ISOLATION_ROUTES))
def test_a_nan_image_stays_inside_itself(bwd, shape):
    T.check_a_nan_image_stays_inside_itself(bwd, shape)


@pytest.mark.parametrize("bwd,shape", KC.ISOLATION_ROUTES, ids=way_ids(KC.ISOLATION_ROUTES))
def test_two_runs_are_bit_identical(bwd, shape):
    T.check_two_runs_are_bit_identical(bwd, shape)


@pytest.mark.parametrize("shape", KC.ISOLATION_WGRAD, ids=ids(KC.ISOLATION_WGRAD))
def test_two_filter_gradient_runs_are_bit_identical(shape):
    T.check_two_filter_gradient_runs_are_bit_identical(shape)
