"""CPU-only: the Anderson kernels (csrc/dpx_anderson.hip) and the DEQ specialization under the SIMT emulator (tests/emul): the kernels
against a float64 restatement at odd, unaligned and aligned shapes, anderson() on a known contraction, DEQSolver against the
reference's stored runs, forward and backward.  The authoritative numerics check is tests/test_gpu_deq.py on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import deq_cases as dc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("shape, P", [((3, 1, 5, 7), 5), ((1, 3, 33, 65), 3), ((2, 3, 64, 64), 5)])
def test_anderson_kernels(shape, P, beta):
    dc.case_kernels(DEV, shape, P, beta)


def test_anderson_tiny_residuals_give_uniform_alpha():
    dc.case_tiny_residuals(DEV)


def test_anderson_contraction():
    dc.case_contraction(DEV)


def test_deq_tv_small():
    dc.case_tv(DEV, "small")


def test_deq_backward():
    dc.case_backward(DEV)
