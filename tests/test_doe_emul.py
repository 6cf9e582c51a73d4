"""CPU-only: the DOE wave-optics model's kernels (csrc/dpx_doe.hip, the k_doe_* kernels of csrc/dpx_fft.hip) under the SIMT emulator
(tests/emul): the parity cases at 20 -> 20, 30 -> 10 and 32 -> 16 of tests/doe_cases.py, forward and backward, and the small entry
points.  The authoritative numerics check is tests/test_gpu_doe.py on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import doe_cases as dc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("R", (20, 30, 32))
@pytest.mark.parametrize("state", dc.STATES)
def test_doe_parity(R, state):
    dc.case_parity(DEV, R, state)


def test_doe_phase_baseline_propagator():
    dc.case_phase_baseline_propagator(DEV)


def test_doe_deterministic():
    dc.case_deterministic(DEV, R=30)


def test_doe_no_grad_stores_no_field():
    dc.case_no_grad_stores_no_field(DEV)


def test_doe_argument_errors():
    dc.case_argument_errors(DEV)


def test_doe_e2e():
    dc.case_e2e(DEV)
