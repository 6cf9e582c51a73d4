"""CPU-only: the hybrid DOE model's kernels and the gradients to explicit arguments (csrc/dpx_doe.hip, the k_doe_* kernels of
csrc/dpx_fft.hip) under the SIMT emulator (tests/emul): the parity cases at 20 -> 20, 30 -> 10, 32 -> 16 and 33 -> 11 of
tests/doe_hybrid_cases.py with both aperture kinds, the wide case, the explicit-argument cases and the small entry points.  The
authoritative numerics check is tests/test_gpu_doe_hybrid.py on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import doe_hybrid_cases as hc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("R", (20, 30, 32, 33))
@pytest.mark.parametrize("kind", sorted(hc.KINDS))
@pytest.mark.parametrize("state", hc.STATES)
def test_doe_hybrid_parity(R, kind, state):
    hc.case_parity(DEV, R, kind, state)


@pytest.mark.parametrize("state", hc.STATES)
def test_doe_hybrid_wide(state):
    hc.case_wide(DEV, state)


def test_doe_explicit_profile():
    hc.case_explicit_profile(DEV)


def test_doe_explicit_height_map():
    hc.case_explicit_height_map(DEV)


def test_doe_explicit_field():
    hc.case_explicit_field(DEV)


def test_doe_hybrid_chain():
    hc.case_chain(DEV)


def test_doe_hybrid_deterministic():
    hc.case_deterministic(DEV, R=30)


def test_doe_hybrid_baseline_and_no_grad():
    hc.case_baseline_and_no_grad(DEV)


def test_doe_hybrid_argument_errors():
    hc.case_argument_errors(DEV)
