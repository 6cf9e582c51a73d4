"""CPU-only: the MINRES kernels (csrc/dpx_minres.hip) and ``dprox.linalg.solve.minres`` under the SIMT emulator (tests/emul): one
Lanczos + update step against a float64 restatement at odd, unaligned and aligned shapes in both element types, and the solver
against the reference's stored float32 and float64 runs.  The authoritative numerics check is tests/test_gpu_minres.py on a real
MI355X."""
import pytest
import torch

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import minres_cases as mc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(1, 5, 1), (2, 33, 3), (1, 256, 4)])
def test_minres_step(shape, dtype):
    mc.case_step(DEV, shape, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_minres_step_preconditioned(dtype):
    mc.case_step(DEV, (2, 33, 3), dtype, prec=True)


def test_minres_reference_own_test():
    mc.case_own(DEV)


def test_minres_one_unknown():
    mc.case_one_unknown(DEV)


@pytest.mark.parametrize("name", mc.F32_CASES)
def test_minres_parity(name):
    mc.case_parity(DEV, name)


def test_minres_deterministic():
    mc.case_deterministic(DEV)
