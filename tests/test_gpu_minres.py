"""-m gpu: the MINRES kernels and ``dprox.linalg.solve.minres`` on a real MI355X -- the shared cases of tests/minres_cases.py
through the C ABI; with DPX_MINRES_PARITY_OUT set, the measured distances of every case are written to the file it names (the
judged copy is committed as profiles/minres_parity_achieved.json)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _hip_lib_loaded():
    from dprox import _backend as be
    assert torch.cuda.is_available()
    assert not be.host_mode()
    assert "libdpx_hip.so" in be.lib().path
    yield
    mc.write_achieved()


import minres_cases as mc  # noqa: E402


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


def test_minres_shifts_from_another_device_and_dtype():
    """a ``shifts`` tensor on the CPU, in float64 or as integers, is moved and cast, not rejected"""
    from dprox.linalg.solve import minres
    A, b, kw = mc.inputs("shift3", DEV)
    want = minres(A, b, **kw)
    for shifts in (torch.tensor([0.0, 0.5, 2.0], dtype=torch.float64, device="cpu"), kw["shifts"].to(DEV)):
        assert torch.equal(minres(A, b, **dict(kw, shifts=shifts)), want)
    ints = minres(A, b, **dict(kw, shifts=torch.tensor([0, 2], device="cpu")))
    assert torch.equal(ints[1], want[2])


def test_linear_solve_minres_gradient():
    mc.case_linear_solve(DEV)
