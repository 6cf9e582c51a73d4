"""-m gpu: the Anderson kernels and the DEQ specialization on a real MI355X -- the shared cases of tests/deq_cases.py through the C
ABI, and TV deconvolution at 1 x 3 x 256 x 256 (power-of-two planes) against the reference's stored run."""
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


import deq_cases as dc  # noqa: E402


@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("shape, P", [((3, 1, 5, 7), 5), ((1, 3, 33, 65), 3), ((2, 3, 64, 64), 5)])
def test_anderson_kernels(shape, P, beta):
    dc.case_kernels(DEV, shape, P, beta)


def test_anderson_tiny_residuals_give_uniform_alpha():
    dc.case_tiny_residuals(DEV)


def test_anderson_contraction():
    dc.case_contraction(DEV)


@pytest.mark.parametrize("which", ["small", "256"])
def test_deq_tv(which):
    dc.case_tv(DEV, which)


def test_deq_backward():
    dc.case_backward(DEV)


def test_specialize_deq_lives_on_the_solvers_device():
    import dprox as dp
    g = dc.load_golden("g41_deq_tv")
    solver = dc.tv_solver(dc.T(g["b"], DEV), g["psf"], DEV)
    model = dp.specialize(solver, method="deq", device=DEV)
    assert isinstance(model, dp.DEQSolver) and model.internal.device.type == "cuda"
