"""-m gpu: the LP kernels and ``dprox.algo.lp`` on a real MI355X -- the shared cases of tests/lp_cases.py through the C ABI; with
DPX_LP_PARITY_OUT set, the measured distances of every case are written to the file it names (the judged copy is committed as
profiles/lp_parity_achieved.json)."""
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
    lc.write_achieved()


import lp_cases as lc  # noqa: E402


@pytest.mark.parametrize("lanes", [1, 8, 64])
@pytest.mark.parametrize("name", lc.STEP_CASES)
def test_lp_steps(name, lanes):
    lc.case_steps(DEV, name, lanes)


@pytest.mark.parametrize("name", lc.CASES)
def test_lp_parity(name):
    lc.case_parity(DEV, name)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_lp_objective(name):
    lc.case_objective(DEV, name)


def test_lp_nan_residual_is_not_done():
    lc.case_nan_residual(DEV)


def test_lp_refused_shapes():
    lc.case_refused_shapes(DEV)


def test_lp_deterministic():
    lc.case_deterministic(DEV, "odd")


def test_lp_public_path():
    lc.case_public(DEV, "odd")
