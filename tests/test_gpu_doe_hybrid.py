"""-m gpu: the hybrid DOE model and the gradients to explicit arguments on a real MI355X -- every fixture case of
tests/doe_hybrid_cases.py forward and backward; the achieved distances go to the file DPX_DOE_HYBRID_PARITY_OUT names
(-> profiles/doe_hybrid_parity_achieved.json)."""
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
    hc.write_achieved()


import doe_hybrid_cases as hc  # noqa: E402


@pytest.mark.parametrize("R", sorted(hc.CASES))
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
    hc.case_deterministic(DEV)


def test_doe_hybrid_baseline_and_no_grad():
    hc.case_baseline_and_no_grad(DEV)


def test_doe_hybrid_argument_errors():
    hc.case_argument_errors(DEV)
