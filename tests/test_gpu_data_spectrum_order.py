"""-m gpu: the data spectrum in the column pass's own lane order (csrc/dpx_common.h, spec_cols_order_index) on a real MI355X -- the
shared cases of tests/data_spectrum_cases.py: producer (dpx_data_spectrum) and consumer (k_cols_p2 through dpx_fourier_solve) at
every column length of the register-radix path against the float64 x-update, the accumulating form, per-image placement, and the
two-kernel iteration's sub-batch chains against one chain."""
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


import data_spectrum_cases as dc  # noqa: E402


@pytest.mark.parametrize("H", dc.HS)
def test_placement(H):
    dc.case_placement(DEV, H)


@pytest.mark.parametrize("H", dc.HS)
def test_accumulate(H):
    dc.case_accumulate(DEV, H)


@pytest.mark.parametrize("H", dc.HS)
def test_per_image_placement(H):
    dc.case_per_image(DEV, H)


def test_sub_batch_chains_are_bit_identical_to_one_chain():
    dc.case_chains(DEV)
