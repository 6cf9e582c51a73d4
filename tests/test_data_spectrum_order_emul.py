"""CPU-only: the data spectrum in the column pass's own lane order under the SIMT emulator (tests/emul) -- the twin of
tests/test_gpu_data_spectrum_order.py on the shared cases of tests/data_spectrum_cases.py: the emulated build includes the same
index map (csrc/dpx_common.h), so producer and consumer are checked at every column length without a GPU.  The authoritative
numerics check is the GPU file."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import data_spectrum_cases as dc  # noqa: E402

DEV = "cpu"


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
