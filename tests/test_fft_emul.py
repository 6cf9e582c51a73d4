"""CPU-only: the FFT cases of tests/fft_cases.py on the same kernel source under the SIMT emulator -- every shape that takes under about
a second there (the 10239 / 20478 lengths and four of the register-radix planes are the GPU module's, tests/test_gpu_fft.py).  The
emulator does not run the register-radix kernels as the hardware does (LDS-DMA, wave exchanges, wait counts): the GPU run is the one
that counts for those."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import fft_cases as fc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("shape", fc.EMUL_SHAPES, ids=fc.sid)
def test_fft_conv(shape):
    fc.case_conv(DEV, shape)


@pytest.mark.parametrize("shape", fc.EMUL_SHAPES, ids=fc.sid)
def test_fft_solve(shape):
    fc.case_solve(DEV, shape)


@pytest.mark.parametrize("shape", fc.CFFT_SHAPES, ids=fc.sid)
def test_cfft2(shape):
    fc.case_cfft2(DEV, shape)


@pytest.mark.parametrize("shape", fc.EMUL_PLANES, ids=fc.sid)
def test_fft_planes_do_not_interact(shape):
    fc.case_planes(DEV, shape)


@pytest.mark.parametrize("name", fc.EMUL_REFUSALS)
def test_fft_refused_length(name):
    fc.case_refusal(DEV, name)


@pytest.mark.parametrize("name", [n for n in fc.REFUSALS if n not in fc.EMUL_REFUSALS])
def test_fft_refused_length_message(name):
    """the refusal itself at the lengths whose accepted neighbour is the GPU module's: error, message, output untouched"""
    fc.case_refusal(DEV, name, neighbour=False)
