"""-m gpu: every FFT path on a real MI355X against numpy's float64 FFT with flat-spectrum operators -- the shared cases of
tests/fft_cases.py at every shape of its lists (the boundaries of make_plan, il_seqs and lds_geom, the largest accepted lengths, every
register-radix plane length), and the achieved distances (DPX_FFT_PARITY_OUT -> profiles/fft_parity_achieved.json).  The emulator's share
is tests/test_fft_emul.py; the runs on guarded workspaces are in tests/test_gpu_guarded.py."""
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
    fc.write_achieved()


import fft_cases as fc  # noqa: E402


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.sid)
def test_fft_conv(shape):
    fc.case_conv(DEV, shape)


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.sid)
def test_fft_solve(shape):
    fc.case_solve(DEV, shape)


@pytest.mark.parametrize("shape", fc.CFFT_SHAPES, ids=fc.sid)
def test_cfft2(shape):
    fc.case_cfft2(DEV, shape)


@pytest.mark.parametrize("shape", fc.PLANES, ids=fc.sid)
def test_fft_planes_do_not_interact(shape):
    fc.case_planes(DEV, shape)


@pytest.mark.parametrize("name", list(fc.REFUSALS))
def test_fft_refused_length(name):
    fc.case_refusal(DEV, name)
