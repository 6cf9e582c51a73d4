"""-m gpu: the GRUNet denoiser prior on a real MI355X -- the shared cases of tests/grunet_cases.py (layers through dpx_qrnn3d_layer, the whole
network through GRUNetDenoiser, the registry, ADMM, determinism, the range trap, errors) and the achieved distances
(DPX_GRUNET_PARITY_OUT -> profiles/grunet_parity_achieved.json).  (The run on guarded workspaces is tests/test_gpu_guard_grunet.py.)"""
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
    gc.write_achieved()


import grunet_cases as gc  # noqa: E402


@pytest.mark.parametrize("name", [n for n in gc.LAYERS if not n.startswith("saturated")])
@pytest.mark.parametrize("mode", [3, 6])
def test_grunet_layer(name, mode):
    gc.case_layer(DEV, name, mode)


def test_grunet_layer_saturated_gates():
    gc.case_saturated(DEV)


def test_grunet_layer_residual_operand_and_channel_offset():
    gc.case_residual_offset(DEV)


@pytest.mark.parametrize("name", list(gc.NETS))
def test_grunet_network(name):
    gc.case_net(DEV, name)


def test_grunet_denoise_and_registry(tmp_path):
    gc.case_registry(DEV, tmp_path)


def test_grunet_scalar_sigma_for_a_batch():
    gc.case_scalar_sigma_batch(DEV)


def test_grunet_admm():
    gc.case_admm(DEV)


def test_grunet_deterministic():
    gc.case_deterministic(DEV)


def test_grunet_range_trap_and_fallback():
    gc.case_range(DEV)


def test_grunet_errors():
    gc.case_errors(DEV)
