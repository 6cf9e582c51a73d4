"""CPU-only: the QRNN3D layer kernels (k_conv3d_gates, k_qrnn_pool, csrc/dpx_qrnn3d.hip) under the SIMT emulator (tests/emul): the layer
cases of tests/grunet_cases.py in the default arithmetic, one of each form in split-bf16, and the host-side errors.  The whole network
(14 million weights through the emulated matrix instruction) is left to tests/test_gpu_grunet.py on a real MI355X, the authoritative
numerics check."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import grunet_cases as gc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("name", [n for n in gc.LAYERS if not n.startswith("saturated")])
def test_grunet_layer(name):
    gc.case_layer(DEV, name)


@pytest.mark.parametrize("name", ["k3_fwd_s1", "down_rev_s1", "deconv_k1_rev_s1", "up_rev_s1", "bide_s1"])
def test_grunet_layer_split_bf16(name):
    gc.case_layer(DEV, name, 6)


def test_grunet_layer_saturated_gates():
    gc.case_saturated(DEV)


def test_grunet_layer_residual_operand_and_channel_offset():
    gc.case_residual_offset(DEV)
