"""CPU-only: the compress_sensing x-update and its gradient (dpx_cs_xupdate / dpx_cs_backward, csrc/dpx_cs.hip) under the SIMT emulator
(tests/emul): every case of tests/cs_cases.py.  The authoritative numerics check is tests/test_gpu_cs.py on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import cs_cases as cc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("name, I", [(n, I) for n, Is in cc.PROX.items() for I in Is])
def test_cs_prox(name, I):
    cc.case_prox(DEV, name, I)


def test_cs_zero_mask_pixel():
    cc.case_zero_mask_pixel(DEV)


def test_cs_sum_in_kernel():
    cc.case_sum_in_kernel(DEV)


def test_cs_vector_path():
    cc.case_vector_path(DEV)


@pytest.mark.parametrize("name", cc.GRADS)
def test_cs_grad(name):
    cc.case_grad(DEV, name)


def test_cs_grad_shared_lam_and_two_inputs():
    cc.case_grad_shared_lam_and_two_inputs(DEV)


def test_cs_no_grad_saves_nothing():
    cc.case_no_grad_saves_nothing(DEV)


@pytest.mark.parametrize("name", cc.ADMM)
def test_cs_admm(name):
    cc.case_admm(DEV, name)


def test_cs_deterministic():
    cc.case_deterministic(DEV)


def test_cs_argument_errors():
    cc.case_argument_errors(DEV)
