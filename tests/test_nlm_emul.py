"""CPU-only: the patch_nlm prior (dpx_nlm, csrc/dpx_nlm.hip) under the SIMT emulator (tests/emul): operator parity on the reference's
fixtures, gray images and non-default windows against a float64 restatement, and the reference's ADMM through the fused plan and the
generic splitting.  The authoritative numerics check is tests/test_gpu_nlm.py on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import nlm_cases as nc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("key", ["op", "wrap", "wrap0"])
def test_nlm_op(key):
    nc.case_op(DEV, key)


def test_patch_nlm_prox():
    nc.case_prox(DEV)


def test_nlm_gray():
    nc.case_restatement(DEV, (2, 1, 21, 70))


def test_nlm_windows_7_3():
    nc.case_restatement(DEV, (1, 3, 19, 23), search=7, patch=3)


@pytest.mark.parametrize("tag", ["admm", "nn"])
@pytest.mark.parametrize("fused", [True, False])
def test_patch_nlm_admm(tag, fused):
    nc.case_admm(DEV, tag, fused)
