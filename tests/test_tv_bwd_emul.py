"""CPU-only: the TV denoiser's gradient (dpx_tv_denoise_rec / dpx_tv_backward, csrc/dpx_tv.hip) under the SIMT emulator (tests/emul): the
reference's autograd fixtures, the extensions against float64 autograd of the restatement, blocked against one-step launches bit for
bit at shapes derived from the plan, the saturation extremes.  The authoritative numerics check is tests/test_gpu_tv_bwd.py on a real
MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import tv_bwd_cases as bc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("via", ["ops", "denoiser"])
@pytest.mark.parametrize("tag", bc.FIXTURES)
def test_tv_bwd_fixture(tag, via):
    bc.case_fixture(DEV, tag, via)


def test_tv_bwd_batch_with_two_sigmas():
    bc.case_extension(DEV, (2, 3, 21, 30), (1, 2), lam=[0.05, 0.3])
    bc.case_extension(DEV, (2, 3, 21, 30), (1, 2, 3), lam=[0.05, 0.3])


def test_tv_bwd_spatial_dims():
    bc.case_extension(DEV, (2, 3, 21, 70), (2, 3), iters=7)


def test_tv_bwd_single_axis():
    bc.case_extension(DEV, (2, 3, 5, 150), (3,), iters=13)
    bc.case_extension(DEV, (1, 2, 40, 3), (2,), iters=6)


def test_tv_bwd_active_axis_of_length_1():
    bc.case_extension(DEV, (1, 1, 9, 7), (1, 2))
    bc.case_extension(DEV, (1, 1, 9, 7), (1, 2, 3))
    bc.case_extension(DEV, (1, 1, 19, 23), (1, 2, 3))          # (3-D form on one plane: the reference returns an empty tensor, so there is no fixture)


def test_tv_bwd_active_axis_of_length_2():
    bc.case_extension(DEV, (1, 2, 9, 7), (1, 2), iters=13)


def test_tv_bwd_one_iteration():
    bc.case_iters1(DEV)


@pytest.mark.parametrize("C, dims, kind", [(3, (1, 2), "plus1"), (3, (1, 2), "three"), (3, (1, 2, 3), "plus1"), (3, (1, 2, 3), "three"),
                                           (3, (1, 2, 3), "short"), (1, (2, 3), "plus1"), (2, (2, 3), "three"), (3, (2, 3), "short")])
def test_tv_bwd_blocked_equals_one_step(C, dims, kind):
    bc.case_blocking(DEV, C, dims, kind)


def test_tv_bwd_saturation_extremes():
    bc.case_saturation(DEV)


def test_tv_bwd_argument_errors():
    bc.case_argument_errors(DEV)


def test_tv_bwd_admm_end_to_end():
    bc.case_admm_grads(DEV)
