"""CPU-only: the TV denoiser (dpx_tv_denoise, csrc/dpx_tv.hip) under the SIMT emulator (tests/emul): operator parity on the reference's
fixtures, the extensions against a float64 restatement, blocked against one-step launches bit for bit at shapes derived from the plan,
and the reference's ADMM through the fused plan and the generic splitting.  The authoritative numerics check is tests/test_gpu_tv.py
on a real MI355X."""
import pytest

import emul_util


@pytest.fixture(scope="module", autouse=True)
def _emulated():
    emul_util.use_emulator()
    yield


import tv_cases as tc  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("tag, vol, it, li", tc.FN_KEYS)
def test_tv_fn(tag, vol, it, li):
    tc.case_fn(DEV, tag, vol, it, li)


@pytest.mark.parametrize("tag", ["den2", "den3"])
def test_tv_denoiser(tag):
    tc.case_den(DEV, tag)


def test_tv_batch_with_two_sigmas():
    tc.case_restatement(DEV, (2, 3, 21, 30), (1, 2), lam=[0.05, 0.3])
    tc.case_restatement(DEV, (2, 3, 21, 30), (1, 2, 3), lam=[0.3, 0.05])


@pytest.mark.parametrize("shape", [(2, 3, 21, 70), (1, 1, 19, 23)])
def test_tv_spatial_dims(shape):
    tc.case_restatement(DEV, shape, (2, 3), iters=7)


def test_tv_active_axis_of_length_1():
    tc.case_restatement(DEV, (1, 1, 9, 7), (1, 2))
    tc.case_restatement(DEV, (1, 1, 9, 7), (1, 2, 3), iters=13)


def test_tv_active_axis_of_length_2():
    tc.case_restatement(DEV, (1, 2, 9, 7), (1, 2), iters=13)
    tc.case_restatement(DEV, (2, 3, 2, 11), (2, 3), iters=6)


def test_tv_single_axis():
    tc.case_restatement(DEV, (2, 3, 5, 150), (3,), iters=13)
    tc.case_restatement(DEV, (1, 2, 40, 3), (2,), iters=6)


def test_tv_axes_are_the_references():
    tc.case_axes_not_fixed(DEV)


def test_tv_lam_zero_is_the_identity():
    tc.case_lam0(DEV)


@pytest.mark.parametrize("C, dims, kind", [(3, (1, 2), "plus1"), (3, (1, 2), "three"), (3, (1, 2, 3), "plus1"), (3, (1, 2, 3), "three"),
                                           (3, (1, 2, 3), "short"), (1, (2, 3), "plus1"), (2, (2, 3), "three"), (3, (2, 3), "short")])
def test_tv_blocked_equals_one_step(C, dims, kind):
    tc.case_blocking(DEV, C, dims, kind)


@pytest.mark.parametrize("tag", ["admm2", "admm3"])
@pytest.mark.parametrize("fused", [True, False])
def test_tv_admm(tag, fused):
    tc.case_admm(DEV, tag, fused)


def test_tv_hqs_runs_fused():
    tc.case_hqs_runs_fused(DEV)


@pytest.mark.parametrize("name", ["tv", "tv3d"])
def test_deep_prior_resolves_tv_by_name(name):
    tc.case_registry_name(DEV, name)


def test_tv_argument_errors():
    tc.case_argument_errors(DEV)
