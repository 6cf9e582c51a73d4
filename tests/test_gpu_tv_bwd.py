"""-m gpu: the TV denoiser's gradient on a real MI355X -- the shared cases of tests/tv_bwd_cases.py through the C ABI, and one
determinism case at a size with many tiles and a chain of launches.  (The run on guarded workspaces is tests/test_gpu_guard_tv_bwd.py.)"""
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


import tv_bwd_cases as bc  # noqa: E402
from dprox import _ops as ops  # noqa: E402


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


def test_tv_bwd_deterministic_over_many_tiles():
    gen = torch.Generator(device=DEV).manual_seed(0)
    v = torch.rand(2, 3, 300, 300, device=DEV, generator=gen)
    g = torch.randn(2, 3, 300, 300, device=DEV, generator=gen)
    p = ops.tv_bwd_plan(v.shape, 7, (2, 3))
    assert p["launches"] > 1 and p["tile"][1] < 300 and p["tile"][2] < 300, p
    runs = []
    for _ in range(2):
        vt = v.clone().requires_grad_(True)
        sigma = torch.tensor([0.1, 0.3], device=DEV, requires_grad=True)
        ops.tv_denoise(vt, sigma, 7, (2, 3), differentiable=True).backward(g)
        runs.append((vt.grad, sigma.grad))
    torch.cuda.synchronize()
    (gy0, gl0), (gy1, gl1) = runs
    assert torch.isfinite(gy0).all() and torch.isfinite(gl0).all() and float(gl0.abs().min()) > 0
    assert torch.equal(gy0, gy1) and torch.equal(gl0, gl1)
