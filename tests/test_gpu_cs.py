"""-m gpu: the compress_sensing x-update and its gradient on a real MI355X -- the shared cases of tests/cs_cases.py through the C ABI, one
case at a size with many workgroups per image, and the achieved distances (DPX_CS_PARITY_OUT -> profiles/cs_parity_achieved.json).
(The run on guarded workspaces is tests/test_gpu_guard_cs.py.)"""
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
    cc.write_achieved()


import cs_cases as cc  # noqa: E402
from dprox import _ops as ops  # noqa: E402


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


def test_cs_deterministic_over_many_workgroups():
    """300 x 301 pixels: 353 workgroups per image, so the last-workgroup sum of glam adds partials across XCDs; a shared mask and a shared y
    make the thread loop over the three images"""
    gen = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randn(3, 5, 300, 301, device=DEV, generator=gen)
    g = torch.randn(3, 5, 300, 301, device=DEV, generator=gen)
    mask = torch.randn(1, 5, 300, 301, device=DEV, generator=gen)
    y = torch.randn(1, 1, 300, 301, device=DEV, generator=gen)
    runs = []
    for _ in range(2):
        ts = [t.clone().requires_grad_(True) for t in (v, y, torch.tensor([0.1, 0.3, 1.0], device=DEV), mask)]
        ops.cs_xupdate([ts[0]], ts[1], ts[3], ts[2], 2).backward(g)
        runs.append([t.grad for t in ts])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and torch.equal(a, b)
    # against the restatement: the batch sums and the reduction at this size
    gv, gy, glam, gmask, _ = cc.restate_grad(g.cpu().numpy(), v.cpu().numpy(), mask.cpu().numpy(), y.cpu().numpy(), [0.1, 0.3, 1.0], 2)
    for ours, ref in zip(runs[0], (gv, gy, glam, gmask)):
        assert cc.rel_l2(ours.cpu().numpy(), ref) <= cc.SLACK
