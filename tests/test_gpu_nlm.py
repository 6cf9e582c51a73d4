"""-m gpu: the patch_nlm prior on a real MI355X -- the shared cases of tests/nlm_cases.py through the C ABI, and size-dependent
properties at the issue's shapes (8 x 3 x 1024^2: finite, in [0, 1], bit-identical over two calls; 1 x 3 x 512^2 against float64)."""
import numpy as np
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


import dprox as dp  # noqa: E402
import nlm_cases as nc  # noqa: E402
from conftest import assert_close  # noqa: E402
from dprox import _ops as ops  # noqa: E402


@pytest.mark.parametrize("key", ["op", "wrap", "wrap0"])
def test_nlm_op(key):
    nc.case_op(DEV, key)


def test_patch_nlm_prox():
    nc.case_prox(DEV)


def test_nlm_gray():
    nc.case_restatement(DEV, (2, 1, 21, 70))


def test_nlm_windows_7_3():
    nc.case_restatement(DEV, (1, 3, 19, 23), search=7, patch=3)


def test_nlm_windows_generic_extremes():
    nc.case_restatement(DEV, (1, 3, 40, 150), search=21, patch=9)
    nc.case_restatement(DEV, (1, 1, 70, 33), search=3, patch=1)


@pytest.mark.parametrize("tag", ["admm", "nn"])
@pytest.mark.parametrize("fused", [True, False])
def test_patch_nlm_admm(tag, fused):
    nc.case_admm(DEV, tag, fused)


def test_patch_nlm_problem_runs_fused():
    g = nc.load_golden("g40_patch_nlm")
    fns, lams, b = nc.admm_problem(g, DEV, "admm")
    prob = dp.Problem(fns)
    with torch.no_grad():
        x = prob.solve(method="admm", device=DEV, x0=b, rhos=nc.T(g["rhos"], DEV), lams=lams, max_iter=5)
    assert prob.solver.last_path == "fused"
    assert_close(x.cpu().numpy(), g["admm_x"], nc.TOL, "Problem.solve x vs reference fp32")


def test_nlm_config2_shape_deterministic():
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.rand(8, 3, 1024, 1024, device=DEV, generator=g)
    sigma = torch.linspace(0.02, 0.1, 8, device=DEV)
    a = ops.nlm(v, sigma)
    b = ops.nlm(v, sigma)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    assert torch.equal(a, b)


def nlm_torch_f64(v, sigma, search=11, patch=5):
    """nlm_cases.nlm_f64 as torch ops in float64 on the device (the roll loop of the formula; the shift stack is never formed)"""
    v = v.double()
    y = 0.299 * v[:, 0] + 0.587 * v[:, 1] + 0.114 * v[:, 2]
    rs, rp = search // 2, patch // 2
    h = (torch.relu(2 * sigma.double()) + 1e-6).view(-1, 1, 1)
    num, den = torch.zeros_like(v), torch.zeros_like(y)
    for dx in range(-rs, rs + 1):
        for dy in range(-rs, rs + 1):
            d2 = (y - torch.roll(y, (dy, dx), (1, 2))) ** 2
            D = torch.zeros_like(d2)
            for oy in range(-rp, rp + 1):
                for ox in range(-rp, rp + 1):
                    D += torch.roll(d2, (oy, ox), (1, 2))
            w = torch.exp(-torch.sqrt(D) / h)
            num += w[:, None] * torch.roll(v, (dy, dx), (2, 3))
            den += w
    return torch.clamp(num / den[:, None], 0, 1)


def test_nlm_512_vs_float64():
    rng = np.random.RandomState(5)
    v = torch.from_numpy((0.5 + 0.2 * rng.randn(1, 3, 512, 512)).astype(np.float32)).to(DEV)
    sigma = torch.tensor([0.05], device=DEV)
    out = ops.nlm(v, sigma)
    ref = nlm_torch_f64(v, sigma)
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), nc.TOL_OP, "nlm 1x3x512^2 vs float64", maxabs_mult=nc.MAXABS_OP)
