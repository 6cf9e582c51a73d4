"""-m gpu: the DOE wave-optics model on a real MI355X -- every fixture case of tests/doe_cases.py forward and backward, the small entry
points, the end-to-end chain, and one case at the default configuration (1496 -> 748), the only size at which the transforms run with
one or a few sequences per workgroup; the achieved distances go to the file DPX_DOE_PARITY_OUT names
(-> profiles/doe_parity_achieved.json)."""
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
    dc.write_achieved()


import doe_cases as dc  # noqa: E402
from dprox.contrib import optic  # noqa: E402


@pytest.mark.parametrize("R", sorted(dc.CASES))
@pytest.mark.parametrize("state", dc.STATES)
def test_doe_parity(R, state):
    dc.case_parity(DEV, R, state)


def test_doe_phase_baseline_propagator():
    dc.case_phase_baseline_propagator(DEV)


def test_doe_deterministic():
    dc.case_deterministic(DEV)


def test_doe_no_grad_stores_no_field():
    dc.case_no_grad_stores_no_field(DEV)


def test_doe_argument_errors():
    dc.case_argument_errors(DEV)


def test_doe_e2e():
    dc.case_e2e(DEV)


def test_doe_default_configuration():
    """1496 -> 748 (M = 2244 = 4 * 3 * 11 * 17: one row, four columns per workgroup, the any-prime pass), the model built from its
    defaults, forward and backward against the float64 restatement of tests/doe_cases.py evaluated with torch on the device.  Bounds:
    1e-5 for the PSF; for the gradient 1e-5 plus the largest float32-vs-float64 gradient distance the reference itself shows in
    g48_doe*.npz.  Two runs give the same bits."""
    g = dc.golden()
    cfg = optic.DOEModelConfig()
    m = optic.build_doe_model(cfg).to(DEV)
    R, P = cfg.wave_resolution[0], cfg.patch_size
    assert (R, P) == (1496, 748) and m.propagator.H.shape == (1, 3, 2244, 2244)
    gen = torch.Generator().manual_seed(1496)
    w = torch.randn(1, 3, P, P, generator=gen).to(DEV)
    with torch.no_grad():
        m.height_map.height_map_sqrt.mul_((1 + 0.2 * torch.rand(1, 1, R, R, generator=gen)).to(DEV))
    psf, grad = dc.psf_and_grad(m, w)
    psf2, grad2 = dc.psf_and_grad(m, w)
    assert torch.equal(psf, psf2) and torch.equal(grad, grad2)
    assert bool((psf >= 0).all()) and abs(float(psf.double().sum()) - 1.0) <= 1e-6
    s64 = m.height_map.height_map_sqrt.detach().double().requires_grad_(True)
    ref = dc.restate(s64, R, P, DEV)
    (ref * w.double()).sum().backward()
    bound_grad = dc.SLACK + max(float(g[f"r{r}_{st}_d_grad"]) for r in dc.CASES for st in dc.STATES)
    for what, ours, want, bound in (("psf", psf, ref.detach(), dc.SLACK), ("grad", grad, s64.grad, bound_grad)):
        r = float((ours.double() - want).norm() / want.norm())
        dc.note("1496->748 pert (vs the float64 restatement)", what, r, bound)
        assert r <= bound, (what, r, bound)
    assert np.isfinite(float(grad.abs().max())) and float(grad.abs().max()) > 0
