"""CPU-only, no kernel: the host side of dprox.contrib.optic -- the float64 restatement of tests/doe_cases.py against the reference's
float64 fixture, the module surface and its defaults, the state dict, the refusals by name, and the aperture rule."""
import dataclasses

import numpy as np
import pytest
import torch

import doe_cases as dc
from dprox.contrib import optic


@pytest.mark.parametrize("R", sorted(dc.CASES))
@pytest.mark.parametrize("state", dc.STATES)
def test_restatement_matches_the_reference_in_float64(R, state):
    dc.case_restatement(R, state)


def test_restatement_of_phase_propagator_and_baseline():
    dc.case_restatement_extras()


def test_surface_and_defaults_equal_the_reference_config():
    g = dc.golden()
    for name in ("DOEModelConfig", "build_doe_model", "RGBCollimator", "HeightMap", "FresnelPropagator", "build_baseline_profile", "get_coordinate",
                 "area_downsampling", "psf2otf", "img_psf_conv", "get_one_phase_shift_thickness", "normalize_psf"):
        assert hasattr(optic, name), name
    cfg = optic.DOEModelConfig()
    assert dataclasses.is_dataclass(cfg)
    assert [f.name for f in dataclasses.fields(cfg)] == ["circular", "aperture_diameter", "sensor_distance", "num_steps", "patch_size", "sample_interval",
                                                         "model_kwargs"]
    assert cfg.refractive_idcs.dtype == torch.float32 and np.array_equal(cfg.refractive_idcs.numpy(), g["cfg_refractive_idcs"])
    assert cfg.wave_lengths.dtype == torch.float32 and np.array_equal(cfg.wave_lengths.numpy(), g["cfg_wave_lengths"])
    assert [cfg.aperture_diameter, cfg.sensor_distance, cfg.sample_interval] == [float(v) for v in g["cfg_scalars"]]
    assert [cfg.num_steps, cfg.patch_size, cfg.wave_resolution[0], cfg.wave_resolution[1], int(cfg.circular)] == [int(v) for v in g["cfg_ints"]]
    assert cfg.model_kwargs == {}


def test_model_buffers_parameter_and_state_dict():
    g = dc.golden()
    m = dc.build(32, 16, "cpu")
    assert isinstance(m, optic.RGBCollimator) and isinstance(m.height_map, optic.HeightMap) and isinstance(m.propagator, optic.FresnelPropagator)
    s = m.height_map.height_map_sqrt
    assert isinstance(s, torch.nn.Parameter) and s.shape == (1, 1, 32, 32) and s.dtype == torch.float32
    # the Fresnel initialisation is the reference's (same float32 expressions)
    assert np.allclose(s.detach().numpy(), g["r32_init_s"], rtol=1e-6, atol=0)
    assert dict(m.named_buffers()).keys() >= {"xx", "yy", "aperture", "input_field"}
    assert m.aperture.shape == (1, 1, 32, 32) and m.input_field.shape == (1, 3, 32, 32) and m.xx.shape == (32, 32)
    assert m.propagator.Mpad == 8 and m.propagator.Npad == 8
    assert list(m.state_dict()) == ["height_map.height_map_sqrt"]
    m.rhos, m.sigmas = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(3))
    assert sorted(m.state_dict()) == ["height_map.height_map_sqrt", "rhos", "sigmas"]
    # a reference checkpoint: ckpt['model'] with the reference's key
    m2 = dc.build(32, 16, "cpu")
    m2.load_state_dict({"height_map.height_map_sqrt": torch.from_numpy(g["r32_pert_s"])}, strict=True)
    assert np.array_equal(m2.height_map.height_map_sqrt.detach().numpy(), g["r32_pert_s"])


@pytest.mark.parametrize("R", (20, 30, 32, 88, 136, 1496))
def test_aperture_rule(R):
    """the exact integer rule equals the reference's float32 rule sqrt(xx^2 + yy^2) < xx.max() at every size used; for even R no lattice
    point lies on the circle"""
    xx, yy = optic.get_coordinate(R, R, 2e-6, 2e-6)
    ref = (torch.sqrt(xx ** 2 + yy ** 2) < xx.max()).numpy()
    assert np.array_equal(dc.aperture(R), ref)
    m = optic.RGBCollimator(15e-3, torch.tensor([1.4648, 1.4599, 1.4568]), torch.tensor([460, 550, 640]) * 1e-9, R // 2, 2e-6, (R, R)) if R <= 136 else None
    if m is not None:
        assert np.array_equal(m.aperture[0, 0].numpy() != 0, ref)
    if R % 2 == 0:
        a = 2 * np.arange(R, dtype=np.int64) - (R - 1)
        assert not ((a[:, None] ** 2 + a[None, :] ** 2) == (R - 1) ** 2).any()


def test_helpers():
    x = torch.arange(2 * 3 * 6 * 6, dtype=torch.float32).reshape(2, 3, 6, 6)
    assert torch.equal(optic.area_downsampling(x, 2), torch.nn.functional.avg_pool2d(x, 3, 3))
    with pytest.raises(NotImplementedError, match="no multiple"):
        optic.area_downsampling(x, 4)
    wl, n = torch.tensor([460e-9, 550e-9]), torch.tensor([1.46, 1.45])
    assert torch.allclose(optic.get_one_phase_shift_thickness(wl, n), wl / (n - 1))
    psf = np.random.RandomState(0).rand(8, 8, 3)
    out = optic.normalize_psf(psf.copy())
    assert out.shape == psf.shape and out.max() == 1.0 and out.min() >= 0
    otf = optic.psf2otf(torch.ones(1, 3, 4, 4) / 16, (1, 3, 8, 8))
    assert otf.shape == (1, 3, 8, 8) and torch.allclose(otf[0, :, 0, 0].real, torch.ones(3))


def test_refusals_by_name():
    ri, wl = torch.tensor([1.4648, 1.4599, 1.4568]), torch.tensor([460, 550, 640]) * 1e-9
    with pytest.raises(NotImplementedError, match="rectangular"):
        optic.RGBCollimator(15e-3, ri, wl, 16, 2e-6, (32, 48))
    with pytest.raises(NotImplementedError, match="three wavelengths"):
        optic.RGBCollimator(15e-3, ri[:2], wl[:2], 16, 2e-6, (32, 32))
    with pytest.raises(NotImplementedError, match="no multiple of the patch size"):
        optic.RGBCollimator(15e-3, ri, wl, 12, 2e-6, (32, 32))
    with pytest.raises(NotImplementedError, match="three"):
        optic.FresnelPropagator((1, 4, 32, 32), 15e-3, 2e-6, torch.ones(4) * 5e-7)
    with pytest.raises(NotImplementedError, match="doe_model_hybrid"):
        import dprox.contrib.optic.doe_model_hybrid  # noqa: F401
    for name in ("U_Net", "Dataset", "load_sample_img", "sanity_check", "plot", "subplot", "plot3d"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(optic, name)()
    # float64 / bf16 parameters, a phase profile that requires a gradient, wrong shapes: refused before anything is launched
    m = dc.build(32, 16, "cpu")
    ctx = type("Ctx", (), {"R": 32, "P": 16})()
    from dprox import _ops as ops
    for dtype, word in ((torch.float64, "float64"), (torch.bfloat16, "bfloat16")):
        with pytest.raises(NotImplementedError, match=word):
            ops.doe_psf(ctx, m.height_map.height_map_sqrt.detach().to(dtype))
    with pytest.raises(NotImplementedError, match="phase_profile"):
        ops.doe_psf_from_profile(ctx, torch.zeros(1, 3, 32, 32, dtype=torch.complex64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="complex128"):
        ops.doe_psf_from_profile(ctx, torch.zeros(1, 3, 32, 32, dtype=torch.complex128))
    with pytest.raises(ValueError, match="shape"):
        ops.doe_psf(ctx, torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="explicit field"):
        ops.doe_propagate(ctx, torch.zeros(1, 3, 32, 32, dtype=torch.complex64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="explicit height map"):
        m.height_map.get_phase_profile(torch.zeros(1, 1, 32, 32, requires_grad=True))
    with pytest.raises(NotImplementedError, match="three"):
        ops.doe_phase(torch.zeros(4, 4), True, [5e-7, 6e-7], [1.4, 1.5])
