"""CPU-only, no kernel: the host side of dprox.contrib.optic.doe_hybrid -- the module surface and its defaults, the state dict,
the refusals, the aperture rules, and the float64 host tables (refractive_len, the Fresnel initialisation) against the reference's
float64 run in tests/golden/g49_doe_hybrid.npz."""
import dataclasses

import numpy as np
import pytest
import torch

import doe_hybrid_cases as hc
from dprox import _ops as ops
from dprox.contrib.optic import doe_hybrid as hyb


def test_surface_and_defaults_equal_the_reference_config():
    g = hc.golden()
    for name in ("HeightMap", "RGBCollimator", "DOEModelConfig", "build_doe_model", "build_baseline_profile", "wvls", "RI"):
        assert hasattr(hyb, name), name
    cfg = hyb.DOEModelConfig()
    assert dataclasses.is_dataclass(cfg)
    assert [f.name for f in dataclasses.fields(cfg)] == ["circular", "aperture_diameter", "aperture_type", "sensor_distance", "num_steps", "patch_size",
                                                         "sample_interval", "model_kwargs"]
    # the values of the reference's float64 run, and within float32 rounding of the reference's shipped float32 values
    assert np.array_equal(cfg.wave_lengths.numpy(), g["cfg_wave_lengths"]) and np.array_equal(cfg.refractive_idcs.numpy(), g["cfg_refractive_idcs"])
    assert np.array_equal(cfg.wave_lengths.float().numpy(), g["cfg_wave_lengths32"])
    assert np.allclose(cfg.refractive_idcs.numpy(), g["cfg_refractive_idcs32"], rtol=2e-7, atol=0)
    assert torch.equal(hyb.wvls, torch.tensor([460, 550, 640])) and hyb.RI is cfg.refractive_idcs
    assert [cfg.aperture_diameter, cfg.sensor_distance, cfg.sample_interval] == [float(v) for v in g["cfg_scalars"][:3]]
    assert [cfg.num_steps, cfg.patch_size, cfg.wave_resolution[0], cfg.wave_resolution[1], int(cfg.circular)] == [int(v) for v in g["cfg_ints"]]
    assert (cfg.aperture_diameter, cfg.sensor_distance, cfg.patch_size, cfg.sample_interval, cfg.wave_resolution) == (9e-3, 50e-3, 512, 5.4e-6, (1536, 1536))
    assert cfg.aperture_type == str(g["cfg_aperture_type"]) == "half_circular" and cfg.model_kwargs == {}


def test_state_dict_is_the_reference_s():
    g = hc.golden()
    m = hc.build(32, 16, "half", "cpu")
    assert isinstance(m, hyb.RGBCollimator) and isinstance(m.height_map, hyb.HeightMap)
    s = m.height_map.height_map_sqrt
    assert isinstance(s, torch.nn.Parameter) and s.shape == (1, 1, 32, 32) and s.dtype == torch.float32
    assert dict(m.named_buffers()).keys() >= {"xx", "yy", "aperture", "input_field", "refractive_len"}
    assert m.refractive_len.shape == (1, 3, 32, 32) and m.refractive_len.dtype == torch.float32
    assert list(m.state_dict()) == ["height_map.height_map_sqrt"]
    m.load_state_dict({"height_map.height_map_sqrt": torch.from_numpy(g["r32_half_pert_s"])}, strict=True)
    assert np.array_equal(m.height_map.height_map_sqrt.detach().numpy(), g["r32_half_pert_s"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({"height_map.height_map_sqrt": torch.from_numpy(g["r32_half_pert_s"]), "refractive_len": m.refractive_len}, strict=True)


def test_the_reference_s_module_name_points_to_this_one():
    """`doe_model_hybrid` keeps raising on import (tests/test_doe_host.py pins that); its message names the module that holds the model"""
    with pytest.raises(NotImplementedError, match="dprox.contrib.optic.doe_hybrid"):
        import dprox.contrib.optic.doe_model_hybrid  # noqa: F401


def test_unknown_aperture_type_raises_import_error():
    cfg = hyb.DOEModelConfig()
    with pytest.raises(ImportError, match="Aperture type square not supported"):
        hyb.RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths, 16, cfg.sample_interval, (32, 32), aperture_type="square")
    assert hyb.RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths, 16, cfg.sample_interval, (32, 32)).aperture_type == "half_circular"


def test_argument_errors():
    cfg = hyb.DOEModelConfig()
    args = (cfg.sensor_distance, cfg.refractive_idcs, cfg.wave_lengths)
    with pytest.raises(NotImplementedError, match="rectangular"):
        hyb.RGBCollimator(*args, 16, cfg.sample_interval, (32, 48))
    with pytest.raises(NotImplementedError, match="three wavelengths"):
        hyb.RGBCollimator(cfg.sensor_distance, cfg.refractive_idcs[:2], cfg.wave_lengths[:2], 16, cfg.sample_interval, (32, 32))
    with pytest.raises(NotImplementedError, match="no multiple of the patch size"):
        hyb.RGBCollimator(*args, 12, cfg.sample_interval, (32, 32))
    m = hc.build(32, 16, "half", "cpu")
    ctx = type("Ctx", (), {"R": 32, "P": 16})()
    for dtype, word in ((torch.float64, "float64"), (torch.bfloat16, "bfloat16")):
        with pytest.raises(NotImplementedError, match=word):
            ops.doe_psf(ctx, m.height_map.height_map_sqrt.detach().to(dtype), ops.DoeOptions(1e-7, m.refractive_len, 1, 1))
    with pytest.raises(NotImplementedError, match="complex128"):
        ops.doe_psf_of_profile(ctx, torch.zeros(1, 3, 32, 32, dtype=torch.complex128, requires_grad=True))
    with pytest.raises(ValueError, match="shape"):
        ops.doe_fresnel(ctx, torch.zeros(1, 3, 16, 16, dtype=torch.complex64, requires_grad=True))
    with pytest.raises(ValueError, match="phase plane"):
        ops.DoeOptions(1e-7, torch.zeros(1, 3, 16, 16), 1, 1).block(ctx)
    with pytest.raises(ValueError, match="phase plane"):
        ops.DoeOptions(1e-7, torch.zeros(1, 3, 32, 32, dtype=torch.float64), 1, 1).block(ctx)
    with pytest.raises(ValueError, match="phase offset"):
        ops.doe_phase(torch.zeros(1, 1, 32, 32), False, cfg.wave_lengths, cfg.refractive_idcs, offset=torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="float64"):
        m.height_map.get_phase_profile(torch.zeros(1, 1, 32, 32, dtype=torch.float64, requires_grad=True))


@pytest.mark.parametrize("R", (20, 30, 32, 33, 88))
def test_aperture_rules(R):
    """the model's aperture buffers are the integer rules; the half keeps every row and darkens the columns 2 j - (R - 1) <= 0, the centre
    column of an odd R included"""
    for kind, half in (("half", True), ("circ", False)):
        m = hc.build(R, hc.CASES[R], kind, "cpu")
        a = m.aperture[0, 0].numpy() != 0
        assert np.array_equal(a, hc.aperture(R, half))
        if half:
            assert not a[:, :(R + 1) // 2].any() and a[:, (R + 1) // 2:].any(axis=1)[1:-1].all()


def test_host_tables_are_float64_evaluations():
    """refractive_len and the Fresnel initialisation equal the reference's float64 run rounded to float32 up to the rounding of the
    float64 evaluation itself (a phase of p radians carries p * 2^-52 of it, a few float32 ulps of 2 pi at most; `% 2 pi` may land either
    side of a wrap).  Bound: 1e-6 rad, three orders below the 7e-4 rad the reference's float32 is off on the wide case."""
    g = hc.golden()
    for prefix, interval in (("r32", None), ("wide", float(g["cfg_scalars"][3]))):
        m = hc.build(32, 16, "half", "cpu", interval=interval)
        d = np.abs(m.refractive_len.numpy().astype(np.float64) - g[prefix + "_reflen64"])
        d = np.minimum(d, 2 * np.pi - d)                                             # (distance on the circle)
        assert d.max() <= 1e-6, (prefix, d.max())
        s = m.height_map.height_map_sqrt.detach().numpy().astype(np.float64)
        assert np.abs(s ** 2 - g[prefix + "_init64"] ** 2).max() <= 1e-6 / (2 * np.pi) * 550e-9 / 0.46, prefix
