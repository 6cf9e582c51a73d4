"""The diffractive-optical-element model of the end-to-end optics application (the reference's ``contrib/optic/doe_model.py``): a
trainable height map behind a circular aperture, Fresnel propagation to the sensor, and the PSF the sensor sees.

``RGBCollimator.get_psf()`` is one ``ops.doe_psf`` call -- three transform launches and a normalising launch forward, a reduction
and three transform launches backward (``csrc/dpx_doe.hip``); the complex field in front of the propagator never exists in memory.
Only ``height_map.height_map_sqrt`` is persistent, so a reference checkpoint loads with ``strict=True``.  Construction (the Fresnel
initialisation, the coordinate and aperture buffers) is torch arithmetic on the host, once."""
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from ... import _ops as ops
from .common import FresnelPropagator, _square_side, get_coordinate, img_psf_conv


class HeightMap(nn.Module):
    """the element's height h = height_map_sqrt^2 (the square keeps it non-negative), one plane for all wavelengths"""

    def __init__(self, height_map_shape, wave_lengths, refractive_idcs, xx, yy, sensor_distance):
        super().__init__()
        self.wave_lengths = wave_lengths
        self.refractive_idcs = refractive_idcs
        self.register_buffer("delta_N", refractive_idcs.view([1, -1, 1, 1]) - 1., persistent=False)
        self.register_buffer("wave_nos", (2. * torch.pi / wave_lengths).view([1, -1, 1, 1]), persistent=False)
        self.xx, self.yy = xx, yy
        self.sensor_distance = sensor_distance
        self.height_map_sqrt = nn.Parameter(self._fresnel_phase_init(1))

    def _fresnel_phase_init(self, idx=1):
        """square root of the height map of a Fresnel lens focusing wavelength ``idx`` at the sensor distance: [1, 1, R, R]"""
        k = 2 * torch.pi / self.wave_lengths[idx]
        r2 = (self.xx ** 2 + self.yy ** 2)[None][None]
        return self.phase_to_height_map(-k * (r2 / (2 * self.sensor_distance)), idx) ** 0.5

    def get_phase_profile(self, height_map=None):
        """exp(i k_c (n_c - 1) h) as complex64 [1, 3, R, R] for h = ``height_map`` (one plane), by default height_map_sqrt^2: one small
        kernel (``dpx_doe_phase``).  An explicit height map that requires a gradient raises here, as it always has: its differentiable
        form is ``ops.doe_phase(height_map, False, wave_lengths, refractive_idcs)`` (``dpx_doe_phase_backward``), which the hybrid
        model's ``HeightMap`` uses.  ``RGBCollimator.get_psf()`` never forms this profile in memory."""
        if height_map is None:
            return ops.doe_phase(self.height_map_sqrt, True, self.wave_lengths, self.refractive_idcs)
        if isinstance(height_map, torch.Tensor) and height_map.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("get_phase_profile: the gradient with respect to an explicit height map is ops.doe_phase's "
                                      "(this method is forward only for an explicit argument)")
        return ops.doe_phase(height_map, False, self.wave_lengths, self.refractive_idcs)

    def phase_to_height_map(self, phi, wave_length_idx=1):
        """the height whose phase delay at wavelength ``wave_length_idx`` is ``phi`` mod 2 pi"""
        k = 2. * torch.pi / self.wave_lengths[wave_length_idx]
        return (phi % (2 * torch.pi)) / k / self.delta_N.view(-1)[wave_length_idx]


class RGBCollimator(nn.Module):
    def __init__(self, sensor_distance, refractive_idcs, wave_lengths, patch_size, sample_interval, wave_resolution):
        super().__init__()
        self.wave_res = wave_resolution
        self.wave_lengths = wave_lengths
        self.sensor_distance = sensor_distance
        self.sample_interval = sample_interval
        self.patch_size = patch_size
        self.refractive_idcs = refractive_idcs
        if len(wave_lengths) != 3 or len(refractive_idcs) != 3:
            raise NotImplementedError(f"RGBCollimator: {len(wave_lengths)} wavelengths / {len(refractive_idcs)} refractive indices (three "
                                      "wavelengths are built)")
        side = _square_side(tuple(wave_resolution), "RGBCollimator")
        if side % int(patch_size):
            raise NotImplementedError(f"RGBCollimator: a wave resolution of {side} is no multiple of the patch size {patch_size}")
        self._init_setup()

    def _context(self):
        s = self.height_map.height_map_sqrt
        return ops.doe_context(self.wave_res[0], self.patch_size, self.sensor_distance, self.sample_interval, self.wave_lengths,
                               self.refractive_idcs, s.device)

    def get_psf(self, phase_profile=None):
        """PSF [1, 3, patch, patch] of the element, normalised to sum 1 over all three channels.  Without an argument: from
        ``height_map_sqrt``, differentiable.  With a complex64 ``phase_profile`` [1, 3, R, R]: that profile behind the aperture,
        differentiable in the profile."""
        if phase_profile is None:
            return ops.doe_psf(self._context(), self.height_map.height_map_sqrt)
        return ops.doe_psf_of_profile(self._context(), phase_profile)

    def forward(self, input_img, phase_profile=None, circular=False):
        psfs = self.get_psf(phase_profile)
        return img_psf_conv(input_img, psfs, circular=circular), psfs

    def _init_setup(self):
        R0, R1 = self.wave_res
        self.register_buffer("input_field", torch.ones((1, len(self.wave_lengths), R0, R1)), persistent=False)
        xx, yy = get_coordinate(R0, R1, self.sample_interval, self.sample_interval)
        self.register_buffer("xx", xx, persistent=False)
        self.register_buffer("yy", yy, persistent=False)
        self.register_buffer("aperture", self._get_circular_aperture(xx, yy), persistent=False)
        self.height_map = HeightMap((1, 3, R0, R1), self.wave_lengths, self.refractive_idcs, self.xx, self.yy, self.sensor_distance)
        self.propagator = FresnelPropagator((1, 3, R0, R1), self.sensor_distance, self.sample_interval, self.wave_lengths)

    def _get_circular_aperture(self, xx, yy):
        """[1, 1, R, R] of 0 / 1: the open disc, by the exact integer rule the kernels evaluate in their loads,
        (2 i - (R - 1))^2 + (2 j - (R - 1))^2 < (R - 1)^2 (the reference's sqrt(xx^2 + yy^2) < xx.max() without its rounding)"""
        R = int(xx.shape[0])
        a = 2 * torch.arange(R, dtype=torch.int64) - (R - 1)
        return ((a[:, None] ** 2 + a[None, :] ** 2) < (R - 1) ** 2).to(xx.dtype)[None][None]


@dataclass
class DOEModelConfig:
    circular: bool = True                                        # circular convolution
    aperture_diameter: float = 3e-3                              # aperture diameter
    sensor_distance: float = 15e-3                               # distance of the sensor to the aperture
    refractive_idcs = torch.tensor([1.4648, 1.4599, 1.4568])     # refractive indices of the phase plate
    wave_lengths = torch.tensor([460, 550, 640]) * 1e-9          # wave lengths that are modelled and optimised for
    num_steps: int = 10001                                       # number of SGD steps
    patch_size: int = 748                                        # side of the image patches = resolution of the simulated sensor
    sample_interval: float = 2e-6                                # sampling interval (one "pixel" of the simulated wavefront)
    wave_resolution = 1496, 1496                                 # resolution of the simulated wavefront
    model_kwargs: dict = field(default_factory=dict)


def build_doe_model(config: DOEModelConfig = DOEModelConfig()):
    """the RGBCollimator of a configuration"""
    return RGBCollimator(config.sensor_distance, refractive_idcs=config.refractive_idcs, wave_lengths=config.wave_lengths,
                         patch_size=config.patch_size, sample_interval=config.sample_interval, wave_resolution=config.wave_resolution)


def build_baseline_profile(rgb_collim_model: RGBCollimator):
    """the phase profile [1, 3, R, R] of the plain Fresnel lens for the middle wavelength: the baseline the trained element is compared
    with (``get_psf(build_baseline_profile(model))``)"""
    m = rgb_collim_model
    k = 2 * torch.pi / m.wave_lengths[1]
    phase = -k * ((m.xx ** 2 + m.yy ** 2)[None][None] / (2 * m.sensor_distance))
    height_map = m.height_map.phase_to_height_map(phase.to(m.height_map.delta_N.device), 1)
    return m.height_map.get_phase_profile(height_map.float().contiguous())
