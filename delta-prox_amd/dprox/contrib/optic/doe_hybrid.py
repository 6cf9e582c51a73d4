"""The hybrid refractive / diffractive model (the reference's ``contrib/optic/doe_model_hybrid.py``; here the module is ``doe_hybrid``:
the name ``doe_model_hybrid`` keeps raising on import, as it always has on this backend): a thin refractive lens in front
of the diffractive element, a circular or half-circular aperture, and a PSF normalised per wavelength.

The phase in front of the propagator is ``k_c (height_map_sqrt + 1e-7)^2 + refractive_len_c``, with ``refractive_len`` the fixed
Fresnel-lens phase of each wavelength.  ``get_psf()`` is one ``ops.doe_psf`` call with a ``DoeOptions`` block -- the launches of
``doe_model`` generalised (``dpx_doe_psf_ex``), the lens phase read as one more plane in the first kernel's load.

``refractive_len`` and the Fresnel initialisation are evaluated in float64 on the host and stored as float32: at the default
configuration the lens phase is thousands of radians, and a float32 ``% 2 pi`` of it is off by 7e-4 rad.  For the same reason the
module's ``RI`` and the configuration's ``wave_lengths`` / ``refractive_idcs`` are float64 tensors (a float32 wavelength is 3e-8 off, 2e-4
rad of lens phase); float32 tensors are accepted and widened.  Only ``height_map.height_map_sqrt`` is persistent, so a reference
checkpoint loads with ``strict=True``."""
import math
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from ... import _ops as ops
from .common import FresnelPropagator, _square_side, get_coordinate, img_psf_conv

EPS = 1e-7                                   # added to height_map_sqrt before the square, as upstream (in float32)
APERTURE_KINDS = {"circular": 0, "half_circular": 1}


def _coordinate64(n, d):
    return (torch.arange(n, dtype=torch.float64) - (n - 1.) / 2) * float(d)


def _fresnel_phase64(xx, yy, wave_length, sensor_distance):
    """(-k r^2 / (2 d)) mod 2 pi of a Fresnel lens focusing ``wave_length`` at ``sensor_distance``, in float64: [1, 1, R, R]"""
    k = 2 * math.pi / float(wave_length)
    r2 = (xx.double() ** 2 + yy.double() ** 2)[None][None]
    return (-k * (r2 / (2 * float(sensor_distance)))) % (2 * math.pi)


class HeightMap(nn.Module):
    """the element's height h = (height_map_sqrt + 1e-7)^2, one plane for all wavelengths"""

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
        """square root of the height map of a Fresnel lens focusing wavelength ``idx`` at the sensor distance, evaluated in float64:
        [1, 1, R, R] float32"""
        phase = _fresnel_phase64(self.xx, self.yy, self.wave_lengths[idx], self.sensor_distance)
        return (self.phase_to_height_map(phase, idx) ** 0.5).float()

    def get_phase_profile(self, height_map=None, refractive_len=None):
        """exp(i (k_c (n_c - 1) h + refractive_len_c)) as complex64 [1, 3, R, R] for h = ``height_map`` (one plane), by default
        (height_map_sqrt + 1e-7)^2; ``refractive_len``: an optional float32 phase [1, 3, R, R].  One small kernel (``dpx_doe_phase_ex``),
        differentiable in the height map (``dpx_doe_phase_backward``)."""
        if height_map is None:
            return ops.doe_phase(self.height_map_sqrt, True, self.wave_lengths, self.refractive_idcs, eps=EPS, offset=refractive_len)
        return ops.doe_phase(height_map, False, self.wave_lengths, self.refractive_idcs, offset=refractive_len)

    def phase_to_height_map(self, phi, wave_length_idx=1):
        """the height whose phase delay at wavelength ``wave_length_idx`` is ``phi`` mod 2 pi (in the precision of ``phi``)"""
        k = 2. * math.pi / float(self.wave_lengths[wave_length_idx])
        return (phi % (2 * math.pi)) / k / (float(self.refractive_idcs.reshape(-1)[wave_length_idx].double()) - 1.)


class RGBCollimator(nn.Module):
    def __init__(self, sensor_distance, refractive_idcs, wave_lengths, patch_size, sample_interval, wave_resolution, aperture_type="half_circular"):
        super().__init__()
        self.wave_res = wave_resolution
        self.wave_lengths = wave_lengths
        self.sensor_distance = sensor_distance
        self.sample_interval = sample_interval
        self.patch_size = patch_size
        self.refractive_idcs = refractive_idcs
        if aperture_type not in APERTURE_KINDS:
            raise ImportError(f"Aperture type {aperture_type} not supported")           # (the exception upstream raises)
        self.aperture_type = aperture_type
        if len(wave_lengths) != 3 or len(refractive_idcs) != 3:
            raise NotImplementedError(f"RGBCollimator: {len(wave_lengths)} wavelengths / {len(refractive_idcs)} refractive indices (three "
                                      "wavelengths are built)")
        side = _square_side(tuple(wave_resolution), "RGBCollimator")
        if side % int(patch_size):
            raise NotImplementedError(f"RGBCollimator: a wave resolution of {side} is no multiple of the patch size {patch_size}")
        self._init_setup(aperture_type)

    def _context(self):
        s = self.height_map.height_map_sqrt
        return ops.doe_context(self.wave_res[0], self.patch_size, self.sensor_distance, self.sample_interval, self.wave_lengths,
                               self.refractive_idcs, s.device)

    def get_psf(self, phase_profile=None):
        """PSF [1, 3, patch, patch] of the lens and the element, every channel normalised to sum 1.  Without an argument: from
        ``height_map_sqrt`` and ``refractive_len``, differentiable in ``height_map_sqrt``.  With a complex64 ``phase_profile``
        [1, 3, R, R]: that profile behind the aperture, differentiable in the profile."""
        kind = APERTURE_KINDS[self.aperture_type]
        if phase_profile is None:
            return ops.doe_psf(self._context(), self.height_map.height_map_sqrt, ops.DoeOptions(EPS, self.refractive_len, kind, 1))
        return ops.doe_psf_of_profile(self._context(), phase_profile, ops.DoeOptions(0.0, None, kind, 1))

    def forward(self, input_img, phase_profile=None, circular=False):
        psfs = self.get_psf(phase_profile)
        return img_psf_conv(input_img, psfs, circular=circular), psfs

    def _init_setup(self, aperture_type):
        R0, R1 = self.wave_res
        self.register_buffer("input_field", torch.ones((1, len(self.wave_lengths), R0, R1)), persistent=False)
        xx, yy = get_coordinate(R0, R1, self.sample_interval, self.sample_interval)
        self.register_buffer("xx", xx, persistent=False)
        self.register_buffer("yy", yy, persistent=False)
        aperture = self._get_halfcircular_aperture(xx, yy) if aperture_type == "half_circular" else self._get_circular_aperture(xx, yy)
        self.register_buffer("aperture", aperture, persistent=False)
        # the host tables are evaluated on float64 coordinates (the float32 buffers above are the reference's surface)
        self._xx64, self._yy64 = torch.meshgrid(_coordinate64(R0, self.sample_interval), _coordinate64(R1, self.sample_interval), indexing="ij")
        self.height_map = HeightMap((1, 1, R0, R1), self.wave_lengths, self.refractive_idcs, self._xx64, self._yy64, self.sensor_distance)
        self.propagator = FresnelPropagator((1, 3, R0, R1), self.sensor_distance, self.sample_interval, self.wave_lengths)
        self.register_buffer("refractive_len", self._get_refractive_len(), persistent=False)

    def _get_circular_aperture(self, xx, yy):
        """[1, 1, R, R] of 0 / 1: the open disc by the exact integer rule the kernels evaluate in their loads,
        (2 i - (R - 1))^2 + (2 j - (R - 1))^2 < (R - 1)^2"""
        R = int(xx.shape[0])
        a = 2 * torch.arange(R, dtype=torch.int64) - (R - 1)
        return ((a[:, None] ** 2 + a[None, :] ** 2) < (R - 1) ** 2).float()[None][None]

    def _get_halfcircular_aperture(self, xx, yy):
        """the disc's half with 2 j - (R - 1) > 0: upstream's ``yy > 0`` is the COLUMN coordinate, so the left half of every row is dark,
        the centre column of an odd R included"""
        R = int(xx.shape[0])
        a = 2 * torch.arange(R, dtype=torch.int64) - (R - 1)
        return self._get_circular_aperture(xx, yy) * (a[None, :] > 0).float()[None][None]

    def _get_refractive_len(self):
        """the lens: the Fresnel phase of every wavelength mod 2 pi, evaluated in float64, stored as float32 [1, 3, R, R]"""
        return torch.cat([_fresnel_phase64(self._xx64, self._yy64, self.wave_lengths[c], self.sensor_distance) for c in range(3)], dim=1).float()


wvls = torch.tensor([460, 550, 640])
wvl_um = wvls.double() * 1e-3
# the Sellmeier equation of fused silica, in float64
RI = (1 + 0.6961663 / (1 - (0.0684043 / wvl_um) ** 2) + 0.4079426 / (1 - (0.1162414 / wvl_um) ** 2) + 0.8974794 / (1 - (9.896161 / wvl_um) ** 2)) ** .5


@dataclass
class DOEModelConfig:
    circular: bool = True                                        # circular convolution
    aperture_diameter: float = 9e-3                              # aperture diameter
    aperture_type: str = 'half_circular'                         # type of aperture: 'half_circular' or 'circular'
    sensor_distance: float = 50e-3                               # distance of the sensor to the aperture
    wave_lengths = wvls.double() * 1e-9                          # wave lengths that are modelled and optimised for
    refractive_idcs = RI                                         # refractive indices of the phase plate
    num_steps: int = 10001                                       # number of SGD steps
    patch_size: int = 512                                        # side of the image patches = resolution of the simulated sensor
    sample_interval: float = 5.4e-6                              # sampling interval (one "pixel" of the simulated wavefront)
    wave_resolution = 1536, 1536                                 # resolution of the simulated wavefront
    model_kwargs: dict = field(default_factory=dict)


def build_doe_model(config: DOEModelConfig = DOEModelConfig()):
    """the RGBCollimator of a configuration"""
    return RGBCollimator(config.sensor_distance, refractive_idcs=config.refractive_idcs, wave_lengths=config.wave_lengths,
                         patch_size=config.patch_size, sample_interval=config.sample_interval, wave_resolution=config.wave_resolution,
                         aperture_type=config.aperture_type)


def build_baseline_profile(rgb_collim_model: RGBCollimator):
    """the phase profile [1, 3, R, R] of the plain Fresnel element for the middle wavelength, as upstream reads it: an explicit height
    map and no lens term (``get_psf(build_baseline_profile(model))``)"""
    m = rgb_collim_model
    phase = _fresnel_phase64(m._xx64, m._yy64, m.wave_lengths[1], m.sensor_distance)
    height_map = m.height_map.phase_to_height_map(phase, 1).float().contiguous()
    return m.height_map.get_phase_profile(height_map.to(m.height_map.height_map_sqrt.device))
