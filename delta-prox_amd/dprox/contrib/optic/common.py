"""Building blocks of the wave-optics model (the reference's ``contrib/optic/common.py``): coordinates, area down-sampling, the
PSF -> OTF quirks, the sensor image of a scene under a PSF, and the Fresnel propagator.

Everything a training step runs is a HIP kernel: the propagator is ``dpx_doe_propagate`` (its transfer function H is evaluated once
per device by ``dpx_doe_propagator_init``, in float64), ``img_psf_conv`` is the ``conv_doe`` operator.  ``get_coordinate`` and
``psf2otf`` are set-up / inspection helpers on torch tensors."""
import numpy as np
import torch
import torch.nn as nn

from ... import _ops as ops


def get_coordinate(nx, ny, dx, dy):
    """(xx, yy) of an nx x ny grid centred on the origin with spacings dx, dy (``indexing='ij'``: xx varies along dim 0)"""
    x = (torch.arange(nx) - (nx - 1.) / 2) * dx
    y = (torch.arange(ny) - (ny - 1.) / 2) * dy
    return torch.meshgrid(x, y, indexing="ij")


def area_downsampling(input, target_side_length):
    """mean over f x f blocks of an NCHW tensor, f = side / target_side_length; a side the target does not divide raises, as upstream"""
    side = int(input.shape[2])
    if side % int(target_side_length):
        raise NotImplementedError(f"area_downsampling: a side of {side} is no multiple of the target side {target_side_length}")
    f = side // int(target_side_length)
    N, C, H, W = input.shape
    return input.reshape(N, C, H // f, f, W // f, f).mean(dim=(3, 5))


def _otf_padding(size, k):
    """(before, after) zeros that bring a PSF axis of k samples to `size`: ceil / floor of half the gap when the gap is odd, and
    half + 1 / half - 1 when it is even -- the reference's rule (an inspection helper keeps it bit for bit)"""
    gap = size - k
    if gap % 2:
        return int(np.ceil(gap / 2)), int(np.floor(gap / 2))
    return gap // 2 + 1, gap // 2 - 1


def psf2otf(psf, output_size):
    """OTF of a PSF [1, C, fh, fw] at output_size (N, C, H, W): zero-pad by the rule above (both axes take the HEIGHT's padding),
    ``ifftshift`` over ALL axes, ``fft2``.  An inspection helper on torch tensors; the solver's own OTF is conv_doe's."""
    fh = int(psf.shape[2])
    if output_size[2] != fh:
        before, after = _otf_padding(int(output_size[2]), fh)
        psf = torch.nn.functional.pad(psf, [before, after, before, after])
    return torch.fft.fft2(torch.fft.ifftshift(psf))


def img_psf_conv(img, psf, circular=True):
    """the sensor image of the scene ``img`` [N, C, H, W] under ``psf`` [1, C, fh, fw]: the ``conv_doe`` operator itself (the same
    padding and all-axes shift as the reference's function of this name, whose ``sanity_check`` asserts the two equal), so it has
    no kernel of its own and is differentiable in ``img`` and ``psf`` exactly as ``conv_doe`` is"""
    from ...linop import Variable, conv_doe
    return conv_doe(Variable(), psf, circular=circular).forward(img.float().contiguous())


def _square_side(shape, what):
    side, other = int(shape[-2]), int(shape[-1])
    if side != other:
        raise NotImplementedError(f"{what}: a {side} x {other} wavefront (square wave resolutions are built; rectangular ones are not)")
    return side


class FresnelPropagator(nn.Module):
    """Fresnel propagation over ``distance`` of a complex field [1, 3, R, R] sampled at ``discretization_size``: zero-pad by R // 4,
    multiply the spectrum by H_c = exp(-i pi distance lambda_c (fx^2 + fy^2)), transform back, crop -- three launches
    (``dpx_doe_propagate``).  ``H`` is [1, 3, M, M] complex64 on the module's device WITH the inverse transform's 1 / M^2 folded in
    (the kernels' table, evaluated in float64); ``Mpad`` = ``Npad`` = R // 4."""

    def __init__(self, input_shape, distance, discretization_size, wave_lengths):
        super().__init__()
        self.input_shape = tuple(input_shape)
        self.distance = distance
        self.discretization_size = discretization_size
        self.wave_lengths = wave_lengths
        self.wave_nos = 2. * torch.pi / wave_lengths
        if len(wave_lengths) != 3 or self.input_shape[1] != 3:
            raise NotImplementedError(f"FresnelPropagator: {len(wave_lengths)} wavelengths (three are built, as the reference's "
                                      "view(1, 3, 1, 1) has it)")
        side = _square_side(self.input_shape, "FresnelPropagator")
        self.Mpad = self.Npad = side // 4
        self.register_buffer("_device_of", torch.empty(0), persistent=False)        # follows .to(device): where H lives

    def _context(self, patch=None):
        side = self.input_shape[-1]
        # (the refractive indices play no part in propagation: ones stand in for them)
        return ops.doe_context(side, side if patch is None else patch, self.distance, self.discretization_size, self.wave_lengths,
                               torch.ones(3), self._device_of.device)

    @property
    def H(self):
        return self._context().H

    def forward(self, input_field):
        return ops.doe_fresnel(self._context(), input_field)


def get_one_phase_shift_thickness(wave_lengths, refractive_index):
    """thickness (in metres) whose phase shift is 2 pi: lambda / (n - 1)"""
    wave_nos = 2. * torch.pi / wave_lengths
    return (2. * torch.pi) / (wave_nos * (refractive_index - 1.))
