"""What the reference's ``contrib/optic/utils.py`` offers the end-to-end optics example.  ``normalize_psf`` is built; the helpers that
need image files, plotting or dataset packages are present by name, so the example's import line works, and raise where they are
called."""
import numpy as np

from .common import img_psf_conv  # noqa: F401


def normalize_psf(psf: np.ndarray, clip_percentile=0.01, bandwise=False):
    """a PSF [H, W, C] prepared for display: normalised to sum 1 (per band if ``bandwise``), clipped to its
    [clip_percentile, 100 - clip_percentile] percentiles, then scaled to a maximum of 1"""
    psf = np.asarray(psf)
    psf = psf / (psf.sum(axis=(0, 1), keepdims=True) if bandwise else psf.sum())
    lo, hi = np.percentile(psf, [clip_percentile, 100 - clip_percentile])
    psf = np.clip(psf, lo, hi)
    return psf / psf.max()


def _not_built(name, needs):
    def raiser(*args, **kwargs):
        raise NotImplementedError(f"dprox.contrib.optic.{name} is not built on this backend ({needs})")
    raiser.__name__ = name
    raiser.__doc__ = f"not built on this backend ({needs}); raises NotImplementedError"
    return raiser


load_sample_img = _not_built("load_sample_img", "it reads an image file with PIL; pass the scene as a tensor")
sanity_check = _not_built("sanity_check", "img_psf_conv IS the conv_doe operator here, there is nothing to compare")
center_crop = _not_built("center_crop", "a PIL helper of load_sample_img")
normalize_psf2 = _not_built("normalize_psf2", "a plotting helper")
subplot = _not_built("subplot", "a matplotlib helper")
plot = _not_built("plot", "a matplotlib helper")
plot3d = _not_built("plot3d", "a matplotlib helper")
Dataset = _not_built("Dataset", "it wraps torchlight's SingleImageDataset and OpenCV")
U_Net = _not_built("U_Net", "the U-Net baseline of the optics example; the unrolled solver is the reconstruction built here")
