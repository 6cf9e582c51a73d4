"""``dprox.contrib.optic``: the wave-optics model of a diffractive optical element for end-to-end computational optics (the
reference's ``contrib/optic``).  Built: ``doe_model``, the hybrid model as ``doe_hybrid`` (a module of its own, as upstream's
``doe_model_hybrid``: its classes share their names with ``doe_model``'s; that name keeps raising on import) and ``common`` on fused HIP kernels.  Not built: the U-Net baseline and the file / plotting helpers of ``utils`` (present by name, raise when called)."""
from .common import (FresnelPropagator, area_downsampling, get_coordinate, get_one_phase_shift_thickness, img_psf_conv,  # noqa: F401
                     psf2otf)
from .doe_model import DOEModelConfig, HeightMap, RGBCollimator, build_baseline_profile, build_doe_model  # noqa: F401
from .utils import (Dataset, U_Net, center_crop, load_sample_img, normalize_psf, normalize_psf2, plot, plot3d, sanity_check,  # noqa: F401
                    subplot)
