"""``dprox.contrib.optic``: the wave-optics model of a diffractive optical element for end-to-end computational optics (the
reference's ``contrib/optic``).  Built: ``doe_model`` and ``common`` on fused HIP kernels.  Not built: ``doe_model_hybrid`` (importing
it raises by name), the U-Net baseline and the file / plotting helpers of ``utils`` (present by name, raise when called)."""
from .common import (FresnelPropagator, area_downsampling, get_coordinate, get_one_phase_shift_thickness, img_psf_conv,  # noqa: F401
                     psf2otf)
from .doe_model import DOEModelConfig, HeightMap, RGBCollimator, build_baseline_profile, build_doe_model  # noqa: F401
from .utils import (Dataset, U_Net, center_crop, load_sample_img, normalize_psf, normalize_psf2, plot, plot3d, sanity_check,  # noqa: F401
                    subplot)
