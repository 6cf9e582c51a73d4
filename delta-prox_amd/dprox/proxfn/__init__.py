from .core import ProxFn
from .fast import compress_sensing, csmri, sisr
from .nlm import patch_nlm
from .pnp import Denoiser, Denoiser2D, DRUNetDenoiser, FFDNetColorDenoiser, FFDNetDenoiser, GRUnet, GRUNetDenoiser, GRUNetTVDenoiser, QRNN3DDenoiser, TVDenoiser, UNetDenoiser, deep_prior
from .quadratic import ext_sum_squares, least_squares, sum_squares, weighted_sum_squares
from .simple import nonneg, norm1, norm2, soft_threshold
