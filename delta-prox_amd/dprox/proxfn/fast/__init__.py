"""Closed-form data terms (reference dprox/proxfn/fast/): the ones on the hot path of the reference's own pipelines."""
from .cs import compress_sensing
from .csmri import csmri
from .sr import sisr
