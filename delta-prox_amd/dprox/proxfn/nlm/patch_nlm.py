"""``patch_nlm`` -- non-local-means prior: the prox is one non-local-means pass at sigma = sqrt(lam)
(reference dprox/proxfn/nlm/patch_nlm.py:5-13 over nlm.py:NonLocalMeansFast)."""
import torch

from ... import _ops as ops
from ..core import ProxFn


class patch_nlm(ProxFn):
    """Non-local-means prior ``g(K x)`` whose proximal operator is ``NLM(v, sigma = sqrt(lam))`` on the reference's windows (search 11,
    patch 5) or any other odd ones.  ``lam`` includes the term's ``alpha`` (``c * patch_nlm(x)`` denoises at sqrt(c * lam)).

    Same constructor as the reference plus the two window sizes.  Behavioural notes for the HIP backend: one ``dpx_nlm`` kernel per call
    (the reference builds [N, C, H, W, search^2] shift stacks); single-channel images are denoised on the plane itself (the reference's
    luminance slicing returns an empty tensor for them); the prior is forward-only -- a call that autograd would have to differentiate
    raises NotImplementedError (the reference's gradient through it is NaN: sqrt'(0) at the zero shift)."""

    def __init__(self, linop, search_window_size=11, patch_size=5):
        super().__init__(linop)
        self.search_window_size = int(search_window_size)
        self.patch_size = int(patch_size)

    def _prox(self, v, lam):
        lam = lam if isinstance(lam, torch.Tensor) else torch.tensor(float(lam))
        if torch.is_grad_enabled() and (v.requires_grad or lam.requires_grad):
            raise NotImplementedError("patch_nlm is forward-only: it has no gradient (the reference's gradient through its non-local means is "
                                      "NaN, sqrt'(0) at the zero shift); call it under torch.no_grad()")
        return ops.nlm(v, lam.sqrt(), self.search_window_size, self.patch_size)

    def __repr__(self):
        return f"patch_nlm(search_window_size={self.search_window_size}, patch_size={self.patch_size})"
