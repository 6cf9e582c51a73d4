"""``compress_sensing`` -- the coded-aperture data term of snapshot compressive imaging with a closed-form x-update
(reference dprox/proxfn/fast/cs.py:6-27).  With A v = sum_c mask_c v_c and I right-hand sides summed into v:

    phi = sum_c mask_c^2;   x = (v + mask (I y - A v) / (phi + I lam)) / I

i.e. the solution of (A^T A + I lam) x = A^T y + lam v -- one ``dpx_cs_xupdate`` launch that also adds up the right-hand sides.

The reference's constructor does not run (it calls ``self.to_parameter``, which does not exist, and hands ``y`` to
``ext_sum_squares`` as ``eps``), and its ``_prox`` reads an ``I`` nothing sets.  The arithmetic has one reading: ``I`` is the
``num_psi`` that ``ext_sum_squares.solve`` passes as ``_prox``'s third argument, as ``csmri`` and ``sisr`` spell it.
"""
import numpy as np
import torch

from ... import _ops as ops
from ..quadratic import ext_sum_squares


class compress_sensing(ext_sum_squares):
    hip_kind = None          # (not sum_squares' built-in prox: as a split term, prox(v, lam) is _prox at num_psi = 1)

    def __init__(self, linop, mask, y):
        super().__init__(linop)
        self.mask = mask
        self.y = y

    def _operand(self, value, device):
        """a mask / measurement as the float32 tensor ops.cs_xupdate takes (its own shape rules apply: the array is not batchified)"""
        if isinstance(value, (np.ndarray, list, tuple)):
            value = torch.as_tensor(np.asarray(value))
        t = self.unwrap(value) if not isinstance(value, torch.Tensor) else value
        if isinstance(t, torch.Tensor) and not t.is_complex() and t.dtype != torch.float32:
            t = t.float()
        return t.to(device) if isinstance(t, torch.Tensor) else t

    def _xupdate(self, bs, lam, num_psi):
        device = bs[0].device if bs else None                      # (no right-hand side: ops.cs_xupdate refuses)
        return ops.cs_xupdate(bs, self._operand(self.y, device), self._operand(self.mask, device), lam, num_psi)

    def solve(self, b, rho, eps=1e-6):
        return self._xupdate(list(b), rho, len(b))

    def _prox(self, v, lam, num_psi=1):
        return self._xupdate([v], lam, num_psi)
