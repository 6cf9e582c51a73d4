"""MINRES for symmetric, possibly indefinite operators on the HIP kernels of csrc/dpx_minres.hip (reference
dprox/linalg/solve/solver_minres.py:21-290, whose semantics are kept literally).

The vector axis is ``dim -2``: a 1-D ``b`` is one system, ``[N, K]`` K independent columns, leading axes ``[..., N, K]`` further
independent systems; every dot product is per system.  ``b`` is scaled per system by its 2-norm (norms below 1e-10 are replaced by 1
and those systems' solutions zero-filled), ``max_iters = min(max_iters, N + 1)`` and the loop runs ``max_iters + 2`` steps, ``beta``
is clamped from below by ``eps``, ``value`` multiplies every operator product, ``shifts`` enter the Givens part only (S shifts share
one Lanczos sequence and give a leading axis of S, squeezed away for a single shift), and ``x0`` is accepted and ignored.  The stop
rule is the reference's: every tenth step, globally over all systems, ``|A(solution[0]) - b| <= rtol |b|`` with the scaled ``b`` and
shift 0's solution (it ignores ``value`` and the shift) -- the loop's one host read per ten steps, one scalar pair.
One difference: the reference applies ``A`` once more before the loop, only to learn the product's shape; here ``A`` must return a
tensor of its argument's shape.

Per step: the operator (the caller's code), then ``dpx_minres_alpha``, ``dpx_minres_lanczos`` and ``dpx_minres_update``; the scalars
of every (shift, system) pair stay in a device-resident state block (``ops.MinresControl``, float64 for both element types) and the
host only issues launches.  With a ``Minv`` callable the second launch splits around it (``lanczos(finish=False)``, ``Minv``,
``dpx_minres_beta``).

dtype: a float64 ``b`` keeps the whole solve in float64 on the device; anything else is computed in float32.
Autograd: the reference notes that its MINRES cannot be unrolled.  Called with something to differentiate, ``minres`` returns the
solution with the implicit-function backward ``cg`` uses (``krylov._ImplicitCG``): one more solve with the symmetric operator and one
operator VJP.  That path takes a single shift."""
import math

import torch

from ... import _ops as ops
from .krylov import _differentiable, _wants_grad, _work


def minres(A, b, x0=None, rtol=1e-6, max_iters=100, verbose=False, Minv=None, eps=1e-25, shifts=None, value=None):
    """Solve ``(value A + shift I) x = b`` for a symmetric operator ``A`` given as a callable, for every shift at once."""
    if not callable(A):
        raise TypeError(f"minres: the operator must be callable, got {type(A).__name__}")
    if Minv is not None and not callable(Minv):
        raise TypeError(f"minres: Minv must be callable, got {type(Minv).__name__}")
    kwargs = dict(x0=x0, rtol=rtol, max_iters=max_iters, verbose=verbose, Minv=Minv, eps=eps, shifts=shifts, value=value)
    if _wants_grad(A, b):
        if shifts is not None and torch.as_tensor(shifts).numel() != 1:
            raise NotImplementedError("minres: the implicit gradient takes a single shift")
        return _differentiable(minres, A, b, kwargs)
    with torch.no_grad():
        return _minres(A, b, rtol, max_iters, verbose, Minv, eps, shifts, value)


def _flat1(t):
    return t.reshape(1, -1)


def _minres(A, b, rtol, max_iters, verbose, Minv, eps, shifts, value):
    b = _work(b)
    squeeze = b.ndim == 1
    if squeeze:
        b = b.unsqueeze(-1)
    shape = tuple(b.shape)
    N, K = shape[-2], shape[-1]
    sys3 = (b.numel() // max(N * K, 1), N, K)
    b3 = b.reshape(sys3)
    if shifts is None:
        shifts = torch.zeros((), dtype=b.dtype)
    shifts = torch.as_tensor(shifts)
    single = shifts.numel() == 1
    ctl = ops.MinresControl(b3, shifts, value, eps)

    def through(fn, t):
        """a caller's callable on the systems' own shape; the result as a [G, N, K] working tensor that does not alias ``t``"""
        out = fn(t.reshape(shape)).detach().to(b.dtype).reshape(sys3).contiguous()
        return out.clone() if out.data_ptr() == t.data_ptr() else out

    # scale the right-hand side (:63-72) and start the Lanczos sequence (:89-101)
    ctl.alpha(b3, b3, value=1.0)
    ctl.init(0)
    bs = torch.empty_like(b3)
    ctl.colscale(bs, b3, 0)
    q = None if Minv is None else through(Minv, bs)
    ctl.alpha(bs, bs if q is None else q, value=1.0)
    ctl.init(1)
    ctl.colscale(ctl.zring[1], bs, 1)
    if q is not None:
        ctl.colscale(q, q, 1)
    bnorm2 = ops.bdot(_flat1(bs), _flat1(bs))
    max_iters = min(int(max_iters), N + 1)
    if verbose:
        print(f"Running MINRES on a {torch.Size(shape)} RHS for {max_iters} iterations (rtol={rtol}). "
              f"Output: {torch.Size((ctl.S,) + shape)}.")
    for i in range(max_iters + 2):
        prod = through(A, ctl.zring[(i + 1) & 1] if q is None else q)
        ctl.alpha(prod, q)
        if q is None:
            ctl.lanczos(prod)
            ctl.update()
        else:
            ctl.lanczos(prod, finish=False)
            qc = through(Minv, ctl.zring[i & 1])
            ctl.beta(qc)
            ctl.update(q, qc)
            q = qc
        if (i + 1) % 10 == 0:
            r = ops.lincomb([(1.0, _flat1(through(A, ctl.solution[0]))), (-1.0, _flat1(bs))])
            rnorm2, bn2 = torch.cat([ops.bdot(r, r), bnorm2]).tolist()          # the one host read
            if math.sqrt(rnorm2) <= rtol * math.sqrt(bn2):
                break
    out = torch.empty_like(ctl.solution)
    for s in range(ctl.S):
        ctl.colscale(out[s], ctl.solution[s], 2)
    out = out.reshape((ctl.S,) + shape)
    if squeeze:
        out = out.squeeze(-1)
    return out.squeeze(0) if single else out
