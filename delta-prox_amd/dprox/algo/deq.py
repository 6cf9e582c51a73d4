"""The DEQ specialization: a solver's iteration run to its fixed point by Anderson acceleration, differentiated implicitly
(reference dprox/algo/specialization/deq/solver.py:13-109, deq/utils/solvers.py:193-254).

The Anderson step works on a piece-major history (``ops.AndersonHistory``): every slot holds the state's pieces x, v_1..v_n, u_1..u_n
as contiguous [B, C, H, W] stacks, so the iteration's fused stages read the point X and write slot k % m of F directly -- no
``pack`` / ``unpack`` copy of the image-sized state inside the loop.  Per step, besides the evaluation of f: ``dpx_anderson_mix``
(the small solve in every workgroup's prologue + the streaming combination) and ``dpx_anderson_gram_row`` (G_k = F_k - X_k, row k of
the Gram matrix, |G_k|^2 and |F_k|^2 for the stop rule), and one host read of 2 B floats.

``DEQSolver`` supports the ``ADMM`` problems the fused plan takes (``fused.plan_admm``).  Forward: under ``no_grad``, one full
iteration per evaluation on the staged fused kernels (right-hand side, Fourier solve, z / dual update), out of place.  Denoiser priors (deep_prior, patch_nlm) are refused by name.
Training mode: one more iteration at z* through the staged autograd path (``autodiff.run`` with ``max_iter=1``) and a backward
node that solves y = J^T y + grad with the same Anderson kernels.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _backend as be
from .. import _ops as ops
from ..proxfn import least_squares
from . import fused
from .driver import Algorithm, move, to_tensor
from .splitting import ADMM


def _check_threshold(threshold):
    if int(threshold) <= 2:
        raise ValueError(f"anderson: threshold={threshold} leaves no accelerated step (the first two evaluations of f only fill the "
                         "history); threshold must be at least 3")


def anderson_pieces(step, x0, m=6, lam=1e-4, threshold=50, eps=1e-3, stop_mode="rel", beta=1.0):
    """Anderson acceleration on a piece-major state.  ``x0``: the state's pieces, float32 tensors of one shape [B, ...];
    ``step(src, dst)`` evaluates f at the pieces ``src`` and writes the result into the pieces ``dst`` (views of the history; it must
    not write ``src``).  Returns the reference's dict with ``result`` as a list of pieces."""
    _check_threshold(threshold)
    if stop_mode not in ("rel", "abs"):
        raise ValueError(f"anderson: stop_mode {stop_mode!r} ('rel' or 'abs')")
    other = "rel" if stop_mode == "abs" else "abs"
    x0 = [ops.require(t, what="anderson state") for t in x0]
    shape = tuple(x0[0].shape)
    if any(tuple(t.shape) != shape for t in x0):
        raise be.DpxError(f"anderson: the state's pieces differ in shape: {[tuple(t.shape) for t in x0]}")
    P, B = len(x0), shape[0]
    hist = ops.AndersonHistory(m, P, B, shape[1:], x0[0].device)
    m = hist.m
    lowest_x = torch.empty_like(hist.X)
    Xp, Fp = list(hist.X.unbind(0)), [list(hist.F[s].unbind(0)) for s in range(m)]    # the piece views, made once
    for p in range(P):
        Xp[p].copy_(x0[p])
    step(Xp, Fp[0])                                                        # X_0 = x0, F_0 = f(x0)
    hist.gram_row(0, 1)
    if m > 1:
        step(Fp[0], Fp[1])                                                 # X_1 = F_0, F_1 = f(F_0)
        hist.gram_row(1, 2, X=hist.F[0])
    trace = {"abs": [], "rel": []}
    lowest = {"abs": 1e8, "rel": 1e8}
    lowest_step = {"abs": 0, "rel": 0}
    for k in range(2, int(threshold)):
        n = min(k, m)
        hist.mix(n, beta, lam)
        ks = k % m
        step(Xp, Fp[ks])
        nrm = hist.gram_row(ks, min(k + 1, m)).cpu().numpy().astype(np.float64)   # (the step's one host read: [B, 2])
        abs_diff = float(np.sqrt(nrm[:, 0].sum()))
        diff = {"abs": abs_diff, "rel": abs_diff / (1e-5 + float(np.sqrt(nrm[:, 1].sum())))}
        trace["abs"].append(diff["abs"])
        trace["rel"].append(diff["rel"])
        for mode in ("rel", "abs"):
            if diff[mode] < lowest[mode]:
                if mode == stop_mode:
                    lowest_x.copy_(hist.X)
                lowest[mode] = diff[mode]
                lowest_step[mode] = k
        if trace[stop_mode][-1] < eps:
            for _ in range(int(threshold) - 1 - k):
                trace[stop_mode].append(lowest[stop_mode])
                trace[other].append(lowest[other])
            break
    if lowest_step[stop_mode] == 0:
        raise be.DpxError(f"anderson: no step reached a {stop_mode} residual below 1e8 (a NaN or a diverging f); traces {trace}")
    return {"result": list(lowest_x.unbind(0)), "lowest": lowest[stop_mode], "nstep": lowest_step[stop_mode], "prot_break": False,
            "abs_trace": trace["abs"], "rel_trace": trace["rel"], "eps": eps, "threshold": threshold}


def anderson(f, x0, m=6, lam=1e-4, threshold=50, eps=1e-3, stop_mode="rel", beta=1.0, **kwargs):
    """Anderson acceleration for the fixed point of ``f`` from the packed 4-D state ``x0`` (deq/utils/solvers.py:193-254: same
    arguments, same returned keys).  ``f`` is opaque here, so each evaluation's result is copied into the history once; a solver's own
    iteration goes through ``anderson_pieces`` instead, which writes the history in place."""
    _check_threshold(threshold)
    if x0.ndim != 4:
        raise be.DpxError(f"anderson: expected a packed [B, d, H, W] state, got shape {tuple(x0.shape)}")

    def step(src, dst):
        dst[0].copy_(f(src[0]))
    with torch.no_grad():
        out = anderson_pieces(step, [x0.detach().contiguous()], m, lam, threshold, eps, stop_mode, beta)
    out["result"] = out["result"][0]
    return out


def _unsupported(solver):
    """what keeps ``solver`` off the DEQ specialization (None: it is supported)"""
    if not isinstance(solver, Algorithm):
        return f"a compiled solver is required, got {type(solver).__name__}"
    if type(solver) is not ADMM:
        return f"solver {type(solver).__name__}: only ADMM problems on the fused plan are supported"
    ls = getattr(solver, "least_square", None)
    if not isinstance(ls, least_squares) or not ls.freq_diagonalizable:
        return "the x-update is not a Fourier solve (a CG / direct x-update has no fused plan)"
    if len(solver.psi_fns) == 0:
        return "the problem has no split term: its ADMM is a direct solve, not a fixed-point iteration"
    plan = fused.plan_admm(solver, (torch.empty(0, 0, 0, 0), [], []))
    if plan is None:
        return ("the fused ADMM plan does not take this problem (data terms on x or conv(x); norm1 / norm2 / nonneg on x, grad(x, 0) "
                "or grad(x, 1))")
    for fn, (_, pc) in zip(solver.psi_fns, plan.codes):
        if pc == be.PROX_EXTERNAL:
            return (f"a denoiser prior ({type(fn).__name__}) in the iteration: only the closed-form proxes norm1 / norm2 / nonneg are "
                    "supported")
    return None


class _FusedStep:
    """one full ADMM iteration (algo/admm.py:49-59) from the pieces ``src`` into the pieces ``dst`` on the fused stages"""

    def __init__(self, solver, plan, x0, rho, lam):
        self.solver, self.plan = solver, plan
        ls = solver.least_square
        dev, B = x0.device, int(x0.shape[0])
        self.psi = list(solver.psi_fns)
        self.n = len(self.psi)
        self.rho = ops.as_batch_vec(rho, B, dev)
        self.lam = [fused._lam_table(fn, ops.as_batch_vec(lam[fn], B, dev)) for fn in self.psi]      # (priors: the noise level)
        self.FK = plan._data_spectrum(x0)
        (self.t0, self.c0), (self.t1, self.c1) = ls.diag_tables(x0.shape, dev, True)
        self.eps = fused.ls_eps(ls)
        self.rhs = torch.empty_like(x0)
        self.terms = {}                   # (source, destination) -> the two stages' term tables: m + 1 pairs over a solve

    def _tables(self, src, dst):
        """the term tables (host-side structs of pointers, passed by value with the launch) of the right-hand-side stage reading
        ``src`` and of the z / dual stage writing ``dst``, built once per pair"""
        n = self.n
        v_in, u_in, v, u = src[1:1 + n], src[1 + n:], dst[1:1 + n], dst[1 + n:]
        specs = [dict(linop=lc, prox=pc, alpha=float(fn.alpha), lam=self.lam[i], v=v_in[i], u=u_in[i])
                 for i, (fn, (lc, pc)) in enumerate(zip(self.psi, self.plan.codes))]
        rhs_terms = ops.make_terms(specs)
        for i, sp in enumerate(specs):                                       # z / dual stage, out of place: (x, u_in) -> (v, u)
            sp["v"], sp["u_out"] = v[i], u[i]
        return rhs_terms, ops.make_terms(specs)

    def __call__(self, src, dst):
        key = (src[0].data_ptr(), dst[0].data_ptr())
        if key not in self.terms:
            self.terms[key] = self._tables(src, dst)
        rhs_terms, z_terms = self.terms[key]
        ops.admm_rhs(self.rhs, None, self.rho, rhs_terms, self.n)
        ops.fourier_solve(self.rhs, self.t0, self.t1, self.c0, self.c1, self.rho, self.eps, out=dst[0], spec_add=self.FK)
        ops.admm_zupdate(dst[0], z_terms, self.n)


class _ImplicitBackward(torch.autograd.Function):
    """identity on f(z*)'s pieces; backward solves y = J_f(z*)^T y + grad by Anderson acceleration (deq/solver.py:42-50)"""

    @staticmethod
    def forward(ctx, owner, z, b_thres, eps, *new):
        ctx.owner, ctx.z, ctx.b_thres, ctx.eps, ctx.new = owner, z, b_thres, eps, new
        return tuple(t.view_as(t) for t in new)

    @staticmethod
    def backward(ctx, *grads):
        new, z = ctx.new, ctx.z
        g = [gi.contiguous() for gi in grads]

        def step(src, dst):
            jy = torch.autograd.grad(new, z, list(src), retain_graph=True, allow_unused=True)
            for p, dp in enumerate(dst):                                     # (x_in does not enter an ADMM iteration: no gradient)
                if jy[p] is None:
                    dp.copy_(g[p])
                else:
                    ops.lincomb([(1.0, jy[p].contiguous()), (1.0, g[p])], out=dp)
        with torch.no_grad():
            out = anderson_pieces(step, [torch.zeros_like(gi) for gi in g], threshold=ctx.b_thres, eps=ctx.eps)
        ctx.owner.last_backward = out
        return (None, None, None, None, *out["result"])


class DEQSolver(nn.Module):
    def __init__(self, solver, learned_params=False, rhos=None, lams=None, f_thres=40, b_thres=40):
        super().__init__()
        why = _unsupported(solver)
        if why is not None:
            raise NotImplementedError(f"specialization 'deq': {why}")
        self.internal = solver
        self.f_thres, self.b_thres = f_thres, b_thres
        self.eps = 1e-3                   # the stop rule's bound of both Anderson solves (the reference's default)
        self.learned_params = learned_params
        if learned_params:
            self.r = nn.Parameter(torch.tensor(1.))
            self.l = nn.Parameter(torch.tensor(1.))
        self.rhos, self.lams = rhos, lams
        self.last_forward = None          # the forward Anderson solve's dict (result: z*'s pieces, traces, nstep) of the last solve
        self.last_backward = None         # the same of the last backward solve

    def solve(self, x0=None, rhos=None, lams=None, f_thres=None, b_thres=None, **kwargs):
        s = self.internal
        f_thres = self.f_thres if f_thres is None else f_thres
        b_thres = self.b_thres if b_thres is None else b_thres
        device = s.device
        if device.type != "cuda" and not be.host_mode():
            raise be.DpxError(f"solver lives on {device}: the MI355X backend has no CPU path; specialize(..., device='cuda')")
        x0 = to_tensor(x0, batch=True)
        x0, rhos, lams, _ = s.defaults(x0, None if rhos is None else to_tensor(rhos), None if lams is None else to_tensor(lams), 1)
        with be.device_guard(device), be.solve_scope("solve"):
            x0, rhos, lams = move(x0, rhos, lams, device=device)
            x0 = x0.contiguous()
            rho = rhos[..., 0]
            lam = {fn: lams[fn][..., 0] for fn in s.psi_fns}
            if self.learned_params:
                rho = self.r * rho
                lam = {fn: val * self.l for fn, val in lam.items()}
            plan = s._plan_for(x0) if s.use_fused else None
            if plan is None:
                raise NotImplementedError(f"specialization 'deq': the fused ADMM plan does not take an iterate of shape {tuple(x0.shape)}, "
                                          f"{x0.dtype}")
            n = len(s.psi_fns)
            with torch.no_grad():
                x, v, u = s.initialize(x0)
                fused.clear_fresh(s)
                step = _FusedStep(s, plan, x0, rho.detach(), {fn: val.detach() for fn, val in lam.items()})
                out = anderson_pieces(step, [x.contiguous()] + [t.contiguous() for t in v] + [t.contiguous() for t in u], threshold=f_thres, eps=self.eps)
            self.last_forward = out
            z = out["result"]
            if not (self.training and torch.is_grad_enabled()):
                # (the reference returns the lowest-residual X itself outside training: z*, not f(z*))
                s.Kall.update_vars([z[0]])
                return z[0]
            z = [t.requires_grad_() for t in z]
            with torch.enable_grad():
                sched = lambda t: t.reshape(1) if t.ndim == 0 else t.reshape(-1, 1)
                new = s.iters((z[0], z[1:1 + n], z[1 + n:]), sched(rho), {fn: sched(val) for fn, val in lam.items()}, 1)
                new = [new[0]] + list(new[1]) + list(new[2])
                new = _ImplicitBackward.apply(self, z, b_thres, self.eps, *new)
            s.Kall.update_vars([new[0].detach()])
            return new[0]

    def forward(self, **kwargs):
        return self.solve(**kwargs)

    def load(self, state_dict, strict=True):
        self.load_state_dict(state_dict["solver"], strict=strict)
        self.rhos = state_dict.get("rhos")
        self.lams = state_dict.get("lams")
