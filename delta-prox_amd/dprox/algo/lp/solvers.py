"""The LP solver on the HIP kernels of csrc/dpx_lp.hip (reference dprox/algo/lp/solvers.py: ``LPProblem``, ``LPSolverADMM``, whose
semantics are kept literally, quirks included): an OSQP-style ADMM in float64 on a sparse constraint matrix, its x-update a
warm-started, Jacobi-preconditioned conjugate-gradient solve that the device controls.

    min c.x   s.t.   A_ub x <= b_ub,   A_eq x == b_eq,   x_lb <= x <= x_ub          (defaults x_lb = 0, x_ub = +inf)

``LPProblem`` does the reference's preprocessing on the host with NumPy (Ruiz equilibration of [A_ub; A_eq; I], the scalings
gamma_c / gamma_b, the column 2-norms of the preconditioner); ``LPSolverADMM.solve`` issues, per outer iteration, ``dpx_lp_pcg_start``,
inner iterations of three launches each until the device's ``done`` flag is seen, and ``dpx_lp_tail``.  The host runs ahead of the
device: it issues as many inner iterations as the previous outer iteration took, then two at a time, and learns of ``done`` from a
pinned copy of the state's control words one chunk late (iterations issued after ``done`` return at once and change nothing).  It
reads results only at the evaluation steps (every ``eval_freq``-th outer iteration), where the reference synchronises too.

Not built (each raises NotImplementedError by name): training the parameters (``adapt_params`` / ``optimize_params``), ``direct``,
``polish``, ``problem_scale``, ``dtype=float32``, a norm other than the infinity norm, the reference's dense preprocessing branch
(dense input runs the sparse branch) and a single-workgroup persistent solve for tiny systems."""
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn

from ... import _backend as be
from ... import _ops as ops
from . import utils
from .utils import NOT_BUILT


class LPConvergenceLoss(nn.Module):
    """log(r_norm / eps_primal) + log(s_norm / eps_dual) (the reference's training loss; the solve here is not differentiable)"""

    def forward(self, r_norm, s_norm, eps_primal, eps_dual):
        return torch.log(r_norm / eps_primal) + torch.log(s_norm / eps_dual)


class LPProblem:
    def __init__(self, c, A_ub, b_ub, A_eq, b_eq, x_lb=None, x_ub=None, norm_ord=float("inf"), dtype=torch.float64, sparse=True, device=None):
        if dtype != torch.float64:
            raise NotImplementedError(f"LPProblem: dtype={dtype} {NOT_BUILT}: the solver is float64")
        if norm_ord != float("inf"):
            raise NotImplementedError(f"LPProblem: norm_ord={norm_ord} {NOT_BUILT}: the infinity norm only")
        self.device = device
        self.c = utils.as_vector(c, "c")
        n = self.n = len(self.c)
        self.A_ub, self.A_eq = utils.as_csr(A_ub, "A_ub"), utils.as_csr(A_eq, "A_eq")
        self.b_ub, self.b_eq = utils.as_vector(b_ub, "b_ub"), utils.as_vector(b_eq, "b_eq")
        self.x_lb = np.zeros(n) if x_lb is None else utils.as_vector(x_lb, "x_lb")
        self.x_ub = np.full(n, np.inf) if x_ub is None else utils.as_vector(x_ub, "x_ub")
        for name, v, length in (("b_ub", self.b_ub, self.A_ub[3][0]), ("b_eq", self.b_eq, self.A_eq[3][0]), ("x_lb", self.x_lb, n), ("x_ub", self.x_ub, n)):
            if len(v) != length:
                raise ValueError(f"LP: {name} has {len(v)} entries, expected {length}")
        self.original_problem = self.c, self.A_ub, self.b_ub, self.A_eq, self.b_eq, self.x_lb, self.x_ub
        self._preprocess()

    def unpack(self):
        return self.original_problem

    def _preprocess(self):
        n, m_ub = self.n, self.A_ub[3][0]
        A = utils.vstack_identity(self.A_ub, self.A_eq, n)
        self.m = A[3][0]
        self.d, self.e, self.gamma_c, self.gamma_b, abar = utils.Ruiz_equilibration_sparse_np(A, self.c, np.concatenate([self.b_ub, self.b_eq, self.x_ub]))
        self.Acnorm = np.sqrt(np.bincount(A[1], weights=abar * abar, minlength=n))
        self.A = (A[0], A[1], abar)
        self.AT = utils.transpose_csr(A[0], A[1], abar, A[3])[:3]
        self.lb = np.concatenate([np.full(m_ub, -np.inf), self.b_eq, self.x_lb])
        self.ub = np.concatenate([self.b_ub, self.b_eq, self.x_ub])

    def get_data(self):
        return self.d.copy(), self.e.copy(), self.gamma_c, self.gamma_b, self.A, self.AT, self.Acnorm, self.ub.copy(), self.lb.copy(), self.c.copy()

    @property
    def problem_scale(self):
        return (self.m, self.n)


class LPSolverADMM(nn.Module):
    def __init__(self, rho=1, problem_scale=None, abstol=1e-4, reltol=1e-3, norm_ord=float("inf"), max_iters=5000, dtype=torch.float64, verbose=True):
        super().__init__()
        if problem_scale is not None:
            raise NotImplementedError(f"LPSolverADMM: problem_scale (learned row / column scalings) {NOT_BUILT}")
        if dtype != torch.float64:
            raise NotImplementedError(f"LPSolverADMM: dtype={dtype} {NOT_BUILT}: the kernels are float64")
        if norm_ord != float("inf"):
            raise NotImplementedError(f"LPSolverADMM: norm_ord={norm_ord} {NOT_BUILT}: the infinity norm only")
        self.problem_scale, self.abstol, self.reltol, self.norm_ord = problem_scale, abstol, reltol, norm_ord
        self.max_iters, self.dtype, self.verbose = max_iters, dtype, verbose
        self.rho = nn.Parameter(torch.tensor(rho, dtype=dtype))
        self.sigma_log = nn.Parameter(torch.tensor(np.log(1e-6), dtype=dtype))
        self.alpha = nn.Parameter(torch.tensor(1.6, dtype=dtype))
        self.gamma_c_mul = nn.Parameter(torch.tensor(1., dtype=dtype))
        self.gamma_b_mul = nn.Parameter(torch.tensor(1., dtype=dtype))
        self.last_stats = None

    def extra_repr(self):
        return (f"rho={self.rho.item():.3e}; sigma={torch.exp(self.sigma_log).item():.3e}; alpha={self.alpha.item():.3e}; "
                f"gamma_c_mul={self.gamma_c_mul.item():.3e}; gamma_b_mul={self.gamma_b_mul.item():.3e};")

    def optimize_params(self, *args, **kwargs):
        raise NotImplementedError(f"LPSolverADMM.optimize_params (training rho, sigma and alpha through the iterations) {NOT_BUILT}")

    def control(self, lpproblem, device):
        """(the device-resident state of a solve of ``lpproblem`` at its start, gamma_c, gamma_b): the scaled cost
        c <- gamma_c d c, the finite bounds scaled by gamma_b e, all iterates zero"""
        p = lpproblem
        gamma_c, gamma_b = float(self.gamma_c_mul.detach()) * p.gamma_c, float(self.gamma_b_mul.detach()) * p.gamma_b
        c = gamma_c * (p.d * p.c)
        lb, ub = p.lb.copy(), p.ub.copy()
        for bound in (lb, ub):
            mask = ~np.isinf(bound)
            bound[mask] *= gamma_b * p.e[mask]
        return ops.LpControl(p.A, p.AT, p.m, p.n, c, p.Acnorm, lb, ub, p.d, p.e, device), gamma_c, gamma_b

    @torch.no_grad()
    def solve(self, lpproblem, rho=None, sigma=None, alpha=None, max_iters=None, eval_freq=25, residual_balance=False, direct=False, polish=False):
        if direct:
            raise NotImplementedError(f"LPSolverADMM.solve: direct=True (a dense inverse as the x-update) {NOT_BUILT}")
        if polish:
            raise NotImplementedError(f"LPSolverADMM.solve: polish=True (solution polishing) {NOT_BUILT}")
        if max_iters is None:
            max_iters = self.max_iters
        p = lpproblem
        device = torch.device(p.device) if p.device is not None else be.default_device()
        rho = float(self.rho.detach() if rho is None else rho)
        sigma = float(torch.exp(self.sigma_log.detach()) if sigma is None else sigma)
        alpha = float(self.alpha.detach() if alpha is None else alpha)
        d = p.d
        with be.device_guard(device):
            ctl, gamma_c, gamma_b = self.control(p, device)
            pacer = _Pacer(ctl)
            history = defaultdict(list)

            def evaluate():
                ctl.eval(gamma_c, gamma_b)
                ev = ctl.fields()["eval"].cpu().numpy()              # the synchronisation of an evaluation step
                objval, r_norm, s_norm = float(ev[0]), float(ev[1]), float(ev[2])
                return objval, r_norm, s_norm, self.abstol + self.reltol * max(ev[3], ev[4]), self.abstol + self.reltol * max(ev[5], ev[6])

            k = -1
            for k in range(max_iters):
                ctl.pcg_start(rho, sigma, utils.pcg_rtol(k))
                pacer.run(rho, sigma)
                ctl.tail(alpha, rho)
                if k % eval_freq == 0:
                    objval, r_norm, s_norm, eps_primal, eps_dual = evaluate()
                    if residual_balance and k % 1000 == 0 and k != 0:
                        if r_norm > 10 * eps_primal or eps_dual > 10 * s_norm:
                            rho = rho * 2
                        elif s_norm > 10 * eps_dual or eps_primal > 10 * r_norm:
                            rho = rho / 2
                    for name, v in (("r_norm", r_norm), ("s_norm", s_norm), ("eps_primal", eps_primal), ("eps_dual", eps_dual), ("objval", objval)):
                        history[name].append(v)
                    stop = not self.training and r_norm < eps_primal and s_norm < eps_dual
                    if not self.training and self.verbose and (stop or k % 1000 == 0):
                        print(f"Obj: {objval:.2e}, res_primal: {r_norm:.2e}, res_dual: {s_norm:.2e}, eps_primal: {eps_primal:.2e}, "
                              f"eps_dual: {eps_dual:.2e}, rho: {rho:.2e}")
                    if stop:
                        break
            results = evaluate()
            res_z = float(ctl.fields()["eval"][7])
            if self.verbose:
                print(f"Obj: {results[0]:.2e}, res_z: {res_z:.2e}, res_primal: {results[1]:.2e}, res_dual: {results[2]:.2e}, "
                      f"eps_primal: {results[3]:.2e}, eps_dual: {results[4]:.2e}, rho: {rho:.2e}")
            self.last_stats = dict(outer_iterations=k + 1, operator_applications=int(ctl.fields()["ops"][0]), launches=ctl.launches, rho=rho,
                                   lanes=ctl.lanes())
            x = ctl.x * torch.from_numpy(d).to(device) / gamma_b
        return x.reshape(-1, 1), history, tuple(torch.tensor(v, dtype=torch.float64) for v in results)


class _Pacer:
    """issues the inner iterations of one PCG ahead of the device: as many as the previous solve took, then ``STEP`` at a time; the
    control words (done, inner, ops) of chunk i are copied to pinned memory behind it and looked at after chunk i + 1 has been
    issued, so the device always has work queued and at most a chunk or two of launches that return at once are wasted.  Without a
    device to run ahead of (the emulated build) the words are read after every iteration."""
    STEP, RING = 2, 4

    def __init__(self, ctl):
        self.ctl = ctl
        self.predicted = 8
        self.on_gpu = ctl.words.is_cuda
        if self.on_gpu:
            self.pins = [torch.empty(3, dtype=torch.int64, pin_memory=True) for _ in range(self.RING)]
            self.events = [torch.cuda.Event() for _ in range(self.RING)]

    def run(self, rho, sigma):
        ctl, cap = self.ctl, self.ctl.MAX_INNER
        if not self.on_gpu:
            while True:
                ctl.pcg_iters(rho, sigma, 1)
                if int(ctl.words[0]):
                    return
        issued, chunk, i, inner = 0, max(1, min(self.predicted, cap)), 0, None
        while inner is None:
            ctl.pcg_iters(rho, sigma, chunk)
            issued += chunk
            self.pins[i % self.RING].copy_(ctl.words, non_blocking=True)
            self.events[i % self.RING].record()
            for j in ((i - 1, i) if issued >= cap else (i - 1,)):        # everything is issued: wait for the newest words as well
                if j >= 0 and inner is None:
                    self.events[j % self.RING].synchronize()
                    if int(self.pins[j % self.RING][0]):
                        inner = int(self.pins[j % self.RING][1])
            i, chunk = i + 1, min(self.STEP, max(cap - issued, 1))
        self.predicted = inner
