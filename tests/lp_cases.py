"""LP-solver cases shared by the GPU tests (-m gpu, real MI355X), the emulated-kernel tests (CPU, the same kernel sources under the
SIMT emulator) and the host tests: every stage of an iteration against a float64 NumPy restatement written here, and
``LPSolverADMM`` against the reference's stored runs (tests/golden/g45_lp*.npz, make_golden_lp.py).

Single stages (the only fixed, derived bounds; u = 2^-52): a row product or reduction over N terms is within
(sqrt(N) + 4) u sum|terms|; an elementwise result within 4 u of the sum of the magnitudes of its terms, plus what the error of an
input computed in the same launch contributes; the clip is exact; ``done``, the inner count and the operator count are exact.  Each
stage is compared given the device's result of the stage before, so the bounds do not compound.

Solver (round-off amplified by the recurrences, so no number chosen in advance): the operator count, the number of evaluations and
the final rho are the reference's; x, and every entry of ``history`` (the series of one quantity over the evaluations), is within
8 perm64 + SLACK64 of the reference's in relative l2, where perm64 is the largest distance of the reference's own x over four runs
with the rows and unknowns permuted and SLACK64 the project's float64 slack (minres_cases.py).  The factor 8: the kernels differ from
the reference by summation order and FMA contraction, rounding-level perturbations of the same kind as a permutation, which four
permutations sample thinly.  (``longrow`` runs 18 outer iterations: make_golden_lp.py says why.)"""
import json
import os

import numpy as np
import torch

from conftest import load_golden, record, rel_l2
from minres_cases import SLACK64

U = 2.0 ** -52
CASES = ["tiny", "small", "odd", "wide", "longrow"]
STEP_CASES = ["tiny", "odd", "longrow"]
SERIES = ("objval", "r_norm", "s_norm", "eps_primal", "eps_dual")
ACHIEVED = {}          # case -> distances; written to the file DPX_LP_PARITY_OUT names, if it is set (write_achieved)

_golden = {}


def golden():
    if not _golden:
        for f in ("g45_lp", "g45_lp_wide"):
            _golden.update(load_golden(f))
    return _golden


def csr_of(name, tag):
    g = golden()
    return g[f"{name}_{tag}_indptr"], g[f"{name}_{tag}_indices"], g[f"{name}_{tag}_data"], tuple(int(s) for s in g[f"{name}_{tag}_shape"])


def problem(name, device=None):
    from dprox.algo import lp
    g = golden()
    return lp.LPProblem(g[f"{name}_c"], csr_of(name, "ub"), g[f"{name}_b_ub"], csr_of(name, "eq"), g[f"{name}_b_eq"], device=device)


def settings(name):
    rho, abstol, reltol, iters, balance = golden()[f"{name}_cfg"]
    return dict(rho=float(rho), abstol=float(abstol), reltol=float(reltol), max_iters=int(iters)), bool(balance)


_solved = {}


def solve(name, device, max_iters=None, keep=False):
    """the stored case with the settings of its reference run (``max_iters``: a shorter one): (x [n], history, results, last_stats);
    ``keep``: the run is computed once and shared (the callers leave it unchanged)"""
    from dprox.algo import lp
    if keep and (name, str(device)) in _solved:
        return _solved[(name, str(device))]
    kw, balance = settings(name)
    if max_iters is not None:
        kw["max_iters"] = max_iters
    solver = lp.LPSolverADMM(verbose=False, **kw).eval()
    x, history, results = solver.solve(problem(name, device), residual_balance=balance)
    assert x.dtype == torch.float64 and x.device.type == torch.device(device).type and x.shape == (len(golden()[f"{name}_c"]), 1)
    out = x.reshape(-1), history, results, solver.last_stats
    if keep:
        _solved[(name, str(device))] = out
    return out


# ---- the solver against the reference's run ----------------------------------------------------------------------------------------

def case_parity(device, name):
    g = golden()
    x, history, results, stats = solve(name, device, keep=True)
    x = x.cpu().numpy()
    ops_ref, perm = int(g[f"{name}_ops"]), float(g[f"{name}_perm64"])
    bound = 8 * perm + SLACK64
    ref_hist = g[f"{name}_history"]
    d_x = rel_l2(x, g[f"{name}_x"])
    d_h = {k: rel_l2(history[k], ref_hist[i]) if len(history[k]) == ref_hist.shape[1] else None for i, k in enumerate(SERIES)}
    d_res = rel_l2([float(r) for r in results], g[f"{name}_results"])
    ACHIEVED[name] = dict(x_vs_ref=d_x, history_vs_ref=d_h, results_vs_ref=d_res, perm64=perm, bound=bound, ops=stats["operator_applications"],
                          ops_ref=ops_ref, ops_ref_permuted=[int(v) for v in g[f"{name}_ops_perm"]], evaluations=len(history["objval"]),
                          rho=stats["rho"], outer_iterations=stats["outer_iterations"], launches=stats["launches"], lanes=list(stats["lanes"]))
    record(f"lp {name} x vs the reference's run", d_x, bound)
    print(f"lp {name}: |x - x_ref| {d_x:.3e} (bound {bound:.3e}, perm64 {perm:.3e}); history {d_h}; ops {stats['operator_applications']} "
          f"(reference {ops_ref}); rho {stats['rho']}")
    assert np.isfinite(x).all()
    assert stats["operator_applications"] == ops_ref, (name, stats["operator_applications"], ops_ref)
    assert all(len(history[k]) == ref_hist.shape[1] for k in SERIES), (name, len(history["objval"]), ref_hist.shape)
    assert stats["rho"] == float(g[f"{name}_rho"]), (name, stats["rho"], float(g[f"{name}_rho"]))
    assert d_x <= bound, (name, d_x, bound)
    for k in SERIES:
        assert d_h[k] <= bound, (name, k, d_h[k], bound)
    if name == "tiny":
        assert stats["outer_iterations"] < settings(name)[0]["max_iters"]            # the early stop
    if name == "small":
        assert stats["rho"] != settings(name)[0]["rho"]                               # the balance step at k = 1000


def case_guarded(device, name, max_iters=None):
    """a run of its own (nothing shared: its buffers are the guarded ones) for tests/guarded_alloc.py: the whole parity case, or,
    cut short at ``max_iters``, the evaluations it contains against the reference's first ones"""
    if max_iters is None:
        _solved.pop((name, str(device)), None)
        case_parity(device, name)
        _solved.pop((name, str(device)), None)
        return
    g = golden()
    x, history, _, stats = solve(name, device, max_iters)
    bound = 8 * float(g[f"{name}_perm64"]) + SLACK64
    evals = len(range(0, max_iters, 25))
    assert torch.isfinite(x).all() and stats["outer_iterations"] == max_iters
    for i, k in enumerate(SERIES):
        assert len(history[k]) == evals and rel_l2(history[k], g[f"{name}_history"][i, :evals]) <= bound, (name, k, history[k])


def case_objective(device, name, x=None):
    """c.x at the stored end is as close to the optimum c.x* as the reference's own objective, plus 1e-9"""
    g = golden()
    if x is None:
        x = solve(name, device, keep=True)[0]
    c, opt = g[f"{name}_c"], float(g[f"{name}_c"] @ g[f"{name}_xstar"])
    ours, theirs = abs(float(c @ x.cpu().numpy()) - opt), abs(float(g[f"{name}_results"][0]) - opt)
    print(f"lp {name}: |c.x - c.x*| {ours:.3e}; the reference's {theirs:.3e}")
    assert ours <= theirs + 1e-9, (name, ours, theirs)


def case_deterministic(device, name="odd", max_iters=None):
    """two solves give the same bits, and so do the two forms of the direction update"""
    from dprox import _backend as be
    a = solve(name, device, max_iters)
    b = solve(name, device, max_iters)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    with be.tuned(lp_split_direction=1):
        c = solve(name, device, max_iters)
    assert torch.equal(a[0], c[0]) and a[1] == c[1]
    assert c[3]["operator_applications"] == a[3]["operator_applications"] and c[3]["launches"] > a[3]["launches"]


def case_public(device, name="odd"):
    """``dp.Problem(c @ x, [A_ub @ x <= b_ub, A_eq @ x == b_eq]).solve()`` is the explicit solver call with Problem's settings"""
    import dprox as dp
    from dprox.algo import lp
    g = golden()
    dense = lambda tag: _dense(*csr_of(name, tag))
    x = dp.Variable()
    prob = dp.Problem(g[f"{name}_c"] @ x, [dense("ub") @ x <= g[f"{name}_b_ub"], dense("eq") @ x == g[f"{name}_b_eq"]])
    out = prob.solve(device=device)
    solver = lp.LPSolverADMM(rho=1e-1, abstol=1e-3, reltol=1e-6, max_iters=20000, verbose=False).eval()
    want, history, _ = solver.solve(problem(name, device), residual_balance=True)
    assert out.dtype == torch.float64 and out.shape == (len(g[f"{name}_c"]),) and out.device.type == torch.device(device).type
    assert torch.equal(out, want.reshape(-1))
    assert solver.last_stats["outer_iterations"] < 20000 and prob.prob.history == history


def _dense(indptr, indices, data, shape):
    D = np.zeros(shape)
    D[np.repeat(np.arange(shape[0]), np.diff(indptr)), indices] = data
    return D


def write_achieved():
    """the measured distances of the cases run so far -> the JSON file the environment variable DPX_LP_PARITY_OUT names (how
    profiles/lp_parity_achieved.json is produced from a GPU run); without the variable nothing is written"""
    path = os.environ.get("DPX_LP_PARITY_OUT")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ACHIEVED, f, indent=1, sort_keys=True)


# ---- single stages against float64 -----------------------------------------------------------------------------------------------

def _np(t):
    return t.detach().cpu().numpy().astype(np.float64).copy()


class _Csr:
    """a CSR matrix on the host: products and the magnitude sums their bounds need"""

    def __init__(self, indptr, indices, data):
        self.ptr, self.idx, self.val = np.asarray(indptr), np.asarray(indices), np.asarray(data)
        self.len = np.diff(self.ptr)

    def rows(self, terms):
        return np.add.reduceat(terms, self.ptr[:-1])

    def dot(self, v, mag=None):
        """(M v, its bound); ``mag``: the magnitudes of the gathered vector's terms when v is itself a sum"""
        ref = self.rows(self.val * v[self.idx])
        tol = (np.sqrt(self.len) + 4.0) * U * self.rows(np.abs(self.val) * (np.abs(v) if mag is None else mag)[self.idx])
        return ref, tol


def _close(dev, ref, tol, what):
    err = np.abs(np.asarray(dev) - np.asarray(ref))
    assert np.all(err <= np.asarray(tol) + 1e-300), (what, float(np.max(err - tol)), float(np.max(err)))


def _red(n):
    return (np.sqrt(n) + 4.0) * U


def case_steps(device, name, lanes, seed=0):
    """every stage once (three inner iterations: the folded direction update and both slots of p come up), with the lane-group
    width forced to ``lanes``, in both forms of the direction update"""
    from dprox import _backend as be
    for split in (0, 1):
        with be.tuned(lp_lanes=lanes, lp_split_direction=split):
            _steps(device, name, lanes, split, seed)


def _steps(device, name, lanes, split, seed):
    from dprox.algo import lp
    kw, _ = settings(name)
    solver = lp.LPSolverADMM(verbose=False, **kw).eval()
    p = problem(name, device)
    ctl, gamma_c, gamma_b = solver.control(p, device)
    assert ctl.lanes() == (lanes, lanes)
    m, n = p.m, p.n
    A, AT = _Csr(*p.A), _Csr(*p.AT)
    rho, sigma, alpha = 0.3, float(torch.exp(solver.sigma_log.detach())), 1.6
    rng = np.random.RandomState(seed)
    put = lambda t, a: t.copy_(torch.from_numpy(a))
    for t, length in ((ctl.x, n), (ctl.xt, n), (ctl.z, m), (ctl.y, m)):
        put(t, rng.randn(length))
    c, acn, lb, ub, d, e = (_np(ctl.buf[k]) for k in ("c", "acn", "lb", "ub", "d", "e"))
    M = sigma + rho * (acn * acn)
    f = ctl.fields()

    # ---- each row product ----
    x, xt, z, y = _np(ctl.x), _np(ctl.xt), _np(ctl.z), _np(ctl.y)
    t = _np(ctl.spmv("a", ctl.xt))
    _close(t, *A.dot(xt), "A xt")
    _close(_np(ctl.spmv("at", ctl.y)), *AT.dot(y), "AT y")
    put(ctl.t, t)

    # ---- pcg_start ----
    ops0 = int(f["ops"][0])
    ctl.pcg_start(rho, sigma, 0.0)                                         # rtol 0: never done
    g1, g1_tol = AT.dot(rho * z - y, np.abs(rho * z) + np.abs(y))
    g2, g2_tol = AT.dot(rho * t)
    right, r, yv = _np(ctl.right), _np(ctl.r), _np(ctl.yv)
    _close(right, sigma * x - c + g1, 4 * U * (np.abs(sigma * x) + np.abs(c) + np.abs(g1)) + g1_tol, "right")
    _close(r, g2 + sigma * xt - right, 4 * U * (np.abs(g2) + np.abs(sigma * xt) + np.abs(right)) + g2_tol, "r at the start")
    _close(yv, r / M, 4 * U * np.abs(r / M), "y = r / M at the start")
    assert np.array_equal(_np(ctl.p)[:n], -yv)
    _close(float(f["ry"][0]), np.sum(r * yv), _red(n) * np.sum(np.abs(r * yv)), "ry at the start")
    assert (int(f["done"][0]), int(f["inner"][0]), int(f["ops"][0]) - ops0, float(f["rtol"][0])) == (0, 0, 1, 0.0)

    # ---- inner iterations ----
    for i in range(3):
        ry, beta_old = float(f["ry"][0]), float(f["beta"][0])
        pbuf, xt, r, yv = _np(ctl.p).reshape(2, n), _np(ctl.xt), _np(ctl.r), _np(ctl.yv)
        ctl.pcg_iters(rho, sigma, 1)
        pnew = _np(ctl.p).reshape(2, n)
        if i == 0 or split:                                                # p of this iteration was there before the launches
            pv = pbuf[i & 1]
        else:                                                              # folded: formed by the product's gather
            pv = pnew[i & 1]
            _close(pv, -yv + beta_old * pbuf[(i + 1) & 1], 4 * U * (np.abs(yv) + np.abs(beta_old * pbuf[(i + 1) & 1])), "p (folded)")
            assert np.array_equal(pnew[(i + 1) & 1], pbuf[(i + 1) & 1])
        t = _np(ctl.t)
        _close(t, *A.dot(pv), "A p")
        g, g_tol = AT.dot(rho * t)
        Ap = _np(ctl.Ap)
        _close(Ap, g + sigma * pv, 4 * U * (np.abs(g) + np.abs(sigma * pv)) + g_tol, "Ap")
        pAp = float(f["pAp"][0])
        _close(pAp, np.sum(pv * Ap), _red(n) * np.sum(np.abs(pv * Ap)), "<p, Ap>")
        a = float(f["a"][0])
        _close(a, ry / pAp, 4 * U * abs(ry / pAp), "a")
        xt2, r2, y2 = _np(ctl.xt), _np(ctl.r), _np(ctl.yv)
        _close(xt2, xt + a * pv, 4 * U * (np.abs(xt) + np.abs(a * pv)), "xt")
        _close(r2, r + a * Ap, 4 * U * (np.abs(r) + np.abs(a * Ap)), "r")
        _close(y2, r2 / M, 4 * U * np.abs(r2 / M), "y = r / M")
        ry2 = float(f["ry"][0])
        _close(ry2, np.sum(r2 * y2), _red(n) * np.sum(np.abs(r2 * y2)), "ry")
        _close(float(f["beta"][0]), ry2 / ry, 4 * U * abs(ry2 / ry), "beta")
        assert float(f["rmax"][0]) == np.abs(r2).max()
        assert (int(f["done"][0]), int(f["inner"][0]), int(f["ops"][0]) - ops0) == (0, i + 1, i + 2)
        if split:                                                          # the launch of its own has written the next p
            nxt = _np(ctl.p).reshape(2, n)[(i + 1) & 1]
            _close(nxt, -y2 + float(f["beta"][0]) * pv, 4 * U * (np.abs(y2) + np.abs(float(f["beta"][0]) * pv)), "p (split)")

    # ---- done: exact, and what is issued behind it changes nothing ----
    put(ctl.t, _np(ctl.spmv("a", ctl.xt)))
    ctl.pcg_start(rho, sigma, 1e300)
    ctl.pcg_iters(rho, sigma, 1)
    assert (int(f["done"][0]), int(f["inner"][0])) == (1, 1)
    frozen = [_np(ctl.buf[k]) for k in ("xt", "r", "yv", "p", "Ap", "t", "state")]
    ctl.pcg_iters(rho, sigma, 2)
    assert all(np.array_equal(a, _np(ctl.buf[k])) for a, k in zip(frozen, ("xt", "r", "yv", "p", "Ap", "t", "state")))

    # ---- the tail ----
    x, xt, z, y = _np(ctl.x), _np(ctl.xt), _np(ctl.z), _np(ctl.y)
    ctl.tail(alpha, rho)
    t = _np(ctl.t)
    _close(t, *A.dot(xt), "A xt (tail)")
    _close(_np(ctl.x), alpha * xt + (1 - alpha) * x, 4 * U * (np.abs(alpha * xt) + np.abs((1 - alpha) * x)), "x (relaxed)")
    zt = alpha * t + (1 - alpha) * z
    zt_tol = 4 * U * (np.abs(alpha * t) + np.abs((1 - alpha) * z))
    v, v_tol = zt + y / rho, zt_tol + 4 * U * (np.abs(zt) + np.abs(y / rho))
    z2 = _np(ctl.z)
    assert np.all(z2 >= lb) and np.all(z2 <= ub)
    _close(z2, np.clip(v, lb, ub), v_tol, "z")
    assert np.array_equal(z2[v > ub + v_tol], ub[v > ub + v_tol]) and np.array_equal(z2[v < lb - v_tol], lb[v < lb - v_tol])       # the clip is exact
    _close(_np(ctl.y), y + rho * (zt - z2), 4 * U * (np.abs(y) + rho * (np.abs(zt) + np.abs(z2))) + rho * zt_tol, "y (dual)")

    # ---- the evaluation ----
    x, z, y = _np(ctl.x), _np(ctl.z), _np(ctl.y)
    ctl.eval(gamma_c, gamma_b)
    ev = _np(f["eval"])
    Ax, Ax_tol = A.dot(x)
    ATy, ATy_tol = AT.dot(y)
    sb, sc = 1 / e / gamma_b, 1 / d / gamma_c

    def norm_close(dev, vec, tol, what):
        _close(dev, np.abs(vec).max(), np.max(tol + 4 * U * np.abs(vec)), what)
    norm_close(ev[1], (Ax - z) * sb, (Ax_tol + 4 * U * (np.abs(Ax) + np.abs(z))) * sb, "r_norm")
    norm_close(ev[3], Ax * sb, Ax_tol * sb, "|A x|")
    norm_close(ev[4], z * sb, 0.0, "|z|")
    norm_close(ev[2], (c + ATy) * sc, (ATy_tol + 4 * U * (np.abs(c) + np.abs(ATy))) * sc, "s_norm")
    norm_close(ev[5], ATy * sc, ATy_tol * sc, "|AT y|")
    norm_close(ev[6], c * sc, 0.0, "|c|")
    assert ev[7] == np.abs(z - np.clip(z, lb, ub)).max()
    terms = (c / d / gamma_c) * (x * d / gamma_b)
    _close(ev[0], terms.sum(), _red(n) * np.abs(terms).sum() + 8 * U * np.abs(terms).sum(), "objval")


def case_nan_residual(device, name="tiny"):
    """a NaN in the residual never passes the stop test: the reference's ``max|r| < rtol`` is false on NaN, and the loop runs on"""
    from dprox.algo import lp
    kw, _ = settings(name)
    solver = lp.LPSolverADMM(verbose=False, **kw).eval()
    p = problem(name, device)
    ctl, _, _ = solver.control(p, device)
    rho, sigma = 0.3, float(torch.exp(solver.sigma_log.detach()))
    rng = np.random.RandomState(0)
    for t, length in ((ctl.x, p.n), (ctl.xt, p.n), (ctl.z, p.m), (ctl.y, p.m)):
        t.copy_(torch.from_numpy(rng.randn(length)))
    ctl.t.copy_(ctl.spmv("a", ctl.xt))
    f = ctl.fields()
    ctl.pcg_start(rho, sigma, 1e300)                                      # every finite residual is below this
    ctl.r[p.n - 1] = float("nan")
    ctl.pcg_iters(rho, sigma, 2)
    assert (int(f["done"][0]), int(f["inner"][0])) == (0, 2) and np.isnan(float(f["rmax"][0]))


def case_refused_shapes(device, name="tiny"):
    """the C ABI refuses, before any launch, a matrix with fewer rows than unknowns (no identity block: x would not be relaxed, the
    folded direction only partly written) and more entries than an int32 offset stepped by 64 lanes can take"""
    from ctypes import c_double
    import pytest
    from dprox import _backend as be
    from dprox.algo import lp
    kw, _ = settings(name)
    p = problem(name, device)
    ctl, gamma_c, gamma_b = lp.LPSolverADMM(verbose=False, **kw).eval().control(p, device)
    before = [_np(ctl.buf[k]) for k in ("xt", "r", "p", "t", "x", "z", "y", "state")]
    L, s, one = be.lib(), be.stream(), c_double(1.0)
    for m, n, nnz, why in ((p.n - 1, p.n, ctl.nnz, "identity block"), (p.m, p.n, 2 ** 31 - 64, "bad shape")):
        for fn, args in (("dpx_lp_pcg_start", (one, one, one)), ("dpx_lp_pcg_iters", (one, one, 1000, 1)), ("dpx_lp_tail", (one, one)),
                         ("dpx_lp_eval", (one, one))):
            with pytest.raises(be.DpxError, match=why):
                L.call(fn, ctl.tab, m, n, nnz, *args, s)
    assert all(np.array_equal(a, _np(ctl.buf[k])) for a, k in zip(before, ("xt", "r", "p", "t", "x", "z", "y", "state")))


# ---- the host layer, no device -----------------------------------------------------------------------------------------------------

def case_preprocess(name):
    """the preprocessing against the reference's stored d, e, gamma, Acnorm, lb, ub: 1e-13 relative, the infinities in place"""
    g, p = golden(), problem(name)
    for key, ours in (("d", p.d), ("e", p.e), ("Acnorm", p.Acnorm), ("lb", p.lb), ("ub", p.ub), ("gamma_c", p.gamma_c), ("gamma_b", p.gamma_b)):
        ref, ours = np.atleast_1d(g[f"{name}_{key}"]), np.atleast_1d(ours)
        assert ours.shape == ref.shape, (name, key, ours.shape, ref.shape)
        fin = np.isfinite(ref)
        assert np.array_equal(ours[~fin], ref[~fin]), (name, key, "infinities")
        assert np.all(np.abs(ours[fin] - ref[fin]) <= 1e-13 * np.abs(ref[fin])), (name, key, float(np.max(np.abs(ours[fin] - ref[fin]))))
    assert p.problem_scale == (len(p.e), len(p.d))
