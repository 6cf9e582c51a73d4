#!/usr/bin/env python
"""Golden vectors of the LP solver -- runs ONLY in the build container (needs the reference checkout and SciPy).

Loads make_golden.py's import shim (runpy: the module-level setup only, none of its fixtures is rebuilt) and runs the reference's
``lp.LPProblem(..., sparse=True, device=cpu)`` and ``lp.LPSolverADMM`` (dprox/algo/lp/solvers.py) in eval mode under ``no_grad``.

Every LP  min c.x  s.t.  A_ub x <= b_ub, A_eq x == b_eq, x >= 0  is built from a primal-dual pair, so it is feasible and bounded:
a point x* >= 0 with about 40 % of its coordinates at zero, b_ub = A_ub x* + slack with half of the slacks zero, b_eq = A_eq x*, and
c = -A_ub^T y_u - A_eq^T y_e + s with y_u >= 0 on the tight rows and s >= 0 on the zero coordinates: x* is optimal.  Matrix entries
are multiples of 1/4; a matrix with an empty row is refused.

Per case ``<name>_*``: the CSR arrays of A_ub and A_eq (``ub_indptr / ub_indices / ub_data``, ``eq_*``), ``c``, ``b_ub``, ``b_eq``,
``xstar``; the reference's preprocessing ``d``, ``e``, ``gamma_c``, ``gamma_b``, ``Acnorm``, ``lb``, ``ub``; its solve ``x``,
``history`` ([5, evaluations]: objval, r_norm, s_norm, eps_primal, eps_dual), ``results`` (the same five after the loop), ``rho``
(the final one), ``ops`` (the cumulative number of LPATA_Func.forward calls: one per PCG start and one per inner iteration), the
settings ``cfg`` (rho, abstol, reltol, max_iters, residual_balance) and ``perm64``: the largest relative l2 distance of ``x`` over
four re-runs with the rows and the unknowns permuted (four seeds), each mapped back.  A case whose four permuted runs do not all
reproduce ``ops`` is refused, and the next draw taken: a test must not rest on a PCG exit that sits on its threshold.  ``ops_perm``
keeps the counts of the four permuted runs (all equal to ``ops``).

    python tests/golden/make_golden_lp.py
"""
import os
import runpy

HERE = os.path.dirname(os.path.abspath(__file__))
G = runpy.run_path(os.path.join(HERE, "make_golden.py"), run_name="make_golden_shim")
np, torch, dp, save = G["np"], G["torch"], G["dp"], G["save"]
import scipy.sparse as sp  # noqa: E402
from dprox.algo import lp  # noqa: E402   (the REFERENCE's)
import dprox.algo.lp.solvers as lp_solvers  # noqa: E402

assert dp.__file__.startswith(G["REF"]), dp.__file__

SEED = 7
PROBLEM_DEFAULTS = dict(rho=1e-1, abstol=1e-3, reltol=1e-6, residual_balance=True)          # the reference's dprox/algo/problem.py
TIGHT = dict(rho=0.1, abstol=1e-7, reltol=1e-6, residual_balance=True)
# name -> ((n, m_ub, m_eq, density), settings)
CASES = {
    "tiny": ((5, 3, 1, 0.6), dict(TIGHT, max_iters=2100)),
    "small": ((40, 24, 8, 0.2), dict(TIGHT, max_iters=1030)),
    "odd": ((257, 130, 40, 0.05), dict(PROBLEM_DEFAULTS, max_iters=60)),
    "wide": ((1000, 600, 150, 0.01), dict(PROBLEM_DEFAULTS, max_iters=60)),
    "longrow": ((300, 60, 20, 0.05), dict(PROBLEM_DEFAULTS, max_iters=18)),
}
# longrow runs 18 outer iterations, not 60.  With a fully dense row the reference's PCG exits sit close to their threshold: over 60
# iterations at least one of the four permuted runs changed the operator count, by 1 .. 6 in 1500, in every one of 80 draws tried (with a dense
# column alone, or no dense row, it never moved), and the runs part early -- in draws 0 .. 5 at outer iteration 3, 2, 0, 3, 18, 4.  At 18
# iterations (about 570 operator applications, one evaluation and the closing one) the rule above holds as for every other case: draws
# 0 .. 3 are refused and draw 4 is stored, its five runs on one path.


def quarter_matrix(rng, m, n, density):
    """m x n, about ``density`` of its entries non-zero multiples of 1/4 in [-2, 2]; a row that came out empty gets one entry"""
    mask = rng.rand(m, n) < density
    vals = rng.randint(1, 9, (m, n)) / 4.0 * np.where(rng.rand(m, n) < 0.5, -1.0, 1.0)
    M = np.where(mask, vals, 0.0)
    for i in np.flatnonzero(~mask.any(axis=1)):
        M[i, rng.randint(n)] = rng.randint(1, 9) / 4.0
    return M


def build_lp(rng, n, m_ub, m_eq, density, longrow=False):
    A_ub, A_eq = quarter_matrix(rng, m_ub, n, density), quarter_matrix(rng, m_eq, n, density)
    if longrow:                                 # one fully dense row and one fully dense column of A_ub
        A_ub[m_ub // 2, :] = rng.randint(1, 9, n) / 4.0
        A_ub[:, n // 3] = rng.randint(1, 9, m_ub) / 4.0
    assert (A_ub != 0).any(axis=1).all() and (A_eq != 0).any(axis=1).all(), "empty row"
    zero = rng.rand(n) < 0.4
    xstar = np.where(zero, 0.0, rng.randint(1, 17, n) / 4.0)
    tight = rng.rand(m_ub) < 0.5
    slack = np.where(tight, 0.0, rng.randint(1, 17, m_ub) / 4.0)
    b_ub, b_eq = A_ub @ xstar + slack, A_eq @ xstar
    y_u = np.where(tight, rng.randint(1, 9, m_ub) / 4.0, 0.0)
    y_e = rng.randint(-8, 9, m_eq) / 4.0
    s = np.where(zero, rng.randint(1, 9, n) / 4.0, 0.0)
    c = -A_ub.T @ y_u - A_eq.T @ y_e + s
    return dict(A_ub=sp.csr_matrix(A_ub), A_eq=sp.csr_matrix(A_eq), c=c, b_ub=b_ub, b_eq=b_eq, xstar=xstar)


class CountedATA(lp_solvers.LPATA_Func):
    """the reference's operator, counting its applications and remembering the rho it was last built with"""
    n_calls = 0
    last_rho = None

    def __init__(self, A, AT, rho, sigma):
        super().__init__(A, AT, rho, sigma)
        CountedATA.last_rho = float(rho)

    def forward(self, x):
        CountedATA.n_calls += 1
        return super().forward(x)


lp_solvers.LPATA_Func = CountedATA


def reference_run(p, cfg):
    CountedATA.n_calls, CountedATA.last_rho = 0, None
    prob = lp.LPProblem(p["c"], p["A_ub"], p["b_ub"], p["A_eq"], p["b_eq"], sparse=True, device=torch.device("cpu"))
    solver = lp.LPSolverADMM(rho=cfg["rho"], abstol=cfg["abstol"], reltol=cfg["reltol"], max_iters=cfg["max_iters"], verbose=False).eval()
    with torch.no_grad():
        x, history, results = solver.solve(prob, residual_balance=cfg["residual_balance"])
    hist = np.array([history[k] for k in ("objval", "r_norm", "s_norm", "eps_primal", "eps_dual")], np.float64)
    return prob, x[:, 0].numpy().copy(), hist, np.array([float(r) for r in results]), CountedATA.last_rho, CountedATA.n_calls


def permuted(p, seed):
    rng = np.random.RandomState(seed)
    pu, pe, q = rng.permutation(p["A_ub"].shape[0]), rng.permutation(p["A_eq"].shape[0]), rng.permutation(p["c"].shape[0])
    return dict(A_ub=sp.csr_matrix(p["A_ub"][pu][:, q]), A_eq=sp.csr_matrix(p["A_eq"][pe][:, q]), c=p["c"][q], b_ub=p["b_ub"][pu],
                b_eq=p["b_eq"][pe]), q


class Refused(Exception):
    pass


def run_case(name, idx, draw=0):
    """``draw``: 0 is the case's first draw of the LP; main() takes the next one when a draw is refused, and says so"""
    (n, m_ub, m_eq, density), cfg = CASES[name]
    p = build_lp(np.random.RandomState([SEED, idx] + ([draw] if draw else [])), n, m_ub, m_eq, density, longrow=name == "longrow")
    prob, x, hist, results, rho, ops = reference_run(p, cfg)
    evals = len(range(0, cfg["max_iters"], 25))
    if name == "tiny":
        assert hist.shape[1] < evals, ("tiny: the reference did not stop early", hist.shape[1], evals)
    if name == "small":
        assert hist.shape[1] == evals and rho != cfg["rho"], ("small: rho did not move at k = 1000", rho)
    perm, ops_perm = 0.0, []
    for seed in range(4):
        pp, q = permuted(p, 100 + seed)
        _, xp, _, _, rho_p, ops_p = reference_run(pp, cfg)
        ops_perm.append(ops_p)
        if ops_p != ops or rho_p != rho:
            raise Refused(f"{name} draw {draw}: a permuted run took another path (ops {ops} / {ops_p}, rho {rho} / {rho_p})")
        back = np.empty_like(xp)
        back[q] = xp
        perm = max(perm, float(np.linalg.norm(back - x) / np.linalg.norm(x)))
    print(f"{name:8s} n {n:5d} m {m_ub + m_eq + n:5d} nnz {p['A_ub'].nnz + p['A_eq'].nnz:6d}  evals {hist.shape[1]:3d}  ops {ops:6d}  rho {rho:g}  "
          f"obj {results[0]:.6e} (c.x* {p['c'] @ p['xstar']:.6e})  r {results[1]:.1e} s {results[2]:.1e}  perm64 {perm:.2e}  ops of the permuted runs {ops_perm}")
    out = dict(c=p["c"], b_ub=p["b_ub"], b_eq=p["b_eq"], xstar=p["xstar"], x=x, history=hist, results=results, rho=rho, ops=ops, ops_perm=np.array(ops_perm), perm64=perm,
               d=prob.d.numpy().ravel(), e=prob.e.numpy().ravel(), gamma_c=float(prob.gamma_c), gamma_b=float(prob.gamma_b),
               Acnorm=prob.Acnorm.numpy().ravel(), lb=prob.lb.numpy().ravel(), ub=prob.ub.numpy().ravel(),
               cfg=np.array([cfg["rho"], cfg["abstol"], cfg["reltol"], cfg["max_iters"], float(cfg["residual_balance"])]))
    for tag, M in (("ub", p["A_ub"]), ("eq", p["A_eq"])):
        M.sort_indices()
        out.update({f"{tag}_indptr": M.indptr.astype(np.int32), f"{tag}_indices": M.indices.astype(np.int32), f"{tag}_data": M.data,
                    f"{tag}_shape": np.array(M.shape)})
    return {f"{name}_{k}": v for k, v in out.items()}


def main():
    small, wide = {}, {}
    for idx, name in enumerate(CASES):
        for draw in range(12):
            try:
                (wide if name == "wide" else small).update(run_case(name, idx, draw))
                break
            except Refused as why:
                print("refused:", why)
        else:
            raise SystemExit(f"{name}: twelve draws refused")
    save("g45_lp", **small)
    save("g45_lp_wide", **wide)


if __name__ == "__main__":
    main()
