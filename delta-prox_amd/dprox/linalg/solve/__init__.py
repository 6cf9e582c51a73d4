from .krylov import bdot, cg, cg2, expand, pcg, ravel
from .minres import minres

# (reference dprox/linalg/solve/__init__.py:1-22 also lists plss / plssw: the only two entries of its registry not built here)
__all__ = available_solvers = ["cg", "cg2", "pcg", "minres"]

SOLVERS = {"cg": cg, "cg2": cg2, "pcg": pcg, "minres": minres}
