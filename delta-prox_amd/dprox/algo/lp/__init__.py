from .solvers import LPConvergenceLoss, LPProblem, LPSolverADMM
from .utils import Ruiz_equilibration_sparse_np, as_csr, pcg_rtol, validate_csr
