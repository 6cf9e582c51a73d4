"""Host-side preprocessing of the LP solver (reference dprox/algo/lp/utils.py and LPProblem._preprocess, sparse branch) with NumPy
on CSR arrays -- the package does not import SciPy: SciPy matrices are accepted by duck typing (``.tocsr()``)."""
import numpy as np
import torch

NOT_BUILT = "is not built on this backend (DESIGN.md, \"LP\")"


def _refuse_float32(a, what):
    dt = getattr(a, "dtype", None)
    if dt in (np.float32, np.float16, torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"LP: {what} is {dt}: dtype=float32 {NOT_BUILT}; pass float64")


def as_vector(a, what):
    """a 1-D float64 NumPy array (a trailing dimension of 1 is dropped, as the reference's [n, 1] columns)"""
    _refuse_float32(a, what)
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 1:
        raise ValueError(f"LP: {what} of shape {a.shape} (expected a vector)")
    return np.ascontiguousarray(a)


def as_csr(M, what):
    """(indptr int64, indices int64, data float64, (rows, cols)) of a matrix given as anything with ``.tocsr()`` (SciPy), as an
    object with indptr / indices / data / shape, as a tuple of those four, or as a dense 2-D array or tensor; validated"""
    if hasattr(M, "tocsr") and not isinstance(M, (np.ndarray, torch.Tensor)):
        M = M.tocsr()
    if all(hasattr(M, k) for k in ("indptr", "indices", "data", "shape")) and not isinstance(M, (np.ndarray, torch.Tensor)):
        M = (M.indptr, M.indices, M.data, M.shape)
    if isinstance(M, tuple) and len(M) == 4 and np.ndim(M[3]) == 1 and len(M[3]) == 2:
        indptr, indices, data, shape = M
        _refuse_float32(data, f"{what}'s data")
        csr = (np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(data, dtype=np.float64),
               (int(shape[0]), int(shape[1])))
    else:
        _refuse_float32(M, what)
        if isinstance(M, torch.Tensor):
            if M.layout != torch.strided:
                M = M.to_dense()
            M = M.detach().cpu().numpy()
        D = np.asarray(M, dtype=np.float64)
        if D.ndim != 2:
            raise ValueError(f"LP: {what} of shape {D.shape} (expected a matrix)")
        r, c = np.nonzero(D)                                   # row-major: rows ascending, columns ascending inside a row
        csr = (np.concatenate([[0], np.cumsum(np.bincount(r, minlength=D.shape[0]))]).astype(np.int64), c.astype(np.int64), D[r, c], D.shape)
    validate_csr(*csr, what=what)
    return csr


def validate_csr(indptr, indices, data, shape, what="matrix"):
    """refuses, before anything is launched: offsets that are not monotone or do not start at 0 and end at nnz, mismatched lengths,
    an index outside [0, cols), an empty row (the reference divides by its zero norm and returns NaN), nnz > 2^31 - 65 (the kernels' limit)"""
    rows, cols = shape
    if indptr.ndim != 1 or indices.ndim != 1 or data.ndim != 1 or len(indptr) != rows + 1 or len(indices) != len(data):
        raise ValueError(f"LP: {what}: CSR arrays of lengths {len(indptr)}, {len(indices)}, {len(data)} for shape {tuple(shape)}")
    if len(data) > 2 ** 31 - 65:
        raise ValueError(f"LP: {what}: {len(data)} entries (row offsets are int32, stepped by up to 64 lanes: at most 2^31 - 65)")
    steps = np.diff(indptr)
    if indptr[0] != 0 or np.any(steps < 0):
        raise ValueError(f"LP: {what}: row offsets are not monotone from 0")
    if indptr[-1] != len(data):
        raise ValueError(f"LP: {what}: indptr[-1] = {indptr[-1]} but {len(data)} entries")
    if len(indices) and (indices.min() < 0 or indices.max() >= cols):
        raise ValueError(f"LP: {what}: a column index outside [0, {cols})")
    if np.any(steps == 0):
        raise ValueError(f"LP: {what}: row {int(np.flatnonzero(steps == 0)[0])} is empty (the equilibration divides by its norm)")
    if not np.all(np.isfinite(data)):
        raise ValueError(f"LP: {what}: a non-finite entry")


def vstack_identity(ub, eq, n):
    """CSR of [A_ub; A_eq; I_n]"""
    if ub[3][1] != n or eq[3][1] != n:
        raise ValueError(f"LP: A_ub of shape {ub[3]} and A_eq of shape {eq[3]} for {n} unknowns")
    nu, ne = len(ub[2]), len(eq[2])
    indptr = np.concatenate([ub[0], nu + eq[0][1:], nu + ne + np.arange(1, n + 1)])
    indices = np.concatenate([ub[1], eq[1], np.arange(n)])
    data = np.concatenate([ub[2], eq[2], np.ones(n)])
    return indptr, indices, data, (ub[3][0] + eq[3][0] + n, n)


def row_of_entry(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def _col_max(indices, mag, n):
    out = np.zeros(n)
    np.maximum.at(out, indices, mag)
    return out


def Ruiz_equilibration_sparse_np(A, c, b, max_iters=20, eps_equil=1e-3):
    """the reference's routine of the same name in the infinity norm: (d [n], e [m], gamma_c, gamma_b, data of Abar = E A D)"""
    indptr, indices, data, (m, n) = A
    rows = row_of_entry(indptr)
    d, e = np.ones(n), np.ones(m)
    abar = data
    for _ in range(max_iters):
        mag = np.abs(abar)
        delta1 = 1 / _col_max(indices, mag, n) ** 0.5
        delta2 = 1 / np.maximum.reduceat(mag, indptr[:-1]) ** 0.5
        d = d * delta1
        e = e * delta2
        abar = (e[rows] * data) * d[indices]
        if max(np.abs(1 - delta1).max(), np.abs(1 - delta2).max()) < eps_equil:
            break
    mag = np.abs(abar)
    Arnorm, Acnorm = np.maximum.reduceat(mag, indptr[:-1]), _col_max(indices, mag, n)
    c_bar = c * d
    mask = ~np.isinf(b)
    b_bar = b[mask] * e[mask]
    gamma_c = 1 / np.abs(c_bar).max() * Arnorm.mean()
    gamma_b = 1 / np.abs(b_bar).max() * Acnorm.mean()
    return d, e, float(gamma_c), float(gamma_b), abar


def transpose_csr(indptr, indices, data, shape):
    """CSR of the transpose (rows ascending inside each of its rows)"""
    m, n = shape
    order = np.argsort(indices, kind="stable")
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n))])
    return t_ptr, row_of_entry(indptr)[order], data[order], (n, m)


_rtols = None


def pcg_rtol(k):
    """the tolerance of outer iteration k: the reference's float32 ``torch.logspace(-6, -10, 10000)[k]`` (1e-10 from k = 10000 on),
    a float32 value compared against a float64 norm"""
    global _rtols
    if _rtols is None:
        _rtols = torch.logspace(-6, -10, 10000).double().numpy()
    return 1e-10 if k >= 10000 else float(_rtols[k])
