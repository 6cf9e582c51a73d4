// The LP solver (the reference's dprox/algo/lp/solvers.py: LPSolverADMM.solve with its warm-started, Jacobi-preconditioned PCG of
// dprox/linalg/solve/solver_cg.py:172-233 as the x-update): float64, the constraint matrix sparse, the inner loop controlled on
// the device.
//
// The matrix Abar (m x n, m = m_ub + m_eq + n) is stored twice, as CSR of Abar and CSR of its transpose, so every product is a
// gather and none a scatter.  The unit is a CSR row product: a group of L lanes (a power of two, 1 .. 64, chosen on the host from
// the mean row length; knob lp_lanes) walks a row in steps of L and sums with the xor butterfly, so a wave handles 64 / L rows and
// a 256-thread workgroup 256 / L.  Every kernel adds its prologue and epilogue to that unit:
//
//   k_lp_spmv_a      t = Abar v  (m rows).  FOLD: v = p_new = -y + beta p_old is formed on the fly from the two gathered vectors,
//                    and the groups of the rows below n also write p_new into the other slot of the double-buffered p
//   k_lp_pcg_start   (n rows of Abar^T) one pass gathers rho z - y and rho t (t = Abar xt): right = sigma x - c + Abar^T(rho z - y),
//                    r = Abar^T(rho t) + sigma xt - right, y = r / M, p = -y, partials of <r, y>; the last workgroup writes ry,
//                    rtol, done = 0, inner = 0
//   k_lp_pcg_at      (n rows of Abar^T) Ap = Abar^T(rho t) + sigma p, partials of <p, Ap>; the last workgroup writes a = ry / <p, Ap>
//   k_lp_pcg_update  (n elements) xt += a p, r += a Ap, y = r / M with M = sigma + rho Acnorm^2, partials of <r, y> and max|r|; the
//                    last workgroup writes beta, the new ry, the inner count and done = max|r| < rtol (or the count at its cap)
//   k_lp_pcg_dir     (n elements) p_new = -y + beta p_old: the direction update as a launch of its own (knob lp_split_direction)
//   k_lp_tail        (m rows) zt = Abar xt (kept in t for the next start), the relaxation, the clip and the dual update of that
//                    row; the groups of the rows below n also relax x
//   k_lp_eval_a      (m rows) Abar x: |(Abar x - z) / e / gamma_b|, |Abar x / e / gamma_b|, |z / e / gamma_b|, |z - clip(z)| (max)
//   k_lp_eval_at     (n rows) Abar^T y: |(c + Abar^T y) / d / gamma_c|, |Abar^T y / d / gamma_c|, |c / d / gamma_c| (max) and the
//                    objective <c / d / gamma_c, x d / gamma_b>
//
// p of inner iteration i lives in slot i & 1 of the double-buffered p.  Once `done` is set, the PCG kernels return at once: the
// iterate stays as it was at the reference's exit, however many iterations the host has issued ahead.
// Reductions are two-stage (dpx_reduce_dev.h): write-through partials, an integer ticket, the last workgroup adds (or maximises)
// them in a fixed order -- no floating-point atomics, no workgroup waits for another, two runs give the same bits.
#include "dpx_reduce_dev.h"

namespace dpx {
namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_BLOCKS = 1024;         // workgroups per launch (rows beyond them: a grid-stride loop); partials per quantity
constexpr int LP_PARTIALS = 4;              // quantities a kernel reduces at most

// the state block: the PCG scalars, the evaluation's outputs, then the control words
struct LpState {
  double ry, a, beta, rtol, pAp, rmax;
  double eval[8];                           // objval, r_norm, s_norm, |Ax|, |z|, |ATy|, |c|, |z - clip(z)|
  long long done, inner, ops;
};

// the pointer table of the C ABI (include/dpx.h, DPX_LP_*), typed
struct LpTab {
  const int *a_ptr, *a_idx;
  const double* a_val;
  const int *at_ptr, *at_idx;
  const double* at_val;
  double *x, *xt, *z, *y, *t;
  const double *c, *acn;
  double *right, *r, *yv, *p, *Ap;
  const double *lb, *ub, *d, *e;
  LpState* st;
  void* ws;
};
LpTab lp_tab(const void* const* tab) {
  LpTab T;
  T.a_ptr = (const int*)tab[DPX_LP_A_PTR], T.a_idx = (const int*)tab[DPX_LP_A_IDX], T.a_val = (const double*)tab[DPX_LP_A_VAL];
  T.at_ptr = (const int*)tab[DPX_LP_AT_PTR], T.at_idx = (const int*)tab[DPX_LP_AT_IDX], T.at_val = (const double*)tab[DPX_LP_AT_VAL];
  T.x = (double*)tab[DPX_LP_X], T.xt = (double*)tab[DPX_LP_XT], T.z = (double*)tab[DPX_LP_Z], T.y = (double*)tab[DPX_LP_Y];
  T.t = (double*)tab[DPX_LP_T], T.c = (const double*)tab[DPX_LP_C], T.acn = (const double*)tab[DPX_LP_ACN];
  T.right = (double*)tab[DPX_LP_RIGHT], T.r = (double*)tab[DPX_LP_R], T.yv = (double*)tab[DPX_LP_YV], T.p = (double*)tab[DPX_LP_P];
  T.Ap = (double*)tab[DPX_LP_AP], T.lb = (const double*)tab[DPX_LP_LB], T.ub = (const double*)tab[DPX_LP_UB];
  T.d = (const double*)tab[DPX_LP_D], T.e = (const double*)tab[DPX_LP_E], T.st = (LpState*)tab[DPX_LP_STATE], T.ws = (void*)tab[DPX_LP_WS];
  return T;
}

// ---- the unit --------------------------------------------------------------------------------------------------------------------
// The rows a workgroup visits: base, base + gridDim.x RPB, ... with RPB = LP_THREADS / L rows per workgroup; the trip count is the
// same for every thread of the workgroup (the butterflies and the reductions behind it need all lanes).
struct LpRows {
  int L, sub;
  long rpb, row0, step;
  __device__ __forceinline__ LpRows(int L_) : L(L_) {
    sub = threadIdx.x & (L - 1);
    rpb = LP_THREADS / L;
    row0 = (long)blockIdx.x * rpb;
    step = (long)gridDim.x * rpb;
  }
  __device__ __forceinline__ long row(long base) const { return base + threadIdx.x / L; }
};
// the sum over a group of L lanes; the result is in every lane of the group
__device__ __forceinline__ double group_sum(double v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// the direction update, written once: both of its forms (folded into k_lp_spmv_a, k_lp_pcg_dir) give the same bits
__device__ __forceinline__ double lp_dir(double beta, double p_old, double y) { return fma(beta, p_old, -y); }

// the maximum of n partials (all >= 0), lane-strided, then the butterfly; the result is in every lane
__device__ __forceinline__ double max_partials(const double* p, int n) {
  double s = 0.0;
  for (int i = threadIdx.x & 63; i < n; i += 64) s = p[i] > s ? p[i] : s;
  return wave_max(s);
}
__device__ __forceinline__ double* lp_partials(void* ws, int q) { return (double*)((char*)ws + 256) + (long)q * LP_MAX_BLOCKS; }

// ---- t = A v -----------------------------------------------------------------------------------------------------------------------
// st == nullptr: the plain product.  Otherwise the product of inner iteration i = st->inner (nothing once st->done): v is slot
// i & 1 of p; FOLD and i > 0: that slot is first formed here, from the other slot and y.
template <bool FOLD>
__global__ void __launch_bounds__(LP_THREADS) k_lp_spmv_a(double* __restrict__ out, const int* __restrict__ ptr, const int* __restrict__ idx,
                                                         const double* __restrict__ val, const double* v, double* p, const double* __restrict__ yv,
                                                         const LpState* st, long rows, long n, int L) {
  bool fold = false;
  double beta = 0.0;
  const double* pold = nullptr;
  double* pnew = nullptr;
  if (st) {
    if (st->done) return;
    const long i = (long)st->inner;
    v = p + (i & 1) * n;
    if (FOLD && i > 0) fold = true, beta = st->beta, pold = p + ((i + 1) & 1) * n, pnew = p + (i & 1) * n;
  }
  const LpRows w(L);
  for (long base = w.row0; base < rows; base += w.step) {
    const long row = w.row(base);
    double acc = 0.0;
    if (row < rows) {
      const int k1 = ptr[row + 1];
      if (FOLD && fold) {
        for (int k = ptr[row] + w.sub; k < k1; k += L) {
          const int j = idx[k];
          acc += val[k] * lp_dir(beta, pold[j], yv[j]);
        }
        if (row < n && w.sub == 0) pnew[row] = lp_dir(beta, pold[row], yv[row]);
      } else {
        for (int k = ptr[row] + w.sub; k < k1; k += L) acc += val[k] * v[idx[k]];
      }
    }
    acc = group_sum(acc, L);
    if (row < rows && w.sub == 0) out[row] = acc;
  }
}

// ---- the PCG start -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LP_THREADS) k_lp_pcg_start(LpTab T, long n, double rho, double sigma, double rtol, int L) {
  __shared__ double sh[LP_THREADS / 64];
  __shared__ int last;
  const LpRows w(L);
  double dot = 0.0;
  for (long base = w.row0; base < n; base += w.step) {
    const long row = w.row(base);
    double g1 = 0.0, g2 = 0.0;
    if (row < n) {
      const int k1 = T.at_ptr[row + 1];
      for (int k = T.at_ptr[row] + w.sub; k < k1; k += L) {
        const int i = T.at_idx[k];
        const double a = T.at_val[k];
        g1 += a * (rho * T.z[i] - T.y[i]);
        g2 += a * (rho * T.t[i]);
      }
    }
    g1 = group_sum(g1, L);
    g2 = group_sum(g2, L);
    if (row < n && w.sub == 0) {
      const double right = sigma * T.x[row] - T.c[row] + g1;
      const double r = g2 + sigma * T.xt[row] - right;
      const double acn = T.acn[row];
      const double y = r / (sigma + rho * (acn * acn));
      T.right[row] = right;
      T.r[row] = r;
      T.yv[row] = y;
      T.p[row] = -y;                           // slot 0: inner iteration 0
      dot += r * y;
    }
  }
  const double s = block_sum(dot, sh);
  double* part = lp_partials(T.ws, 0);
  if (threadIdx.x == 0) dpx_st_agent(part + blockIdx.x, s);
  if (!dpx_last_block((unsigned*)T.ws, gridDim.x, &last)) return;
  if (threadIdx.x < 64) {
    const double ry = sum_partials_f64(part, (int)gridDim.x);
    if (threadIdx.x == 0) {
      T.st->ry = ry;
      T.st->rtol = rtol;
      T.st->done = 0;
      T.st->inner = 0;
      T.st->ops += 1;
    }
  }
}

// ---- Ap = A^T(rho t) + sigma p, a = ry / <p, Ap> ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(LP_THREADS) k_lp_pcg_at(LpTab T, long n, double rho, double sigma, int L) {
  __shared__ double sh[LP_THREADS / 64];
  __shared__ int last;
  if (T.st->done) return;
  const double ry = T.st->ry;
  const double* p = T.p + ((long)T.st->inner & 1) * n;
  const LpRows w(L);
  double dot = 0.0;
  for (long base = w.row0; base < n; base += w.step) {
    const long row = w.row(base);
    double g = 0.0;
    if (row < n) {
      const int k1 = T.at_ptr[row + 1];
      for (int k = T.at_ptr[row] + w.sub; k < k1; k += L) g += T.at_val[k] * (rho * T.t[T.at_idx[k]]);
    }
    g = group_sum(g, L);
    if (row < n && w.sub == 0) {
      const double pv = p[row], ap = g + sigma * pv;
      T.Ap[row] = ap;
      dot += pv * ap;
    }
  }
  const double s = block_sum(dot, sh);
  double* part = lp_partials(T.ws, 0);
  if (threadIdx.x == 0) dpx_st_agent(part + blockIdx.x, s);
  if (!dpx_last_block((unsigned*)T.ws, gridDim.x, &last)) return;
  if (threadIdx.x < 64) {
    const double pAp = sum_partials_f64(part, (int)gridDim.x);
    if (threadIdx.x == 0) {
      T.st->pAp = pAp;
      T.st->a = ry / pAp;
      T.st->ops += 1;
    }
  }
}

// ---- xt += a p, r += a Ap, y = r / M; beta, ry, the count and the stop test ----------------------------------------------------------
__global__ void __launch_bounds__(LP_THREADS) k_lp_pcg_update(LpTab T, long n, double rho, double sigma, long max_inner) {
  __shared__ double sh[LP_THREADS / 64];
  __shared__ int last;
  if (T.st->done) return;
  const double a = T.st->a, ry_old = T.st->ry, rtol = T.st->rtol;
  const long inner = (long)T.st->inner;
  const double* p = T.p + (inner & 1) * n;
  double dot = 0.0, mx = 0.0;
  for (long i = (long)blockIdx.x * LP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * LP_THREADS) {
    T.xt[i] += a * p[i];
    const double r = T.r[i] + a * T.Ap[i];
    const double acn = T.acn[i];
    const double y = r / (sigma + rho * (acn * acn));
    T.r[i] = r;
    T.yv[i] = y;
    dot += r * y;
    mx = fmax(mx, fabs(r));
  }
  const double s = block_sum(dot, sh);
  const double m = block_sum<double, true>(mx, sh);
  double *part = lp_partials(T.ws, 0), *pmax = lp_partials(T.ws, 1);
  if (threadIdx.x == 0) {
    dpx_st_agent(part + blockIdx.x, s);
    dpx_st_agent(pmax + blockIdx.x, m);
  }
  if (!dpx_last_block((unsigned*)T.ws, gridDim.x, &last)) return;
  if (threadIdx.x < 64) {
    const double ry = sum_partials_f64(part, (int)gridDim.x);
    double rmax = max_partials(pmax, (int)gridDim.x);
    // the maxima drop a NaN, the sum keeps it: a residual with a NaN gives ry = NaN, and then rmax is NaN as the reference's max|r|
    // is, so the test below is false and the loop runs to its cap as the reference's does
    if (ry != ry) rmax = ry;
    if (threadIdx.x == 0) {
      T.st->beta = ry / ry_old;
      T.st->ry = ry;
      T.st->rmax = rmax;
      T.st->inner = inner + 1;
      T.st->done = (rmax < rtol || inner + 1 >= max_inner) ? 1 : 0;
    }
  }
}

// ---- p = -y + beta p as a launch of its own: slot inner & 1 from the other one (inner is already the next iteration's) ---------------
__global__ void __launch_bounds__(LP_THREADS) k_lp_pcg_dir(LpTab T, long n) {
  if (T.st->done) return;
  const long inner = (long)T.st->inner;
  const double beta = T.st->beta;
  const double* pold = T.p + ((inner + 1) & 1) * n;
  double* pnew = T.p + (inner & 1) * n;
  for (long i = (long)blockIdx.x * LP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * LP_THREADS) pnew[i] = lp_dir(beta, pold[i], T.yv[i]);
}

// ---- the rest of an outer iteration -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LP_THREADS) k_lp_tail(LpTab T, long m, long n, double alpha, double rho, double inv_rho, int L) {
  const LpRows w(L);
  for (long base = w.row0; base < m; base += w.step) {
    const long row = w.row(base);
    double acc = 0.0;
    if (row < m) {
      const int k1 = T.a_ptr[row + 1];
      for (int k = T.a_ptr[row] + w.sub; k < k1; k += L) acc += T.a_val[k] * T.xt[T.a_idx[k]];
    }
    acc = group_sum(acc, L);
    if (row < m && w.sub == 0) {
      T.t[row] = acc;                                         // A xt: the next start's
      const double zold = T.z[row], y = T.y[row];
      const double zt = alpha * acc + (1.0 - alpha) * zold;
      const double znew = fmin(fmax(zt + inv_rho * y, T.lb[row]), T.ub[row]);
      T.z[row] = znew;
      T.y[row] = y + rho * (zt - znew);
    }
    // x is gathered by no row of this launch (xt is): the group of row < n relaxes it
    if (row < n && w.sub == 0) T.x[row] = alpha * T.xt[row] + (1.0 - alpha) * T.x[row];
  }
}

__global__ void __launch_bounds__(LP_THREADS) k_lp_eval_a(LpTab T, long m, double gamma_b, int L) {
  __shared__ double sh[LP_THREADS / 64];
  __shared__ int last;
  const LpRows w(L);
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  for (long base = w.row0; base < m; base += w.step) {
    const long row = w.row(base);
    double acc = 0.0;
    if (row < m) {
      const int k1 = T.a_ptr[row + 1];
      for (int k = T.a_ptr[row] + w.sub; k < k1; k += L) acc += T.a_val[k] * T.x[T.a_idx[k]];
    }
    acc = group_sum(acc, L);
    if (row < m && w.sub == 0) {
      const double z = T.z[row], e = T.e[row];
      q[0] = fmax(q[0], fabs((acc - z) / e / gamma_b));
      q[1] = fmax(q[1], fabs(acc / e / gamma_b));
      q[2] = fmax(q[2], fabs(z / e / gamma_b));
      q[3] = fmax(q[3], fabs(z - fmin(fmax(z, T.lb[row]), T.ub[row])));
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double v = block_sum<double, true>(q[j], sh);
    if (threadIdx.x == 0) dpx_st_agent(lp_partials(T.ws, j) + blockIdx.x, v);
  }
  if (!dpx_last_block((unsigned*)T.ws, gridDim.x, &last)) return;
  if (threadIdx.x < 64) {
    const int slot[4] = {1, 3, 4, 7};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double v = max_partials(lp_partials(T.ws, j), (int)gridDim.x);
      if (threadIdx.x == 0) T.st->eval[slot[j]] = v;
    }
  }
}

__global__ void __launch_bounds__(LP_THREADS) k_lp_eval_at(LpTab T, long n, double gamma_c, double gamma_b, int L) {
  __shared__ double sh[LP_THREADS / 64];
  __shared__ int last;
  const LpRows w(L);
  double q[3] = {0.0, 0.0, 0.0}, obj = 0.0;
  for (long base = w.row0; base < n; base += w.step) {
    const long row = w.row(base);
    double acc = 0.0;
    if (row < n) {
      const int k1 = T.at_ptr[row + 1];
      for (int k = T.at_ptr[row] + w.sub; k < k1; k += L) acc += T.at_val[k] * T.y[T.at_idx[k]];
    }
    acc = group_sum(acc, L);
    if (row < n && w.sub == 0) {
      const double c = T.c[row], d = T.d[row];
      const double cs = c / d / gamma_c;
      q[0] = fmax(q[0], fabs((c + acc) / d / gamma_c));
      q[1] = fmax(q[1], fabs(acc / d / gamma_c));
      q[2] = fmax(q[2], fabs(cs));
      obj += cs * (T.x[row] * d / gamma_b);
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double v = block_sum<double, true>(q[j], sh);
    if (threadIdx.x == 0) dpx_st_agent(lp_partials(T.ws, j) + blockIdx.x, v);
  }
  const double s = block_sum(obj, sh);
  if (threadIdx.x == 0) dpx_st_agent(lp_partials(T.ws, 3) + blockIdx.x, s);
  if (!dpx_last_block((unsigned*)T.ws, gridDim.x, &last)) return;
  if (threadIdx.x < 64) {
    const int slot[3] = {2, 5, 6};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = max_partials(lp_partials(T.ws, j), (int)gridDim.x);
      if (threadIdx.x == 0) T.st->eval[slot[j]] = v;
    }
    const double o = sum_partials_f64(lp_partials(T.ws, 3), (int)gridDim.x);
    if (threadIdx.x == 0) T.st->eval[0] = o;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// lanes per row: the smallest power of two that covers the mean row length, 1 .. 64 (knob lp_lanes: a power of two forces it)
int lp_lanes(long rows, long nnz) {
  const int knob = tune(TUNE_LP_LANES);
  if (knob >= 1 && knob <= 64 && (knob & (knob - 1)) == 0) return knob;
  const long mean = rows > 0 ? (nnz + rows - 1) / rows : 1;
  int L = 1;
  while (L < 64 && L < mean) L <<= 1;
  return L;
}
int lp_row_blocks(long rows, int L) {
  const long nb = (rows * L + LP_THREADS - 1) / LP_THREADS;
  return (int)(nb < 1 ? 1 : nb > LP_MAX_BLOCKS ? LP_MAX_BLOCKS : nb);
}
// nnz stops 64 short of 2^31 - 1: the row loops step an int offset by L <= 64 past the row's end before they test it
constexpr long LP_MAX_NNZ = 2147483647L - 64;
bool lp_shape_ok(const char* who, long m, long n, long nnz) {
  if (m >= 1 && n >= 1 && nnz >= 1 && nnz <= LP_MAX_NNZ && m < 2147483647L && n < 2147483647L) return true;
  set_error("%s: bad shape m=%ld n=%ld nnz=%ld (m, n 1 .. 2^31 - 2, nnz 1 .. 2^31 - 65)", who, m, n, nnz);
  return false;
}
// the solver's matrix ends with the identity block: the rows below n of A are there to relax x and to write the folded direction
bool lp_solver_shape_ok(const char* who, long m, long n, long nnz) {
  if (!lp_shape_ok(who, m, n, nnz)) return false;
  if (m >= n) return true;
  set_error("%s: m %ld < n %ld (the matrix ends with the identity block)", who, m, n);
  return false;
}
bool lp_tab_ok(const char* who, const void* const* tab) {
  if (tab)
    for (int i = 0; i < DPX_LP_TAB_COUNT; ++i)
      if (!tab[i]) tab = nullptr;
  if (tab) return true;
  set_error("%s: null pointer in the table", who);
  return false;
}

}  // namespace
}  // namespace dpx

extern "C" size_t dpx_lp_state_bytes(void) { return sizeof(dpx::LpState); }

extern "C" size_t dpx_lp_ws_bytes(long m, long n) {
  if (m < 1 || n < 1) return 0;
  return 256 + (size_t)dpx::LP_PARTIALS * dpx::LP_MAX_BLOCKS * sizeof(double);
}

extern "C" int dpx_lp_lanes(long rows, long nnz) { return dpx::lp_lanes(rows, nnz); }

extern "C" int dpx_lp_spmv_chain(void* out, const int* indptr, const int* indices, const void* data, const void* v, long rows, long nnz, int reps,
                                 dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(out && indptr && indices && data && v && reps >= 1, "dpx_lp_spmv: null pointer or reps %d < 1", reps);
  if (!lp_shape_ok("dpx_lp_spmv", rows, 1, nnz)) return DPX_ERR_ARG;
  const int L = lp_lanes(rows, nnz);
  for (int i = 0; i < reps; ++i)
    DPX_LAUNCH("k_lp_spmv_a", (k_lp_spmv_a<false>), dim3(lp_row_blocks(rows, L)), dim3(LP_THREADS), 0, (hipStream_t)stream, (double*)out, indptr, indices,
               (const double*)data, (const double*)v, (double*)nullptr, (const double*)nullptr, (const LpState*)nullptr, rows, 0L, L);
  return launch_status("dpx_lp_spmv");
}

extern "C" int dpx_lp_spmv(void* out, const int* indptr, const int* indices, const void* data, const void* v, long rows, long nnz, dpx_stream_t stream) {
  return dpx_lp_spmv_chain(out, indptr, indices, data, v, rows, nnz, 1, stream);
}

extern "C" int dpx_lp_pcg_start(const void* const* tab, long m, long n, long nnz, double rho, double sigma, double rtol, dpx_stream_t stream) {
  using namespace dpx;
  if (!lp_tab_ok("dpx_lp_pcg_start", tab) || !lp_solver_shape_ok("dpx_lp_pcg_start", m, n, nnz)) return DPX_ERR_ARG;
  const LpTab T = lp_tab(tab);
  const int L = lp_lanes(n, nnz);
  DPX_LAUNCH("k_lp_pcg_start", k_lp_pcg_start, dim3(lp_row_blocks(n, L)), dim3(LP_THREADS), 0, (hipStream_t)stream, T, n, rho, sigma, rtol, L);
  return launch_status("dpx_lp_pcg_start");
}

extern "C" int dpx_lp_pcg_iters(const void* const* tab, long m, long n, long nnz, double rho, double sigma, long max_inner, int iters,
                                dpx_stream_t stream) {
  using namespace dpx;
  if (!lp_tab_ok("dpx_lp_pcg_iters", tab) || !lp_solver_shape_ok("dpx_lp_pcg_iters", m, n, nnz)) return DPX_ERR_ARG;
  DPX_REQUIRE(iters >= 0 && max_inner >= 1, "dpx_lp_pcg_iters: iters %d, max_inner %ld", iters, max_inner);
  const LpTab T = lp_tab(tab);
  const hipStream_t s = (hipStream_t)stream;
  const int LA = lp_lanes(m, nnz), LT = lp_lanes(n, nnz);
  const bool split = tune(TUNE_LP_SPLIT_DIRECTION) != 0;
  const dim3 ga(lp_row_blocks(m, LA)), gt(lp_row_blocks(n, LT)), ge(lp_row_blocks(n, 1)), blk(LP_THREADS);
  for (int it = 0; it < iters; ++it) {
    if (split)
      DPX_LAUNCH("k_lp_spmv_a", (k_lp_spmv_a<false>), ga, blk, 0, s, T.t, T.a_ptr, T.a_idx, T.a_val, (const double*)nullptr, T.p, (const double*)T.yv,
                 (const LpState*)T.st, m, n, LA);
    else
      DPX_LAUNCH("k_lp_spmv_a", (k_lp_spmv_a<true>), ga, blk, 0, s, T.t, T.a_ptr, T.a_idx, T.a_val, (const double*)nullptr, T.p, (const double*)T.yv,
                 (const LpState*)T.st, m, n, LA);
    DPX_LAUNCH("k_lp_pcg_at", k_lp_pcg_at, gt, blk, 0, s, T, n, rho, sigma, LT);
    DPX_LAUNCH("k_lp_pcg_update", k_lp_pcg_update, ge, blk, 0, s, T, n, rho, sigma, max_inner);
    if (split) DPX_LAUNCH("k_lp_pcg_dir", k_lp_pcg_dir, ge, blk, 0, s, T, n);
  }
  return launch_status("dpx_lp_pcg_iters");
}

extern "C" int dpx_lp_tail(const void* const* tab, long m, long n, long nnz, double alpha, double rho, dpx_stream_t stream) {
  using namespace dpx;
  if (!lp_tab_ok("dpx_lp_tail", tab) || !lp_solver_shape_ok("dpx_lp_tail", m, n, nnz)) return DPX_ERR_ARG;
  const LpTab T = lp_tab(tab);
  const int L = lp_lanes(m, nnz);
  DPX_LAUNCH("k_lp_tail", k_lp_tail, dim3(lp_row_blocks(m, L)), dim3(LP_THREADS), 0, (hipStream_t)stream, T, m, n, alpha, rho, 1.0 / rho, L);
  return launch_status("dpx_lp_tail");
}

extern "C" int dpx_lp_eval(const void* const* tab, long m, long n, long nnz, double gamma_c, double gamma_b, dpx_stream_t stream) {
  using namespace dpx;
  if (!lp_tab_ok("dpx_lp_eval", tab) || !lp_solver_shape_ok("dpx_lp_eval", m, n, nnz)) return DPX_ERR_ARG;
  const LpTab T = lp_tab(tab);
  const int LA = lp_lanes(m, nnz), LT = lp_lanes(n, nnz);
  DPX_LAUNCH("k_lp_eval_a", k_lp_eval_a, dim3(lp_row_blocks(m, LA)), dim3(LP_THREADS), 0, (hipStream_t)stream, T, m, gamma_b, LA);
  DPX_LAUNCH("k_lp_eval_at", k_lp_eval_at, dim3(lp_row_blocks(n, LT)), dim3(LP_THREADS), 0, (hipStream_t)stream, T, n, gamma_c, gamma_b, LT);
  return launch_status("dpx_lp_eval");
}
