// Device-side declarations shared by the row kernels of the two-kernel ADMM iteration (dpx_iter.hip: the streaming and the lock-step
// kernel; dpx_iter_par.hip: the row-parallel kernel of launches with few planes).  Not part of the C ABI.
#pragma once
#include "dpx_dispatch.h"
#include "dpx_fft_reg.h"
#include "dpx_prox_dev.h"

namespace dpx {

struct IterTerm {
  int linop, prox;
  float alpha;
  const float* lam;
  const float* u_in;
  float* u_out;
  float* v_out;
};
struct IterTerms {
  IterTerm t[DPX_MAX_TERMS];
  int n;
  float dual;          // 1: ADMM.  0: half-quadratic splitting (DPX_TERM_NO_DUAL) -- the incoming duals count as zero and the right-hand side
                       // sees v_i alone; applied as fma(dual, u, K x) / fma(-dual, u', v): the same instructions, and exact for dual = 1
  int emit_bf16;       // x_out / v_out / rhs_out are bf16 planes (the bf16 history of the unrolled forward pass) instead of fp32
  int vxu;             // 1: ADMM in the order v, x, u (DPX_TERM_VXU, algo/admm.py:103-120) -- the stream in `u` carries q = u' - v (u' = -u):
                       // t = q + x, d = K x + t, v = prox(d), q' = t - v goes out, the next right-hand side sees v - t
  int u_live;          // 0: the incoming duals are all zero (DPX_TERM_U_ZERO, first iteration after ADMM.initialize) -- the streaming kernel then
                       // fetches every u row from row 0 of plane 0 (cache hits) instead of streaming the planes from HBM, the lock-step
                       // kernel does not load them at all
  float* rhs_out;      // nullable: the next x-update's right-hand-side increment rho' sum K_i^T (v_i - u_i) as an image (the unrolled
                       // forward pass keeps it for the backward pass); like x_out / v_out an emit store, never counted in the waits
};

// Soft threshold of V pixel pairs, v = sign(d) max(|d| - lam, 0) (proxfn/norm.py), as  d - median(d, -lam, lam): one v_med3_f32 per
// value and a packed subtraction per pair instead of the compare / select form's six vector instructions per value -- the same
// values (d - lam and d + lam are the same single roundings as |d| - lam with the sign put back; inside the band d - d = 0).  The
// median form needs lam >= 0: a wave that holds a negative threshold anywhere (one vote per term and row) takes the general form.
template <int V> __device__ __forceinline__ void soft_threshold_pairs(const float2 (&d)[V], float2 (&v)[V], float lam) {
  if (__ballot(lam < 0.f) == 0) {
#pragma unroll
    for (int m = 0; m < V; ++m) {
#ifdef DPX_EMULATED
      const float cx = fminf(fmaxf(d[m].x, -lam), lam), cy = fminf(fmaxf(d[m].y, -lam), lam);
#else
      const float cx = __builtin_amdgcn_fmed3f(d[m].x, -lam, lam), cy = __builtin_amdgcn_fmed3f(d[m].y, -lam, lam);
#endif
      v[m] = make_float2(d[m].x - cx, d[m].y - cy);
    }
  } else {
#pragma unroll
    for (int m = 0; m < V; ++m) v[m] = make_float2(prox_eval(DPX_PROX_NORM1, d[m].x, lam), prox_eval(DPX_PROX_NORM1, d[m].y, lam));
  }
}

// The instantiation of the streaming (k_iter_rows_seq) and of the row-parallel (k_iter_rows_par) kernel that serves a pass, and the
// emit_v it is handed: ONE rule for both, which is what keeps the row-parallel kernel bit-identical to the streaming one.
struct IterVariant {
  bool dual, vxu;
  int emit_v;
};
static inline IterVariant iter_variant(const IterTerms& TT, int emit_v, const float* x_out, const float* rho_next) {
  // emit_v == 2 (x only: the last pass of a solve() that returns x alone) runs on the no-dual instantiation whatever the solver
  if (emit_v == 2 && x_out && !rho_next) return {false, false, 2};
  if (TT.vxu) return {true, true, emit_v ? 1 : 0};
  // (half-quadratic splitting on the general kernel would be bit-identical at 36 instead of 20 B per pixel)
  return {TT.dual != 0.f, false, emit_v ? 1 : 0};
}
// f(DUAL tag, VXU tag) for the three forms that exist (VXU is a DUAL form)
template <class F> static inline void dispatch_iter_variant(const IterVariant& v, F&& f) {
  if (!v.dual) f(std::false_type{}, std::false_type{});
  else if (v.vxu) f(std::true_type{}, std::true_type{});
  else f(std::true_type{}, std::false_type{});
}

// Cache policy of the row kernels' four streams (dpx_common.h): spectrum in / u in (loads, 1 = nt), u out / spectrum out
// (stores, 2 = nt); see the comment in front of k_iter_rows_seq (dpx_iter.hip).
constexpr int R_LDX = 0, R_LDU = 1, R_STU = 2;
constexpr int R_STX = 1;  // the spectrum handed to the next kernel: write-through (`sc1`), nothing left dirty at the kernel boundary (+0.5 ... 1 %)

}  // namespace dpx
