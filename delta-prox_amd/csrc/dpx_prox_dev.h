// The pieces the image-domain ("staged") ADMM passes are written on, each defined once so that every path rounds alike: the closed-form
// proximal operators (also the row kernels' and the PGD row pass's), the prox Jacobian recovered from the saved output, a group of
// VEC pixels of a row with its circular neighbours, the three linops K / K^T on such a group, and the host rule that picks VEC.
// Used by dpx_elementwise.hip (forward passes), dpx_autodiff.hip (backward passes), dpx_split.hip, dpx_conv_bf16.hip (head pass of
// dpx_admm_cg_pnp_iter), dpx_fft_pow2.hip (PGD row pass) and, through dpx_iter_dev.h, the row kernels; dpx_fft.hip takes TermPack.
// Not part of the C ABI.
#pragma once
#include "dpx_reduce_dev.h"

namespace dpx {

// soft threshold / nonneg / v / (1 + 2 lam)          dprox/proxfn/norm.py:6-27, nonneg.py:10-11, sum_square.py:26-27
// Closed forms only: the caller has checked `kind` (any other value would evaluate as the last form).
__device__ __forceinline__ float prox_eval(int kind, float d, float lam) {
  if (kind == DPX_PROX_NORM1) {                              // sign(d) * max(|d| - lam, 0)
    const float m = fmaxf(fabsf(d) - lam, 0.f);
    return d > 0.f ? m : (d < 0.f ? -m : 0.f * m);
  }
  if (kind == DPX_PROX_NONNEG) return fmaxf(d, 0.f);
  return d / (1.f + 2.f * lam);
}

// J = dprox/dd and dl = dprox/dlam recovered from the saved OUTPUT v = prox(d, lam): soft-threshold passes where v != 0, nonneg where v > 0
__device__ __forceinline__ void prox_jac(int kind, float v, float lam, float& J, float& dl) {
  if (kind == DPX_PROX_NORM1) {
    J = v != 0.f ? 1.f : 0.f;
    dl = v > 0.f ? -1.f : (v < 0.f ? 1.f : 0.f);
  } else if (kind == DPX_PROX_NONNEG) {
    J = v > 0.f ? 1.f : 0.f;
    dl = 0.f;
  } else {
    const float s = 1.f / (1.f + 2.f * lam);
    J = s;
    dl = -2.f * v * s;                                       // d = v (1 + 2 lam):  -2 d s^2 = -2 v s
  }
}

struct TermPack {
  dpx_term t[DPX_MAX_TERMS];
  int n;
};

// VEC (1 or 4) consecutive pixels of one row of a [B][C][H][W] batch (W % VEC == 0): group number i counts groups over the whole batch.
// Offsets are in pixels from the batch's first; left / right are single pixels, up / down groups; all four wrap around (circular).
template <int VEC> struct PixGroup {
  int b;                 // image
  long off;              // the group's first pixel
  long left, right;      // the pixel left of the first / right of the last one
  long up, down;         // the group one row up / down
  __device__ __forceinline__ PixGroup(long i, int C, int H, int W) {
    const int Wv = W / VEC, wv = (int)(i % Wv);
    const long row = i / Wv;                                 // (b * C + c) * H + h
    const int h = (int)(row % H);
    b = (int)(row / H / C);
    off = row * W + (long)wv * VEC;
    left = row * W + (wv == 0 ? W - 1 : wv * VEC - 1);
    right = row * W + (wv + 1 == Wv ? 0 : (wv + 1) * VEC);
    up = off + (long)((h == 0 ? H - 1 : h - 1) - h) * W;
    down = off + (long)((h + 1 == H ? 0 : h + 1) - h) * W;
  }
  using V = Vec<float, VEC>;
  __device__ __forceinline__ static V ld(const float* p, long at) { return V::ld(p + at, 0); }
  __device__ __forceinline__ static V ld0(const float* p, long at) { return p ? ld(p, at) : V{}; }          // a null plane reads as zeros
  __device__ __forceinline__ static void st(float* p, long at, const V& v) { v.st(p + at, 0); }
  // a history plane (fp32, or bf16 slots)
  __device__ __forceinline__ static V hist(const float* p, int bf16, long at) {
    if constexpr (VEC == 4) {
      const float4 t = dpx_hist_load4(p, bf16, at);
      return V{{t.x, t.y, t.z, t.w}};
    } else {
      return V{{dpx_hist_load(p, bf16, at)}};
    }
  }
};

// (K x)[e] at pixel e of a group: identity, or the circular forward difference along W (x[w + 1] - x[w]) / H (x[h + 1] - x[h]).
// c: x on the group; right: x at the group's right neighbour; down: x on the group below (each read only by the linop that needs it)
template <int VEC> __device__ __forceinline__ float lin_K(int linop, int e, const float (&c)[VEC], float right, const float (&down)[VEC]) {
  if (linop == DPX_LIN_IDENTITY) return c[e];
  if (linop == DPX_LIN_GRAD_W) return (e + 1 < VEC ? c[(e + 1) % VEC] : right) - c[e];
  return down[e] - c[e];
}
// acc += K^T y on a group (adjoints: y[w - 1] - y[w], y[h - 1] - y[h]).  left() gives y at the group's left neighbour, up(u) fills y on the
// group above: callables, run only by the linop that needs them (the fused passes recompute those values)
template <int VEC, class L, class U>
__device__ __forceinline__ void lin_KT_add(int linop, const float (&y)[VEC], float (&acc)[VEC], L&& left, U&& up) {
  if (linop == DPX_LIN_IDENTITY) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += y[e];
  } else if (linop == DPX_LIN_GRAD_W) {
    acc[0] += left() - y[0];
#pragma unroll
    for (int e = 1; e < VEC; ++e) acc[e] += y[e - 1] - y[e];
  } else {
    float u[VEC];
    up(u);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += u[e] - y[e];
  }
}

// ---- host side: the one launch rule of the staged passes ------------------------------------------------------------------------
// 4 pixels per thread where the width allows it and every plane handed in may be accessed 16 bytes at a time (`hist`: history planes, whose
// bf16 form is read 8 bytes at a time); else 1
static inline int staged_vec(int W, std::initializer_list<const void*> planes, std::initializer_list<const void*> hist = {}, int hist_bf16 = 0) {
  if (W % 4 != 0 || !aligned16(planes)) return 1;
  for (const void* p : hist)
    if ((size_t)p % (hist_bf16 ? 8 : 16) != 0) return 1;
  return 4;
}
// ... and the launch of the instantiation it picked
#define DPX_LAUNCH_VEC(vec, name, kernel4, kernel1, ...)   \
  do {                                                     \
    if ((vec) == 4) DPX_LAUNCH(name, kernel4, __VA_ARGS__); \
    else DPX_LAUNCH(name, kernel1, __VA_ARGS__);           \
  } while (0)

}  // namespace dpx
