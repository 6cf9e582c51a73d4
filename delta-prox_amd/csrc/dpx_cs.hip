// compress_sensing: the coded-aperture data term of snapshot compressive imaging (the reference's dprox/proxfn/fast/cs.py:6-27) as the
// closed-form x-update of ADMM, and its gradient.  A v = sum_c m_c v_c folds the C channels of a pixel into one measurement, so
// A^T A + I lam is a rank-one update of a multiple of the identity PER PIXEL and Sherman-Morrison solves it with one channel sum:
//
//   s = sum_c m_c v_c     phi = sum_c m_c^2     d = phi + I lam     r = (I y - s) / d     x_c = (v_c + m_c r) / I
//
// v = the sum of the I = num_psi right-hand sides ADMM hands over (ext_sum_squares.solve), lam = lam[n] per image.  One kernel,
// k_cs_xupdate: a thread owns a pixel (n, h, w) -- four neighbouring ones, 16 bytes per access, where a plane is a multiple of four
// pixels and the buffers are aligned (measured in one process on the 8 x 31 x 512^2 cube: 0.219 against 0.253 ms) -- and walks the
// channel axis, so the lanes of a wave read neighbouring w of one plane -- coalesced, no LDS --, adds the nb <= 4 inputs as it reads
// them, and for C <= 32 keeps the summed v_c and the m_c in registers between the reduction pass and the write pass (KC = 8 / 16 /
// 24 / 32: a compile-time-unrolled walk, predicated by k < C); wider pixels read both again (KC = 0).  Traffic per pixel:
// nb C + C + 1 floats read, C written, nothing image-sized in between.  Both widths give the same bits.
//
// The gradient (k_cs_bwd) recomputes r from the forward's inputs.  With the cotangent g, t = sum_c m_c g_c and q = t / d:
//
//   gv_c = (g_c - m_c q) / I     gy = q     glam[n] = -sum_{h,w} q r     gmask_c = (g_c r - q (v_c + 2 m_c r)) / I
//
// Where the mask (or y) is shared by the N images its gradient is the sum over n: the thread itself loops over the images of its
// pixel and adds in n order; glam adds q r per workgroup in float64 and the last workgroup of an image to arrive adds the
// workgroups' sums in a fixed order (dpx_reduce_dev.h).  No floating-point atomics anywhere: two runs give the same bits.
#include "dpx_common.h"
#include "dpx_reduce_dev.h"

namespace dpx {
namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_MAX_IN = 4;       // right-hand sides one launch adds up
constexpr int CS_KEEP_MAX = 32;    // channels a thread keeps in registers between its two passes

struct CsIn {
  const float* b[CS_MAX_IN];
};

// v = b_0 + b_1 + ... in argument order, for the V pixels of vector i
template <int V> __device__ __forceinline__ Vec<float, V> cs_sum(const CsIn& in, int nb, size_t i) {
  Vec<float, V> v = Vec<float, V>::ld(in.b[0], (long)i);
#pragma unroll
  for (int j = 1; j < CS_MAX_IN; ++j)
    if (j < nb) {
      const Vec<float, V> t = Vec<float, V>::ld(in.b[j], (long)i);
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] += t.v[e];
    }
  return v;
}

// f(k) for the channels k = 0 .. C - 1 of a pixel: unrolled at compile time over KC >= C slots (k is then a constant: what f keeps
// per channel stays in registers), or a plain loop (KC = 0)
template <int KC, class F> __device__ __forceinline__ void cs_channels(int C, F&& f) {
  if constexpr (KC > 0) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k < C) f(k);
  } else {
    for (int k = 0; k < C; ++k) f(k);
  }
}

// ---- the arithmetic of a pixel, written once: every product-sum is one named fma and nothing else is contracted, so that every
// instantiation (and the host emulation) rounds alike -- the four-pixel form gives the one-pixel form's bits
__device__ __forceinline__ float cs_acc(float a, float b, float sum) { return fmaf(a, b, sum); }          // a channel sum's step
__device__ __forceinline__ float cs_denominator(float phi, float lam, float fI) { return fmaf(fI, lam, phi); }
__device__ __forceinline__ float cs_residual(float y, float s, float d, float fI) { return fmaf(fI, y, -s) / d; }
__device__ __forceinline__ float cs_x(float v, float m, float r, float fI) { return fmaf(m, r, v) / fI; }
__device__ __forceinline__ float cs_gv(float g, float m, float q, float fI) { return fmaf(-m, q, g) / fI; }
__device__ __forceinline__ float cs_gmask(float g, float v, float m, float r, float q, float fI) {
#pragma clang fp contract(off)
  const float qa = q * fmaf(2.f * m, r, v);
  return fmaf(g, r, -qa) / fI;
}

// the workgroup of a launch: blockIdx.x counts the bpi workgroups of an image fastest
struct CsWhere {
  unsigned group;    // image (forward) / group of n_per images (backward)
  unsigned blk;      // workgroup of the image
  size_t p;          // pixel of the plane, < HW where the thread has one
};
__device__ __forceinline__ CsWhere cs_where(unsigned bpi) {
  CsWhere w;
  w.group = blockIdx.x / bpi;
  w.blk = blockIdx.x % bpi;
  w.p = (size_t)w.blk * CS_THREADS + threadIdx.x;
  return w;
}

// V = 4: a thread owns four neighbouring pixels and moves 16 bytes per access (planes of a multiple of four pixels, aligned buffers);
// V = 1: one pixel, any plane.  HWv = H W / V, the vectors of a plane; all indices below count vectors.
template <int KC, int V>
__global__ __launch_bounds__(CS_THREADS) void k_cs_xupdate(CsIn in, int nb, const float* __restrict__ y, const float* __restrict__ mask,
                                                           const float* __restrict__ lam, float fI, float* __restrict__ x, int C, size_t HWv,
                                                           unsigned bpi, int mask_n, int y_n) {
  using Px = Vec<float, V>;
  const CsWhere w = cs_where(bpi);
  if (w.p >= HWv) return;
  const size_t n = w.group, base = n * C * HWv + w.p, mbase = mask_n > 1 ? base : w.p;
  Px vk[KC > 0 ? KC : 1], mk[KC > 0 ? KC : 1];
  float s[V], phi[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[e] = phi[e] = 0.f;
  cs_channels<KC>(C, [&](int k) {
    const Px vc = cs_sum<V>(in, nb, base + (size_t)k * HWv), mc = Px::ld(mask, (long)(mbase + (size_t)k * HWv));
    if constexpr (KC > 0) vk[k] = vc, mk[k] = mc;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      s[e] = cs_acc(mc.v[e], vc.v[e], s[e]);
      phi[e] = cs_acc(mc.v[e], mc.v[e], phi[e]);
    }
  });
  const Px yv = Px::ld(y, (long)((y_n > 1 ? n * HWv : 0) + w.p));
  const float lam_n = lam[n];
  float r[V];
#pragma unroll
  for (int e = 0; e < V; ++e) r[e] = cs_residual(yv.v[e], s[e], cs_denominator(phi[e], lam_n, fI), fI);
  cs_channels<KC>(C, [&](int k) {
    Px vc, mc, xc;
    if constexpr (KC > 0) vc = vk[k], mc = mk[k];
    else vc = cs_sum<V>(in, nb, base + (size_t)k * HWv), mc = Px::ld(mask, (long)(mbase + (size_t)k * HWv));
#pragma unroll
    for (int e = 0; e < V; ++e) xc.v[e] = cs_x(vc.v[e], mc.v[e], r[e], fI);
    xc.st(x, (long)(base + (size_t)k * HWv));
  });
}

// what the glam reduction works on (all null when no gradient of lam is asked for)
struct CsBwdRed {
  double* partial;    // [N][bpi]: the workgroups' sums of q r
  unsigned* counter;  // [N] tickets, zero before the launch
  float* glam;        // [N]
};

// A workgroup answers for the images n0 .. n0 + n_per - 1 of its pixels: n_per = N where a gradient is summed over the batch (a shared
// mask's, a shared y's), else 1.
template <int KC>
__global__ __launch_bounds__(CS_THREADS) void k_cs_bwd(const float* __restrict__ g, const float* __restrict__ v, const float* __restrict__ y,
                                                       const float* __restrict__ mask, const float* __restrict__ lam, float fI,
                                                       float* __restrict__ gv, float* __restrict__ gy, float* __restrict__ gmask, CsBwdRed red,
                                                       int C, size_t HW, unsigned bpi, int n_per, int mask_n, int y_n) {
  __shared__ double sh[CS_THREADS / 64];
  __shared__ int last;
  const CsWhere w = cs_where(bpi);
  const bool live = w.p < HW;
  const int n0 = (int)w.group * n_per;
  const bool sum_mask = gmask && mask_n == 1 && n_per > 1, sum_y = gy && y_n == 1 && n_per > 1;
  float gm[KC > 0 ? KC : 1];         // a shared mask's gradient, added up over the images in n order
  float gys = 0.f;                   // a shared y's
  for (int n = n0; n < n0 + n_per; ++n) {
    float qr = 0.f;
    if (live) {
      const size_t base = (size_t)n * C * HW + w.p;
      const float* m = mask + (mask_n > 1 ? base : w.p);
      float gk[KC > 0 ? KC : 1], vk[KC > 0 ? KC : 1], mk[KC > 0 ? KC : 1];
      float s = 0.f, phi = 0.f, t = 0.f;
      cs_channels<KC>(C, [&](int k) {
        const size_t i = base + (size_t)k * HW;
        const float gc = g[i], vc = v[i], mc = m[(size_t)k * HW];
        if constexpr (KC > 0) gk[k] = gc, vk[k] = vc, mk[k] = mc;
        s = cs_acc(mc, vc, s);
        phi = cs_acc(mc, mc, phi);
        t = cs_acc(mc, gc, t);
      });
      const float d = cs_denominator(phi, lam[n], fI);
      const float r = cs_residual(y[(y_n > 1 ? (size_t)n * HW : 0) + w.p], s, d, fI), q = t / d;
      if (gv || gmask)
        cs_channels<KC>(C, [&](int k) {
          const size_t i = base + (size_t)k * HW;
          float gc, vc, mc;
          if constexpr (KC > 0) gc = gk[k], vc = vk[k], mc = mk[k];
          else gc = g[i], vc = v[i], mc = m[(size_t)k * HW];
          if (gv) gv[i] = cs_gv(gc, mc, q, fI);
          if (gmask) {
            const float gmc = cs_gmask(gc, vc, mc, r, q, fI);
            if (!sum_mask) {
              gmask[(mask_n > 1 ? base : w.p) + (size_t)k * HW] = gmc;
            } else if constexpr (KC > 0) {
              gm[k] = n == n0 ? gmc : gm[k] + gmc;
            } else {                                           // (this thread's own cell: written for n0, added to after)
              float* o = gmask + w.p + (size_t)k * HW;
              *o = n == n0 ? gmc : *o + gmc;
            }
          }
        });
      if (sum_y) gys = n == n0 ? q : gys + q;
      else if (gy) gy[(y_n > 1 ? (size_t)n * HW : 0) + w.p] = q;
      qr = q * r;
    }
    if (red.partial) {                                         // glam[n] = -sum q r (block-uniform: every thread of the workgroup is here)
      const double sum = block_sum<double>((double)qr, sh);
      if (threadIdx.x == 0) dpx_st_agent(red.partial + (size_t)n * bpi + w.blk, sum);
      const bool finish = dpx_last_block(red.counter + n, bpi, &last);
      if (finish && threadIdx.x < 64) {
        const double all = sum_partials_f64(red.partial + (size_t)n * bpi, (int)bpi);
        if (threadIdx.x == 0) red.glam[n] = (float)(-all);
      }
    }
  }
  if (!live) return;
  if constexpr (KC > 0)
    if (sum_mask) cs_channels<KC>(C, [&](int k) { gmask[w.p + (size_t)k * HW] = gm[k]; });
  if (sum_y) gy[w.p] = gys;
}

// f(std::integral_constant<int, KC>) for the channel count of a call: the one place that names the five instantiations
template <int KC> struct CsKeep {
  static constexpr int value = KC;
};
template <class F> void cs_dispatch(int C, F&& f) {
  if (C <= 8) f(CsKeep<8>{});
  else if (C <= 16) f(CsKeep<16>{});
  else if (C <= 24) f(CsKeep<24>{});
  else if (C <= CS_KEEP_MAX) f(CsKeep<32>{});
  else f(CsKeep<0>{});
}

inline size_t cs_bpi(int H, int W) { return ((size_t)H * W + CS_THREADS - 1) / CS_THREADS; }

bool cs_args_ok(const char* who, int num_psi, int N, int C, int H, int W, int mask_batch, int y_batch) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return set_error("%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W), false;
  if (num_psi < 1) return set_error("%s: num_psi=%d (at least 1)", who, num_psi), false;
  if (mask_batch != 1 && mask_batch != N) return set_error("%s: mask_batch=%d (1 or N=%d)", who, mask_batch, N), false;
  if (y_batch != 1 && y_batch != N) return set_error("%s: y_batch=%d (1 or N=%d)", who, y_batch, N), false;
  if (cs_bpi(H, W) * (size_t)N > 0x7fffffffu) return set_error("%s: %zu workgroups (at most 2^31 - 1)", who, cs_bpi(H, W) * (size_t)N), false;
  return true;
}

}  // namespace
}  // namespace dpx

extern "C" int dpx_cs_xupdate(const float* const* b, int nb, const float* y, const float* mask, const float* lam, int num_psi, float* x, int N,
                              int C, int H, int W, int mask_batch, int y_batch, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(nb >= 1 && nb <= CS_MAX_IN, "dpx_cs_xupdate: nb=%d right-hand sides (1 .. %d)", nb, CS_MAX_IN);
  DPX_REQUIRE(b && y && mask && lam && x, "dpx_cs_xupdate: null pointer");
  if (!cs_args_ok("dpx_cs_xupdate", num_psi, N, C, H, W, mask_batch, y_batch)) return DPX_ERR_ARG;
  CsIn in{};
  const size_t HW = (size_t)H * W;
  bool vec = HW % 4 == 0 && aligned16({y, mask, x});
  for (int i = 0; i < nb; ++i) {
    DPX_REQUIRE(b[i], "dpx_cs_xupdate: null pointer (right-hand side %d)", i);
    DPX_REQUIRE(b[i] != x, "dpx_cs_xupdate: the output must not be an input (no in-place call)");
    in.b[i] = b[i];
    vec = vec && aligned16({b[i]});
  }
  const size_t HWv = vec ? HW / 4 : HW, bpi = (HWv + CS_THREADS - 1) / CS_THREADS;
  const dim3 grid((unsigned)(bpi * N)), block(CS_THREADS);
  cs_dispatch(C, [&](auto keep) {
    constexpr int KC = decltype(keep)::value;
    if (vec)
      DPX_LAUNCH("k_cs_xupdate", (k_cs_xupdate<KC, 4>), grid, block, 0, (hipStream_t)stream, in, nb, y, mask, lam, (float)num_psi, x, C, HWv,
                 (unsigned)bpi, mask_batch, y_batch);
    else
      DPX_LAUNCH("k_cs_xupdate", (k_cs_xupdate<KC, 1>), grid, block, 0, (hipStream_t)stream, in, nb, y, mask, lam, (float)num_psi, x, C, HWv,
                 (unsigned)bpi, mask_batch, y_batch);
  });
  return launch_status("dpx_cs_xupdate");
}

extern "C" size_t dpx_cs_bwd_ws_bytes(int N, int C, int H, int W) {
  using namespace dpx;
  if (!cs_args_ok("dpx_cs_bwd_ws_bytes", 1, N, C, H, W, 1, 1)) return 0;
  return ticket_bytes((size_t)N) + (size_t)N * cs_bpi(H, W) * sizeof(double);
}

extern "C" int dpx_cs_backward(const float* g, const float* v, const float* y, const float* mask, const float* lam, int num_psi, float* gv,
                               float* gy, float* glam, float* gmask, int N, int C, int H, int W, int mask_batch, int y_batch, void* ws,
                               dpx_stream_t stream) {
  using namespace dpx;
  hipStream_t s = (hipStream_t)stream;
  DPX_REQUIRE(g && v && y && mask && lam, "dpx_cs_backward: null pointer");
  if (!cs_args_ok("dpx_cs_backward", num_psi, N, C, H, W, mask_batch, y_batch)) return DPX_ERR_ARG;
  DPX_REQUIRE(gv != g && gv != v && gmask != g && gmask != v && gmask != mask && gy != y, "dpx_cs_backward: a gradient must not be an input (no in-place call)");
  DPX_REQUIRE(ws || !glam, "dpx_cs_backward: null workspace (the reduction of the gradient of lam)");
  if (!gv && !gy && !glam && !gmask) return DPX_OK;
  const size_t HW = (size_t)H * W, bpi = cs_bpi(H, W);
  CsBwdRed red{nullptr, nullptr, nullptr};
  if (glam) {
    red = CsBwdRed{(double*)((char*)ws + ticket_bytes((size_t)N)), (unsigned*)ws, glam};
    DPX_REQUIRE(hipMemsetAsync(ws, 0, ticket_bytes((size_t)N), s) == hipSuccess, "dpx_cs_backward: zero fill failed");
  }
  const int n_per = N > 1 && ((gmask && mask_batch == 1) || (gy && y_batch == 1)) ? N : 1;
  cs_dispatch(C, [&](auto keep) {
    DPX_LAUNCH("k_cs_bwd", k_cs_bwd<decltype(keep)::value>, dim3((unsigned)(bpi * (N / n_per))), dim3(CS_THREADS), 0, s, g, v, y, mask, lam,
               (float)num_psi, gv, gy, gmask, red, C, HW, (unsigned)bpi, n_per, mask_batch, y_batch);
  });
  return launch_status("dpx_cs_backward");
}
