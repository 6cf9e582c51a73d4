// Unrolled ADMM with closed-form proxes, forward and backward, as two C-side loops (config 5: specialize(method='unroll'),
// reference dprox/algo/specialization/unroll.py:14-58 differentiating dprox/algo/admm.py:49-59 with PyTorch autograd).
//
// This file sequences stage kernels without returning to the host language between stages (issued from Python, a 10-iteration
// training step's launches cost ~4 ms of issue time for ~2.3 ms of run time).  Forward: on power-of-two planes the two-kernel
// iteration of dpx_admm_run (dpx_iter.hip) whose row kernel emits the history -- x, v_i, the next right-hand side; fp32 or bf16 --,
// otherwise dpx_admm_rhs / dpx_fourier_solve / dpx_admm_zupdate.  Backward: the stage kernels of dpx_autodiff.hip with the sums
// between the stages folded in and one finishing launch per iteration for its three reductions.
//
// History buffer (caller-owned): iteration `it` occupies (2 + 2 n) planes of px = B*C*H*W floats:
//     [rhs][x][v_0 .. v_{n-1}][u_0 .. u_{n-1}]
// the backward pass reads rhs, x and v_i of every iteration (u_i only as the forward's running state).
//
// bf16 mode (BASELINE config 5 is quoted in bf16): the forward iteration, every transform and every reduction stay fp32 -- the
// x-update divides by |H|^2 + rho sum|G|^2, which amplifies round-off by up to 1e5, bf16 state would lose
// the iterate -- but what is KEPT for the backward pass is stored in bf16: per iteration rhs, x and v_i (u_i is not needed),
// (2 + n) x 2 bytes per pixel instead of (2 + 2n) x 4.  The soft-threshold / clipping masks the backward reads from v_i survive
// the rounding exactly (v = 0 stays 0); d loss / d rho_t (inner products with x and rhs, signed sums that largely cancel) carry the bf16
// rounding: ~1e-3 relative at config 5's size, 6e-5 ... 2e-2 measured on one or two small planes after one or two iterations.
// Slot `it` of that history is [rhs][x][v_0 .. v_{n-1}] in 16 bits; the iteration itself runs in caller-owned fp32 work planes
//     [rhs][x] + two generations of [v_0 .. v_{n-1}][u_0 .. u_{n-1}]
// (the last iteration writes the caller's x_out / v_out / u_out instead) and a packing launch rounds rhs, x, v_i into the slot -- except
// on the two-kernel loop, whose row kernel writes the non-last iterations' x, v_i and the next rhs into the slots as bf16 itself (nothing
// but u_i and the spectra is read back by the next iteration): there only rhs(0) and u_i are work planes, and only rhs(0) and the last
// iteration's x / v_i go through the packing kernel.  Both formats run the same two loops over one description of these places (FwdPlanes).
#include "dpx_prox_dev.h"

using namespace dpx;

namespace dpx {
// fp32 planes -> consecutive bf16 planes of a history slot, round-to-nearest-even
struct PlanePack {
  float* p[2 + DPX_MAX_TERMS];
  int n;
};
__global__ void k_hist_pack_bf16(PlanePack P, unsigned short* __restrict__ slot, long px) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < px * P.n; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / px);
    const unsigned u = __float_as_uint(P.p[k][i - k * px]);
    slot[i] = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
}
}  // namespace dpx

namespace {
struct Hist {
  float* base;
  size_t px;
  int n;
  float* rhs(int it) const { return base + (size_t)it * (2 + 2 * n) * px; }
  float* x(int it) const { return rhs(it) + px; }
  float* v(int it, int i) const { return rhs(it) + (size_t)(2 + i) * px; }
  float* u(int it, int i) const { return rhs(it) + (size_t)(2 + n + i) * px; }
};

// One iteration's planes, as the forward loops see them
struct IterPlanes {
  float* rhs;
  float* x;
  float* v[DPX_MAX_TERMS];
  float* u[DPX_MAX_TERMS];
};
// Where the forward loops keep their iterations (the layouts: the comment at the top): at(it, two_kernel) is filled in one of two ways
struct FwdPlanes {
  float* hist;               // fp32 history, or NULL and:
  unsigned short* hist16;    // bf16 history,
  float* work;               //   its fp32 work planes,
  float* x_out;              //   and the last iteration's destinations
  float* const* v_out;
  float* const* u_out;
  size_t px;
  int n, T;
  unsigned short* slot(int it) const { return hist16 + (size_t)it * (2 + n) * px; }
  IterPlanes at(int it, bool two_kernel) const {
    IterPlanes q;
    if (hist) {                                            // fp32 history: everything is its own plane of the history
      const Hist h{hist, px, n};
      q.rhs = h.rhs(it);
      q.x = h.x(it);
      for (int i = 0; i < n; ++i) q.v[i] = h.v(it, i), q.u[i] = h.u(it, i);
      return q;
    }
    // bf16 history: work planes [rhs][x] + generation it & 1 of [v_i][u_i]; the last iteration's x, v_i, u_i are the caller's; the
    // two-kernel loop's row kernel writes rhs (it > 0) and the non-last x, v_i into the slot itself
    float* gen = work + (size_t)(2 + (it & 1) * 2 * n) * px;
    const bool last = it == T - 1;
    q.rhs = (two_kernel && it) ? (float*)slot(it) : work;
    q.x = last ? x_out : two_kernel ? (float*)(slot(it) + px) : work + px;
    for (int i = 0; i < n; ++i) {
      q.v[i] = last ? v_out[i] : two_kernel ? (float*)(slot(it) + (size_t)(2 + i) * px) : gen + (size_t)i * px;
      q.u[i] = last ? u_out[i] : gen + (size_t)(n + i) * px;
    }
    return q;
  }
};
}  // namespace

#define DPX_TRY(call)            \
  do {                           \
    const int dpx_rc_ = (call);  \
    if (dpx_rc_ != DPX_OK) return dpx_rc_; \
  } while (0)

// The forward iterations of both history formats.  `name`: the entry point, for its messages.  DPX_OK = everything was issued (the bf16
// entry asks launch_status() for its packing launches itself).
static int unrolled_forward_impl(const char* name, const FwdPlanes& p, const float* const* v0, const float* const* u0, const int* linops,
                                 const int* proxes, const float* alphas, const float* rho_tab, const float* const* lam_tabs, const void* spec_add,
                                 const void* dd, float eps, int B, int C, int H, int W, const void* table, void* spectrum_ws,
                                 const float* fresh_x0, dpx_stream_t stream) {
  const int n = p.n, T = p.T;
  const size_t px = p.px;
  // bf16 history: planes first .. first + count - 1 of iteration `it`'s [rhs][x][v_i] (at q) rounded into its slot
  auto pack = [&](int it, const IterPlanes& q, int first, int count) {
    PlanePack P;
    P.n = count;
    for (int k = first; k < first + count; ++k) P.p[k - first] = k == 0 ? q.rhs : k == 1 ? q.x : q.v[k - 2];
    DPX_LAUNCH("k_hist_pack_bf16", k_hist_pack_bf16, dim3(grid_for((long)(px * count), 256, 8192)), dim3(256), 0, (hipStream_t)stream, P,
               p.slot(it) + (size_t)first * px, (long)px);
  };
  dpx_term rt[DPX_MAX_TERMS], zt[DPX_MAX_TERMS];
  for (int i = 0; i < n; ++i) zt[i] = dpx_term{linops[i], proxes[i], alphas[i], 0, lam_tabs[i], nullptr, (float*)u0[i], nullptr};
  // power-of-two planes with stencil terms: the two-kernel iteration of dpx_admm_run, its row kernel emitting the history (x, v_i, the next
  // right-hand side; u_i are its outputs anyway) -- 2 launches per iteration instead of 5
  if (dpx_admm_iter_supported(H, W, zt, n) && dpx_spectrum_bytes(B * C, H, W) > 0) {
    char* spec_a = (char*)spectrum_ws;
    char* spec_b = spec_a + dpx_spectrum_bytes(B * C, H, W) / 2;
    for (int i = 0; i < n; ++i) rt[i] = dpx_term{linops[i], proxes[i], 1.0f, 0, nullptr, (float*)v0[i], (float*)u0[i], nullptr};
    IterPlanes q = p.at(0, true), prev;
    // fresh_x0: the state is ADMM.initialize(x0) untouched (v_i = K_i x0, u_i = 0) and need not exist -- the first right-hand side is formed
    // from x0 and the first iteration does not stream the (zero) duals (DPX_TERM_U_ZERO: row 0 of plane 0 of every image of u0[i] is zero)
    if (fresh_x0) DPX_TRY(dpx_admm_rhs_fresh(q.rhs, fresh_x0, rho_tab, linops, n, B, C, H, W, stream));
    else DPX_TRY(dpx_admm_rhs(q.rhs, nullptr, rho_tab, rt, n, B, C, H, W, stream));
    DPX_TRY(dpx_rfft_rows(q.rhs, spec_a, B, C, H, W, table, stream));
    if (p.hist16) pack(0, q, 0, 1);
    for (int it = 0; it < T; ++it) {
      DPX_TRY(dpx_admm_iter_cols(spec_a, spec_b, spec_add, dd, rho_tab + (size_t)it * B, eps, B, C, H, W, table, stream));
      for (int i = 0; i < n; ++i)
        zt[i] = dpx_term{linops[i], proxes[i], alphas[i], (it == 0 && fresh_x0) ? DPX_TERM_U_ZERO : 0, lam_tabs[i] + (size_t)it * B, q.v[i],
                         it ? prev.u[i] : (float*)u0[i], q.u[i]};
      const bool last = it == T - 1;
      const IterPlanes next = last ? q : p.at(it + 1, true);
      // (bf16 history: the non-last iterations' x, v_i and next rhs are 16-bit planes of the slots)
      DPX_TRY(iter_rows_impl(spec_b, last ? nullptr : spec_a, zt, n, last ? nullptr : rho_tab + (size_t)(it + 1) * B, q.x, 1,
                             last ? nullptr : next.rhs, (p.hist16 && !last) ? 1 : 0, B, C, H, W, table, stream));
      prev = q;
      q = next;
    }
    if (p.hist16) pack(T - 1, q, 1, 1 + n);
    return DPX_OK;
  }
  DPX_REQUIRE(!fresh_x0, "%s: fresh_x0 needs the two-kernel iteration (plane %d x %d is not on it): pass the initial state", name, H, W);
  IterPlanes prev;
  for (int it = 0; it < T; ++it) {
    const IterPlanes q = p.at(it, false);
    for (int i = 0; i < n; ++i) {
      float* pv = it ? prev.v[i] : (float*)v0[i];
      float* pu = it ? prev.u[i] : (float*)u0[i];
      rt[i] = dpx_term{linops[i], proxes[i], 1.0f, 0, nullptr, pv, pu, nullptr};
      zt[i] = dpx_term{linops[i], proxes[i], alphas[i], 0, lam_tabs[i] + (size_t)it * B, q.v[i], pu, q.u[i]};
    }
    const float* rho = rho_tab + (size_t)it * B;
    DPX_TRY(dpx_admm_rhs(q.rhs, nullptr, rho, rt, n, B, C, H, W, stream));
    DPX_TRY(dpx_fourier_solve(q.rhs, q.x, spec_add, dd, rho, eps, B, C, H, W, table, spectrum_ws, stream));
    DPX_TRY(dpx_admm_zupdate(q.x, zt, n, B, C, H, W, stream));
    if (p.hist16) pack(it, q, 0, 2 + n);
    prev = q;
  }
  return DPX_OK;
}

extern "C" size_t dpx_admm_unrolled_hist_bytes(int nterms, int T, int B, int C, int H, int W) {
  return (size_t)T * (2 + 2 * nterms) * B * C * H * W * sizeof(float);
}

extern "C" int dpx_admm_unrolled_forward(float* hist, const float* const* v0, const float* const* u0, const int* linops, const int* proxes,
                                         const float* alphas, int nterms, const float* rho_tab, const float* const* lam_tabs, int T,
                                         const void* spec_add, const void* dd, float eps, int B, int C, int H, int W, const void* table,
                                         void* spectrum_ws, const float* fresh_x0, dpx_stream_t stream) {
  DPX_REQUIRE(hist && v0 && u0 && linops && proxes && alphas && rho_tab && lam_tabs && dd && table && spectrum_ws,
              "dpx_admm_unrolled_forward: null pointer");
  DPX_REQUIRE(nterms >= 1 && nterms <= DPX_MAX_TERMS && T >= 1 && B > 0 && C > 0 && H > 0 && W > 0, "dpx_admm_unrolled_forward: bad sizes");
  const FwdPlanes p{hist, nullptr, nullptr, nullptr, nullptr, nullptr, (size_t)B * C * H * W, nterms, T};
  return unrolled_forward_impl("dpx_admm_unrolled_forward", p, v0, u0, linops, proxes, alphas, rho_tab, lam_tabs, spec_add, dd, eps, B, C, H, W, table,
                               spectrum_ws, fresh_x0, stream);
}

extern "C" size_t dpx_admm_unrolled_hist_bytes_bf16(int nterms, int T, int B, int C, int H, int W) {
  return (size_t)T * (2 + nterms) * B * C * H * W * sizeof(unsigned short);
}
// fp32 working planes of the bf16-history forward: rhs, x, and two generations of v_i / u_i
extern "C" size_t dpx_admm_unrolled_work_bytes_bf16(int nterms, int B, int C, int H, int W) {
  return (size_t)(2 + 4 * nterms) * B * C * H * W * sizeof(float);
}

// The final state is written to x_out, v_out[i], u_out[i] (fp32).
extern "C" int dpx_admm_unrolled_forward_bf16(void* hist_bf16, void* work, float* x_out, float* const* v_out, float* const* u_out,
                                              const float* const* v0, const float* const* u0, const int* linops, const int* proxes,
                                              const float* alphas, int nterms, const float* rho_tab, const float* const* lam_tabs, int T,
                                              const void* spec_add, const void* dd, float eps, int B, int C, int H, int W,
                                              const void* table, void* spectrum_ws, const float* fresh_x0, dpx_stream_t stream) {
  DPX_REQUIRE(hist_bf16 && work && x_out && v_out && u_out && v0 && u0 && linops && proxes && alphas && rho_tab && lam_tabs && dd && table &&
                  spectrum_ws, "dpx_admm_unrolled_forward_bf16: null pointer");
  DPX_REQUIRE(nterms >= 1 && nterms <= DPX_MAX_TERMS && T >= 1 && B > 0 && C > 0 && H > 0 && W > 0, "dpx_admm_unrolled_forward_bf16: bad sizes");
  const FwdPlanes p{nullptr, (unsigned short*)hist_bf16, (float*)work, x_out, v_out, u_out, (size_t)B * C * H * W, nterms, T};
  DPX_TRY(unrolled_forward_impl("dpx_admm_unrolled_forward_bf16", p, v0, u0, linops, proxes, alphas, rho_tab, lam_tabs, spec_add, dd, eps, B, C, H, W,
                                table, spectrum_ws, fresh_x0, stream));
  return launch_status("dpx_admm_unrolled_forward_bf16");
}

// workspace: (4 + 6 n) planes + 2 B floats, followed by the partial sums of one iteration's three reductions ((n + 2) B rows)
extern "C" size_t dpx_admm_unrolled_bwd_ws_bytes(int nterms, int B, int C, int H, int W) {
  return ((size_t)(4 + 6 * nterms) * B * C * H * W + 2 * (size_t)B + 64) * sizeof(float) +
         (size_t)(DPX_MAX_TERMS + 2) * B * ad_partial_blocks(C, H, W) * sizeof(float);
}

// gx / gv_in[i] / gu_in[i]: gradients w.r.t. the final x, v_i, u_i (any may be NULL = 0).
// Out: gv0[i], gu0[i] (w.r.t. the initial split / dual variables), grho [T][B], glam [T][n][B], goff[k] (w.r.t. the k-th
// Omega offset: K g_rhs summed over the iterations; off_otf[k] = that term's OTF table or NULL for the identity; goff[k]
// NULL = not wanted).
static int unrolled_backward_impl(const float* hist, const unsigned short* hist16, const float* gx, const float* const* gv_in, const float* const* gu_in,
                                          float* const* gv0, float* const* gu0, float* grho, float* glam, float* const* goff,
                                          const void* const* off_otf, int n_off, const int* linops, const int* proxes, const float* alphas,
                                          int nterms, const float* rho_tab, const float* const* lam_tabs, int T, const void* dd, float eps,
                                          int B, int C, int H, int W, const void* table, void* spectrum_ws, void* ws, dpx_stream_t stream) {
  DPX_REQUIRE((hist || hist16) && gv0 && gu0 && grho && glam && linops && proxes && alphas && rho_tab && lam_tabs && dd && table &&
                  spectrum_ws && ws, "dpx_admm_unrolled_backward: null pointer");
  DPX_REQUIRE(nterms >= 1 && nterms <= DPX_MAX_TERMS && T >= 1 && B > 0 && n_off >= 0 && (n_off == 0 || (goff && off_otf)),
              "dpx_admm_unrolled_backward: bad sizes");
  const int n = nterms;
  const size_t px = (size_t)B * C * H * W;
  // fp32 history: pointers into it; bf16 history: iteration `it` is expanded into the (2 + n) staging planes first
  const Hist h32{(float*)hist, px, n};
  // (bf16 history: the stage kernels read the 16-bit slots themselves)
  const int hb = hist ? 0 : 1;
  auto slot16 = [&](int it) { return hist16 + (size_t)it * (2 + n) * px; };
  auto H_rhs = [&](int it) { return hist ? h32.rhs(it) : (float*)slot16(it); };
  auto H_x = [&](int it) { return hist ? h32.x(it) : (float*)(slot16(it) + px); };
  auto H_v = [&](int it, int i) { return hist ? h32.v(it, i) : (float*)(slot16(it) + (size_t)(2 + i) * px); };
  float* w = (float*)ws;
  float* gxz = w;
  float* gtot = w + px;
  float* grhs = w + 2 * px;
  float* tmp = w + 3 * px;
  float* gu_a = w + 4 * px;                  // n planes
  float* gu_b = gu_a + n * px;               // n planes
  float* set[2] = {gu_b + n * px, gu_b + 3 * n * px};   // each: gv[n] then gu[n]
  float* rho_a = set[1] + 2 * n * px;
  float *part_lam, *part_a, *part_b;
  auto own_partials = [&] {                                // the workspace's partial-sum rows: [n B][nblk], [B][nblk], [B][nblk]
    part_lam = rho_a + ((2 * B + 63) / 64) * 64;
    part_a = part_lam + (size_t)DPX_MAX_TERMS * B * ad_partial_blocks(C, H, W);
    part_b = part_a + (size_t)B * ad_partial_blocks(C, H, W);
  };
  own_partials();
  const hipStream_t st = (hipStream_t)stream;
  const float one2[2] = {1.f, 1.f};
  const float* cur_gv[DPX_MAX_TERMS];
  const float* cur_gu[DPX_MAX_TERMS];
  for (int i = 0; i < n; ++i) {
    cur_gv[i] = gv_in ? gv_in[i] : nullptr;
    cur_gu[i] = gu_in ? gu_in[i] : nullptr;
  }
  bool off_started[DPX_MAX_TERMS] = {false, false, false, false};
  DPX_REQUIRE(n_off <= DPX_MAX_TERMS, "dpx_admm_unrolled_backward: at most %d offsets", DPX_MAX_TERMS);
  // the offsets' share of one iteration: goff_k += K_k g_rhs
  auto add_offsets = [&]() -> int {
    for (int k = 0; k < n_off; ++k) {
      if (!goff[k]) continue;
      if (off_otf[k]) {
        float* dst = off_started[k] ? tmp : goff[k];
        DPX_TRY(dpx_fft_conv(grhs, dst, off_otf[k], 0, B, C, H, W, table, spectrum_ws, stream));
        if (off_started[k]) {
          const float* xs[2] = {goff[k], tmp};
          DPX_TRY(dpx_lincomb(goff[k], 2, xs, one2, nullptr, B, (long)(px / B), stream));
        }
      } else {
        const float* xs[2] = {grhs, goff[k]};
        DPX_TRY(dpx_lincomb(goff[k], off_started[k] ? 2 : 1, xs, one2, nullptr, B, (long)(px / B), stream));
      }
      off_started[k] = true;
    }
    return DPX_OK;
  };
  // iteration `it`'s terms for a z stage: incoming g_v / g_u (NULL: none), its share of the dual gradient into the planes at `ga` (NULL: the
  // fused stages take a_in / a_out instead)
  auto bwd_terms = [&](dpx_bwd_term* bt, int it, const float* const* gv, const float* const* gu, float* ga) {
    for (int i = 0; i < n; ++i)
      bt[i] = dpx_bwd_term{linops[i], proxes[i], alphas[i], 0, lam_tabs[i] + (size_t)it * B, H_v(it, i), gv ? gv[i] : nullptr, gu ? gu[i] : nullptr,
                           ga ? ga + i * px : nullptr};
  };
  // how the two fused loops start: the z stage of iteration T - 1 (dual share into gu_a), its lambda gradients, *g = gx + its g_x
  auto last_z_stage = [&](const float** g) -> int {
    dpx_bwd_term bt[DPX_MAX_TERMS];
    bwd_terms(bt, T - 1, cur_gv, cur_gu, gu_a);
    DPX_TRY(zupdate_bwd_partials(gxz, bt, n, part_lam, hb, B, C, H, W, st));
    DPX_TRY(finish_iter(part_lam, part_a, part_b, glam + (size_t)(T - 1) * n * B, nullptr, rho_tab + (size_t)(T - 1) * B, n, B, C, H, W, st));
    *g = gxz;
    if (gx) {
      const float* xs[2] = {gx, gxz};
      DPX_TRY(dpx_lincomb(gtot, 2, xs, one2, nullptr, B, (long)(px / B), stream));
      *g = gtot;
    }
    return DPX_OK;
  };
  // ... and how they end: iteration 0's rhs stage on grhs (dual share so far in the planes at `ga`) into the caller's gv0 / gu0, and d / d rho_0
  auto first_rhs_stage = [&](const float* ga) -> int {
    const float* gua[DPX_MAX_TERMS];
    for (int i = 0; i < n; ++i) gua[i] = ga + (size_t)i * px;
    DPX_TRY(solve_rhs_bwd_partials(grhs, H_x(0), H_rhs(0), rho_tab, linops, n, gv0, gu0, gua, part_a, part_b, hb, B, C, H, W, st));
    return finish_iter(part_lam, part_a, part_b, nullptr, grho, rho_tab, n, B, C, H, W, st);
  };
  // ---- power-of-two planes: TWO launches per backward iteration (+ the finishing launch), the mirror image of the forward loop --
  //        z(T-1) | rows | cols(T-1) | [rows^-1 + rhs(T-1) + z(T-2) + rows] | cols(T-2) | ... | cols(0) | rows^-1 | rhs(0)
  //      g_rhs and g_x stay in the Fourier domain between the stages (k_bwd_rows, dpx_bwd_rows.hip).  The offsets' gradient
  //      sum_t K g_rhs_t = K sum_t g_rhs_t is formed once at the end from the sum of the g_rhs images (emitted by the row kernel only
  //      when an offset gradient is wanted).  Knob unroll_bwd_staged: 0 = this loop where it applies, 2 = the image-domain fused
  //      stage below, 1 = the staged loop.
  const int slots = (T > 1 && tune(TUNE_UNROLL_BWD_STAGED) == 0) ? bwd_rows_slots(B, C, H, W, ad_partial_blocks(C, H, W)) : 0;
  if (slots > 0 && dpx_spectrum_bytes(B * C, H, W) > 0) {
    const int P = B * C;
    float2* spec_a = (float2*)spectrum_ws;
    float2* spec_b = (float2*)((char*)spectrum_ws + dpx_spectrum_bytes(P, H, W) / 2);
    float* abuf[2] = {gu_a, gu_b};
    int cur = 0;
    bool want_off = false;
    for (int k = 0; k < n_off; ++k) want_off = want_off || goff[k];
    const float* g;
    DPX_TRY(last_z_stage(&g));
    DPX_TRY(rows_r2c_pow2(g, spec_a, P, H, W, table, st));
    SpecArgs sa{};
    sa.dd = (const float2*)dd;
    sa.eps = eps;
    sa.eps_num = 0.f;
    sa.scale = 1.0f / ((float)H * (float)W);
    // the iterations' partial sums side by side in the planes only the staged loop uses, finished by ONE launch behind the loop (a
    // finishing launch per iteration is 9 of the loop's 27 launches); if they do not fit: one finishing launch per iteration
    const long pstride = (long)(n + 2) * B * slots;
    const bool all_at_once = (size_t)(T - 1) * pstride <= (size_t)2 * n * px;
    for (int it = T - 1; it >= 1; --it) {
      const float* rho = rho_tab + (size_t)it * B;
      sa.rho = rho;
      if (all_at_once) {
        part_lam = set[0] + (size_t)(T - 1 - it) * pstride;
        part_a = part_lam + (size_t)n * B * slots;
        part_b = part_a + (size_t)B * slots;
      }
      DPX_TRY(cols_solve_pow2(spec_a, spec_b, sa, P, C, H, W, table, st));
      dpx_bwd_term bt[DPX_MAX_TERMS];
      const float* ain[DPX_MAX_TERMS];
      float* aout[DPX_MAX_TERMS];
      bwd_terms(bt, it - 1, nullptr, nullptr, nullptr);
      for (int i = 0; i < n; ++i) {
        ain[i] = abuf[cur] + i * px;
        aout[i] = abuf[cur ^ 1] + i * px;
      }
      DPX_TRY(bwd_rows_fused(spec_b, spec_a, H_x(it), H_rhs(it), rho, bt, n, ain, aout, want_off ? tmp : nullptr, it != T - 1, part_a, part_b, part_lam, hb,
                             B, C, H, W, table, st));
      if (!all_at_once) DPX_TRY(finish_iter_n(part_lam, part_a, part_b, glam + (size_t)(it - 1) * n * B, grho + (size_t)it * B, rho, n, B, slots, st));
      cur ^= 1;
    }
    if (all_at_once) {
      DPX_TRY(finish_all(set[0], pstride, glam, grho, rho_tab, n, B, slots, T, T - 1, st));
      own_partials();                                       // (for the last stage below)
    }
    sa.rho = rho_tab;
    DPX_TRY(cols_solve_pow2(spec_a, spec_b, sa, P, C, H, W, table, st));
    DPX_TRY(rows_c2r_pow2(spec_b, grhs, P, H, W, table, st));
    if (want_off) {
      const float* xs[2] = {grhs, tmp};
      DPX_TRY(dpx_lincomb(tmp, 2, xs, one2, nullptr, B, (long)(px / B), stream));      // sum_t g_rhs_t
      for (int k = 0; k < n_off; ++k) {
        if (!goff[k]) continue;
        if (off_otf[k]) {
          DPX_TRY(dpx_fft_conv(tmp, goff[k], off_otf[k], 0, B, C, H, W, table, spectrum_ws, stream));
        } else {
          const float* one[1] = {tmp};
          DPX_TRY(dpx_lincomb(goff[k], 1, one, one2, nullptr, B, (long)(px / B), stream));
        }
      }
    }
    return first_rhs_stage(abuf[cur]);
  }
  // ---- the loop with the rhs stage of iteration `it` and the z stage of iteration `it - 1` as ONE pass (k_rhs_z_bwd4, where staged_vec() gives 4):
  //        z(T-1) | solve(T-1) | [rhs(T-1) + z(T-2)] | solve(T-2) | ... | [rhs(1) + z(0)] | solve(0) | rhs(0)
  //      4 launches per iteration (3 of them the transform) + 1 finishing launch instead of 5 + 1, no g_v / g_u planes in between.
  //      Knob unroll_bwd_staged = 1 keeps the staged loop below (A/B and tests).
  //      (every plane of the loop sits a multiple of px elements into the history or the workspace: with W % 4 == 0 those two decide the rule)
  if (tune(TUNE_UNROLL_BWD_STAGED) != 1 && staged_vec(W, {ws}, {hist ? (const void*)hist : hist16}, hb) == 4) {
    float* abuf[2] = {gu_a, gu_b};
    int cur = 0;
    // (experiment) the fused stage's last workgroup finishes the iteration's reductions itself (one arrival counter in the workspace's
    // scalar slot, zeroed once per call and reset by its last user) instead of a finishing launch per iteration.
    // Knob unroll_bwd_fold_finish, OFF: measured at 4x3x512^2 the step went from 1.55 - 1.61 to 1.78 ms -- 1536 workgroups taking a ticket
    // on one counter (~12 ns each) and one workgroup adding up 12 x 384 partials cost more than the 4.6-us finishing launch they replace.
    unsigned* counter = tune(TUNE_UNROLL_BWD_FOLD_FINISH) ? (unsigned*)rho_a : nullptr;
    if (counter && T > 1 && hipMemsetAsync(counter, 0, sizeof(unsigned), st) != hipSuccess) {
      set_error("dpx_admm_unrolled_backward: hipMemsetAsync failed");
      return DPX_ERR_LAUNCH;
    }
    const float* g;
    DPX_TRY(last_z_stage(&g));
    for (int it = T - 1; it >= 1; --it) {
      const float* rho = rho_tab + (size_t)it * B;
      DPX_TRY(dpx_fourier_apply_inv(g, grhs, dd, rho, eps, B, C, H, W, table, spectrum_ws, stream));
      DPX_TRY(add_offsets());
      dpx_bwd_term bt[DPX_MAX_TERMS];
      const float* ain[DPX_MAX_TERMS];
      float* aout[DPX_MAX_TERMS];
      bwd_terms(bt, it - 1, nullptr, nullptr, nullptr);
      for (int i = 0; i < n; ++i) {
        ain[i] = abuf[cur] + i * px;
        aout[i] = abuf[cur ^ 1] + i * px;
      }
      float* glam_it = glam + (size_t)(it - 1) * n * B;
      float* grho_it = grho + (size_t)it * B;
      if (!rhs_z_bwd_fused(grhs, H_x(it), H_rhs(it), rho, bt, n, ain, aout, gxz, part_a, part_b, part_lam, hb, B, C, H, W, st, counter,
                           glam_it, grho_it)) {
        set_error("dpx_admm_unrolled_backward: fused stage refused a plane it was selected for");
        return DPX_ERR_LAUNCH;
      }
      if (!counter) DPX_TRY(finish_iter(part_lam, part_a, part_b, glam_it, grho_it, rho, n, B, C, H, W, st));
      cur ^= 1;
      g = gxz;
    }
    DPX_TRY(dpx_fourier_apply_inv(g, grhs, dd, rho_tab, eps, B, C, H, W, table, spectrum_ws, stream));
    DPX_TRY(add_offsets());
    return first_rhs_stage(abuf[cur]);
  }
  for (int it = T - 1; it >= 0; --it) {
    const float* rho = rho_tab + (size_t)it * B;
    dpx_bwd_term bt[DPX_MAX_TERMS];
    bwd_terms(bt, it, cur_gv, cur_gu, gu_a);
    DPX_TRY(zupdate_bwd_partials(gxz, bt, n, part_lam, hb, B, C, H, W, st));
    const float* g = gxz;
    if (it == T - 1 && gx) {
      const float* xs[2] = {gx, gxz};
      DPX_TRY(dpx_lincomb(gtot, 2, xs, one2, nullptr, B, (long)(px / B), stream));
      g = gtot;
    }
    DPX_TRY(dpx_fourier_apply_inv(g, grhs, dd, rho, eps, B, C, H, W, table, spectrum_ws, stream));
    DPX_TRY(add_offsets());
    // gradients w.r.t. the previous iteration's v_i, u_i (the last step writes the caller's outputs directly)
    float* nv[DPX_MAX_TERMS];
    float* nu[DPX_MAX_TERMS];
    for (int i = 0; i < n; ++i) {
      nv[i] = it ? set[it & 1] + (size_t)i * px : gv0[i];
      nu[i] = it ? set[it & 1] + (size_t)(n + i) * px : gu0[i];
    }
    // the x-update's rho gradient and the rhs stage in one pass over g_rhs, with the sum of the two stages' shares of the dual
    // gradient folded in: gu_prev_i = gu_a_i - gv_i
    const float* gua[DPX_MAX_TERMS];
    for (int i = 0; i < n; ++i) gua[i] = gu_a + (size_t)i * px;
    DPX_TRY(solve_rhs_bwd_partials(grhs, H_x(it), H_rhs(it), rho, linops, n, nv, nu, gua, part_a, part_b, hb, B, C, H, W, st));
    // ... and the iteration's three reductions (d/d lam_i, the two shares of d/d rho) finished by one launch
    DPX_TRY(finish_iter(part_lam, part_a, part_b, glam + (size_t)it * n * B, grho + (size_t)it * B, rho, n, B, C, H, W, st));
    for (int i = 0; i < n; ++i) {
      cur_gv[i] = nv[i];
      cur_gu[i] = nu[i];
    }
  }
  return DPX_OK;
}

extern "C" int dpx_admm_unrolled_backward(const float* hist, const float* gx, const float* const* gv_in, const float* const* gu_in,
                                          float* const* gv0, float* const* gu0, float* grho, float* glam, float* const* goff,
                                          const void* const* off_otf, int n_off, const int* linops, const int* proxes, const float* alphas,
                                          int nterms, const float* rho_tab, const float* const* lam_tabs, int T, const void* dd, float eps,
                                          int B, int C, int H, int W, const void* table, void* spectrum_ws, void* ws, dpx_stream_t stream) {
  DPX_REQUIRE(hist, "dpx_admm_unrolled_backward: null history");
  return unrolled_backward_impl(hist, nullptr, gx, gv_in, gu_in, gv0, gu0, grho, glam, goff, off_otf, n_off, linops, proxes, alphas, nterms,
                                rho_tab, lam_tabs, T, dd, eps, B, C, H, W, table, spectrum_ws, ws, stream);
}

// bf16 history: the stage kernels read the 16-bit slots directly, the workspace is that of the fp32 pass
extern "C" size_t dpx_admm_unrolled_bwd_ws_bytes_bf16(int nterms, int B, int C, int H, int W) {
  return dpx_admm_unrolled_bwd_ws_bytes(nterms, B, C, H, W);
}
extern "C" int dpx_admm_unrolled_backward_bf16(const void* hist_bf16, const float* gx, const float* const* gv_in, const float* const* gu_in,
                                               float* const* gv0, float* const* gu0, float* grho, float* glam, float* const* goff,
                                               const void* const* off_otf, int n_off, const int* linops, const int* proxes,
                                               const float* alphas, int nterms, const float* rho_tab, const float* const* lam_tabs, int T,
                                               const void* dd, float eps, int B, int C, int H, int W, const void* table, void* spectrum_ws,
                                               void* ws, dpx_stream_t stream) {
  DPX_REQUIRE(hist_bf16 && ws, "dpx_admm_unrolled_backward_bf16: null pointer");
  return unrolled_backward_impl(nullptr, (const unsigned short*)hist_bf16, gx, gv_in, gu_in, gv0, gu0, grho, glam, goff, off_otf, n_off, linops,
                                proxes, alphas, nterms, rho_tab, lam_tabs, T, dd, eps, B, C, H, W, table, spectrum_ws, ws, stream);
}
