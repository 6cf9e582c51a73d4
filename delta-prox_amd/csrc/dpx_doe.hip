// The wave-optics model of a diffractive optical element: height map -> point spread function, and its gradient.
//
// Restates RGBCollimator.get_psf of the reference (dprox/contrib/optic/doe_model.py:88-107 with common.py:121-160): for the three
// wavelengths lambda_c with refractive indices n_c, a wavefront of R x R samples at interval D, sensor distance d, p = R / 4,
// M = R + 2 p, a psf of P x P pixels (f = R / P):
//   h = s^2                                   s: height_map_sqrt [R][R]
//   u_c = a exp(i k_c h)                      k_c = (2 pi / lambda_c)(n_c - 1);  a: the circular aperture
//   w_c = crop_RxR( ifft2( fft2( zero-pad_p(u_c) ) . H_c ) )
//   q_c = f x f block mean of |w_c|^2,   psf = q / sum_{c,y,x} q          (ONE sum over all three channels)
// Forward = three transform launches (dpx_fft.hip: doe_rows_in / doe_cols / doe_rows_out; the optics ride in the first one's load and
// the last one's store, which also leaves sum q) + k_doe_normalise, a launch of its own over the 3 P^2 values.
// Backward = k_doe_dot (<g, psf>), then the same three launches in reverse order of meaning: rows in from
// g_w = 2 (g - <g, psf>) / (f^2 sum q) w, columns with conj(H_c) -- the adjoint of crop . F^-1 . H . F . pad is
// crop . F^-1 . conj(H) . F . pad with the same 1 / M^2, because F^H = M^2 F^-1 -- and rows out to
// g_s = 2 s sum_c k_c Im(conj(u_c) g_u_c), with u_c recomputed from s.  No floating-point atomics: two runs give the same bits.
//
// The hybrid model (a refractive lens plus the element, the reference's doe_model_hybrid.py) is the same pipeline with
//   u_c = a exp(i (k_c (s + eps)^2 + phi_c)),  a: the disc or its right half,  psf_c = q_c / sum_{y,x} q_c  (one sum per channel)
// through dpx_doe_psf_ex / dpx_doe_psf_backward_ex and their options block; the defaults are the base model and launch its kernels.
// With opts.g_field the backward pass stores the cotangent of the field in front of the propagator instead of projecting it onto s:
// the gradient to an explicit phase profile.  dpx_doe_propagate_backward is the propagator's own adjoint, dpx_doe_phase_backward the
// elementwise backward of dpx_doe_phase.  Complex cotangents follow torch's convention for a real loss: dL/dRe + i dL/dIm.
//
// H_c[k][l] = exp(-i pi d lambda_c (fx_k^2 + fy_l^2)) / M^2 with fx = ifftshift((arange(M) - (M - 1) / 2) / (D M)) is evaluated once
// per model in float64 (k_doe_propagator: sincospi of the phase in half turns, up to 1.2e3 of them at the default configuration) and
// stored as complex64.
#include "dpx_common.h"
#include "dpx_reduce_dev.h"

namespace dpx {
namespace {

constexpr int DOE_THREADS = 256;

__global__ void k_doe_propagator(float2* __restrict__ H, int M, double d, double interval, double l0, double l1, double l2) {
  const size_t n = (size_t)M * M;
  const double inv = 1.0 / ((double)M * (double)M), fs = 1.0 / (interval * (double)M), mid = 0.5 * (double)(M - 1);
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < 3 * n; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e / n);
    const size_t r = e - (size_t)c * n;
    const int k = (int)(r / M), l = (int)(r - (size_t)k * M);
    const double fx = ((double)((k + M / 2) % M) - mid) * fs, fy = ((double)((l + M / 2) % M) - mid) * fs;
    double sn, cs;
    sincospi(-d * (c == 0 ? l0 : c == 1 ? l1 : l2) * (fx * fx + fy * fy), &sn, &cs);
    H[e] = make_float2((float)(cs * inv), (float)(sn * inv));
  }
}

// out [3][n] = exp(i (kc[c] h + off_c)), h = x^2 (squared) or x;  EX: x + eps in place of x under the square, off [3][n] or NULL
template <bool EX>
__global__ void k_doe_phase(const float* __restrict__ x, int squared, float kc0, float kc1, float kc2, float2* __restrict__ out, size_t n, float eps,
                            const float* __restrict__ off) {
  const float kc[3] = {kc0, kc1, kc2};
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float v = (EX && squared) ? x[e] + eps : x[e], h = squared ? v * v : v;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float sn, cs;
      float ph = kc[c] * h;
      if (EX && off) ph += off[(size_t)c * n + e];
      sincosf(ph, &sn, &cs);
      out[(size_t)c * n + e] = make_float2(cs, sn);
    }
  }
}

// the backward of k_doe_phase: gx = sum_c kc[c] Im(conj(out_c) g_c), times 2 (x + eps) when squared; out is recomputed
__global__ void k_doe_phase_bwd(const float2* __restrict__ g, const float* __restrict__ x, int squared, float kc0, float kc1, float kc2,
                                float* __restrict__ gx, size_t n, float eps, const float* __restrict__ off) {
  const float kc[3] = {kc0, kc1, kc2};
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float v = squared ? x[e] + eps : x[e], h = squared ? v * v : v;
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float sn, cs;
      float ph = kc[c] * h;
      if (off) ph += off[(size_t)c * n + e];
      sincosf(ph, &sn, &cs);
      const float2 gc = g[(size_t)c * n + e];
      t = fmaf(kc[c], fmaf(cs, gc.y, -sn * gc.x), t);
    }
    gx[e] = squared ? 2.f * v * t : t;
  }
}

// PERCH: n values per channel, channel c divided by stat[2 c] (its own sum); otherwise all of them by stat[0]
template <bool PERCH>
__global__ void k_doe_normalise(float* __restrict__ psf, const double* __restrict__ stat, size_t n) {
  const double inv = 1.0 / stat[PERCH ? 2 * blockIdx.y : 0];
  float* p = psf + (size_t)blockIdx.y * n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) p[e] = (float)((double)p[e] * inv);
}

// stat[1] = <g, psf>: per-workgroup partials in float64, added by the last workgroup.  A grid of (blocks, 3) takes n values per
// channel and leaves stat[2 c + 1] = <g_c, psf_c>: each channel's partials are consecutive and added in the same fixed order.
__global__ void __launch_bounds__(DOE_THREADS) k_doe_dot(const float* __restrict__ g, const float* __restrict__ psf, size_t n, double* __restrict__ partial,
                                                         unsigned* __restrict__ counter, double* __restrict__ stat) {
  __shared__ double shred[DOE_THREADS / 64];
  __shared__ int shlast;
  double acc = 0.0;
  const size_t base = (size_t)blockIdx.y * n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) acc += (double)g[base + e] * (double)psf[base + e];
  acc = block_sum(acc, shred);
  if (threadIdx.x == 0) dpx_st_agent(partial + blockIdx.y * gridDim.x + blockIdx.x, acc);
  if (!dpx_last_block(counter, gridDim.x * gridDim.y, &shlast)) return;
  if (threadIdx.x < 64) {
    for (int c = 0; c < (int)gridDim.y; ++c) {
      const double t = sum_partials_f64(partial + c * gridDim.x, (int)gridDim.x);
      if (threadIdx.x == 0) stat[2 * c + 1] = t;
    }
  }
}

int dot_blocks(int P) { return grid_for(3L * P * P, DOE_THREADS, 512); }
int dot_blocks_channel(int P) { return grid_for((long)P * P, DOE_THREADS, 170); }       // (three of them <= dot_blocks' cap)

// workspace: tickets (2) | stat (sum q, <g, psf>; per channel: sum q_c at 2 c, <g_c, psf_c> at 2 c + 1) | partial sums | Z [3][R][M] |
// w [3][R][R] (keep_field)
struct DoeWs {
  unsigned* tickets;
  double* stat;
  double* partial;
  float2* Z;
  float2* w;
  size_t bytes;
};
DoeWs doe_ws(void* ws, int R, int P, int keep_field) {
  const int M = R + 2 * (R / 4);
  const int rb = doe_rows_out_blocks(R, R / P), db = dot_blocks(P), dc = 3 * dot_blocks_channel(P);
  const size_t npart = (size_t)(rb > db ? (rb > dc ? rb : dc) : (db > dc ? db : dc));
  char* b = (char*)ws;
  DoeWs W;
  size_t off = 0;
  W.tickets = (unsigned*)(b + off);
  off += ticket_bytes(2);
  W.stat = (double*)(b + off);
  off += 256;
  W.partial = (double*)(b + off);
  off += (npart * sizeof(double) + 255) & ~(size_t)255;
  W.Z = (float2*)(b + off);
  off += ((size_t)3 * R * M * sizeof(float2) + 255) & ~(size_t)255;
  W.w = keep_field ? (float2*)(b + off) : nullptr;
  if (keep_field) off += (size_t)3 * R * R * sizeof(float2);
  W.bytes = off;
  return W;
}

bool doe_shape_ok(const char* who, int R, int P) {
  if (R < 4 || P < 1 || R % P != 0) return set_error("%s: wavefront R=%d, psf P=%d (R >= 4, P >= 1 dividing R)", who, R, P), false;
  if (!doe_fits(R, R / P))
    return set_error("%s: R=%d, P=%d: a padded row of %d samples (times the %d rows of a block) is beyond the LDS-resident transforms", who, R, P,
                     R + 2 * (R / 4), R / P),
           false;
  return true;
}
bool doe_cols_ok(const char* who, int R, int cols_per_wg) {
  if (cols_per_wg < 0 || cols_per_wg > doe_cols_widest(R))
    return set_error("%s: cols_per_wg=%d (0 = the library's choice, or 1 .. %d at R=%d)", who, cols_per_wg, doe_cols_widest(R), R), false;
  return true;
}
void doe_kc(const double* wave_lengths, const double* refractive_idcs, float* kc) {
  for (int c = 0; c < 3; ++c) kc[c] = (float)(2.0 * 3.14159265358979323846 / wave_lengths[c] * (refractive_idcs[c] - 1.0));
}
bool doe_optics_ok(const char* who, const double* wave_lengths, const double* refractive_idcs) {
  if (!wave_lengths || !refractive_idcs) return set_error("%s: null pointer (wave lengths / refractive indices: 3 host doubles each)", who), false;
  for (int c = 0; c < 3; ++c)
    if (!(wave_lengths[c] > 0.0)) return set_error("%s: wave length %d is %g (positive)", who, c, wave_lengths[c]), false;
  return true;
}

}  // namespace
}  // namespace dpx

using namespace dpx;

extern "C" size_t dpx_doe_propagator_bytes(int R) {
  if (R < 4) return 0;
  const size_t M = (size_t)R + 2 * (R / 4);
  return 3 * M * M * sizeof(float2);
}

extern "C" int dpx_doe_propagator_init(void* H, int R, double distance, double sample_interval, const double* wave_lengths, dpx_stream_t stream) {
  DPX_REQUIRE(H, "dpx_doe_propagator_init: null pointer");
  DPX_REQUIRE(R >= 4, "dpx_doe_propagator_init: R=%d (at least 4)", R);
  DPX_REQUIRE(sample_interval > 0.0, "dpx_doe_propagator_init: sample interval %g (positive)", sample_interval);
  DPX_REQUIRE(wave_lengths, "dpx_doe_propagator_init: null pointer (wave lengths: 3 host doubles)");
  const int M = R + 2 * (R / 4);
  DPX_LAUNCH("k_doe_propagator", k_doe_propagator, dim3(grid_for(3L * M * M, DOE_THREADS)), dim3(DOE_THREADS), 0, (hipStream_t)stream, (float2*)H, M,
             distance, sample_interval, wave_lengths[0], wave_lengths[1], wave_lengths[2]);
  return launch_status("dpx_doe_propagator_init");
}

extern "C" size_t dpx_doe_ws_bytes(int R, int P, int keep_field) {
  if (!doe_shape_ok("dpx_doe_ws_bytes", R, P)) return 0;
  return doe_ws(nullptr, R, P, keep_field).bytes;
}

extern "C" int dpx_doe_cols_per_wg(int R, int widest) {
  if (R < 4 || !doe_fits(R, 1)) return 0;
  return widest ? doe_cols_widest(R) : doe_cols_default(R);
}

namespace dpx {
namespace {
bool doe_opts_ok(const char* who, const dpx_doe_opts* o) {
  if (!o) return true;
  if (o->aperture_kind != 0 && o->aperture_kind != 1)
    return set_error("%s: aperture_kind=%d (0 = circular, 1 = half-circular)", who, o->aperture_kind), false;
  if (o->norm_mode != 0 && o->norm_mode != 1) return set_error("%s: norm_mode=%d (0 = one sum over all channels, 1 = one per channel)", who, o->norm_mode), false;
  if (!(o->eps >= 0.f)) return set_error("%s: eps=%g (non-negative)", who, (double)o->eps), false;
  return true;
}
DoeEx doe_ex(const dpx_doe_opts* o) {
  DoeEx E;
  if (o) E.phi = o->phi, E.eps = o->eps, E.kind = o->aperture_kind, E.norm = o->norm_mode;
  return E;
}
}  // namespace
}  // namespace dpx

extern "C" int dpx_doe_psf_ex(const float* s, const void* phase_profile, const double* wave_lengths, const double* refractive_idcs, float* psf,
                              const void* H, const void* table, int R, int P, int keep_field, int cols_per_wg, const dpx_doe_opts* opts, void* ws,
                              dpx_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  DPX_REQUIRE((s || phase_profile) && psf && H && table && ws, "dpx_doe_psf: null pointer");
  if (!doe_shape_ok("dpx_doe_psf", R, P) || !doe_cols_ok("dpx_doe_psf", R, cols_per_wg) || !doe_opts_ok("dpx_doe_psf", opts)) return DPX_ERR_ARG;
  float kc[3] = {0.f, 0.f, 0.f};
  if (!phase_profile) {
    if (!doe_optics_ok("dpx_doe_psf", wave_lengths, refractive_idcs)) return DPX_ERR_ARG;
    doe_kc(wave_lengths, refractive_idcs, kc);
  }
  const DoeEx E = doe_ex(opts);
  const DoeWs W = doe_ws(ws, R, P, keep_field);
  const int f = R / P, ct = cols_per_wg ? cols_per_wg : doe_cols_default(R);
  DPX_REQUIRE(hipMemsetAsync(W.tickets, 0, ticket_bytes(2), st) == hipSuccess, "dpx_doe_psf: zero fill failed");
  int rc = doe_rows_in(phase_profile ? 1 : 0, s, (const float2*)phase_profile, nullptr, nullptr, kc, 1, W.Z, R, f, table, st, E);
  if (rc == DPX_OK) rc = doe_cols(W.Z, (const float2*)H, 0, R, ct, table, st);
  if (rc == DPX_OK) rc = doe_rows_out(W.Z, W.w, psf, W.partial, W.tickets, W.stat, R, f, table, st, E.norm);
  if (rc != DPX_OK) return rc;
  if (E.norm) {
    const size_t n = (size_t)P * P;
    DPX_LAUNCH("k_doe_normalise", k_doe_normalise<true>, dim3(grid_for((long)n, DOE_THREADS), 3), dim3(DOE_THREADS), 0, st, psf, (const double*)W.stat, n);
  } else {
    const size_t n = (size_t)3 * P * P;
    DPX_LAUNCH("k_doe_normalise", k_doe_normalise<false>, dim3(grid_for((long)n, DOE_THREADS)), dim3(DOE_THREADS), 0, st, psf, (const double*)W.stat, n);
  }
  return launch_status("dpx_doe_psf");
}

extern "C" int dpx_doe_psf(const float* s, const void* phase_profile, const double* wave_lengths, const double* refractive_idcs, float* psf,
                           const void* H, const void* table, int R, int P, int keep_field, int cols_per_wg, void* ws, dpx_stream_t stream) {
  DPX_REQUIRE(!(keep_field && phase_profile), "dpx_doe_psf: keep_field with an explicit phase profile (dpx_doe_psf_ex keeps its field)");
  return dpx_doe_psf_ex(s, phase_profile, wave_lengths, refractive_idcs, psf, H, table, R, P, keep_field, cols_per_wg, nullptr, ws, stream);
}

extern "C" int dpx_doe_psf_backward_ex(const float* g, const float* psf, const float* s, const double* wave_lengths, const double* refractive_idcs,
                                       const void* H, const void* table, int R, int P, int cols_per_wg, const dpx_doe_opts* opts, void* ws,
                                       dpx_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  DPX_REQUIRE(opts, "dpx_doe_psf_backward: null pointer (the options block names the output)");
  float* gs = opts->gs;
  float2* gf = (float2*)opts->g_field;
  DPX_REQUIRE(g && psf && H && table && ws && (gs || gf), "dpx_doe_psf_backward: null pointer");
  DPX_REQUIRE(!(gs && gf), "dpx_doe_psf_backward: both gs and g_field (one output: the gradient to s, or to an explicit phase profile)");
  DPX_REQUIRE(!gs || s, "dpx_doe_psf_backward: null pointer");
  DPX_REQUIRE(!gs || gs != s, "dpx_doe_psf_backward: the gradient must not be an input (no in-place call)");
  if (!doe_shape_ok("dpx_doe_psf_backward", R, P) || !doe_cols_ok("dpx_doe_psf_backward", R, cols_per_wg) || !doe_opts_ok("dpx_doe_psf_backward", opts))
    return DPX_ERR_ARG;
  float kc[3] = {0.f, 0.f, 0.f};
  if (gs) {
    if (!doe_optics_ok("dpx_doe_psf_backward", wave_lengths, refractive_idcs)) return DPX_ERR_ARG;
    doe_kc(wave_lengths, refractive_idcs, kc);
  }
  const DoeEx E = doe_ex(opts);
  const DoeWs W = doe_ws(ws, R, P, 1);                   // (the workspace of the dpx_doe_psf call with keep_field = 1: its w and sum q)
  const int f = R / P, ct = cols_per_wg ? cols_per_wg : doe_cols_default(R);
  DPX_REQUIRE(hipMemsetAsync(W.tickets, 0, ticket_bytes(2), st) == hipSuccess, "dpx_doe_psf_backward: zero fill failed");
  if (E.norm)
    DPX_LAUNCH("k_doe_dot", k_doe_dot, dim3(dot_blocks_channel(P), 3), dim3(DOE_THREADS), 0, st, g, psf, (size_t)P * P, W.partial, W.tickets + 1, W.stat);
  else
    DPX_LAUNCH("k_doe_dot", k_doe_dot, dim3(dot_blocks(P)), dim3(DOE_THREADS), 0, st, g, psf, (size_t)3 * P * P, W.partial, W.tickets + 1, W.stat);
  int rc = launch_status("dpx_doe_psf_backward");
  if (rc == DPX_OK) rc = doe_rows_in(2, nullptr, W.w, g, W.stat, nullptr, 0, W.Z, R, f, table, st, E);
  if (rc == DPX_OK) rc = doe_cols(W.Z, (const float2*)H, 1, R, ct, table, st);
  if (rc == DPX_OK) rc = gs ? doe_rows_grad(W.Z, s, gs, kc, R, table, st, E) : doe_rows_grad_field(W.Z, gf, 1, E.kind, R, table, st);
  return rc;
}

extern "C" int dpx_doe_psf_backward(const float* g, const float* psf, const float* s, const double* wave_lengths, const double* refractive_idcs,
                                    float* gs, const void* H, const void* table, int R, int P, int cols_per_wg, void* ws, dpx_stream_t stream) {
  DPX_REQUIRE(g && psf && s && gs && H && table && ws, "dpx_doe_psf_backward: null pointer");
  dpx_doe_opts o{};
  o.gs = gs;
  return dpx_doe_psf_backward_ex(g, psf, s, wave_lengths, refractive_idcs, H, table, R, P, cols_per_wg, &o, ws, stream);
}

extern "C" int dpx_doe_propagate(const void* field, void* out, const void* H, const void* table, int R, int cols_per_wg, void* ws,
                                 dpx_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  DPX_REQUIRE(field && out && H && table && ws, "dpx_doe_propagate: null pointer");
  if (!doe_shape_ok("dpx_doe_propagate", R, R) || !doe_cols_ok("dpx_doe_propagate", R, cols_per_wg)) return DPX_ERR_ARG;
  const DoeWs W = doe_ws(ws, R, R, 0);                   // (dpx_doe_ws_bytes(R, R, 0))
  const int ct = cols_per_wg ? cols_per_wg : doe_cols_default(R);
  int rc = doe_rows_in(1, nullptr, (const float2*)field, nullptr, nullptr, nullptr, 0, W.Z, R, 1, table, st);
  if (rc == DPX_OK) rc = doe_cols(W.Z, (const float2*)H, 0, R, ct, table, st);
  if (rc == DPX_OK) rc = doe_rows_out(W.Z, (float2*)out, nullptr, nullptr, nullptr, nullptr, R, 1, table, st);
  return rc;
}

extern "C" int dpx_doe_propagate_backward(const void* g_out, void* g_field, const void* H, const void* table, int R, int cols_per_wg, void* ws,
                                          dpx_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  DPX_REQUIRE(g_out && g_field && H && table && ws, "dpx_doe_propagate_backward: null pointer");
  DPX_REQUIRE(g_out != g_field, "dpx_doe_propagate_backward: the gradient must not be an input (no in-place call)");
  if (!doe_shape_ok("dpx_doe_propagate_backward", R, R) || !doe_cols_ok("dpx_doe_propagate_backward", R, cols_per_wg)) return DPX_ERR_ARG;
  const DoeWs W = doe_ws(ws, R, R, 0);                   // (dpx_doe_ws_bytes(R, R, 0))
  const int ct = cols_per_wg ? cols_per_wg : doe_cols_default(R);
  int rc = doe_rows_in(1, nullptr, (const float2*)g_out, nullptr, nullptr, nullptr, 0, W.Z, R, 1, table, st);
  if (rc == DPX_OK) rc = doe_cols(W.Z, (const float2*)H, 1, R, ct, table, st);
  if (rc == DPX_OK) rc = doe_rows_grad_field(W.Z, (float2*)g_field, 0, 0, R, table, st);
  return rc;
}

extern "C" int dpx_doe_phase_ex(const float* x, int squared, float eps, const float* offset, const double* wave_lengths, const double* refractive_idcs,
                                void* out, long n, dpx_stream_t stream) {
  DPX_REQUIRE(x && out, "dpx_doe_phase: null pointer");
  DPX_REQUIRE(n >= 1, "dpx_doe_phase: n=%ld (at least 1)", n);
  DPX_REQUIRE(eps >= 0.f, "dpx_doe_phase: eps=%g (non-negative)", (double)eps);
  if (!doe_optics_ok("dpx_doe_phase", wave_lengths, refractive_idcs)) return DPX_ERR_ARG;
  float kc[3];
  doe_kc(wave_lengths, refractive_idcs, kc);
  const dim3 grid(grid_for(n, DOE_THREADS));
  if (eps != 0.f || offset)
    DPX_LAUNCH("k_doe_phase", k_doe_phase<true>, grid, dim3(DOE_THREADS), 0, (hipStream_t)stream, x, squared, kc[0], kc[1], kc[2], (float2*)out, (size_t)n,
               eps, offset);
  else
    DPX_LAUNCH("k_doe_phase", k_doe_phase<false>, grid, dim3(DOE_THREADS), 0, (hipStream_t)stream, x, squared, kc[0], kc[1], kc[2], (float2*)out,
               (size_t)n, 0.f, (const float*)nullptr);
  return launch_status("dpx_doe_phase");
}

extern "C" int dpx_doe_phase(const float* x, int squared, const double* wave_lengths, const double* refractive_idcs, void* out, long n,
                             dpx_stream_t stream) {
  return dpx_doe_phase_ex(x, squared, 0.f, nullptr, wave_lengths, refractive_idcs, out, n, stream);
}

extern "C" int dpx_doe_phase_backward(const void* g, const float* x, int squared, float eps, const float* offset, const double* wave_lengths,
                                      const double* refractive_idcs, float* gx, long n, dpx_stream_t stream) {
  DPX_REQUIRE(g && x && gx, "dpx_doe_phase_backward: null pointer");
  DPX_REQUIRE(gx != x, "dpx_doe_phase_backward: the gradient must not be an input (no in-place call)");
  DPX_REQUIRE(n >= 1, "dpx_doe_phase_backward: n=%ld (at least 1)", n);
  DPX_REQUIRE(eps >= 0.f, "dpx_doe_phase_backward: eps=%g (non-negative)", (double)eps);
  if (!doe_optics_ok("dpx_doe_phase_backward", wave_lengths, refractive_idcs)) return DPX_ERR_ARG;
  float kc[3];
  doe_kc(wave_lengths, refractive_idcs, kc);
  DPX_LAUNCH("k_doe_phase_bwd", k_doe_phase_bwd, dim3(grid_for(n, DOE_THREADS)), dim3(DOE_THREADS), 0, (hipStream_t)stream, (const float2*)g, x, squared,
             kc[0], kc[1], kc[2], gx, (size_t)n, eps, offset);
  return launch_status("dpx_doe_phase_backward");
}
