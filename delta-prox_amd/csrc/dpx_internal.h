// Every function of namespace dpx that one .hip file defines and another one calls, declared ONCE: dpx_common.h includes this header
// at its end, so the defining file sees the declaration too and the compiler checks the definition against it (return type, default
// arguments).  A function with one user file is `static` in that file and is not listed here (tests/test_host_logic.py holds both).
#pragma once

namespace dpx {

struct IterTerms;      // dpx_iter_dev.h
struct BwdRowTerms;    // dpx_bwd_dev.h

// ---- dpx_autodiff.hip: stages of the unrolled backward pass ------------------------------------------------
int ad_partial_blocks(int C, int H, int W);
// the stage kernels of the unrolled backward pass without their finishing launches: partial sums [rows][nblk] into `part`
int zupdate_bwd_partials(float* gx, const dpx_bwd_term* terms, int nterms, float* part, int hist_bf16, int B, int C, int H, int W, hipStream_t s);
int solve_rhs_bwd_partials(const float* g, const float* x, const float* rhs, const float* rho, const int* linops, int nterms, float* const* gv,
                           float* const* gu, const float* const* gu_add, float* part_a, float* part_b, int hist_bf16, int B, int C, int H, int W,
                           hipStream_t s);
// glam == NULL: only the rho reductions; grho == NULL: only the lambda reductions; nblk: partial sums per row
int finish_iter_n(const float* part_lam, const float* part_a, const float* part_b, float* glam, float* grho, const float* rho, int nterms, int B,
                  int nblk, hipStream_t s);
int finish_all(const float* part, long stride, float* glam, float* grho, const float* rho_tab, int nterms, int B, int nblk, int T, int nst,
               hipStream_t s);
int finish_iter(const float* part_lam, const float* part_a, const float* part_b, float* glam, float* grho, const float* rho, int nterms, int B,
                int C, int H, int W, hipStream_t s);
// rhs stage of iteration `it` + z stage of iteration `it - 1` (k_rhs_z_bwd4); false: the planes do not fit it (staged_vec: W % 4 or alignment)
bool rhs_z_bwd_fused(const float* g, const float* x, const float* rhs, const float* rho, const dpx_bwd_term* terms, int nterms, const float* const* a_in,
                     float* const* a_out, float* gx, float* part_a, float* part_b, float* part_lam, int hist_bf16, int B, int C, int H, int W,
                     hipStream_t s, unsigned* counter, float* glam, float* grho);

// ---- dpx_bwd_rows.hip: the row half of one backward iteration ----------------------------------------------
// workgroups (= partial-sum slots) per image of the launch below; 0: planes this kernel does not take
int bwd_rows_slots(int B, int C, int H, int W, int max_slots);
// One backward iteration's row half.  spec_in: the column kernel's output (g_rhs^ of iteration t); spec_out: the row transform of g_x.
// x / rhs: history of iteration t; terms[i].v / lam: iteration t - 1; partial sums as bwd_rows_slots(...) slots per image.
int bwd_rows_fused(const void* spec_in, void* spec_out, const float* x, const float* rhs, const float* rho, const dpx_bwd_term* terms, int nterms,
                   const float* const* a_in, float* const* a_out, float* g_out, int g_acc, float* part_a, float* part_b, float* part_lam, int hist_bf16,
                   int B, int C, int H, int W, const void* table, hipStream_t s);

// ---- dpx_bwd_rows_par.hip: its row-parallel kernel ---------------------------------------------------------
// own rows per workgroup (0: the lock-step kernel keeps the launch): launches of up to `unroll_bwd_par_max_rows` rows (planes x H; the
// library's rule: 12288 -- config 5's twelve 512-row planes in one round of 16-wave workgroups), knob < 0 = never
int bwd_rows_par_own(int P, int H, int W);
int bwd_rows_par_launch(const float2* sin, float2* sout, const BwdRowTerms& TT, const float* rho, float* part_a, float* part_b, float* part_lam, int B,
                        int C, int H, int W, int bands, const float2* twW, hipStream_t s);

// ---- dpx_conv_bf16.hip -------------------------------------------------------------------------------------
// device address of the split-f16 overflow word, for the kernels of other translation units, which receive it as an argument
unsigned* f16_overflow_flag();

// ---- dpx_elementwise.hip -----------------------------------------------------------------------------------
// Gram pass + finish + stop rule in one launch (dpx_cg_masked_fft's fused iteration, B <= 32); ws: B * B * gram_blocks floats
// x / p / Ap non-null: the pending update x += alpha p, r -= alpha A p of the previous iteration is applied on the way (r is written)
int gram_test_fused(float* r, float* G, void* state, int B, long n_per_batch, void* ws, unsigned* counter, float init_rtol, float* x, const float* p,
                    const float* Ap, int* host_flags, int host_tag, hipStream_t s);

// ---- dpx_fft.hip: the masked-Fourier normal operator of dpx_cg_masked_fft ----------------------------------
// does a plane fit the LDS-resident transforms of masked_normal_apply?
bool masked_normal_fits(int H, int W);
// z: one complex [B][H][W] scratch plane set.  Returns DPX_ERR_UNSUPPORTED for planes beyond the LDS-resident transform.
int masked_normal_apply(const float* p, float* Ap, float2* z, const float* mask2, int mask_images, const float* rho, float c, const int* done,
                        int B, int H, int W, const void* table, hipStream_t s);
size_t masked_normal_fused_ws_floats(int B, int H, int W);      // (one partial per workgroup; at most one workgroup per row)
// The matvec of dpx_cg_masked_fft's fused iteration: masked_normal_apply's three launches with the CG direction update in front (p = r +
// beta p formed in the first kernel's load) and <p, Ap> behind (partial sums in the last kernel's store, finished by its last workgroup
// into the CG state).  `mask` is the mask itself (squared on the fly).  dotws: masked_normal_fused_ws_floats floats.
int masked_normal_apply_fused(float* p, const float* r, float* Ap, float2* z, const float* mask, int mask_images, const float* rho, float c,
                              float* state, float* dotws, unsigned* counter, int B, int H, int W, const void* table, hipStream_t s);

// ---- dpx_fft.hip: the Fresnel propagator of the DOE model (dpx_doe.hip), w = crop(F^-1(H . F(zero-pad(u)))) -----------------
// A wavefront of R x R samples padded by R / 4 on every side, three wavelengths, on a compact spectrum Z [3][R][R + 2 (R / 4)] complex.
bool doe_fits(int R, int f);                // every kernel's workgroup fits a CU's LDS (f: side of the psf's averaging block, divides R)
int doe_cols_widest(int R);                 // the most columns a column workgroup holds
int doe_cols_default(int R);                // ... and the number the library launches with (one: measured)
int doe_rows_out_blocks(int R, int f);      // workgroups of doe_rows_out = partial sums it hands to its last workgroup
// mode 0: u_c = a exp(i kc[c] sq^2) from the height map's square root sq [R][R]; 1: `field` [3][R][R] (times the aperture a if asked);
// 2: the backward pass's g_w from field = w, the psf's cotangent g [3][R / f][R / f] and stat = (sum q, <g, psf>).  kc: host, 3 values
// E: the hybrid model's generalisation -- u_c = a exp(i (kc[c] (sq + eps)^2 + phi_c)) with phi [3][R][R] (nullable), the aperture kind
// (0: the disc, 1: its right half, which mode 1's `aperture` follows too) and, in mode 2, one normalisation per channel (norm = 1:
// stat[2 c] = sum q_c, stat[2 c + 1] = <g_c, psf_c>).  The defaults launch the base model's kernels.
struct DoeEx {
  const float* phi = nullptr;
  float eps = 0.f;
  int kind = 0;
  int norm = 0;
};
int doe_rows_in(int mode, const float* sq, const float2* field, const float* g, const double* stat, const float* kc, int aperture, float2* Z, int R,
                int f, const void* table, hipStream_t s, const DoeEx& E = DoeEx());
// H: [3][M][M] with the inverse transforms' 1 / M^2 folded in; conj: multiply by its conjugate; ct: columns per workgroup
int doe_cols(float2* Z, const float2* H, int conj, int R, int ct, const void* table, hipStream_t s);
// w [3][R][R] (nullable) = the propagated field; q [3][R / f][R / f] (nullable) = block mean of |w|^2, stat[0] = its sum (partial:
// doe_rows_out_blocks doubles, counter: one zeroed ticket); perch: stat[2 c] = the sum of channel c instead
int doe_rows_out(const float2* Z, float2* w, float* q, double* partial, unsigned* counter, double* stat, int R, int f, const void* table,
                 hipStream_t s, int perch = 0);
// gs [R][R] = 2 (sq + eps) sum_c kc[c] Im(conj(u_c) g_u_c) on the aperture, 0 outside
int doe_rows_grad(const float2* Z, const float* sq, float* gs, const float* kc, int R, const void* table, hipStream_t s, const DoeEx& E = DoeEx());
// g_field [3][R][R] = the cotangent g_u itself (dL/dRe + i dL/dIm), times the aperture of `kind` if asked
int doe_rows_grad_field(const float2* Z, float2* g_field, int aperture, int kind, int R, const void* table, hipStream_t s);

// ---- dpx_fft_pow2.hip: transforms of the power-of-two planes (pow2_path_available) -------------------------
size_t pow2_spec_elems(int P, int H, int W);
int seed_rows_pow2(const dpx_term* terms, int nterms, const float* rho, const float* x0, float2* spec, int B, int C, int H, int W, const void* table,
                   hipStream_t stream);
int cols_solve_pow2(const float2* spec_in, float2* spec_out, const SpecArgs& A, int P, int C, int H, int W, const void* table, hipStream_t stream);
int rows_r2c_pow2(const float* x, float2* spec, int P, int H, int W, const void* table, hipStream_t stream);
int rows_c2r_pow2(const float2* spec, float* y, int P, int H, int W, const void* table, hipStream_t stream);
int spectral_apply_pow2(const float* x, float* y, int op, const SpecArgs& A, int B, int C, int H, int W, const void* table, void* ws,
                        hipStream_t stream);

// ---- dpx_iter.hip: the streaming row passes ----------------------------------------------------------------
// false: the plane / batch does not fit the streaming kernel (the caller keeps k_pgd_rows, which serves every plane)
bool pgd_rows_seq_pow2(const float2* sin, float2* sout, float* x, const float* ktb, const float* rho, const float* lam, float alpha, int prox, int P,
                       int C, int H, int W, const void* table, hipStream_t s);
// false: the plane / batch does not fit the streaming kernel (the caller keeps k_seed_rows<FRESH>)
bool seed_rows_seq_pow2(const int* linops, int n, const float* rho, const float* x0, float2* spec, int P, int C, int H, int W, const void* table,
                        hipStream_t s);
// dpx_admm_iter_rows + rhs_out (nullable): the right-hand-side increment handed to the next x-update, also written as an image;
// + emit_bf16: x_out, terms[i].v and rhs_out are bf16 planes (written with round-to-nearest-even)
int iter_rows_impl(const void* spec_in, void* spec_out, const dpx_term* terms, int nterms, const float* rho_next, float* x_out, int emit_v,
                   float* rhs_out, int emit_bf16, int B, int C, int H, int W, const void* table, dpx_stream_t stream);

// ---- dpx_iter_par.hip --------------------------------------------------------------------------------------
// Row-parallel kernel for launches that cannot fill the chip with band walkers: P * H rows up to `iter_par_max_rows` (knob; the
// library's rule: 8192 rows of 1024 / 512 / 256 pixels -- 1 .. 2 rounds of one 16-wave workgroup per CU), or forced (iter_rows = 3).
// false: not applicable -- the caller keeps the streaming kernel
bool launch_iter_rows_par(const float2* sin, float2* sout, const IterTerms& TT, const float* rho_next, float* x_out, int emit_v, int C, int H, int W,
                          int P, const float2* twW, hipStream_t s, bool forced);

// ---- dpx_wgrad_c8.hip: weight / bias gradients of the split-arithmetic convolutions ------------------------
size_t wgrad_c8_ws_floats(int cout_max, int cin_max);
// G: C8 [B][Gg][H][W][8], A: C8 [B][Ga][H][W][8]; gw: [Cout][Cin_w][9], gb: [Cout] (Cout <= 8 Gg, Cin_w <= 8 Ga, both <= 96);
// mode 3: split-f16 (G scaled into the binary16 range by the caller), 6: split-bf16; mul (device, nullable): the sums leave multiplied by *mul
void launch_wgrad_c8(int mode, const float* G, const float* A, float* gw, float* gb, int Cout, int Cin_w, int Gg, int Ga, int B, int H, int W,
                     float* ws, const float* mul, hipStream_t s);

}  // namespace dpx
