// Non-local means on the luminance patch distance (patch_nlm prior): the reference's NonLocalMeansFast,
// dprox/proxfn/nlm/nlm.py:8-27, in one launch without its [N, C, H, W, S^2] shift stacks.
//
//   y       = 0.299 R + 0.587 G + 0.114 B                      (C = 3; C = 1: the plane itself)
//   D_s(p)  = sum_{o in [-rp, rp]^2} (y(p - o) - y(p - o - s))^2 ,  s in [-rs, rs]^2, indices circular (torch.roll)
//   w_s(p)  = exp(-sqrt(D_s(p)) / (relu(2 sigma) + 1e-6))
//   out(p)  = clamp(sum_s w_s(p) v(p - s) / sum_s w_s(p), 0, 1)
//
// A workgroup (4 waves) owns a tile of 64 - 2 rp columns x 4 R rows of one image.  It stages the tile's luminance with a halo of
// rs + rp and its colour planes with a halo of rs in LDS (the circular wrap applied while loading), once.  Lanes lie along x, lane l
// at column x0 - rp + l, and every lane owns a column of R outputs of its wave's R rows; the 2 rp lanes at the wave's edges only
// supply column sums to their neighbours.  Per horizontal shift dx a lane reads its shifted luminance column (R + 2 rp + 2 rs values)
// and colour columns (R + 2 rs values each) from LDS into registers once; every vertical shift dy then runs on registers: d^2 over
// the column, the vertical patch sums (direct sums of non-negative terms: no running-sum cancellation before the square root), the
// horizontal patch sum from the neighbouring lanes (DPP wave shifts), the weight as exp2 with -log2(e) / (h + eps) folded into one
// per-image constant (split into two floats), and the accumulation.  No barrier inside the shift loop; shifts are summed in one fixed order (dx ascending,
// dy descending), so a call is bit-reproducible.
//
// Instantiations: the reference's windows (11, 5) with R = 8 and every loop bound a constant; any odd search window 3 .. 21 and odd
// patch 1 .. 9 through one generic kernel (R = 4, register arrays sized for the largest windows, uniform guards on the runtime bounds).
#include "dpx_common.h"

namespace dpx {
namespace {

constexpr int NLM_THREADS = 256;          // 4 waves along y
constexpr double NLM_LOG2E = 1.4426950408889634;

__device__ __forceinline__ int nlm_wrap(int i, int n) {
  i %= n;
  return i < 0 ? i + n : i;
}

// the reference's luminance: three fp32 products summed left to right, nothing contracted (nlm.py:104)
__device__ __forceinline__ float nlm_luma(float r, float g, float b) {
#pragma clang fp contract(off)
  const float rg = 0.299f * r + 0.587f * g;
  return rg + 0.114f * b;
}

// value of lane - 1 / lane + 1 (whole-wave DPP shifts; the edge lanes get their own value back and are never outputs)
__device__ __forceinline__ float nlm_from_left(float v) {
#ifdef DPX_EMULATED
  return __shfl_up(v, 1);
#else
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138, 0xF, 0xF, false));   // wave_shr:1
#endif
}
__device__ __forceinline__ float nlm_from_right(float v) {
#ifdef DPX_EMULATED
  return __shfl_down(v, 1);
#else
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x130, 0xF, 0xF, false));   // wave_shl:1
#endif
}

// exp(-sqrt(D) / den) as exp2(sqrt(D) k), k = -log2(e) / den carried as khi + klo: the exponent is the product to within an ulp
// (one rounded fp32 k would add |exponent| x 2^-24 of relative error to every weight)
__device__ __forceinline__ float nlm_weight(float D, float khi, float klo) {
#ifdef DPX_EMULATED
  const float s = sqrtf(D);
  return exp2f(fmaf(s, khi, s * klo));
#else
  const float s = __builtin_amdgcn_sqrtf(D);
  return __builtin_amdgcn_exp2f(fmaf(s, khi, s * klo));
#endif
}

// C: 1 or 3 channels; R: output rows per lane; RSM / RPM: search / patch radius (FIXED) or the largest the arrays hold (generic)
template <int C, int R, int RSM, int RPM, bool FIXED>
__global__ __launch_bounds__(NLM_THREADS) void k_nlm(const float* __restrict__ v, float* __restrict__ out, const float* __restrict__ sigma,
                                                     int H, int W, int rs_arg, int rp_arg) {
  constexpr int LCM = 64 + 2 * RSM, LRM = 4 * R + 2 * (RSM + RPM), CRM = 4 * R + 2 * RSM;
  constexpr int YO = R + 2 * RPM, YS = R + 2 * RPM + 2 * RSM, CS = R + 2 * RSM;
  __shared__ float s_lum[LRM * LCM];
  __shared__ float s_col[C * CRM * LCM];
  const int rs = FIXED ? RSM : rs_arg, rp = FIXED ? RPM : rp_arg;
  const int LC = 64 + 2 * rs, LR = 4 * R + 2 * (rs + rp), CR = 4 * R + 2 * rs;
  const int b = blockIdx.z;
  const int xl0 = (int)blockIdx.x * (64 - 2 * rp) - rp;          // image column of lane 0
  const int y0 = (int)blockIdx.y * 4 * R;                          // first output row of the tile
  const size_t plane = (size_t)H * W;
  const float* vb = v + (size_t)b * C * plane;

  // ---- stage: luminance rows y0 - rs - rp .., colour rows y0 - rs .., columns xl0 - rs .. (wrapped) ----
  for (int i = threadIdx.x; i < LR * LC; i += NLM_THREADS) {
    const int rr = i / LC, cc = i - rr * LC;
    const size_t o = (size_t)nlm_wrap(y0 - rs - rp + rr, H) * W + nlm_wrap(xl0 - rs + cc, W);
    s_lum[rr * LC + cc] = C == 3 ? nlm_luma(vb[o], vb[plane + o], vb[2 * plane + o]) : vb[o];
  }
  for (int i = threadIdx.x; i < C * CR * LC; i += NLM_THREADS) {
    const int c = i / (CR * LC), j = i - c * CR * LC;
    const int rr = j / LC, cc = j - rr * LC;
    s_col[i] = vb[c * plane + (size_t)nlm_wrap(y0 - rs + rr, H) * W + nlm_wrap(xl0 - rs + cc, W)];
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wr = (threadIdx.x >> 6) * R;   // wr: the wave's first row within the tile
  float yo[YO];                                                      // own luminance, rows wr - rp ..
#pragma unroll
  for (int j = 0; j < YO; ++j)
    yo[j] = j < R + 2 * rp ? s_lum[(wr + j + rs) * LC + lane + rs] : 0.f;
  const float h = 2.f * sigma[b];
  const double k = -NLM_LOG2E / (double)(fmaxf(h, 0.f) + 1e-6f);     // (relu(h) + 1e-6 in fp32, as the reference forms it)
  const float khi = (float)k, klo = (float)(k - (double)khi);
  float acc[C][R], wsum[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    wsum[r] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c][r] = 0.f;
  }

#pragma unroll 1
  for (int dx = -rs; dx <= rs; ++dx) {
    const int col = lane + rs - dx;                                  // LDS column of image column (lane's) - dx
    float ys[YS], cs[C][CS];
#pragma unroll
    for (int m = 0; m < YS; ++m)
      ys[m] = m < R + 2 * rp + 2 * rs ? s_lum[(wr + m) * LC + col] : 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int m = 0; m < CS; ++m)
        cs[c][m] = m < R + 2 * rs ? s_col[(c * CR + wr + m) * LC + col] : 0.f;
    // e = rs - dy: the shifted luminance of own row j is ys[j + e], the shifted colour of output row r is cs[r + e]
#pragma unroll
    for (int e = 0; e <= 2 * RSM; ++e) {
      if (e > 2 * rs) continue;                                      // (uniform; a constant in the fixed instantiation)
      float d2[YO];
#pragma unroll
      for (int j = 0; j < YO; ++j) {
        const float d = yo[j] - ys[j + e];
        d2[j] = d * d;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float cv = d2[r];                                            // vertical patch sum of this lane's column
#pragma unroll
        for (int q = 1; q <= 2 * RPM; ++q)
          if (q <= 2 * rp) cv += d2[r + q];
        float D = cv, lt = cv, rt = cv;                              // + the 2 rp neighbouring columns
#pragma unroll
        for (int q = 1; q <= RPM; ++q)
          if (q <= rp) {
            lt = nlm_from_left(lt);
            rt = nlm_from_right(rt);
            D += lt + rt;
          }
        const float w = nlm_weight(D, khi, klo);
        wsum[r] += w;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c][r] = fmaf(w, cs[c][r + e], acc[c][r]);
      }
    }
  }

  const int x = xl0 + lane;
  if (lane < rp || lane >= 64 - rp || x >= W) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int y = y0 + wr + r;
    if (y >= H) break;
#pragma unroll
    for (int c = 0; c < C; ++c)
      out[((size_t)b * C + c) * plane + (size_t)y * W + x] = fminf(fmaxf(acc[c][r] / wsum[r], 0.f), 1.f);
  }
}

typedef void (*NlmKernel)(const float*, float*, const float*, int, int, int, int);

template <int C> NlmKernel nlm_kernel(bool fixed) {
  return fixed ? k_nlm<C, 8, 5, 2, true> : k_nlm<C, 4, 10, 4, false>;
}

}  // namespace
}  // namespace dpx

extern "C" int dpx_nlm(const float* v, float* out, const float* sigma, int B, int C, int H, int W, int search, int patch,
                       dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(v && out && sigma, "dpx_nlm: null pointer");
  DPX_REQUIRE((const void*)v != (const void*)out, "dpx_nlm: the output must not be the input (no in-place call)");
  DPX_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "dpx_nlm: bad shape B=%d H=%d W=%d", B, H, W);
  DPX_REQUIRE(C == 1 || C == 3, "dpx_nlm: C=%d (1 or 3 channels)", C);
  DPX_REQUIRE(search % 2 == 1 && search >= 3 && search <= 21, "dpx_nlm: search window %d (odd, 3 .. 21)", search);
  DPX_REQUIRE(patch % 2 == 1 && patch >= 1 && patch <= 9, "dpx_nlm: patch %d (odd, 1 .. 9)", patch);
  const int rs = search / 2, rp = patch / 2;
  const bool fixed = rs == 5 && rp == 2;
  const int rows = fixed ? 4 * 8 : 4 * 4;
  const dim3 grid((W + 63 - 2 * rp) / (64 - 2 * rp), (H + rows - 1) / rows, B);
  const NlmKernel kern = C == 3 ? nlm_kernel<3>(fixed) : nlm_kernel<1>(fixed);
  DPX_LAUNCH("k_nlm", kern, grid, dim3(NLM_THREADS), 0, (hipStream_t)stream, v, out, sigma, H, W, rs, rp);
  return launch_status("dpx_nlm");
}
