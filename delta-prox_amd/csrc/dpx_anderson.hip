// Anderson acceleration of a fixed-point iteration z = f(z) on the packed solver state (the DEQ specialization; the reference's
// deq/utils/solvers.py:193-254 composes it from bmm / linalg.solve / two alpha products / two norms per step).
//
// History layout, piece-major: F and G = F - X hold m slots of P pieces, every piece a contiguous [B][D] image stack
// (F[slot][piece][image][D]); a slot's pieces are what the solver's iteration kernels read and write directly.  X is never kept:
// X_i = F_i - G_i where the mix needs it (beta != 1).  Per step, besides the evaluation of f, two launches:
//
//   dpx_anderson_gram_row   G_k = F_k - X_k written; per image row / column k of the Gram matrix <G_k, G_j>, j < n, and |F_k|^2.
//                           Reads n + 1 image-sized vectors, writes 1.  Two-stage reduction: per-workgroup partial sums in a
//                           workspace, added up in one fixed order by the last workgroup of each image to arrive (an integer ticket,
//                           no floating-point atomics): two calls give the same bits.
//   dpx_anderson_mix        every workgroup solves the bordered (n + 1) x (n + 1) system [[0, 1^T], [1, G G^T + lam I]] [nu; alpha] =
//                           [1; 0] of its image in its prologue (float64 Gauss-Jordan with partial pivoting in LDS: H[0][0] = 0),
//                           then streams X_new = beta sum_i alpha_i F_i + (1 - beta) sum_i alpha_i (F_i - G_i).
//                           Reads n image-sized vectors (2 n with beta != 1), writes 1.
//
// 16-byte accesses when D % 4 == 0 and the buffers are 16-byte aligned (every [image][D] segment is then aligned too); any other D
// runs the same kernels element by element.
#include "dpx_dispatch.h"
#include "dpx_reduce_dev.h"

namespace dpx {
namespace {

constexpr int AND_MAXN = 8;                 // history slots a call can mix
constexpr int AND_NRED = AND_MAXN + 1;      // reduced values per image: the Gram row and |F_k|^2
constexpr int AND_THREADS = 256;

// grid (nblk, B).  partial: [B][AND_NRED][nblk]; counter: [B] tickets, zero between launches.
template <int V>
__global__ void __launch_bounds__(AND_THREADS) k_anderson_gram_row(const float* __restrict__ X, const float* __restrict__ F, float* __restrict__ G,
                                                                   float* __restrict__ Hm, float* __restrict__ nrm, float* __restrict__ partial,
                                                                   unsigned* __restrict__ counter, int ks, int n, int m, int P, long D, int nblk) {
  __shared__ float red[AND_THREADS / 64][AND_NRED];
  __shared__ int last;
  const int b = blockIdx.y, B = gridDim.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long slot = (long)P * B * D, DV = D / V;
  float acc[AND_NRED];
#pragma unroll
  for (int j = 0; j < AND_NRED; ++j) acc[j] = 0.f;
  for (int p = 0; p < P; ++p) {
    const long seg = ((long)p * B + b) * D;
    const float* xs = X + seg;
    const float* fs = F + ks * slot + seg;
    float* gs = G + ks * slot + seg;
    for (long i = blockIdx.x * (long)AND_THREADS + tid; i < DV; i += (long)nblk * AND_THREADS) {
      const Vec<float, V> f = Vec<float, V>::ld(fs, i), x = Vec<float, V>::ld(xs, i);
      Vec<float, V> g;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        g.v[e] = f.v[e] - x.v[e];
        acc[AND_MAXN] = fmaf(f.v[e], f.v[e], acc[AND_MAXN]);
      }
      g.st(gs, i);
#pragma unroll
      for (int j = 0; j < AND_MAXN; ++j) {
        if (j >= n) continue;                 // (uniform)
        if (j == ks) {
#pragma unroll
          for (int e = 0; e < V; ++e) acc[j] = fmaf(g.v[e], g.v[e], acc[j]);
        } else {
          const Vec<float, V> o = Vec<float, V>::ld(G + j * slot + seg, i);
#pragma unroll
          for (int e = 0; e < V; ++e) acc[j] = fmaf(g.v[e], o.v[e], acc[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < AND_NRED; ++j) {
    const float s = wave_sum(acc[j]);
    if (lane == 0) red[wave][j] = s;
  }
  __syncthreads();
  if (tid < AND_NRED) {
    float s = red[0][tid];
    for (int w = 1; w < AND_THREADS / 64; ++w) s += red[w][tid];
    dpx_st_agent(partial + ((long)b * AND_NRED + tid) * nblk + blockIdx.x, s);
  }
  if (!dpx_last_block(counter + b, (unsigned)nblk, &last)) return;
  for (int e = wave; e < AND_NRED; e += AND_THREADS / 64) {
    if (e >= n && e != AND_MAXN) continue;    // (uniform per wave)
    const double s = sum_partials_f64(partial + ((long)b * AND_NRED + e) * nblk, nblk);
    if (lane == 0) {
      const float v = (float)s;
      if (e == AND_MAXN) {
        nrm[2 * b + 1] = v;
      } else {
        Hm[((long)b * m + ks) * m + e] = v;
        Hm[((long)b * m + e) * m + ks] = v;
        if (e == ks) nrm[2 * b] = v;
      }
    }
  }
}

// grid (nblk, B).  Hm: [B][m][m] Gram matrices (no ridge); alpha_out: [B][n].
template <int V, bool BETA1>
__global__ void __launch_bounds__(AND_THREADS) k_anderson_mix(const float* __restrict__ F, const float* __restrict__ G, const float* __restrict__ Hm,
                                                              float* __restrict__ Xout, float* __restrict__ alpha_out, int n, int m, float beta,
                                                              float lam, int P, long D, int nblk) {
  __shared__ double A[AND_MAXN + 1][AND_MAXN + 2];       // the bordered system, augmented with its right-hand side
  __shared__ float al[AND_MAXN];
  const int b = blockIdx.y, B = gridDim.y, tid = threadIdx.x;
  const int N = n + 1;
  const int r = tid >> 4, c = tid & 15;
  const bool mine = r < N && c <= N;
  if (mine) {
    double v;
    if (c == N) v = r == 0 ? 1.0 : 0.0;
    else if (r == 0) v = c == 0 ? 0.0 : 1.0;
    else if (c == 0) v = 1.0;
    else v = (double)Hm[((long)b * m + (r - 1)) * m + (c - 1)] + (r == c ? (double)lam : 0.0);
    A[r][c] = v;
  }
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    int pr = k;                                          // partial pivoting: every thread finds the same row
    double best = fabs(A[k][k]);
    for (int q = k + 1; q < N; ++q) {
      const double a = fabs(A[q][k]);
      if (a > best) best = a, pr = q;
    }
    __syncthreads();
    if (pr != k && tid <= N) {
      const double t = A[k][tid];
      A[k][tid] = A[pr][tid];
      A[pr][tid] = t;
    }
    __syncthreads();
    // Gauss-Jordan: rows r != k, columns c > k (reads touch column k and row k only, writes neither)
    if (mine && r != k && c > k) A[r][c] -= A[r][k] / A[k][k] * A[k][c];
    __syncthreads();
  }
  if (tid < n) {
    const float a = (float)(A[tid + 1][N] / A[tid + 1][tid + 1]);
    al[tid] = a;
    if (blockIdx.x == 0) alpha_out[(long)b * n + tid] = a;
  }
  __syncthreads();
  float a[AND_MAXN];
#pragma unroll
  for (int j = 0; j < AND_MAXN; ++j) a[j] = j < n ? al[j] : 0.f;
  const long slot = (long)P * B * D, DV = D / V;
  for (int p = 0; p < P; ++p) {
    const long seg = ((long)p * B + b) * D;
    float* xo = Xout + seg;
    for (long i = blockIdx.x * (long)AND_THREADS + tid; i < DV; i += (long)nblk * AND_THREADS) {
      Vec<float, V> sf, sx;
#pragma unroll
      for (int e = 0; e < V; ++e) sf.v[e] = sx.v[e] = 0.f;
#pragma unroll
      for (int j = 0; j < AND_MAXN; ++j) {
        if (j >= n) continue;                            // (uniform)
        const Vec<float, V> f = Vec<float, V>::ld(F + j * slot + seg, i);
#pragma unroll
        for (int e = 0; e < V; ++e) sf.v[e] = fmaf(a[j], f.v[e], sf.v[e]);
        if constexpr (!BETA1) {
          const Vec<float, V> g = Vec<float, V>::ld(G + j * slot + seg, i);
#pragma unroll
          for (int e = 0; e < V; ++e) sx.v[e] = fmaf(a[j], f.v[e] - g.v[e], sx.v[e]);
        }
      }
      if constexpr (!BETA1) {
#pragma unroll
        for (int e = 0; e < V; ++e) sf.v[e] = beta * sf.v[e] + (1.f - beta) * sx.v[e];
      }
      sf.st(xo, i);
    }
  }
}

int and_blocks(int B, long D) {
  long nb = (D + 1023) / 1024;
  const long cap = B >= 256 ? 8 : 2048 / B;
  return (int)(nb > cap ? cap : (nb < 1 ? 1 : nb));
}

}  // namespace
}  // namespace dpx

extern "C" size_t dpx_anderson_ws_bytes(int B, int P, long D) {
  if (B < 1 || P < 1 || D < 1) return 0;
  return dpx::ticket_bytes(B) + (size_t)B * dpx::AND_NRED * dpx::and_blocks(B, D) * sizeof(float);
}

extern "C" int dpx_anderson_gram_row(const float* X, const float* F, float* G, float* Hm, float* nrm, int ks, int n, int m, int P, int B, long D,
                                     void* ws, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(X && F && G && Hm && nrm && ws, "dpx_anderson_gram_row: null pointer");
  DPX_REQUIRE(m >= 1 && m <= AND_MAXN && n >= 1 && n <= m && ks >= 0 && ks < n, "dpx_anderson_gram_row: slot %d of n=%d valid, m=%d (1 <= n <= m <= %d)",
              ks, n, m, AND_MAXN);
  DPX_REQUIRE(P >= 1 && B >= 1 && B <= 65535 && D >= 1, "dpx_anderson_gram_row: bad shape P=%d B=%d D=%ld", P, B, D);
  const int nblk = and_blocks(B, D);
  unsigned* counter = (unsigned*)ws;
  float* partial = (float*)((char*)ws + ticket_bytes(B));
  const dim3 grid(nblk, B, 1);
  dispatch_flag(D % 4 == 0 && aligned16({X, F, G}), [&](auto vec) {
    constexpr int V = decltype(vec)::value ? 4 : 1;
    DPX_LAUNCH("k_anderson_gram_row", k_anderson_gram_row<V>, grid, dim3(AND_THREADS), 0, (hipStream_t)stream, X, F, G, Hm, nrm, partial, counter, ks, n, m,
               P, D, nblk);
  });
  return launch_status("dpx_anderson_gram_row");
}

extern "C" int dpx_anderson_mix(const float* F, const float* G, const float* Hm, float* Xout, float* alpha, int n, int m, float beta, float lam,
                                int P, int B, long D, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(F && G && Hm && Xout && alpha, "dpx_anderson_mix: null pointer");
  DPX_REQUIRE(m >= 1 && m <= AND_MAXN && n >= 1 && n <= m, "dpx_anderson_mix: n=%d of m=%d slots (1 <= n <= m <= %d)", n, m, AND_MAXN);
  DPX_REQUIRE(P >= 1 && B >= 1 && B <= 65535 && D >= 1, "dpx_anderson_mix: bad shape P=%d B=%d D=%ld", P, B, D);
  const int nblk = and_blocks(B, D);
  const dim3 grid(nblk, B, 1);
  dispatch_flag(beta == 1.f, [&](auto beta1) {
    dispatch_flag(D % 4 == 0 && aligned16({F, G, Xout}), [&](auto vec) {
      constexpr int V = decltype(vec)::value ? 4 : 1;
      DPX_LAUNCH("k_anderson_mix", (k_anderson_mix<V, decltype(beta1)::value>), grid, dim3(AND_THREADS), 0, (hipStream_t)stream, F, G, Hm, Xout, alpha, n, m,
                 beta, lam, P, D, nblk);
    });
  });
  return launch_status("dpx_anderson_mix");
}
