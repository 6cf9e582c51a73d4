// Anisotropic TV denoiser (TVDenoiser prior): the reference's TV_denoising / TV_denoising3d,
// dprox/proxfn/pnp/denoisers/models/TV_denoising.py:4-34, as a stencil iteration on an LDS tile.
//
//   volume y[N][D0][D1][D2]; A = active axes, k = |A|; theta_n = lam_n / 2; z_a^0 = 0
//   x^t   = (1/k) sum_{a in A} (y - D_a^T z_a^{t-1})          (D_a^T z)[i] = z[i-1] - z[i],  z[-1] = z[n_a - 1] = 0
//   z_a^t = clip(z_a^{t-1} + (1/5) D_a x^t, -theta, +theta)   (D_a x)[i]   = x[i+1] - x[i],  i < n_a - 1
//   out   = x^T                                               (the last z update is not computed)
//
// One kernel, k_tv<AXES>, runs `steps` of these on a tile: a workgroup stages its core t0 x t1 x t2 plus a halo of h_a cells on
// either side of every active axis it does not hold whole (h_a = the S steps a launch of the plan runs) -- y and the k dual fields
// -- in LDS, alternates the x pass and the z pass on a box that shrinks by one cell per step on the haloed sides (what lies outside
// has lost its neighbours' updates), and writes its core: z for the next launch of a chain, x from the last one.  At the volume's own
// borders the halo is the boundary rule, not memory: the boxes are clipped to the volume.  S = 1 is the one-step form (halo 1: x at
// the +1 neighbours is recomputed from the halo, never stored between launches); iters > S is a chain over two z buffers (a tile
// reads its neighbours' old z); the first launch knows z = 0 and reads none.
//
// The arithmetic of a voxel is tv_term / tv_mean / tv_dual below and nothing else, in the reference's own rounding order with
// contraction off, and a cell's value never depends on which tile or step count computed it: results are bit-identical for every S
// and every tile geometry.  Lanes lie along D2 (LDS rows are read and written conflict-free); global rows move 16 bytes per lane
// where D2 is a multiple of 4 and the buffers are aligned.
//
// The gradient (dpx_tv_denoise_rec + dpx_tv_backward).  Given the clip state c_a^t in {-1, 0, +1} of every dual update (w < -theta,
// inside -- equality included, as torch.clamp's backward counts it --, w > theta), the reverse sweep is linear in the cotangent g and
// needs neither y nor lam:
//   p = g, q_a = 0, gy = 0, gtheta = 0;   for t = T .. 1:   gy += p;   q_a += (1/k) (p[i] - p[i+1])   (i < n_a - 1);   t == 1: stop;
//   gtheta += sum q_a c_a^{t-1};   q_a = q_a [c_a^{t-1} == 0];   p = (1/5) sum_a (q_a[i-1] - q_a[i])   (the forward's boundary rule)
// The states come from the recording instantiation of k_tv (REC = TvRec: one byte per voxel and step t = 1 .. T-1, two bits per active
// axis, [T-1][N][V]; in the shipped instantiation, REC = TvNoRec, the recording is compiled out).  k_tv_bwd<AXES> is the forward's blocking run
// backwards on the forward's own tiles (tv_plan): p, a gy accumulator and the k fields q_a for core + halo S in LDS, S reverse steps on
// a box that shrinks by one cell per step on the haloed sides, the core written back; a chain hands p and q_a over through two buffers
// each and accumulates gy in place (a tile reads and writes only its own core of gy).  A cell reads its own state byte only, straight
// from global memory.  The arithmetic of a voxel is tv_bwd_dual / tv_bwd_prim and nothing else: gy is bit-identical for every S and
// tiling.  gtheta: every workgroup sums q_a c_a over its CORE cells in float64, the last workgroup of an image to arrive adds the
// workgroups' sums in a fixed order (dpx_reduce_dev.h): no floating-point atomics, the same bits from run to run.
#include "dpx_common.h"
#include "dpx_reduce_dev.h"

#include <algorithm>
#include <type_traits>

namespace dpx {
namespace {

constexpr int TV_LDS_MAX = 160 * 1024;     // the CU's LDS: bounds a blocked tile (one 16-wave workgroup per CU)
constexpr int TV_LDS_ONE_STEP = 64 * 1024; // one-step tiles: two 8-wave workgroups per CU
constexpr int TV_STEPS = 5;                // steps per launch where D0 is held whole or is not differenced
constexpr int TV_STEPS_DEEP = 2;           // ... where D0 is differenced and tiled (halo on all three axes)
constexpr int TV_WHOLE_D0 = 4;             // an active D0 up to this extent is always held whole (gray, RGB)

// ---- the arithmetic of one voxel (written once; every instantiation and every step count runs exactly this) ----------------------
// y - D_a^T z at a cell: zm = z_a[i - 1], zc = z_a[i] (0 beyond the ends)
__device__ __forceinline__ float tv_term(float y, float zm, float zc) {
#pragma clang fp contract(off)
  return y - (zm - zc);
}
// the mean over the k active axes of their summed terms (TV_denoising.py:13, 30: a division by k)
template <int K> __device__ __forceinline__ float tv_mean(float sum) {
  return K == 1 ? sum : K == 2 ? sum * 0.5f : sum / 3.0f;
}
// clip(z + (1/5) (xn - xc), -theta, theta): product and sum rounded separately, as the reference's eager ops do
__device__ __forceinline__ float tv_dual(float z, float xc, float xn, float theta) {
#pragma clang fp contract(off)
  const float step = 0.2f * (xn - xc);
  return fminf(fmaxf(z + step, -theta), theta);
}

// the argument of that clip, w = z + (1/5) (xn - xc), in the same two roundings, and its state: 0 inside [-theta, theta], 1 above, 2 below
__device__ __forceinline__ float tv_dual_arg(float z, float xc, float xn) {
#pragma clang fp contract(off)
  const float step = 0.2f * (xn - xc);
  return z + step;
}
__device__ __forceinline__ unsigned tv_state(float w, float theta) { return w > theta ? 1u : w < -theta ? 2u : 0u; }
// the reverse sweep: q_a + (1/k) (p[i] - p[i+1]) -- the adjoint of tv_term under tv_mean -- and (1/5) sum_a (q_a[i-1] - q_a[i])
template <int K> __device__ __forceinline__ float tv_bwd_dual(float q, float pc, float pn) {
#pragma clang fp contract(off)
  const float d = tv_mean<K>(pc - pn);
  return q + d;
}
__device__ __forceinline__ float tv_bwd_prim(float sum) {
#pragma clang fp contract(off)
  return 0.2f * sum;
}

// what the recording forward adds to the launch: the state bytes [T-1][N][V] and the global step of the launch's first step
struct TvNoRec {
  static constexpr bool on = false;
};
struct TvRec {
  static constexpr bool on = true;
  unsigned char* codes;
  int t0;
};

struct TvGeom {
  int N;
  int D[3];        // volume extents
  int t[3];        // core tile extents
  int h[3];        // halo on either side (> 0: the axis is active and tiled)
  int E[3];        // t + 2 h
  int nt[3];       // tiles per axis
};

// what one workgroup knows about its tile
struct TvTile {
  int o[3];        // global coordinate of local cell 0 (core origin - h)
  int vlo[3], vhi[3];   // local cells [vlo, vhi) lie inside the volume
};

// the tile of this workgroup (blockIdx.x counts tiles along D2 fastest, images slowest); returns the image
__device__ __forceinline__ int tv_block_tile(const TvGeom& g, TvTile& T) {
  unsigned b = blockIdx.x;
  const unsigned b2 = b % g.nt[2]; b /= g.nt[2];
  const unsigned b1 = b % g.nt[1]; b /= g.nt[1];
  const unsigned b0 = b % g.nt[0];
  const unsigned tb[3] = {b0, b1, b2};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T.o[a] = (int)tb[a] * g.t[a] - g.h[a];
    T.vlo[a] = max(0, -T.o[a]);
    T.vhi[a] = min(g.E[a], g.D[a] - T.o[a]);
  }
  return (int)(b / g.nt[0]);
}

// a local cell of the tile's core (the cells this workgroup answers for)
__device__ __forceinline__ bool tv_core(const TvGeom& g, int i0, int i1, int i2) {
  return i0 >= g.h[0] && i0 < g.h[0] + g.t[0] && i1 >= g.h[1] && i1 < g.h[1] + g.t[1] && i2 >= g.h[2] && i2 < g.h[2] + g.t[2];
}

// n / d by a multiplication: magic = 2^32 / d + 1 (exact while n d < 2^32; the tile's cell counts are far below)
__host__ __device__ __forceinline__ unsigned long long tv_magic(int d) { return (1ull << 32) / (unsigned)(d > 0 ? d : 1) + 1; }
__device__ __forceinline__ int tv_div(int n, unsigned long long magic) { return (int)(((unsigned long long)(unsigned)n * magic) >> 32); }

// local rows [lo0, lo0 + n0) x [lo1, lo1 + n1), one wave per row at a time; f(i0, i1, local row base)
template <class F> __device__ __forceinline__ void tv_rows(const TvGeom& g, int lo0, int n0, int lo1, int n1, F f) {
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int rows = n0 > 0 && n1 > 0 ? n0 * n1 : 0;
  const unsigned long long m1 = tv_magic(n1);
  for (int r = wave; r < rows; r += nw) {
    const int q = tv_div(r, m1);
    const int i0 = lo0 + q, i1 = lo1 + (r - q * n1);
    f(i0, i1, (i0 * g.E[1] + i1) * g.E[2]);
  }
}

// The aligned quads of columns that cover global columns [glo, ghi) of local rows [lo0, lo0 + n0) x [lo1, lo1 + n1), dealt to the
// threads of the workgroup one by one (every lane busy whatever the row length), four per thread and round: the four global
// accesses of a round are issued before anything waits on them.  f(u, valid, global row index, first column of the quad, local row base)
constexpr int TV_BATCH = 4;
struct TvQuads {
  int lo0, n1, lo1, nq, q0, total;
  unsigned long long mq, m1;
};
__device__ __forceinline__ TvQuads tv_quads(int lo0, int n0, int lo1, int n1, int glo, int ghi) {
  TvQuads Q;
  Q.lo0 = lo0, Q.lo1 = lo1, Q.n1 = n1;
  Q.q0 = glo >> 2;
  Q.nq = ((ghi + 3) >> 2) - Q.q0;
  Q.total = n0 > 0 && n1 > 0 && Q.nq > 0 ? n0 * n1 * Q.nq : 0;
  Q.mq = tv_magic(Q.nq), Q.m1 = tv_magic(n1);
  return Q;
}
// quad `idx`: local i0, i1 and the quad's first global column
__device__ __forceinline__ void tv_quad(const TvQuads& Q, int idx, int& i0, int& i1, int& c) {
  const int r = tv_div(idx, Q.mq);
  c = 4 * (Q.q0 + idx - r * Q.nq);
  const int a = tv_div(r, Q.m1);
  i0 = Q.lo0 + a, i1 = Q.lo1 + r - a * Q.n1;
}

// global -> LDS: every cell of the tile that lies inside the volume; 16-byte loads on aligned quads that lie wholly inside
__device__ __forceinline__ void tv_load(const float* __restrict__ src, float* s, const TvGeom& g, const TvTile& T, int vec) {
  const int glo = T.o[2] + T.vlo[2], ghi = T.o[2] + T.vhi[2];        // global columns [glo, ghi), 0 <= glo, ghi <= D2
  const TvQuads Q = tv_quads(T.vlo[0], T.vhi[0] - T.vlo[0], T.vlo[1], T.vhi[1] - T.vlo[1], glo, ghi);
  for (int first = threadIdx.x; first < Q.total; first += TV_BATCH * blockDim.x) {
    float4 v[TV_BATCH];
    int dst[TV_BATCH], col[TV_BATCH];
#pragma unroll
    for (int u = 0; u < TV_BATCH; ++u) {
      const int idx = first + u * (int)blockDim.x;
      col[u] = -8;                                                     // (no column of this quad is in range)
      dst[u] = 0;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < Q.total) {
        int i0, i1, c;
        tv_quad(Q, idx, i0, i1, c);
        const float* row = src + ((size_t)(T.o[0] + i0) * g.D[1] + (T.o[1] + i1)) * g.D[2];
        if (vec && c >= glo && c + 4 <= ghi) {
          v[u] = *(const float4*)(row + c);
        } else {
          if (c >= glo && c < ghi) v[u].x = row[c];
          if (c + 1 >= glo && c + 1 < ghi) v[u].y = row[c + 1];
          if (c + 2 >= glo && c + 2 < ghi) v[u].z = row[c + 2];
          if (c + 3 >= glo && c + 3 < ghi) v[u].w = row[c + 3];
        }
        col[u] = c;
        dst[u] = (i0 * g.E[1] + i1) * g.E[2] - T.o[2] + c;             // LDS cell of global column c
      }
    }
#pragma unroll
    for (int u = 0; u < TV_BATCH; ++u) {
      const int c = col[u];
      if (c >= glo && c < ghi) s[dst[u]] = v[u].x;
      if (c + 1 >= glo && c + 1 < ghi) s[dst[u] + 1] = v[u].y;
      if (c + 2 >= glo && c + 2 < ghi) s[dst[u] + 2] = v[u].z;
      if (c + 3 >= glo && c + 3 < ghi) s[dst[u] + 3] = v[u].w;
    }
  }
}

// LDS -> global: the tile's core (clipped to the volume); the core starts on a multiple of 4 columns
__device__ __forceinline__ void tv_store(float* __restrict__ dst, const float* s, const TvGeom& g, const TvTile& T, int vec) {
  int lo[3], n[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = g.h[a];
    n[a] = min(g.h[a] + g.t[a], T.vhi[a]) - lo[a];
  }
  const int glo = T.o[2] + lo[2], ghi = glo + n[2];                    // glo: a multiple of 4
  const TvQuads Q = tv_quads(lo[0], n[0], lo[1], n[1], glo, ghi);
  for (int idx = threadIdx.x; idx < Q.total; idx += blockDim.x) {
    int i0, i1, c;
    tv_quad(Q, idx, i0, i1, c);
    float* row = dst + ((size_t)(T.o[0] + i0) * g.D[1] + (T.o[1] + i1)) * g.D[2];
    const float* srow = s + (i0 * g.E[1] + i1) * g.E[2] - T.o[2];      // indexed by the global column
    if (vec && c + 4 <= ghi) {
      *(float4*)(row + c) = make_float4(srow[c], srow[c + 1], srow[c + 2], srow[c + 3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < ghi) row[c + e] = srow[c + e];
    }
  }
}

// AX: bit a set = differences along axis a.  zin == null: the first launch (z = 0); zout == null: the last one (writes x to out).
// z buffers: [k][N][D0 D1 D2], the j-th active axis' field of image n at ((j N + n) V).
// REC = TvRec: every z pass also writes the core cells' clip states of its step (rec.codes).
template <int AX, class REC>
__global__ __launch_bounds__(1024) void k_tv(const float* __restrict__ y, float* __restrict__ out, const float* __restrict__ lam,
                                             const float* __restrict__ zin, float* __restrict__ zout, TvGeom g, int steps, int vec, REC rec) {
  constexpr int K = (AX & 1) + ((AX >> 1) & 1) + ((AX >> 2) & 1);
  HIP_DYNAMIC_SHARED(float, smem_tv)
  const int cells = g.E[0] * g.E[1] * g.E[2];
  float* sy = smem_tv;
  float* sx = sy + cells;
  float* sz = sx + cells;                     // K fields of `cells`
  const int stride[3] = {g.E[1] * g.E[2], g.E[2], 1};

  TvTile T;
  const int n = tv_block_tile(g, T);
  const size_t V = (size_t)g.D[0] * g.D[1] * g.D[2];
  const float theta = 0.5f * lam[n];
  const int lane = threadIdx.x & 63;

  tv_load(y + (size_t)n * V, sy, g, T, vec);
  if (zin) {
#pragma unroll
    for (int j = 0; j < K; ++j) tv_load(zin + ((size_t)j * g.N + n) * V, sz + j * cells, g, T, vec);
  } else {
    for (int i = threadIdx.x; i < K * cells; i += blockDim.x) sz[i] = 0.f;
  }
  __syncthreads();

  for (int s = 1; s <= steps; ++s) {
    int lo[3], nx[3], nz[3];                   // this step's box: x on [lo, lo + nx), z on [lo, lo + nz)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const bool tiled = g.h[a] > 0;
      lo[a] = max(tiled ? s : 0, T.vlo[a]);
      nx[a] = min(tiled ? g.E[a] - s + 1 : g.E[a], T.vhi[a]) - lo[a];
      nz[a] = min(tiled ? g.E[a] - s : g.E[a], T.vhi[a]) - lo[a];
    }
    tv_rows(g, lo[0], nx[0], lo[1], nx[1], [&](int i0, int i1, int base) {
      const int gi01[2] = {T.o[0] + i0, T.o[1] + i1};
      for (int i2 = lo[2] + lane; i2 < lo[2] + nx[2]; i2 += 64) {
        const int c = base + i2;
        const float yv = sy[c];
        float sum = 0.f;
        int j = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
          if ((AX >> a) & 1) {
            const int gi = a == 2 ? T.o[2] + i2 : gi01[a];
            const float zm = gi > 0 ? sz[j * cells + c - stride[a]] : 0.f;
            const float zc = gi < g.D[a] - 1 ? sz[j * cells + c] : 0.f;
            const float t = tv_term(yv, zm, zc);
            sum = j == 0 ? t : sum + t;
            ++j;
          }
        sx[c] = tv_mean<K>(sum);
      }
    });
    __syncthreads();
    if (s == steps && !zout) break;
    tv_rows(g, lo[0], nz[0], lo[1], nz[1], [&](int i0, int i1, int base) {
      const int gi01[2] = {T.o[0] + i0, T.o[1] + i1};
      for (int i2 = lo[2] + lane; i2 < lo[2] + nz[2]; i2 += 64) {
        const int c = base + i2;
        const float xc = sx[c];
        unsigned code = 0;
        int j = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
          if ((AX >> a) & 1) {
            const int gi = a == 2 ? T.o[2] + i2 : gi01[a];
            float* z = sz + j * cells + c;
            if constexpr (REC::on)
              if (gi < g.D[a] - 1) code |= tv_state(tv_dual_arg(*z, xc, sx[c + stride[a]]), theta) << (2 * j);
            *z = gi < g.D[a] - 1 ? tv_dual(*z, xc, sx[c + stride[a]], theta) : 0.f;
            ++j;
          }
        if constexpr (REC::on)
          if (tv_core(g, i0, i1, i2))
            rec.codes[((size_t)(rec.t0 + s - 2) * g.N + n) * V + ((size_t)gi01[0] * g.D[1] + gi01[1]) * g.D[2] + T.o[2] + i2] = (unsigned char)code;
      }
    });
    __syncthreads();
  }

  if (zout) {
#pragma unroll
    for (int j = 0; j < K; ++j) tv_store(zout + ((size_t)j * g.N + n) * V, sz + j * cells, g, T, vec);
  } else {
    tv_store(out + (size_t)n * V, theta == 0.f ? sy : sx, g, T, vec);     // lam = 0: y itself, bit for bit
  }
}

// what the gtheta reduction of a backward launch works on (all null when no gradient of lam is asked for)
struct TvBwdRed {
  double* partial;    // [N][tiles of an image]: the workgroups' sums of this launch
  unsigned* counter;  // [N] tickets, zero before the launch
  double* total;      // [N] running sums over the launches of a chain
  float* glam;        // [N]: written by the chain's last launch, 0.5 total
};
constexpr size_t TV_BWD_LDS_MIN = 256;   // the reduction's scratch (16 wave sums and a flag) reuses the tile's LDS

// The reverse steps t = t_hi .. t_hi - steps + 1 on a tile.  qin == null: the first launch of the reverse chain (p = the cotangent g, q = 0,
// gy = 0: nothing else is read); pout == null: the last one (ends at t = 1 and writes gy only).  q buffers as the forward's z buffers.
template <int AX>
__global__ __launch_bounds__(1024) void k_tv_bwd(const float* __restrict__ pin, const float* __restrict__ qin, float* __restrict__ pout,
                                                 float* __restrict__ qout, float* __restrict__ gy, const unsigned char* __restrict__ codes,
                                                 TvBwdRed red, TvGeom g, int t_hi, int steps, int vec) {
  constexpr int K = (AX & 1) + ((AX >> 1) & 1) + ((AX >> 2) & 1);
  HIP_DYNAMIC_SHARED(float, smem_tv)
  const int cells = g.E[0] * g.E[1] * g.E[2];
  float* sp = smem_tv;
  float* sg = sp + cells;
  float* sq = sg + cells;                     // K fields of `cells`
  const int stride[3] = {g.E[1] * g.E[2], g.E[2], 1};

  TvTile T;
  const int n = tv_block_tile(g, T);
  const size_t V = (size_t)g.D[0] * g.D[1] * g.D[2];
  const int lane = threadIdx.x & 63;

  tv_load(pin + (size_t)n * V, sp, g, T, vec);
  if (qin) {
    tv_load(gy + (size_t)n * V, sg, g, T, vec);
#pragma unroll
    for (int j = 0; j < K; ++j) tv_load(qin + ((size_t)j * g.N + n) * V, sq + j * cells, g, T, vec);
  } else {
    for (int i = threadIdx.x; i < (1 + K) * cells; i += blockDim.x) sg[i] = 0.f;
  }
  __syncthreads();

  double acc = 0.0;                            // this thread's share of sum q_a c_a over the core
  for (int s = 1; s <= steps; ++s) {
    const int t = t_hi - s + 1;
    int lq[3], nq[3], lp[3], np[3];            // this step's boxes: q (and gy) on [lq, lq + nq), the new p on [lp, lp + np)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const bool tiled = g.h[a] > 0;
      const int hi = min(tiled ? g.E[a] - s : g.E[a], T.vhi[a]);
      lq[a] = max(tiled ? s - 1 : 0, T.vlo[a]);
      lp[a] = max(tiled ? s : 0, T.vlo[a]);
      nq[a] = hi - lq[a];
      np[a] = hi - lp[a];
    }
    const unsigned char* code_t = t > 1 ? codes + ((size_t)(t - 2) * g.N + n) * V : nullptr;
    tv_rows(g, lq[0], nq[0], lq[1], nq[1], [&](int i0, int i1, int base) {
      const int gi01[2] = {T.o[0] + i0, T.o[1] + i1};
      for (int i2 = lq[2] + lane; i2 < lq[2] + nq[2]; i2 += 64) {
        const int c = base + i2;
        const bool core = tv_core(g, i0, i1, i2);
        const unsigned code = code_t ? code_t[((size_t)gi01[0] * g.D[1] + gi01[1]) * g.D[2] + T.o[2] + i2] : 0u;
        const float pc = sp[c];
        if (core) sg[c] += pc;
        int j = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
          if ((AX >> a) & 1) {
            const int gi = a == 2 ? T.o[2] + i2 : gi01[a];
            float q = 0.f;
            if (gi < g.D[a] - 1) {
              q = tv_bwd_dual<K>(sq[j * cells + c], pc, sp[c + stride[a]]);
              const unsigned st = (code >> (2 * j)) & 3u;
              if (st) {
                if (core) acc += (double)(st == 1u ? q : -q);
                q = 0.f;
              }
            }
            sq[j * cells + c] = q;
            ++j;
          }
      }
    });
    __syncthreads();
    if (t == 1) break;
    tv_rows(g, lp[0], np[0], lp[1], np[1], [&](int i0, int i1, int base) {
      const int gi01[2] = {T.o[0] + i0, T.o[1] + i1};
      for (int i2 = lp[2] + lane; i2 < lp[2] + np[2]; i2 += 64) {
        const int c = base + i2;
        float sum = 0.f;
        int j = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
          if ((AX >> a) & 1) {
            const int gi = a == 2 ? T.o[2] + i2 : gi01[a];
            const float qm = gi > 0 ? sq[j * cells + c - stride[a]] : 0.f;
            const float qc = gi < g.D[a] - 1 ? sq[j * cells + c] : 0.f;
            const float d = qm - qc;
            sum = j == 0 ? d : sum + d;
            ++j;
          }
        sp[c] = tv_bwd_prim(sum);
      }
    });
    __syncthreads();
  }

  tv_store(gy + (size_t)n * V, sg, g, T, vec);
  if (pout) {
    tv_store(pout + (size_t)n * V, sp, g, T, vec);
#pragma unroll
    for (int j = 0; j < K; ++j) tv_store(qout + ((size_t)j * g.N + n) * V, sq + j * cells, g, T, vec);
  }
  if (!red.partial) return;

  // gtheta of image n: this workgroup's sum, then the last workgroup of the image adds all of them in a fixed order
  __syncthreads();                             // (the tile's LDS becomes the reduction's scratch)
  double* sh = (double*)smem_tv;
  int* flag = (int*)(sh + 16);
  const unsigned tiles = (unsigned)(g.nt[0] * g.nt[1] * g.nt[2]);
  const double sum = block_sum<double>(acc, sh);
  if (threadIdx.x == 0) dpx_st_agent(red.partial + (size_t)n * tiles + blockIdx.x % tiles, sum);
  if (!dpx_last_block(red.counter + n, tiles, flag)) return;
  if (threadIdx.x < 64) {
    const double all = sum_partials_f64(red.partial + (size_t)n * tiles, (int)tiles);
    if (threadIdx.x == 0) {
      const double tot = (qin ? red.total[n] : 0.0) + all;
      red.total[n] = tot;
      if (!pout) red.glam[n] = (float)(0.5 * tot);
    }
  }
}

struct TvPlan {
  int S, launches, threads;
  size_t lds;
  TvGeom g;
};

inline int tv_count(int axes) { return (axes & 1) + ((axes >> 1) & 1) + ((axes >> 2) & 1); }

// The tile of an S-step launch: the geometry with the largest share of core cells (weighted by how full the waves' 64-lane passes
// along D2 are) among rows of 64 / 128 cells along D2 and every split of the remaining LDS between D0 and D1.  An axis that fits is
// held whole (no halo); an inactive axis has none.  false: no tile with this halo fits the LDS.
bool tv_tile(const int D[3], int axes, int S, TvGeom& best) {
  const int cell_bytes = 4 * (2 + tv_count(axes));
  const int cells = (S == 1 ? TV_LDS_ONE_STEP : TV_LDS_MAX) / cell_bytes;
  double best_score = 0.0;
  for (int e2c = 64; e2c <= 128; e2c += 64) {
    TvGeom g{};
    for (int a = 0; a < 3; ++a) g.D[a] = D[a];
    if (D[2] <= e2c) g.t[2] = D[2], g.h[2] = 0;
    else if (axes & 4) g.t[2] = (e2c - 2 * S) & ~3, g.h[2] = S;
    else g.t[2] = e2c, g.h[2] = 0;
    if (g.t[2] < 1) continue;
    g.E[2] = g.t[2] + 2 * g.h[2];
    const int rows = cells / g.E[2];
    const bool tile0 = (axes & 1) && D[0] > TV_WHOLE_D0;
    const int e0_lo = !(axes & 1) ? 1 : !tile0 ? D[0] : 2 * S + 1;
    const int e0_hi = tile0 ? std::min(rows, D[0] + 2 * S) : e0_lo;
    for (int e0 = e0_lo; e0 <= e0_hi; ++e0) {
      if (tile0 && e0 - 2 * S >= D[0]) g.t[0] = D[0], g.h[0] = 0;
      else if (tile0) g.t[0] = e0 - 2 * S, g.h[0] = S;
      else g.t[0] = e0, g.h[0] = 0;
      g.E[0] = g.t[0] + 2 * g.h[0];
      const int e1 = rows / g.E[0];
      if (e1 < 1) break;
      if (D[1] <= e1) g.t[1] = D[1], g.h[1] = 0;
      else if (axes & 2) g.t[1] = e1 - 2 * S, g.h[1] = S;
      else g.t[1] = e1, g.h[1] = 0;
      if (g.t[1] < 1) continue;
      g.E[1] = g.t[1] + 2 * g.h[1];
      const double core = (double)g.t[0] * g.t[1] * g.t[2], passes = (double)g.E[0] * g.E[1] * ((g.E[2] + 63) / 64) * 64;
      if (core / passes > best_score) best_score = core / passes, best = g;
    }
  }
  return best_score > 0.0;
}

bool tv_plan(int N, const int D[3], int axes, int iters, TvPlan& p) {
  const bool deep = (axes & 1) && D[0] > TV_WHOLE_D0;
  int S = deep ? TV_STEPS_DEEP : TV_STEPS;
  const int knob = tune(TUNE_TV_STEPS);
  if (knob > 0) S = std::min(S, knob);
  S = std::min(S, iters);
  while (S >= 1 && !tv_tile(D, axes, S, p.g)) --S;
  if (S < 1) return false;
  p.S = S;
  p.launches = (iters + S - 1) / S;
  p.g.N = N;
  for (int a = 0; a < 3; ++a) p.g.nt[a] = (D[a] + p.g.t[a] - 1) / p.g.t[a];
  const int cells = p.g.E[0] * p.g.E[1] * p.g.E[2];
  p.lds = (size_t)cells * 4 * (2 + tv_count(axes));
  p.threads = cells <= 2048 ? 256 : S == 1 ? 512 : 1024;
  return true;
}

bool tv_args_ok(const char* who, int N, int D0, int D1, int D2, int axes, int iters) {
  if (N < 1 || D0 < 1 || D1 < 1 || D2 < 1) return set_error("%s: bad shape N=%d D=(%d, %d, %d)", who, N, D0, D1, D2), false;
  if (axes < 1 || axes > 7) return set_error("%s: axes=%d (a non-empty set of bits 0 .. 2)", who, axes), false;
  if (iters < 1) return set_error("%s: iters=%d (at least 1)", who, iters), false;
  return true;
}

// f(std::integral_constant<int, AXES>) for the axis set of a call: the one place that names the seven instantiations
template <class F> void tv_dispatch_axes(int axes, F&& f) {
  switch (axes) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 7>{}); break;
  }
}

// the forward chain of dpx_tv_denoise (codes == null) and of dpx_tv_denoise_rec
int tv_forward(const char* who, const float* y, float* out, const float* lam, unsigned char* codes, int N, int D0, int D1, int D2, int axes,
               int iters, void* ws, hipStream_t stream) {
  DPX_REQUIRE(y && out && lam, "%s: null pointer", who);
  DPX_REQUIRE((const void*)y != (const void*)out, "%s: the output must not be the input (no in-place call)", who);
  if (!tv_args_ok(who, N, D0, D1, D2, axes, iters)) return DPX_ERR_ARG;
  const int D[3] = {D0, D1, D2};
  TvPlan p;
  DPX_REQUIRE(tv_plan(N, D, axes, iters, p), "%s: no tile fits the LDS", who);
  const size_t tiles = (size_t)N * p.g.nt[0] * p.g.nt[1] * p.g.nt[2];
  DPX_REQUIRE(tiles <= 0x7fffffffu, "%s: %zu tiles (at most 2^31 - 1)", who, tiles);
  DPX_REQUIRE(p.launches == 1 || ws, "%s: null workspace for a chain of %d launches", who, p.launches);
  const size_t field = (size_t)tv_count(axes) * N * D0 * D1 * D2;
  float* zbuf[2] = {(float*)ws, (float*)ws + field};
  const int vec = D2 % 4 == 0 && aligned16({y, out, ws});
  for (int l = 0; l < p.launches; ++l) {
    const float* zin = l == 0 ? nullptr : zbuf[(l - 1) & 1];
    float* zout = l == p.launches - 1 ? nullptr : zbuf[l & 1];
    const int steps = std::min(p.S, iters - l * p.S);
    tv_dispatch_axes(axes, [&](auto ax) {
      constexpr int AX = decltype(ax)::value;
      if (codes)
        DPX_LAUNCH_LDS("k_tv_rec", (k_tv<AX, TvRec>), dim3((unsigned)tiles), dim3(p.threads), p.lds, stream, y, out, lam, zin, zout, p.g, steps, vec,
                       TvRec{codes, l * p.S + 1});
      else
        DPX_LAUNCH_LDS("k_tv", (k_tv<AX, TvNoRec>), dim3((unsigned)tiles), dim3(p.threads), p.lds, stream, y, out, lam, zin, zout, p.g, steps, vec,
                       TvNoRec{});
    });
  }
  return launch_status(who);
}

// the backward's workspace: [N tickets][N running sums][N x tiles workgroup sums][chain: 2 p buffers, 2 x k q buffers], offsets in bytes
struct TvBwdWs {
  size_t total, partial, chain, bytes;
};
TvBwdWs tv_bwd_layout(const TvPlan& p, int axes) {
  const size_t N = (size_t)p.g.N, tiles = (size_t)p.g.nt[0] * p.g.nt[1] * p.g.nt[2], V = (size_t)p.g.D[0] * p.g.D[1] * p.g.D[2];
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  TvBwdWs w;
  w.total = ticket_bytes(N);
  w.partial = w.total + pad(N * sizeof(double));
  w.chain = w.partial + pad(N * tiles * sizeof(double));
  w.bytes = w.chain + (p.launches > 1 ? (size_t)2 * (1 + tv_count(axes)) * N * V * sizeof(float) : 0);
  return w;
}

}  // namespace
}  // namespace dpx

extern "C" size_t dpx_tv_ws_bytes(int N, int D0, int D1, int D2, int axes, int iters) {
  using namespace dpx;
  const int D[3] = {D0, D1, D2};
  TvPlan p;
  if (!tv_args_ok("dpx_tv_ws_bytes", N, D0, D1, D2, axes, iters) || !tv_plan(N, D, axes, iters, p) || p.launches == 1) return 0;
  return (size_t)2 * tv_count(axes) * N * D0 * D1 * D2 * sizeof(float);
}

extern "C" int dpx_tv_plan(int D0, int D1, int D2, int axes, int iters, int* out6) {
  using namespace dpx;
  DPX_REQUIRE(out6, "dpx_tv_plan: null pointer");
  if (!tv_args_ok("dpx_tv_plan", 1, D0, D1, D2, axes, iters)) return DPX_ERR_ARG;
  const int D[3] = {D0, D1, D2};
  TvPlan p;
  DPX_REQUIRE(tv_plan(1, D, axes, iters, p), "dpx_tv_plan: no tile fits the LDS");
  out6[0] = p.S, out6[1] = p.launches, out6[2] = p.g.t[0], out6[3] = p.g.t[1], out6[4] = p.g.t[2], out6[5] = (int)p.lds;
  return DPX_OK;
}

extern "C" int dpx_tv_denoise(const float* y, float* out, const float* lam, int N, int D0, int D1, int D2, int axes, int iters, void* ws,
                              dpx_stream_t stream) {
  return dpx::tv_forward("dpx_tv_denoise", y, out, lam, nullptr, N, D0, D1, D2, axes, iters, ws, (hipStream_t)stream);
}

extern "C" size_t dpx_tv_codes_bytes(int N, int D0, int D1, int D2, int axes, int iters) {
  if (!dpx::tv_args_ok("dpx_tv_codes_bytes", N, D0, D1, D2, axes, iters)) return 0;
  return (size_t)(iters - 1) * N * D0 * D1 * D2;
}

extern "C" int dpx_tv_denoise_rec(const float* y, float* out, const float* lam, unsigned char* codes, int N, int D0, int D1, int D2, int axes,
                                  int iters, void* ws, dpx_stream_t stream) {
  using namespace dpx;
  if (iters == 1 || !tv_args_ok("dpx_tv_denoise_rec", N, D0, D1, D2, axes, iters))      // (one step has no clip state: the plain forward)
    return tv_forward("dpx_tv_denoise_rec", y, out, lam, nullptr, N, D0, D1, D2, axes, iters, ws, (hipStream_t)stream);
  DPX_REQUIRE(codes, "dpx_tv_denoise_rec: null pointer (the clip states of %d steps)", iters - 1);
  return tv_forward("dpx_tv_denoise_rec", y, out, lam, codes, N, D0, D1, D2, axes, iters, ws, (hipStream_t)stream);
}

extern "C" size_t dpx_tv_bwd_ws_bytes(int N, int D0, int D1, int D2, int axes, int iters) {
  using namespace dpx;
  const int D[3] = {D0, D1, D2};
  TvPlan p;
  if (!tv_args_ok("dpx_tv_bwd_ws_bytes", N, D0, D1, D2, axes, iters) || iters == 1 || !tv_plan(N, D, axes, iters, p)) return 0;
  return tv_bwd_layout(p, axes).bytes;
}

extern "C" int dpx_tv_bwd_plan(int D0, int D1, int D2, int axes, int iters, int* out6) {
  using namespace dpx;
  DPX_REQUIRE(out6, "dpx_tv_bwd_plan: null pointer");
  if (!tv_args_ok("dpx_tv_bwd_plan", 1, D0, D1, D2, axes, iters)) return DPX_ERR_ARG;
  const int D[3] = {D0, D1, D2};
  TvPlan p;
  DPX_REQUIRE(tv_plan(1, D, axes, iters, p), "dpx_tv_bwd_plan: no tile fits the LDS");
  out6[0] = p.S, out6[1] = p.launches, out6[2] = p.g.t[0], out6[3] = p.g.t[1], out6[4] = p.g.t[2];
  out6[5] = (int)std::max(p.lds, TV_BWD_LDS_MIN);
  return DPX_OK;
}

extern "C" int dpx_tv_backward(const float* g, const unsigned char* codes, float* gy, float* glam, int N, int D0, int D1, int D2, int axes,
                               int iters, void* ws, dpx_stream_t stream) {
  using namespace dpx;
  hipStream_t s = (hipStream_t)stream;
  DPX_REQUIRE(g && gy, "dpx_tv_backward: null pointer");
  DPX_REQUIRE((const void*)g != (const void*)gy, "dpx_tv_backward: the gradient must not be the cotangent (no in-place call)");
  if (!tv_args_ok("dpx_tv_backward", N, D0, D1, D2, axes, iters)) return DPX_ERR_ARG;
  const size_t V = (size_t)D0 * D1 * D2;
  if (iters == 1) {                                        // out = x^1 = y: gy = g, and lam does not enter
    DPX_REQUIRE(hipMemcpyAsync(gy, g, (size_t)N * V * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess, "dpx_tv_backward: copy failed");
    DPX_REQUIRE(!glam || hipMemsetAsync(glam, 0, (size_t)N * sizeof(float), s) == hipSuccess, "dpx_tv_backward: zero fill failed");
    return launch_status("dpx_tv_backward");
  }
  DPX_REQUIRE(codes, "dpx_tv_backward: null pointer (the clip states of %d steps)", iters - 1);
  const int D[3] = {D0, D1, D2};
  TvPlan p;
  DPX_REQUIRE(tv_plan(N, D, axes, iters, p), "dpx_tv_backward: no tile fits the LDS");
  const size_t tiles = (size_t)N * p.g.nt[0] * p.g.nt[1] * p.g.nt[2];
  DPX_REQUIRE(tiles <= 0x7fffffffu, "dpx_tv_backward: %zu tiles (at most 2^31 - 1)", tiles);
  DPX_REQUIRE(ws || (p.launches == 1 && !glam), "dpx_tv_backward: null workspace (a chain of %d launches%s)", p.launches,
              glam ? ", the reduction of the gradient of lam" : "");
  const TvBwdWs w = tv_bwd_layout(p, axes);
  TvBwdRed red{nullptr, nullptr, nullptr, nullptr};
  if (glam) {
    red = TvBwdRed{(double*)((char*)ws + w.partial), (unsigned*)ws, (double*)((char*)ws + w.total), glam};
    DPX_REQUIRE(hipMemsetAsync(ws, 0, w.partial, s) == hipSuccess, "dpx_tv_backward: zero fill failed");
  }
  const size_t NV = (size_t)N * V;
  float* chain = (float*)((char*)ws + w.chain);
  float* pbuf[2] = {chain, chain + NV};
  float* qbuf[2] = {chain + 2 * NV, chain + (2 + tv_count(axes)) * NV};
  const int vec = D2 % 4 == 0 && aligned16({g, gy, ws});
  const size_t lds = std::max(p.lds, TV_BWD_LDS_MIN);
  for (int l = p.launches - 1; l >= 0; --l) {              // the forward's launches, last to first
    const bool first = l == p.launches - 1, last = l == 0;
    const int t_hi = std::min((l + 1) * p.S, iters), steps = t_hi - l * p.S;
    const float* pin = first ? g : pbuf[(l + 1) & 1];
    const float* qin = first ? nullptr : qbuf[(l + 1) & 1];
    float* pout = last ? nullptr : pbuf[l & 1];
    float* qout = last ? nullptr : qbuf[l & 1];
    tv_dispatch_axes(axes, [&](auto ax) {
      DPX_LAUNCH_LDS("k_tv_bwd", k_tv_bwd<decltype(ax)::value>, dim3((unsigned)tiles), dim3(p.threads), lds, s, pin, qin, pout, qout, gy, codes, red, p.g,
                     t_hi, steps, vec);
    });
  }
  return launch_status("dpx_tv_backward");
}
