// MINRES (the reference's dprox/linalg/solve/solver_minres.py:21-290 composes a step from about twenty eager elementwise and reduction
// ops besides the operator): the Lanczos recurrence, the Givens rotations of every shift and the search / solution updates on three
// streaming launches per step, the scalars in a device-resident state block.
//
// Vectors are [G][N][K]: G leading systems, N unknowns, K contiguous columns; system (g, k) has its element of row n at
// (g N + n) K + k, and every dot product is per system.  The state block (float64 for both element types) holds per system alpha,
// beta[2], the right-hand side's norm and its "is zero" mark, per (shift, system) cos[3], sin[3], subsub, sub, diag, scale[2], then
// the shifts and the step counter.  The roles "prev2 / prev1 / curr" are index arithmetic on the counter: beta_prev = beta[step & 1],
// scale_prev = scale[step & 1], the rotation of step i is slot i % 3, z_prev2 (overwritten by z_curr) is slot step & 1 of the ring
// of two Lanczos vectors and search_prev2 (overwritten by search_curr) slot step & 1 of the search ring.
//
//   dpx_minres_alpha    alpha = value <prod, q>                                                    reads 2 vectors
//   dpx_minres_lanczos  z = value prod - alpha z1 - beta_prev z2 written over z2, <z, z>;          reads 3, writes 1
//                       the last workgroup of a leading system finishes beta_curr = max(sqrt(.), eps) and the scalar part of
//                       _jit_minres_updates (:258-282) for every shift and column of that system, one pair per thread
//   dpx_minres_update   z /= beta_curr (with the identity preconditioner also the next q);         reads 5, writes 3 at one shift;
//                       search_curr[s] = (q - sub s1 - subsub s2) / diag over s2;                  every further shift reads 4, writes 2
//                       solution[s] += search_curr[s] scale_prev; the last workgroup of the launch advances the counter
//   with a preconditioner: dpx_minres_lanczos without the reduction, the caller's qc = Minv(z), dpx_minres_beta = <z, qc> and the
//   scalar finish, and dpx_minres_update also normalises qc.
//
// Reductions are two-stage: per-thread sums in the element type, then per column inside the workgroup (wave shuffles and one LDS
// pass when the row length in vectors divides 64, two LDS passes otherwise), write-through partials, and the last workgroup to take an
// integer ticket adds them in a fixed order in float64 -- no floating-point atomics, two calls give the same bits.
// A thread keeps the same columns for the whole launch (its stride over the flat index is a multiple of the row length), so the
// per-column scalars are registers.  16-byte accesses when K == 1 and N is a multiple of the vector length, or else K is, and the
// buffers are 16-byte aligned; element by element otherwise (no peeled head or tail).
#include "dpx_dispatch.h"
#include "dpx_reduce_dev.h"

namespace dpx {
namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_WAVES = MR_THREADS / 64;
enum { MR_DOT_ALPHA = 0, MR_LANCZOS = 1, MR_LANCZOS_PLAIN = 2, MR_DOT_BETA = 3 };

struct MrState {
  double* d;
  int S, G, K;
  __host__ __device__ long GK() const { return (long)G * K; }
  __host__ __device__ long P() const { return (long)S * G * K; }
  __host__ __device__ double* alpha() const { return d; }
  __host__ __device__ double* beta(int slot) const { return d + (1 + slot) * GK(); }
  __host__ __device__ double* norm() const { return d + 3 * GK(); }
  __host__ __device__ double* zero() const { return d + 4 * GK(); }
  __host__ __device__ double* pairs() const { return d + 5 * GK(); }
  __host__ __device__ double* cosr(int slot) const { return pairs() + slot * P(); }
  __host__ __device__ double* sinr(int slot) const { return pairs() + (3 + slot) * P(); }
  __host__ __device__ double* subsub() const { return pairs() + 6 * P(); }
  __host__ __device__ double* sub() const { return pairs() + 7 * P(); }
  __host__ __device__ double* diag() const { return pairs() + 8 * P(); }
  __host__ __device__ double* scale(int slot) const { return pairs() + (9 + slot) * P(); }
  __host__ __device__ double* shifts() const { return pairs() + 11 * P(); }
  __host__ __device__ long long* step() const { return (long long*)(shifts() + S); }
  __host__ __device__ static size_t doubles(long S, long G, long K) { return (size_t)(5 * G * K + 11 * S * G * K + S + 1); }
};

// Which flat vector indices of a leading system a thread visits: i = t, t + stride, ... with stride the largest multiple of the
// row length (in vectors) that the launch's threads cover, so that i % KV -- the thread's column group -- never changes.
struct MrWalk {
  long first, stride, count;     // count: vectors per leading system
  int KV, cg;                    // column groups per row; this thread's
  bool active;
  __device__ __forceinline__ MrWalk(long N, int K, int V, int nblk) {
    KV = K == 1 ? 1 : K / V;
    count = N * K / V;
    const long T = (long)nblk * MR_THREADS, t = (long)blockIdx.x * MR_THREADS + threadIdx.x;
    stride = T / KV * KV;
    active = t < stride;
    first = t;
    cg = (int)(t % KV);
  }
  // the system-local column of this thread's element e (K == 1: every element is column 0)
  __device__ __forceinline__ int col(int K, int V, int e) const { return K == 1 ? 0 : cg * V + e; }
};

// The scalar part of a step (solver_minres.py:258-282) for one (shift, system) pair.
__device__ __forceinline__ void mr_givens(const MrState& st, long step, long pair, long sys, int s) {
  const int bs = (int)(step & 1), cur = (int)(step % 3), p1 = (int)((step + 2) % 3), p2 = (int)((step + 1) % 3);
  const double bp = st.beta(bs)[sys], bc = st.beta(1 - bs)[sys], al = st.alpha()[sys] + st.shifts()[s];
  const double c2 = st.cosr(p2)[pair], s2 = st.sinr(p2)[pair], c1 = st.cosr(p1)[pair], s1 = st.sinr(p1)[pair];
  const double subsub = s2 * bp;
  double sub = c2 * bp;
  double diag = al * c1 - s1 * sub;
  sub = sub * c1 + s1 * al;
  const double radius = sqrt(diag * diag + bc * bc);
  const double cc = diag / radius, sc = bc / radius;
  diag = diag * cc + sc * bc;
  const double sp = st.scale(bs)[pair];
  st.cosr(cur)[pair] = cc;
  st.sinr(cur)[pair] = sc;
  st.subsub()[pair] = subsub;
  st.sub()[pair] = sub;
  st.diag()[pair] = diag;
  st.scale(1 - bs)[pair] = -sp * sc;
  st.scale(bs)[pair] = sp * cc;
}

// grid (nblk, min(G, 65535)).  partial: [G][K][nblk]; counter: [G] tickets, zero between launches.
//   MR_DOT_ALPHA      alpha = value <x, y>  (y == nullptr: the Lanczos ring's previous vector, which is q without a preconditioner)
//   MR_LANCZOS        x = prod; z written over the ring's slot step & 1; <z, z>, beta_curr, rotations
//   MR_LANCZOS_PLAIN  the same without the reduction
//   MR_DOT_BETA       x = z (nullptr: the ring's current slot), y = qc; <z, qc>, beta_curr, rotations
template <class T, int V, int MODE>
__global__ void __launch_bounds__(MR_THREADS) k_minres_pass(const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ zring, MrState st,
                                                           T* __restrict__ partial, unsigned* __restrict__ counter, long N, double value,
                                                           double eps, int nblk) {
  __shared__ T sh[V][MR_THREADS];
  __shared__ int last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, K = st.K, G = st.G;
  const long step = (long)*st.step(), GNK = (long)G * N * K;
  const int cur = (int)(step & 1);
  const MrWalk w(N, K, V, nblk);
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const long seg = (long)g * N * K;
    T acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = T(0);
    if (w.active) {
      if constexpr (MODE == MR_DOT_ALPHA || MODE == MR_DOT_BETA) {
        const T* xs = (x ? x : zring + cur * GNK) + seg;
        const T* ys = (y ? y : zring + (1 - cur) * GNK) + seg;
        for (long i = w.first; i < w.count; i += w.stride) {
          const Vec<T, V> a = Vec<T, V>::ld(xs, i), b = Vec<T, V>::ld(ys, i);
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] += a.v[e] * b.v[e];
        }
      } else {
        T al[V], bp[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const long sys = (long)g * K + w.col(K, V, e);
          al[e] = (T)st.alpha()[sys];
          bp[e] = (T)st.beta(cur)[sys];
        }
        const T val = (T)value;
        const T* ps = x + seg;
        const T* z1 = zring + (1 - cur) * GNK + seg;
        T* z2 = zring + cur * GNK + seg;
        for (long i = w.first; i < w.count; i += w.stride) {
          const Vec<T, V> p = Vec<T, V>::ld(ps, i), a = Vec<T, V>::ld(z1, i), b = Vec<T, V>::ld(z2, i);
          Vec<T, V> z;
#pragma unroll
          for (int e = 0; e < V; ++e) {
            z.v[e] = val * p.v[e] - al[e] * a.v[e] - bp[e] * b.v[e];
            acc[e] += z.v[e] * z.v[e];
          }
          z.st(z2, i);
        }
      }
    }
    if constexpr (MODE == MR_LANCZOS_PLAIN) continue;
    // stage one: this workgroup's sum per column, written through
    if (64 % w.KV == 0) {                                   // a wave's lanes l, l + KV, ... hold column group l % KV
      const int ncol = K == 1 ? 1 : V;
      if (K == 1) {
#pragma unroll
        for (int e = 1; e < V; ++e) acc[0] += acc[e];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (e >= ncol) continue;
        T s = acc[e];
        for (int o = 32; o >= w.KV; o >>= 1) s += __shfl_xor(s, o);
        if (lane < w.KV) sh[e][wave * 64 + lane] = s;
      }
      __syncthreads();
      if (tid < w.KV) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (e >= ncol) continue;
          T s = sh[e][tid];
          for (int q = 1; q < MR_WAVES; ++q) s += sh[e][q * 64 + tid];
          dpx_st_agent(partial + ((long)g * K + w.col(K, V, e)) * nblk + blockIdx.x, s);
        }
      }
    } else {                                                // the threads tid = j, j + KV, ... hold column group c
#pragma unroll
      for (int e = 0; e < V; ++e) sh[e][tid] = acc[e];
      __syncthreads();
      const int t0 = (int)(((long)blockIdx.x * MR_THREADS) % w.KV);
      if (w.KV <= MR_THREADS / 2) {                         // two levels: R threads per column group, then one
        const int R = MR_THREADS / w.KV < 8 ? MR_THREADS / w.KV : 8;
        const int c = tid % w.KV, r = tid / w.KV, j = ((c - t0) % w.KV + w.KV) % w.KV;
        T s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          s[e] = T(0);
          if (r < R)
            for (int q = j + r * w.KV; q < MR_THREADS; q += R * w.KV) s[e] += sh[e][q];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < V; ++e) sh[e][tid] = s[e];
        __syncthreads();
        if (tid < w.KV) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            T t = sh[e][tid];
            for (int q = 1; q < R; ++q) t += sh[e][q * w.KV + tid];
            dpx_st_agent(partial + ((long)g * K + tid * V + e) * nblk + blockIdx.x, t);
          }
        }
      } else {
        for (int c = tid; c < w.KV; c += MR_THREADS) {
          const int j = ((c - t0) % w.KV + w.KV) % w.KV;
#pragma unroll
          for (int e = 0; e < V; ++e) {
            T t = T(0);
            for (int q = j; q < MR_THREADS; q += w.KV) t += sh[e][q];
            dpx_st_agent(partial + ((long)g * K + c * V + e) * nblk + blockIdx.x, t);
          }
        }
      }
    }
    // stage two: the last workgroup of this leading system adds the partial sums and finishes the scalars
    if (!dpx_last_block(counter + g, (unsigned)nblk, &last)) continue;
    for (int c = wave; c < K; c += MR_WAVES) {
      const double s = sum_partials_f64(partial + ((long)g * K + c) * nblk, nblk);
      if (lane == 0) {
        const long sys = (long)g * K + c;
        if constexpr (MODE == MR_DOT_ALPHA) st.alpha()[sys] = value * s;
        else st.beta(1 - cur)[sys] = fmax(sqrt(s), eps);
      }
    }
    if constexpr (MODE != MR_DOT_ALPHA) {
      __syncthreads();
      for (long p = tid; p < (long)st.S * K; p += MR_THREADS) {
        const int s = (int)(p / K), k = (int)(p % K);
        const long sys = (long)g * K + k;
        mr_givens(st, step, (long)s * st.GK() + sys, sys, s);
      }
    }
  }
}

// grid (nblk, min(G, 65535)).  search: [2][S][G][N][K]; sol: [S][G][N][K]; q == nullptr: the ring's previous vector; qc nullable.
template <class T, int V>
__global__ void __launch_bounds__(MR_THREADS) k_minres_update(T* __restrict__ zring, const T* __restrict__ q, T* __restrict__ qc, T* __restrict__ search,
                                                             T* __restrict__ sol, MrState st, unsigned* __restrict__ ticket, long N, int nblk) {
  __shared__ int last;
  const int K = st.K, G = st.G, S = st.S;
  const long step = (long)*st.step(), GNK = (long)G * N * K;
  const int cur = (int)(step & 1);
  const MrWalk w(N, K, V, nblk);
  for (int g = blockIdx.y; g < G && w.active; g += gridDim.y) {
    const long seg = (long)g * N * K;
    T* z = zring + cur * GNK + seg;
    const T* qs = (q ? q : zring + (1 - cur) * GNK) + seg;
    for (int s = 0; s < S; ++s) {
      T bc[V], sub[V], subsub[V], diag[V], scale[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const long sys = (long)g * K + w.col(K, V, e), pair = (long)s * st.GK() + sys;
        bc[e] = (T)st.beta(1 - cur)[sys];
        sub[e] = (T)st.sub()[pair];
        subsub[e] = (T)st.subsub()[pair];
        diag[e] = (T)st.diag()[pair];
        scale[e] = (T)st.scale(cur)[pair];
      }
      const T* s1 = search + ((long)(1 - cur) * S + s) * GNK + seg;
      T* s2 = search + ((long)cur * S + s) * GNK + seg;
      T* xs = sol + (long)s * GNK + seg;
      for (long i = w.first; i < w.count; i += w.stride) {
        if (s == 0) {
          Vec<T, V> zv = Vec<T, V>::ld(z, i);
#pragma unroll
          for (int e = 0; e < V; ++e) zv.v[e] /= bc[e];
          zv.st(z, i);
          if (qc) {
            Vec<T, V> cv = Vec<T, V>::ld(qc + seg, i);
#pragma unroll
            for (int e = 0; e < V; ++e) cv.v[e] /= bc[e];
            cv.st(qc + seg, i);
          }
        }
        const Vec<T, V> qv = Vec<T, V>::ld(qs, i), a = Vec<T, V>::ld(s1, i);
        Vec<T, V> b = Vec<T, V>::ld(s2, i), xv = Vec<T, V>::ld(xs, i);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          b.v[e] = (qv.v[e] - sub[e] * a.v[e] - subsub[e] * b.v[e]) / diag[e];
          xv.v[e] += b.v[e] * scale[e];
        }
        b.st(s2, i);
        xv.st(xs, i);
      }
    }
  }
  // every workgroup has read the counter before it takes its ticket: the last one advances it
  if (dpx_last_block(ticket, gridDim.x * gridDim.y, &last) && threadIdx.x == 0) *st.step() = step + 1;
}

// mode 0: out = in / norm; 1: out = in / beta[0]; 2: out = zero ? 0 : in * norm   (per system; grid as above)
template <class T, int V>
__global__ void __launch_bounds__(MR_THREADS) k_minres_colscale(T* __restrict__ out, const T* __restrict__ in, MrState st, int mode, long N, int nblk) {
  const int K = st.K, G = st.G;
  const MrWalk w(N, K, V, nblk);
  if (!w.active) return;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const long seg = (long)g * N * K;
    T c[V];
    bool zero[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const long sys = (long)g * K + w.col(K, V, e);
      c[e] = (T)(mode == 1 ? st.beta(0)[sys] : st.norm()[sys]);
      zero[e] = mode == 2 && st.zero()[sys] != 0.0;
    }
    for (long i = w.first; i < w.count; i += w.stride) {
      Vec<T, V> v = Vec<T, V>::ld(in + seg, i);
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] = mode == 2 ? (zero[e] ? T(0) : v.v[e] * c[e]) : v.v[e] / c[e];
      v.st(out + seg, i);
    }
  }
}

// one workgroup.  phase 0: alpha holds <b, b>: norm and the "is zero" mark (:69-71).  phase 1: alpha holds <z, q> of the scaled
// right-hand side: beta_prev, the rotations, the scales (:95-129), and the counter.
__global__ void __launch_bounds__(MR_THREADS) k_minres_init(MrState st, int phase) {
  const long GK = st.GK(), P = st.P();
  if (phase == 0) {
    for (long i = threadIdx.x; i < GK; i += MR_THREADS) {
      const double n = sqrt(st.alpha()[i]);
      const bool z = n < 1e-10;
      st.norm()[i] = z ? 1.0 : n;
      st.zero()[i] = z ? 1.0 : 0.0;
    }
    return;
  }
  for (long i = threadIdx.x; i < GK; i += MR_THREADS) {
    st.beta(0)[i] = sqrt(st.alpha()[i]);
    st.beta(1)[i] = 0.0;
  }
  for (long p = threadIdx.x; p < P; p += MR_THREADS) {
    for (int r = 0; r < 3; ++r) st.cosr(r)[p] = 1.0, st.sinr(r)[p] = 0.0;
    st.subsub()[p] = st.sub()[p] = st.diag()[p] = 0.0;
    st.scale(0)[p] = sqrt(st.alpha()[p % GK]);
    st.scale(1)[p] = 0.0;
  }
  if (threadIdx.x == 0) *st.step() = 0;
}

// elements of a leading system per workgroup (up to the cap of 2048 workgroups per launch)
constexpr int MR_BLOCK_ELEMS = 4096;
int mr_blocks(int G, long N, int K) {
  long nb = (N * K + MR_BLOCK_ELEMS - 1) / MR_BLOCK_ELEMS;
  const long cap = G >= 2048 ? 1 : 2048 / G, floor_ = ((long)K + MR_THREADS - 1) / MR_THREADS;
  if (nb > cap) nb = cap;
  if (nb < floor_) nb = floor_;
  return (int)nb;
}
// the C ABI's is_f64 as the element type: f(double()) or f(float())
template <class F> void mr_dispatch_type(int is_f64, F&& f) {
  dispatch_flag(is_f64 != 0, [&](auto f64) { f(std::conditional_t<decltype(f64)::value, double, float>()); });
}
// the vector length of a launch as IntTag<V>: 16 bytes when the layout and every buffer (a null one does not object) allow it, or 1
template <class T, class F> void mr_dispatch_vec(long N, int K, std::initializer_list<const void*> bufs, F&& f) {
  constexpr int V = 16 / sizeof(T);
  dispatch_flag((K == 1 ? N % V == 0 : K % V == 0) && aligned16(bufs), [&](auto vec) { f(IntTag<decltype(vec)::value ? V : 1>()); });
}
bool mr_shape_ok(const char* who, int S, int G, long N, int K) {
  if (S >= 1 && G >= 1 && N >= 1 && K >= 1 && (double)G * (double)N * (double)K * (double)S < 9.0e18) return true;
  set_error("%s: bad shape S=%d G=%d N=%ld K=%d", who, S, G, N, K);
  return false;
}

template <class T, int MODE>
void mr_launch_pass(const void* x, const void* y, void* zring, const MrState& st, void* ws, long N, double value, double eps, hipStream_t stream) {
  const int nblk = mr_blocks(st.G, N, st.K);
  const dim3 grid(nblk, st.G < 65535 ? st.G : 65535, 1);
  unsigned* counter = (unsigned*)ws;
  T* partial = (T*)((char*)ws + ticket_bytes(st.G + 1));
  mr_dispatch_vec<T>(N, st.K, {x, y, zring}, [&](auto v) {
    DPX_LAUNCH("k_minres_pass", (k_minres_pass<T, decltype(v)::value, MODE>), grid, dim3(MR_THREADS), 0, stream, (const T*)x, (const T*)y, (T*)zring, st,
               partial, counter, N, value, eps, nblk);
  });
}

template <class T>
void mr_launch_update(void* zring, const void* q, void* qc, void* search, void* sol, const MrState& st, void* ws, long N, hipStream_t stream) {
  const int nblk = mr_blocks(st.G, N, st.K);
  const dim3 grid(nblk, st.G < 65535 ? st.G : 65535, 1);
  unsigned* ticket = (unsigned*)ws + st.G;
  mr_dispatch_vec<T>(N, st.K, {zring, q, qc, search, sol}, [&](auto v) {
    DPX_LAUNCH("k_minres_update", (k_minres_update<T, decltype(v)::value>), grid, dim3(MR_THREADS), 0, stream, (T*)zring, (const T*)q, (T*)qc, (T*)search,
               (T*)sol, st, ticket, N, nblk);
  });
}

template <class T> void mr_launch_colscale(void* out, const void* in, const MrState& st, int mode, long N, hipStream_t stream) {
  const int nblk = mr_blocks(st.G, N, st.K);
  const dim3 grid(nblk, st.G < 65535 ? st.G : 65535, 1);
  mr_dispatch_vec<T>(N, st.K, {out, in}, [&](auto v) {
    DPX_LAUNCH("k_minres_colscale", (k_minres_colscale<T, decltype(v)::value>), grid, dim3(MR_THREADS), 0, stream, (T*)out, (const T*)in, st, mode, N, nblk);
  });
}

}  // namespace
}  // namespace dpx

extern "C" size_t dpx_minres_state_bytes(int S, int G, int K) {
  if (S < 1 || G < 1 || K < 1) return 0;
  return dpx::MrState::doubles(S, G, K) * sizeof(double);
}

extern "C" size_t dpx_minres_ws_bytes(int G, long N, int K) {
  if (G < 1 || N < 1 || K < 1) return 0;
  return dpx::ticket_bytes(G + 1) + (size_t)G * K * dpx::mr_blocks(G, N, K) * sizeof(double);
}

extern "C" int dpx_minres_init(void* state, int phase, int S, int G, int K, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(state, "dpx_minres_init: null pointer");
  DPX_REQUIRE(phase == 0 || phase == 1, "dpx_minres_init: phase %d (0 or 1)", phase);
  if (!mr_shape_ok("dpx_minres_init", S, G, 1, K)) return DPX_ERR_ARG;
  const MrState st{(double*)state, S, G, K};
  DPX_LAUNCH("k_minres_init", k_minres_init, dim3(1), dim3(MR_THREADS), 0, (hipStream_t)stream, st, phase);
  return launch_status("dpx_minres_init");
}

extern "C" int dpx_minres_colscale(void* out, const void* in, void* state, int mode, int S, int G, long N, int K, int is_f64, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(out && in && state, "dpx_minres_colscale: null pointer");
  DPX_REQUIRE(mode >= 0 && mode <= 2, "dpx_minres_colscale: mode %d (0 .. 2)", mode);
  if (!mr_shape_ok("dpx_minres_colscale", S, G, N, K)) return DPX_ERR_ARG;
  const MrState st{(double*)state, S, G, K};
  mr_dispatch_type(is_f64, [&](auto t) { mr_launch_colscale<decltype(t)>(out, in, st, mode, N, (hipStream_t)stream); });
  return launch_status("dpx_minres_colscale");
}

extern "C" int dpx_minres_alpha(const void* prod, const void* q, const void* zring, double value, void* state, int S, int G, long N, int K, int is_f64,
                                void* ws, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(prod && (q || zring) && state && ws, "dpx_minres_alpha: null pointer");
  if (!mr_shape_ok("dpx_minres_alpha", S, G, N, K)) return DPX_ERR_ARG;
  const MrState st{(double*)state, S, G, K};
  mr_dispatch_type(is_f64, [&](auto t) { mr_launch_pass<decltype(t), MR_DOT_ALPHA>(prod, q, (void*)zring, st, ws, N, value, 0.0, (hipStream_t)stream); });
  return launch_status("dpx_minres_alpha");
}

extern "C" int dpx_minres_lanczos(const void* prod, void* zring, double value, double eps, int finish, void* state, int S, int G, long N, int K,
                                  int is_f64, void* ws, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(prod && zring && state && ws, "dpx_minres_lanczos: null pointer");
  if (!mr_shape_ok("dpx_minres_lanczos", S, G, N, K)) return DPX_ERR_ARG;
  const MrState st{(double*)state, S, G, K};
  const hipStream_t s = (hipStream_t)stream;
  mr_dispatch_type(is_f64, [&](auto t) {
    if (finish) mr_launch_pass<decltype(t), MR_LANCZOS>(prod, nullptr, zring, st, ws, N, value, eps, s);
    else mr_launch_pass<decltype(t), MR_LANCZOS_PLAIN>(prod, nullptr, zring, st, ws, N, value, eps, s);
  });
  return launch_status("dpx_minres_lanczos");
}

extern "C" int dpx_minres_beta(const void* zring, const void* qc, double eps, void* state, int S, int G, long N, int K, int is_f64, void* ws,
                               dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(zring && qc && state && ws, "dpx_minres_beta: null pointer");
  if (!mr_shape_ok("dpx_minres_beta", S, G, N, K)) return DPX_ERR_ARG;
  const MrState st{(double*)state, S, G, K};
  mr_dispatch_type(is_f64, [&](auto t) { mr_launch_pass<decltype(t), MR_DOT_BETA>(nullptr, qc, (void*)zring, st, ws, N, 1.0, eps, (hipStream_t)stream); });
  return launch_status("dpx_minres_beta");
}

extern "C" int dpx_minres_update(void* zring, const void* q, void* qc, void* search, void* solution, void* state, int S, int G, long N, int K,
                                 int is_f64, void* ws, dpx_stream_t stream) {
  using namespace dpx;
  DPX_REQUIRE(zring && search && solution && state && ws, "dpx_minres_update: null pointer");
  if (!mr_shape_ok("dpx_minres_update", S, G, N, K)) return DPX_ERR_ARG;
  const MrState st{(double*)state, S, G, K};
  mr_dispatch_type(is_f64, [&](auto t) { mr_launch_update<decltype(t)>(zring, q, qc, search, solution, st, ws, N, (hipStream_t)stream); });
  return launch_status("dpx_minres_update");
}
