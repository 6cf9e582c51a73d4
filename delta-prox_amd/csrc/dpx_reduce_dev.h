// The reduction pieces every solver kernel shares, each written once: the wave butterflies, the block-level sum, 16-byte-or-element
// vector access, and the deterministic two-stage reduction's hand-over ("the last workgroup to arrive finishes": no spinning, a
// workgroup never waits for another one) with the host-side tests that go with them.  Not part of the C ABI.
#pragma once
#include <initializer_list>

#include "dpx_common.h"

namespace dpx {

// ---- one wave: the 64-lane xor butterfly (float or double); the result is in every lane -------------------------------------
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// ---- one workgroup: sum (MAX: maximum of values >= 0) over its blockDim.x = 64 .. 1024 threads, a multiple of 64 -------------
// sh: one T per wave.  The result is valid in thread 0.  The barrier in front of the write to sh makes repeated calls on one sh
// safe: no wave overwrites a slot that wave 0 of the previous call has yet to read.
template <class T, bool MAX = false> __device__ __forceinline__ T block_sum(T v, T* sh) {
  v = MAX ? wave_max(v) : wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  T r = T(0);
  if (wid == 0) {
    r = lane < (int)(blockDim.x >> 6) ? sh[lane] : T(0);
    r = MAX ? wave_max(r) : wave_sum(r);
  }
  return r;                                              // valid in thread 0
}

// ---- V consecutive elements: one 16-byte access (V = 16 / sizeof(T): float4 / double2; p 16-byte aligned) or V = 1 -----------
// i counts vectors.
template <class T, int V> struct Vec {
  static_assert(V == 1 || V * sizeof(T) == 16, "one element or 16 bytes");
  T v[V];
  __device__ __forceinline__ static Vec ld(const T* p, long i) {
    Vec r;
    if constexpr (V == 1) {
      r.v[0] = p[i];
    } else if constexpr (sizeof(T) == 4) {
      const float4 t = ((const float4*)p)[i];
      r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
      const double2 t = ((const double2*)p)[i];
      r.v[0] = t.x, r.v[1] = t.y;
    }
    return r;
  }
  __device__ __forceinline__ void st(T* p, long i) const {
    if constexpr (V == 1) p[i] = v[0];
    else if constexpr (sizeof(T) == 4) ((float4*)p)[i] = make_float4(v[0], v[1], v[2], v[3]);
    else ((double2*)p)[i] = make_double2(v[0], v[1]);
  }
};

// ---- the two-stage reduction: write-through partials, an integer ticket, the last workgroup adds them in a fixed order ---------
// The contract, in one place:
//   1. every workgroup writes the partial results it hands over with dpx_st_agent, nothing else;
//   2. then every thread of it calls dpx_last_block (block-uniform control flow) on a counter that was zero before the launch;
//   3. the one workgroup that gets `true` -- and only that one -- reads all partials with plain loads (dpx_ld_agent,
//      sum_partials_f64) and finishes; the counter is zero again for the next launch.
// No floating-point atomics, no workgroup waits for another: two launches give the same bits.

// a value another workgroup (possibly behind another XCD's L2) wrote before it took its ticket.  dpx_last_block's acquire fence
// (agent scope: the L2's non-coherent lines are invalidated) makes plain loads safe; atomic (sc1) loads here serialised into one
// memory round trip each -- 13 .. 200 dependent round trips per wave: the fused iteration ran 20 % SLOWER than the unfused one.
__device__ __forceinline__ float dpx_ld_agent(const float* p) { return *p; }

// Every workgroup calls this after its own results are written: release them (agent scope), take a ticket, and learn -- uniformly --
// whether it is the last of `nblocks` to arrive; the last one acquires and resets the counter for the next launch.
//
// The results a workgroup hands over must have been written with dpx_st_agent (write-through stores): the release side is then just
// "my stores have completed" (s_waitcnt) in front of an agent-scope ticket -- a full release fence writes the XCD's whole L2 back,
// once per workgroup: measured 47 us on an 800-workgroup launch whose own work takes 9 us.  Only the last workgroup pays an acquire
// (L2 invalidate) before it reads the others' results with plain loads.
__device__ __forceinline__ void dpx_st_agent(float* p, float v) {
#ifdef DPX_EMULATED
  *p = v;
#else
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ void dpx_st_agent(double* p, double v) {
#ifdef DPX_EMULATED
  *p = v;
#else
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ bool dpx_last_block(unsigned* counter, unsigned nblocks, int* sh_flag) {
#ifdef DPX_EMULATED
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ticket = atomicAdd(counter, 1u);
    *sh_flag = (ticket == nblocks - 1);
    if (ticket == nblocks - 1) *counter = 0u;
  }
  __syncthreads();
  return *sh_flag != 0;
#else
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *sh_flag = (ticket == nblocks - 1);
    if (ticket == nblocks - 1) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const bool last = *sh_flag != 0;
  if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return last;
#endif
}

// the finishing step of one wave of the last workgroup: n partials (float or double) added in lane-strided order in float64, then
// the butterfly; the sum is in every lane
template <class T> __device__ __forceinline__ double sum_partials_f64(const T* p, int n) {
  double s = 0.0;
  for (int i = threadIdx.x & 63; i < n; i += 64) s += (double)p[i];
  return wave_sum(s);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// every buffer may be accessed 16 bytes at a time (an absent, null buffer does not object)
static inline bool aligned16(std::initializer_list<const void*> bufs) {
  for (const void* p : bufs)
    if ((size_t)p % 16 != 0) return false;
  return true;
}
// bytes of n tickets at the head of a workspace: rounded up to 256, so that the partials behind them keep the workspace's alignment
static inline size_t ticket_bytes(size_t n) { return (n * sizeof(unsigned) + 255) & ~(size_t)255; }

}  // namespace dpx
