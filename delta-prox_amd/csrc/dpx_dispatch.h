// Host-side launch dispatch of the row kernels ("Launching"): run-time plane width / term count / flags -> compile-time
// tags, each written once.  A dispatcher calls the generic lambda `f` with the tag of the value it was given; launchers nest them
// and issue DPX_LAUNCH_LDS in the innermost lambda, whose call operator is instantiated once per kernel instantiation (so is the
// launch's function-local LdsGrant).  Not part of the C ABI.
#pragma once
#include <type_traits>

namespace dpx {

// a row of W = 2 M real pixels = M complex points, transformed by T lanes
template <int M_, int T_> struct RowShape { static constexpr int M = M_, T = T_; };
template <int N> using IntTag = std::integral_constant<int, N>;

// The two width maps.  f returns whether it launched; both maps return that, and false (without calling f) for a width they do not
// hold.  A launcher whose kernel exists for a subset says so with one `if constexpr` on the shape that returns false.
// One wave per row (the streaming and row-parallel kernels, k_seed_rows): 768-wide rows as M = 384 = 6 * 8 * 8 on 64 lanes.
template <class F> static inline bool dispatch_rows_wave(int W, F&& f) {
  switch (W) {
    case 256: return f(RowShape<128, 16>{});
    case 512: return f(RowShape<256, 32>{});
    case 768: return f(RowShape<384, 64>{});
    case 1024: return f(RowShape<512, 64>{});
    default: return false;
  }
}
// The plain row kernels (k_rows_r2c_p2 / k_rows_c2r_p2, k_pgd_rows, the lock-step iteration kernels): 768 and 1536 on 16 / 32 lanes.
template <class F> static inline bool dispatch_rows_plain(int W, F&& f) {
  switch (W) {
    case 256: return f(RowShape<128, 16>{});
    case 512: return f(RowShape<256, 32>{});
    case 768: return f(RowShape<384, 16>{});
    case 1536: return f(RowShape<768, 32>{});            // (the three-times-a-power-of-two widths on a third of the lanes of 2 W / 3)
    case 1024: return f(RowShape<512, 64>{});
    case 2048: return f(RowShape<1024, 64>{});
    default: return false;
  }
}

// lanes per row of the one-wave map, which the lock-step kernels share for 256 / 512 / 1024 (0: a width the map does not hold) -- for
// the host rules that count rows in flight
static inline int rows_wave_lanes(int W) {
  int T = 0;
  dispatch_rows_wave(W, [&](auto shape) { T = decltype(shape)::T; return true; });
  return T;
}

// number of Psi terms, 1 .. DPX_MAX_TERMS (= 4); the entry points have checked the range
template <class F> static inline void dispatch_nterms(int n, F&& f) {
  switch (n) {
    case 1: f(IntTag<1>{}); break;
    case 2: f(IntTag<2>{}); break;
    case 3: f(IntTag<3>{}); break;
    default: f(IntTag<4>{}); break;
  }
}

// a kernel's boolean template flag (DUAL, VXU, HB, KTB, FRESH)
template <class F> static inline void dispatch_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// "Every T-lane group of the launch resident, rounded UP to a power of two": the band count the streaming kernels start from
// (2 workgroups of 4 waves of G groups on each of the 256 CUs, shared by the planes of `share` chains).  H is a power of two times
// 1 or 3, so bands of equal length exist; each launcher applies its own caps and factors to the result.
static inline int resident_bands_pow2(int G, int P, int share) {
  const int nb = (256 * 2 * 4 * G) / (P * share);
  int p2 = 1;
  while (p2 < nb) p2 <<= 1;
  return p2;
}

}  // namespace dpx
