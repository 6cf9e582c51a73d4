// GRUNet, the hyperspectral denoiser of the reference's hsi_* examples (models/qrnn/grunet.py, layer.py, conv.py): every layer is a 3-D
// convolution that produces GATES, followed by QRNN "f-pooling" along the band axis D,
//
//   Z = tanh(gates[:C])   F = sigmoid(gates[C:])      h_0 = (1 - f_0) z_0      h_d = f_d h_{d-1} + (1 - f_d) z_d        (reverse: d from D - 1 down)
//
// Two kernels per layer:
//   k_conv3d_gates   the convolution as an implicit GEMM on the 16-bit matrix cores at fp32 accuracy: dpx_mma_dev.h's split-f16 (mode 3, three
//                    products, operands inside the binary16 range -- the range trap of dpx_conv_bf16.hip watches them) or split-bf16 (mode 6,
//                    six products, any range).  M = gate channels (A = packed weights), N = 32 output pixels, K = 16 input channels of one tap.
//   k_qrnn_pool      one streaming pass: activations, the scan along D in registers, the block's second pooled operand, the final + x.
//
// Layout: activations and gates are band-major C8, [N][D][C/8][H][W][8] fp32 -- a band is one C8 image of dpx_conv_bf16.hip's layout, a
// (pixel, 8-channel group) is the B operand of one lane, and a depth tap is a whole-band offset, so a band outside [0, D) is skipped
// by the whole wave.  A wave owns 64 consecutive pixels of one band (two B tiles) times MT x 32 gate channels and runs the K loop over
// (depth taps) x (16-channel chunks) x (in-plane taps); operands come straight from global memory (the weights of a layer are shared by
// every wave and stay in L2), are split in registers and go to the matrix instruction: no LDS, no barrier.
// The four convolution forms are variants of this one kernel -- they differ in the SOURCE ADDRESS of a tap only, so none of them moves a byte
// more than the plain form: stride (1, 2, 2) doubles the pixel coordinate, k = 1 has one tap, and upsample-input (trilinear, depth factor 1,
// align_corners: in-plane bilinear) interpolates the four source pixels of the tap on the fly, the zero padding applying to the upsampled
// plane.  ConvTranspose3d (k = 3, s = 1, p = 1  ==  the convolution with flipped taps and swapped channel axes) is a matter of the packing
// kernel.
#include "dpx_common.h"
#include "dpx_mma_dev.h"

namespace dpx {
namespace {

enum QForm { Q_K3 = 0, Q_DOWN = 1, Q_K1 = 2, Q_UP = 3 };
enum QDir { Q_FWD = 0, Q_REV = 1, Q_BI = 2 };

constexpr int Q_THREADS = 256, Q_WAVES = Q_THREADS / 64, Q_PIX = 64;       // a wave's pixels: two B tiles of 32

constexpr int q_planes(int mode) { return mode == 3 ? 2 : 3; }
constexpr int q_taps(int form) { return form == Q_K1 ? 1 : 27; }
constexpr int q_chunks(int cin) { return (cin + 15) / 16; }
constexpr int q_groups(int c) { return 2 * q_chunks(c); }                  // channel groups of a C8 buffer: whole 16-channel chunks
constexpr int q_m32(int cout) { return cout <= 32 ? 32 : (cout + 63) / 64 * 64; }      // gate rows of the packed layer (MT = 1 / MT = 2 tiles)
inline int q_out(int form, int n) { return form == Q_DOWN ? (n - 1) / 2 + 1 : (form == Q_UP ? 2 * n : n); }
inline bool q_mode_ok(int mode) { return mode == 3 || mode == 6; }
inline bool q_form_ok(int form) { return form >= Q_K3 && form <= Q_UP; }

// packed layer: [chunk][tap][plane NPW][k-group 2][gate row M32][8] 16-bit, then the bias fp32 [M32]
inline size_t q_weight_elems(int form, int cin, int cout, int mode) {
  return (size_t)q_chunks(cin) * q_taps(form) * q_planes(mode) * 2 * q_m32(cout) * 8;
}
inline size_t q_layer_bytes(int form, int cin, int cout, int mode) { return q_weight_elems(form, cin, cout, mode) * 2 + (size_t)q_m32(cout) * 4; }

// w: Conv3d [cout][cin][taps] or, tr, ConvTranspose3d [cin][cout][taps] with the taps flipped; b [cout] (nullable)
__global__ void k_qrnn_pack(const float* __restrict__ w, const float* __restrict__ b, unsigned short* __restrict__ dst, int cin, int cout, int taps,
                            int tr, int mode, unsigned* __restrict__ ovf) {
  const int chunks = q_chunks(cin), M32 = q_m32(cout), NPW = q_planes(mode);
  const long nw = (long)chunks * taps * NPW * 2 * M32 * 8;
  float* bias = (float*)(dst + nw);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nw + M32; i += (long)gridDim.x * blockDim.x) {
    if (i >= nw) {
      const int k = (int)(i - nw);
      bias[k] = (k < cout && b) ? b[k] : 0.f;
      continue;
    }
    const int j = (int)(i % 8);
    long r = i / 8;
    const int co = (int)(r % M32);
    r /= M32;
    const int kg = (int)(r % 2);
    r /= 2;
    const int plane = (int)(r % NPW);
    r /= NPW;
    const int tap = (int)(r % taps), chunk = (int)(r / taps);
    const int ci = chunk * 16 + kg * 8 + j;
    const float v = (co < cout && ci < cin) ? (tr ? w[((long)ci * cout + co) * taps + (taps - 1 - tap)] : w[((long)co * cin + ci) * taps + tap]) : 0.f;
    unsigned h, m, l;
    if (mode == 3) {
      split2_f16(v, h, m);
      l = 0u;
      if (!(fabsf(v) <= 6.0e4f)) atomicOr(ovf, 1u);
    } else {
      split3(v, h, m, l);
    }
    dst[i] = (unsigned short)((plane == 0 ? h : (plane == 1 ? m : l)) >> 16);
  }
}

// x [N][C][D][H W] -> band-major C8 [N][D][G][H W][8]; channel C = sigma[n] where sigma is given; the channels behind: zero
__global__ void k_qrnn_to_c8(const float* __restrict__ x, const float* __restrict__ sigma, float* __restrict__ a, int N, int C, int D, long HW, int G) {
  const long total = (long)N * D * G * HW * 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i % 8);
    long r = i / 8;
    const long p = r % HW;
    r /= HW;
    const int g = (int)(r % G);
    r /= G;
    const int d = (int)(r % D), n = (int)(r / D), c = g * 8 + j;
    a[i] = c < C ? x[(((long)n * C + c) * D + d) * HW + p] : ((c == C && sigma) ? sigma[n] : 0.f);
  }
}

struct QConv {
  const float* in;      // C8 [N][D][Gin][Hi Wi][8]
  float* out;           // gates, C8 [N][D][Gout][Ho Wo][8]
  const char* wpk;
  unsigned* ovf;        // the split-f16 range trap's word
  int Gin, chunks;      // groups of the input buffer; 16-channel chunks read (from group 0: a prefix of the buffer's channels)
  int D, Hi, Wi, Ho, Wo;
  int Gout, M32;
  int tiles_c, tiles_p; // gate-channel tiles of MT x 32, pixel tiles of Q_PIX
  int items;            // N D tiles_c tiles_p
  float sy, sx;         // Q_UP: (Hi - 1) / (Ho - 1), (Wi - 1) / (Wo - 1)
};

// the eight channels of group `gb` (a band's group base) at source position (iy, ix) of tap (kh, kw) for output pixel (oy, ox); zero padding
template <int FORM> __device__ __forceinline__ void q_fetch(const QConv& A, const float* __restrict__ gb, bool live, int oy, int ox, int kh, int kw, float v[8]) {
  int iy, ix;
  if constexpr (FORM == Q_K1) iy = oy, ix = ox;
  else if constexpr (FORM == Q_DOWN) iy = 2 * oy + kh - 1, ix = 2 * ox + kw - 1;
  else iy = oy + kh - 1, ix = ox + kw - 1;
  if constexpr (FORM == Q_UP) {
    const bool ok = live && iy >= 0 && iy < A.Ho && ix >= 0 && ix < A.Wo;       // (the padding applies to the upsampled plane)
    if (!ok) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
      return;
    }
    const float fy = A.sy * (float)iy, fx = A.sx * (float)ix;
    const int y0 = min((int)fy, A.Hi - 1), x0 = min((int)fx, A.Wi - 1);
    const int y1 = y0 + (y0 < A.Hi - 1 ? 1 : 0), x1 = x0 + (x0 < A.Wi - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
    const float my = 1.f - ly, mx = 1.f - lx;
    const float* p00 = gb + ((size_t)y0 * A.Wi + x0) * 8;
    const float* p01 = gb + ((size_t)y0 * A.Wi + x1) * 8;
    const float* p10 = gb + ((size_t)y1 * A.Wi + x0) * 8;
    const float* p11 = gb + ((size_t)y1 * A.Wi + x1) * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 a = *(const float4*)(p00 + 4 * h), b = *(const float4*)(p01 + 4 * h), c = *(const float4*)(p10 + 4 * h), d = *(const float4*)(p11 + 4 * h);
      v[4 * h + 0] = my * (mx * a.x + lx * b.x) + ly * (mx * c.x + lx * d.x);
      v[4 * h + 1] = my * (mx * a.y + lx * b.y) + ly * (mx * c.y + lx * d.y);
      v[4 * h + 2] = my * (mx * a.z + lx * b.z) + ly * (mx * c.z + lx * d.z);
      v[4 * h + 3] = my * (mx * a.w + lx * b.w) + ly * (mx * c.w + lx * d.w);
    }
  } else {
    const bool ok = live && iy >= 0 && iy < A.Hi && ix >= 0 && ix < A.Wi;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (ok) {
      const float* p = gb + ((size_t)iy * A.Wi + ix) * 8;
      a = *(const float4*)p;
      b = *(const float4*)(p + 4);
    }
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
}

// MT: 32-row gate tiles of a wave; MODE 3 split-f16 / 6 split-bf16; FORM: the source address of a tap.  No bias-free form: the bias plane of
// a layer without one is zero.
template <int MT, int MODE, int FORM>
__global__ void __launch_bounds__(Q_THREADS) k_conv3d_gates(const QConv A) {
  constexpr int NPL = MODE == 3 ? 2 : 3, KD = FORM == Q_K1 ? 1 : 3, KHW = FORM == Q_K1 ? 1 : 3;
  const int lane = threadIdx.x & 63, n = lane & 31, kg = lane >> 5;
  const int item = (int)blockIdx.x * Q_WAVES + (int)(threadIdx.x >> 6);           // wave-uniform
  if (item >= A.items) return;
  const int pt = item % A.tiles_p;
  int r_ = item / A.tiles_p;
  const int ct = r_ % A.tiles_c;
  r_ /= A.tiles_c;
  const int d = r_ % A.D, nb = r_ / A.D;
  const int HWo = A.Ho * A.Wo;
  const size_t HWi = (size_t)A.Hi * A.Wi;
  bool live[2];
  int oy[2], ox[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int p = pt * Q_PIX + r * 32 + n;
    live[r] = p < HWo;
    oy[r] = live[r] ? p / A.Wo : 0;
    ox[r] = live[r] ? p - oy[r] * A.Wo : 0;
  }
  f32x16 acc[MT][2];
  f32x16 accx[MODE == 3 ? MT : 1][2];                                 // split-f16: the two cross terms, scaled by 2^11
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        acc[mt][r][i] = 0.f;
        if (MODE == 3) accx[MODE == 3 ? mt : 0][r][i] = 0.f;
      }
  float f16_max = 0.f;
  const size_t tapb = (size_t)NPL * 2 * A.M32 * 16;                    // bytes of one (chunk, tap) of the packed layer
  const char* wrow = A.wpk + ((size_t)kg * A.M32 + (size_t)ct * MT * 32 + n) * 16;

#pragma unroll 1
  for (int kd = 0; kd < KD; ++kd) {
    const int dd = d + kd - (KD == 3 ? 1 : 0);
    if (dd < 0 || dd >= A.D) continue;                                 // a band outside the cube contributes nothing (wave-uniform)
    const float* band = A.in + ((size_t)nb * A.D + dd) * A.Gin * HWi * 8;
#pragma unroll 1
    for (int c = 0; c < A.chunks; ++c) {
      const float* gb = band + (size_t)(2 * c + kg) * HWi * 8;
      const char* wc = wrow + ((size_t)c * (KD * KHW * KHW) + (size_t)kd * (KHW * KHW)) * tapb;
#pragma unroll 1
      for (int kh = 0; kh < KHW; ++kh) {
#pragma unroll
        for (int kw = 0; kw < KHW; ++kw) {
          uint4 bf[2][NPL];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            float v[8];
            q_fetch<FORM>(A, gb, live[r], oy[r], ox[r], kh, kw, v);
            if constexpr (MODE == 3) {
              unsigned hw[4], lw[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) split2_f16_pair(v[2 * j], v[2 * j + 1], hw[j], lw[j]);
              bf[r][0] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
              bf[r][1] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
              f16_max = fmaxf(f16_max, fmaxf(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))),
                                             fmaxf(fmaxf(fabsf(v[4]), fabsf(v[5])), fmaxf(fabsf(v[6]), fabsf(v[7])))));
            } else {
              unsigned h[8], m[8], l[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) split3(v[j], h[j], m[j], l[j]);
              bf[r][0] = make_uint4(pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]), pack_hi16(h[4], h[5]), pack_hi16(h[6], h[7]));
              bf[r][1] = make_uint4(pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]), pack_hi16(m[4], m[5]), pack_hi16(m[6], m[7]));
              bf[r][NPL - 1] = make_uint4(pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]), pack_hi16(l[4], l[5]), pack_hi16(l[6], l[7]));
            }
          }
          const char* wt = wc + (size_t)(kh * KHW + kw) * tapb;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            uint4 af[NPL];
#pragma unroll
            for (int p = 0; p < NPL; ++p) af[p] = *(const uint4*)(wt + ((size_t)p * 2 * A.M32 + mt * 32) * 16);
            if constexpr (MODE == 3) {
              accx[mt][0] = mfma_f16(af[1], bf[0][0], accx[mt][0]);     // wl ah   (x 2^11)
              accx[mt][1] = mfma_f16(af[1], bf[1][0], accx[mt][1]);
              acc[mt][0] = mfma_f16(af[0], bf[0][0], acc[mt][0]);       // wh ah
              acc[mt][1] = mfma_f16(af[0], bf[1][0], acc[mt][1]);
              accx[mt][0] = mfma_f16(af[0], bf[0][1], accx[mt][0]);     // wh al   (x 2^11)
              accx[mt][1] = mfma_f16(af[0], bf[1][1], accx[mt][1]);
            } else {
              // small terms first, the leading product last (k_conv3x3_bf16's order)
#pragma unroll
              for (int r = 0; r < 2; ++r) acc[mt][r] = mfma_bf16(af[1], bf[r][1], acc[mt][r]);    // wm am
#pragma unroll
              for (int r = 0; r < 2; ++r) acc[mt][r] = mfma_bf16(af[NPL - 1], bf[r][0], acc[mt][r]);    // wl ah
#pragma unroll
              for (int r = 0; r < 2; ++r) acc[mt][r] = mfma_bf16(af[0], bf[r][NPL - 1], acc[mt][r]);    // wh al
#pragma unroll
              for (int r = 0; r < 2; ++r) acc[mt][r] = mfma_bf16(af[1], bf[r][0], acc[mt][r]);    // wm ah
#pragma unroll
              for (int r = 0; r < 2; ++r) acc[mt][r] = mfma_bf16(af[0], bf[r][1], acc[mt][r]);    // wh am
#pragma unroll
              for (int r = 0; r < 2; ++r) acc[mt][r] = mfma_bf16(af[0], bf[r][0], acc[mt][r]);    // wh ah
            }
          }
        }
      }
    }
  }
  if (MODE == 3 && !(f16_max <= 6.0e4f)) atomicOr(A.ovf, 1u);          // (NaN counts)
  // ---- epilogue: bias, C8 store.  D layout: col = lane & 31 (pixel), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (gate channel) ----
  const float* bias = (const float*)(A.wpk + (size_t)A.chunks * (KD * KHW * KHW) * tapb);
  float* ob = A.out + ((size_t)nb * A.D + d) * A.Gout * (size_t)HWo * 8;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int p = pt * Q_PIX + r * 32 + n;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cl = (ct * MT + mt) * 32 + 8 * q + 4 * kg, cg = cl >> 3;
        if (cg >= A.Gout || !live[r]) continue;
        float4 v;
        v.x = acc[mt][r][4 * q + 0] + bias[cl + 0];
        v.y = acc[mt][r][4 * q + 1] + bias[cl + 1];
        v.z = acc[mt][r][4 * q + 2] + bias[cl + 2];
        v.w = acc[mt][r][4 * q + 3] + bias[cl + 3];
        if constexpr (MODE == 3) {
          constexpr float s = 1.0f / F16_LO_SCALE;
          v.x = fmaf(accx[mt][r][4 * q + 0], s, v.x);
          v.y = fmaf(accx[mt][r][4 * q + 1], s, v.y);
          v.z = fmaf(accx[mt][r][4 * q + 2], s, v.z);
          v.w = fmaf(accx[mt][r][4 * q + 3], s, v.w);
        }
        *(float4*)(ob + ((size_t)cg * HWo + p) * 8 + 4 * kg) = v;
      }
    }
}

struct QPool {
  const float* g;       // gates of the layer, C8 [N][D][Gg][HW][8]: Z = channels [0, C), F = [C, 2C) (bidirectional: F1, then F2 = [2C, 3C))
  const float* g2;      // nullable: the gates of a second layer of the same C and direction, pooled in the same pass and added
  const float* addx;    // nullable (plain destinations): [N][C][D][HW], added last
  float* dst;           // C8 [N][D][Gdst][HW][8] written from channel group `off` on, or plain [N][Cdst][D][HW] from channel `off` on
  int N, C, D, Gg, Gg2, dir, plain, Cdst, off;
  long HW;
};

__device__ __forceinline__ float q_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }      // (x = -100: 1 / inf = 0; no NaN at either end)
__device__ __forceinline__ float q_gate(const float* __restrict__ g, int Gg, long HW, long band, long p, int ch) {
  return g[((band * Gg + (ch >> 3)) * HW + p) * 8 + (ch & 7)];
}
// h_d of one operand: the first step has no h behind it
__device__ __forceinline__ float q_step(float z, float f, float h, bool first) {
  const float zz = (1.f - f) * z;
  return first ? zz : fmaf(f, h, zz);
}

// A thread owns one (image, channel, pixel) and walks the bands with h in a register.  C8 destinations: the eight channels of a pixel on
// neighbouring lanes (32 contiguous bytes per pixel, read and written); plain destinations: neighbouring pixels on neighbouring lanes.
// Bidirectional layers run the walk twice, forward with F1 and backward with F2 (Z read once per direction); the second walk adds to what
// the first one stored in the thread's own cells.
__global__ void __launch_bounds__(256) k_qrnn_pool(const QPool P) {
  const int Cg = P.plain ? P.C : (P.C + 7) / 8 * 8;
  const long total = (long)P.N * Cg * P.HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int c, n;
    long p;
    if (P.plain) {
      p = i % P.HW;
      const long r = i / P.HW;
      c = (int)(r % P.C), n = (int)(r / P.C);
    } else {
      const int j = (int)(i % 8);
      long r = i / 8;
      p = r % P.HW;
      r /= P.HW;
      const int G = Cg / 8;
      c = (int)(r % G) * 8 + j, n = (int)(r / G);
      if (c >= P.C) continue;
    }
    const int passes = P.dir == Q_BI ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
      const bool rev = P.dir == Q_BI ? pass == 1 : P.dir == Q_REV;
      const int fch = P.C * (1 + pass) + c;
      float h = 0.f, h2 = 0.f;
      for (int s = 0; s < P.D; ++s) {
        const int d = rev ? P.D - 1 - s : s;
        const long band = (long)n * P.D + d;
        h = q_step(tanhf(q_gate(P.g, P.Gg, P.HW, band, p, c)), q_sigmoid(q_gate(P.g, P.Gg, P.HW, band, p, fch)), h, s == 0);
        float v = h;
        if (P.g2) {
          h2 = q_step(tanhf(q_gate(P.g2, P.Gg2, P.HW, band, p, c)), q_sigmoid(q_gate(P.g2, P.Gg2, P.HW, band, p, fch)), h2, s == 0);
          v += h2;
        }
        float* o = P.plain ? P.dst + (((long)n * P.Cdst + P.off + c) * P.D + d) * P.HW + p
                           : P.dst + ((band * (P.Cdst / 8) + (P.off + c) / 8) * P.HW + p) * 8 + ((P.off + c) & 7);
        if (pass == 1) v = *o + v;
        if (P.addx && pass == passes - 1) v += P.addx[(((long)n * P.C + c) * P.D + d) * P.HW + p];
        *o = v;
      }
    }
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
// the names a launch is timed under (dpx_timing_report): the network's launches carry their layer class
struct QNames {
  const char *conv, *pool;
};
constexpr QNames QN_LAYER{"k_conv3d_gates", "k_qrnn_pool"}, QN_CONV1{"k_conv3d_gates.Conv1", "k_qrnn_pool.Conv1"},
    QN_DOWN{"k_conv3d_gates.Down", "k_qrnn_pool.Down"}, QN_ENC{"k_conv3d_gates.Conv2-5", "k_qrnn_pool.Conv2-5"}, QN_UP{"k_conv3d_gates.Up", "k_qrnn_pool.Up"},
    QN_DEC{"k_conv3d_gates.Up_conv", "k_qrnn_pool.Up_conv"}, QN_LAST{"k_conv3d_gates.Conv", "k_qrnn_pool.Conv"};

template <int MT, int MODE> void launch_conv_form(const char* name, int form, const QConv& A, dim3 grid, hipStream_t s) {
  switch (form) {
    case Q_K3: DPX_LAUNCH(name, (k_conv3d_gates<MT, MODE, Q_K3>), grid, dim3(Q_THREADS), 0, s, A); break;
    case Q_DOWN: DPX_LAUNCH(name, (k_conv3d_gates<MT, MODE, Q_DOWN>), grid, dim3(Q_THREADS), 0, s, A); break;
    case Q_K1: DPX_LAUNCH(name, (k_conv3d_gates<MT, MODE, Q_K1>), grid, dim3(Q_THREADS), 0, s, A); break;
    default: DPX_LAUNCH(name, (k_conv3d_gates<MT, MODE, Q_UP>), grid, dim3(Q_THREADS), 0, s, A); break;
  }
}

// one gate convolution: `in` C8 with Gin groups of which the first cin channels are read (cin a multiple of 16, or the whole zero-padded
// buffer), gates C8 with ceil(cout / 8) groups on the output plane of the form
void launch_conv(const QNames& nm, int form, int mode, const float* in, int Gin, int cin, float* gates, const char* wpk, int cout, int N, int D, int Hi,
                 int Wi, hipStream_t s) {
  QConv A{};
  A.in = in, A.out = gates, A.wpk = wpk, A.ovf = f16_overflow_flag();
  A.Gin = Gin, A.chunks = q_chunks(cin), A.D = D, A.Hi = Hi, A.Wi = Wi, A.Ho = q_out(form, Hi), A.Wo = q_out(form, Wi);
  A.Gout = (cout + 7) / 8, A.M32 = q_m32(cout);
  const int MT = A.M32 == 32 ? 1 : 2;
  A.tiles_c = A.M32 / (MT * 32), A.tiles_p = (A.Ho * A.Wo + Q_PIX - 1) / Q_PIX;
  const long items = (long)N * D * A.tiles_c * A.tiles_p;
  if (items > 0x7fffffffL - Q_WAVES) return launch_fail("k_conv3d_gates: %ld wave tiles (at most 2^31)", items);
  A.items = (int)items;
  A.sy = A.Ho > 1 ? (float)(Hi - 1) / (float)(A.Ho - 1) : 0.f, A.sx = A.Wo > 1 ? (float)(Wi - 1) / (float)(A.Wo - 1) : 0.f;
  const dim3 grid((unsigned)((items + Q_WAVES - 1) / Q_WAVES));
  if (MT == 1) {
    if (mode == 3) launch_conv_form<1, 3>(nm.conv, form, A, grid, s);
    else launch_conv_form<1, 6>(nm.conv, form, A, grid, s);
  } else {
    if (mode == 3) launch_conv_form<2, 3>(nm.conv, form, A, grid, s);
    else launch_conv_form<2, 6>(nm.conv, form, A, grid, s);
  }
}

void launch_pool(const QNames& nm, const float* g, const float* g2, int C, int dir, float* dst, int plain, int Cdst, int off, const float* addx, int N, int D,
                 long HW, hipStream_t s) {
  QPool P{};
  const int gate_ch = (dir == Q_BI ? 3 : 2) * C;
  P.g = g, P.g2 = g2, P.addx = addx, P.dst = dst, P.N = N, P.C = C, P.D = D, P.Gg = P.Gg2 = (gate_ch + 7) / 8, P.dir = dir, P.plain = plain;
  P.Cdst = Cdst, P.off = off, P.HW = HW;
  const long total = (long)N * (plain ? C : (C + 7) / 8 * 8) * HW;
  DPX_LAUNCH(nm.pool, k_qrnn_pool, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, P);
}

void launch_to_c8(const float* x, const float* sigma, float* a, int N, int C, int D, long HW, int G, hipStream_t s) {
  DPX_LAUNCH("k_qrnn_to_c8", k_qrnn_to_c8, dim3(grid_for((long)N * D * G * HW * 8, 256, 256 * 32)), dim3(256), 0, s, x, sigma, a, N, C, D, HW, G);
}

size_t c8_bytes(int N, int D, int groups, int H, int W) { return ((size_t)N * D * groups * H * W * 8 * sizeof(float) + 255) / 256 * 256; }

bool q_shape_ok(const char* who, int N, int D, int H, int W) {
  if (N < 1 || D < 1 || H < 1 || W < 1) return set_error("%s: bad shape N=%d D=%d H=%d W=%d (every extent at least 1)", who, N, D, H, W), false;
  if ((size_t)N * D * H * W > ((size_t)1 << 40)) return set_error("%s: %zu voxels", who, (size_t)N * D * H * W), false;
  return true;
}

// ---- the network's layer table, in the reference's state-dict order ----------------------------------------------------------------
struct QLayer {
  int form, cin, hidden, dir, tr;
  int gates() const { return (dir == Q_BI ? 3 : 2) * hidden; }
};
constexpr int GRU_LAYERS = 34;
enum { L_DOWN = 0, L_CONV1 = 4, L_ENC = 5, L_DEC = 17, L_LAST = 33 };        // Down1..4 | Conv1 | Conv2..5 (3 each) | (Up, Up_conv x 3) x 4 | Conv
void grunet_layers(int in_ch, QLayer* L) {
  for (int l = 0; l < 4; ++l) L[L_DOWN + l] = QLayer{Q_DOWN, 16 << l, 16 << l, Q_REV, 0};
  L[L_CONV1] = QLayer{Q_K3, in_ch, 16, Q_BI, 0};
  for (int l = 0; l < 4; ++l) {
    const int ci = 16 << l, co = 32 << l;
    L[L_ENC + 3 * l] = QLayer{Q_K3, ci, co, Q_FWD, 0};
    L[L_ENC + 3 * l + 1] = QLayer{Q_K3, co, co, Q_FWD, 0};
    L[L_ENC + 3 * l + 2] = QLayer{Q_K1, ci, co, Q_FWD, 0};
  }
  for (int l = 0; l < 4; ++l) {                                              // Up5 / Up_conv5 first
    const int ci = 256 >> l, co = 128 >> l;
    L[L_DEC + 4 * l] = QLayer{Q_UP, ci, co, Q_REV, 0};
    L[L_DEC + 4 * l + 1] = QLayer{Q_K3, ci, co, Q_FWD, 1};
    L[L_DEC + 4 * l + 2] = QLayer{Q_K3, co, co, Q_FWD, 1};
    L[L_DEC + 4 * l + 3] = QLayer{Q_K1, ci, co, Q_FWD, 1};
  }
  L[L_LAST] = QLayer{Q_K3, 16, 1, Q_BI, 1};
}
size_t grunet_layer_offset(const QLayer* L, int l, int mode) {
  size_t o = 0;
  for (int i = 0; i < l; ++i) o += (q_layer_bytes(L[i].form, L[i].cin, L[i].gates(), mode) + 255) / 256 * 256;
  return o;
}

// the workspace: per level l (plane H / 2^l) the concatenation buffer cat_l (skip | up, 32 * 2^l channels, l < 4), the Down output t_l
// (8 * 2^l, l >= 1), a block's inner activation h_l and its output d_l (16 * 2^l each); the 16-channel input; two gate buffers
struct GruWs {
  size_t in0, cat[4], t[5], h[5], d[5], ga, gb, total;
};
GruWs grunet_ws(int N, int D, int H, int W) {
  GruWs w{};
  size_t o = 0, gmax = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += bytes; return at; };
  w.in0 = take(c8_bytes(N, D, 2, H, W));
  for (int l = 0; l < 5; ++l) {
    const int h = H >> l, ww = W >> l;
    if (l < 4) w.cat[l] = take(c8_bytes(N, D, 4 << l, h, ww));
    if (l >= 1) w.t[l] = take(c8_bytes(N, D, q_groups(8 << l), h, ww));
    w.h[l] = take(c8_bytes(N, D, 2 << l, h, ww));
    w.d[l] = take(c8_bytes(N, D, 2 << l, h, ww));
    // the widest gates of the level: 48 channels at level 0 (Conv1), 2 * 16 * 2^l in the blocks and the Up layer of level l >= 1
    const size_t gl = c8_bytes(N, D, l == 0 ? 6 : 4 << l, h, ww);
    gmax = gl > gmax ? gl : gmax;
  }
  w.ga = take(gmax);
  w.gb = take(gmax);
  w.total = o;
  return w;
}

}  // namespace
}  // namespace dpx

using namespace dpx;

extern "C" size_t dpx_qrnn3d_packed_bytes(int form, int cin, int cout, int mode) {
  if (!q_form_ok(form) || !q_mode_ok(mode) || cin < 1 || cin > 256 || cout < 1 || cout > 1024) {
    set_error("dpx_qrnn3d_packed_bytes: form=%d cin=%d cout=%d mode=%d (form 0..3, cin 1..256, gate cout 1..1024, mode 3 or 6)", form, cin, cout, mode);
    return 0;
  }
  return q_layer_bytes(form, cin, cout, mode);
}

extern "C" int dpx_qrnn3d_pack(void* packed, const float* w, const float* bias, int form, int cin, int cout, int transposed, int mode,
                               dpx_stream_t stream) {
  DPX_REQUIRE(packed && w, "dpx_qrnn3d_pack: null pointer");
  DPX_REQUIRE(q_mode_ok(mode), "dpx_qrnn3d_pack: unknown mode %d (3: split-f16, 6: split-bf16)", mode);
  DPX_REQUIRE(q_form_ok(form) && cin >= 1 && cin <= 256 && cout >= 1 && cout <= 1024, "dpx_qrnn3d_pack: form=%d cin=%d cout=%d (form 0..3, cin 1..256, gate cout 1..1024)",
              form, cin, cout);
  DPX_REQUIRE(!transposed || form == Q_K3 || form == Q_K1, "dpx_qrnn3d_pack: a transposed layer has stride 1 (form 0 or 2), got form %d", form);
  const long n = (long)q_weight_elems(form, cin, cout, mode) + q_m32(cout);
  DPX_LAUNCH("k_qrnn_pack", k_qrnn_pack, dim3(grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, w, bias, (unsigned short*)packed, cin, cout,
             q_taps(form), transposed ? 1 : 0, mode, f16_overflow_flag());
  return launch_status("dpx_qrnn3d_pack");
}

static bool q_layer_args_ok(const char* who, int form, int form_r, int N, int cin, int cin_r, int hidden, int dir, int D, int H, int W) {
  if (!q_shape_ok(who, N, D, H, W)) return false;
  if (!q_form_ok(form) || (cin_r > 0 && !q_form_ok(form_r))) return set_error("%s: unknown form %d / %d", who, form, form_r), false;
  if (dir < Q_FWD || dir > Q_BI) return set_error("%s: direction %d (0 forward, 1 reverse, 2 bidirectional)", who, dir), false;
  if (cin < 1 || cin > 256 || cin_r < 0 || cin_r > 256 || hidden < 1 || 3 * hidden > 1024)
    return set_error("%s: cin=%d cin_r=%d hidden=%d (cin 1..256, gate channels up to 1024)", who, cin, cin_r, hidden), false;
  if (cin_r > 0 && (q_out(form_r, H) != q_out(form, H) || q_out(form_r, W) != q_out(form, W)))
    return set_error("%s: the second operand's output plane differs (forms %d and %d)", who, form, form_r), false;
  return true;
}

extern "C" size_t dpx_qrnn3d_layer_ws_bytes(int form, int form_r, int N, int cin, int cin_r, int hidden, int direction, int D, int H, int W) {
  if (!q_layer_args_ok("dpx_qrnn3d_layer_ws_bytes", form, form_r, N, cin, cin_r, hidden, direction, D, H, W)) return 0;
  const int Ho = q_out(form, H), Wo = q_out(form, W), gg = ((direction == Q_BI ? 3 : 2) * hidden + 7) / 8;
  size_t n = c8_bytes(N, D, q_groups(cin), H, W) + c8_bytes(N, D, gg, Ho, Wo);
  if (cin_r > 0) n += c8_bytes(N, D, q_groups(cin_r), H, W) + c8_bytes(N, D, gg, Ho, Wo);
  return n;
}

// out[:, out_offset : out_offset + hidden] = pool(conv(x)) (+ pool(conv_r(xr)));  x [N][cin][D][H][W], xr [N][cin_r][D][H][W] (cin_r = 0: none),
// out [N][out_channels][D][Ho][Wo]
extern "C" int dpx_qrnn3d_layer(const float* x, const void* packed, const float* xr, const void* packed_r, float* out, int form, int form_r, int N,
                                int cin, int cin_r, int hidden, int direction, int D, int H, int W, int out_channels, int out_offset, int mode, void* ws,
                                dpx_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DPX_REQUIRE(q_mode_ok(mode), "dpx_qrnn3d_layer: unknown mode %d (3: split-f16, 6: split-bf16)", mode);
  if (!q_layer_args_ok("dpx_qrnn3d_layer", form, form_r, N, cin, cin_r, hidden, direction, D, H, W)) return DPX_ERR_ARG;
  DPX_REQUIRE(x && packed && out && ws && (cin_r == 0 || (xr && packed_r)), "dpx_qrnn3d_layer: null pointer");
  DPX_REQUIRE(out_offset >= 0 && out_offset + hidden <= out_channels, "dpx_qrnn3d_layer: channels [%d, %d) of a destination of %d", out_offset,
              out_offset + hidden, out_channels);
  const int Ho = q_out(form, H), Wo = q_out(form, W), gch = (direction == Q_BI ? 3 : 2) * hidden, gg = (gch + 7) / 8;
  char* p = (char*)ws;
  float* a = (float*)p;
  p += c8_bytes(N, D, q_groups(cin), H, W);
  float* g = (float*)p;
  p += c8_bytes(N, D, gg, Ho, Wo);
  float* g2 = nullptr;
  launch_to_c8(x, nullptr, a, N, cin, D, (long)H * W, q_groups(cin), s);
  launch_conv(QN_LAYER, form, mode, a, q_groups(cin), cin, g, (const char*)packed, gch, N, D, H, W, s);
  if (cin_r > 0) {
    float* ar = (float*)p;
    p += c8_bytes(N, D, q_groups(cin_r), H, W);
    g2 = (float*)p;
    launch_to_c8(xr, nullptr, ar, N, cin_r, D, (long)H * W, q_groups(cin_r), s);
    launch_conv(QN_LAYER, form_r, mode, ar, q_groups(cin_r), cin_r, g2, (const char*)packed_r, gch, N, D, H, W, s);
  }
  launch_pool(QN_LAYER, g, g2, hidden, direction, out, 1, out_channels, out_offset, nullptr, N, D, (long)Ho * Wo, s);
  return launch_status("dpx_qrnn3d_layer");
}

static bool grunet_args_ok(const char* who, int N, int D, int H, int W) {
  if (!q_shape_ok(who, N, D, H, W)) return false;
  if (H % 16 || W % 16) return set_error("%s: H=%d W=%d -- both must be multiples of 16 (four stride-2 levels)", who, H, W), false;
  return true;
}

extern "C" size_t dpx_grunet_packed_bytes(int in_ch, int mode) {
  if ((in_ch != 1 && in_ch != 2) || !q_mode_ok(mode)) {
    set_error("dpx_grunet_packed_bytes: in_ch=%d mode=%d (in_ch 1 or 2, mode 3 or 6)", in_ch, mode);
    return 0;
  }
  QLayer L[GRU_LAYERS];
  grunet_layers(in_ch, L);
  return grunet_layer_offset(L, GRU_LAYERS, mode);
}

// w: the 34 weight tensors in the reference's state-dict order (Down1..4, Conv1, Conv2..5 x (conv1, conv2, conv_residual), (Up_l, Up_conv_l x 3)
// for l = 5..2, Conv); bias: Conv's, 3 values
extern "C" int dpx_grunet_pack(void* packed, const float* const* w, const float* bias, int in_ch, int mode, dpx_stream_t stream) {
  DPX_REQUIRE(packed && w && bias, "dpx_grunet_pack: null pointer");
  DPX_REQUIRE(q_mode_ok(mode), "dpx_grunet_pack: unknown mode %d (3: split-f16, 6: split-bf16)", mode);
  DPX_REQUIRE(in_ch == 1 || in_ch == 2, "dpx_grunet_pack: in_ch=%d (1 or 2)", in_ch);
  QLayer L[GRU_LAYERS];
  grunet_layers(in_ch, L);
  for (int l = 0; l < GRU_LAYERS; ++l) {
    DPX_REQUIRE(w[l], "dpx_grunet_pack: layer %d has null weights", l);
    const int rc = dpx_qrnn3d_pack((char*)packed + grunet_layer_offset(L, l, mode), w[l], l == L_LAST ? bias : nullptr, L[l].form, L[l].cin, L[l].gates(),
                                   L[l].tr, mode, stream);
    if (rc != DPX_OK) return rc;
  }
  return DPX_OK;
}

extern "C" size_t dpx_grunet_ws_bytes(int N, int D, int H, int W) {
  if (!grunet_args_ok("dpx_grunet_ws_bytes", N, D, H, W)) return 0;
  return grunet_ws(N, D, H, W).total;
}

// y = net(cat(x, sigma)) + x;  x, y [N][D][H][W] (D = bands), sigma [N] on the device (in_ch = 2; ignored for in_ch = 1)
extern "C" int dpx_grunet_forward(const float* x, const float* sigma, float* y, const void* packed, int in_ch, int mode, int N, int D, int H, int W,
                                  void* ws, dpx_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DPX_REQUIRE(q_mode_ok(mode), "dpx_grunet_forward: unknown mode %d (3: split-f16, 6: split-bf16)", mode);
  DPX_REQUIRE(in_ch == 1 || in_ch == 2, "dpx_grunet_forward: in_ch=%d (1 or 2)", in_ch);
  if (!grunet_args_ok("dpx_grunet_forward", N, D, H, W)) return DPX_ERR_ARG;
  DPX_REQUIRE(x && y && packed && ws && (in_ch == 1 || sigma), "dpx_grunet_forward: null pointer");
  DPX_REQUIRE(x != y, "dpx_grunet_forward: the output must not be the input (no in-place call)");
  QLayer L[GRU_LAYERS];
  grunet_layers(in_ch, L);
  const GruWs w = grunet_ws(N, D, H, W);
  char* base = (char*)ws;
  auto buf = [&](size_t o) { return (float*)(base + o); };
  auto wp = [&](int l) { return (const char*)packed + grunet_layer_offset(L, l, mode); };
  float *ga = buf(w.ga), *gb = buf(w.gb);
  // conv + pool of layer l: in (Gin groups, plane h x ww) -> dst C8 (Gdst groups, from channel off on)
  auto layer = [&](const QNames& nm, int l, const float* in, int Gin, int h, int ww, float* dst, int Gdst, int off) {
    launch_conv(nm, L[l].form, mode, in, Gin, L[l].cin, ga, wp(l), L[l].gates(), N, D, h, ww, s);
    launch_pool(nm, ga, nullptr, L[l].hidden, L[l].dir, dst, 0, Gdst * 8, off, nullptr, N, D, (long)q_out(L[l].form, h) * q_out(L[l].form, ww), s);
  };
  // conv2(conv1(in)) + conv_residual(in): layers l, l + 1, l + 2; the two last poolings share one pass
  auto block = [&](const QNames& nm, int l, const float* in, int Gin, int h, int ww, float* hbuf, float* dst, int Gdst) {
    const int co = L[l].hidden;
    layer(nm, l, in, Gin, h, ww, hbuf, co / 8, 0);
    launch_conv(nm, L[l + 1].form, mode, hbuf, co / 8, co, ga, wp(l + 1), 2 * co, N, D, h, ww, s);
    launch_conv(nm, L[l + 2].form, mode, in, Gin, L[l + 2].cin, gb, wp(l + 2), 2 * co, N, D, h, ww, s);
    launch_pool(nm, ga, gb, co, Q_FWD, dst, 0, Gdst * 8, 0, nullptr, N, D, (long)h * ww, s);
  };
  launch_to_c8(x, in_ch == 2 ? sigma : nullptr, buf(w.in0), N, 1, D, (long)H * W, 2, s);
  layer(QN_CONV1, L_CONV1, buf(w.in0), 2, H, W, buf(w.cat[0]), 4, 0);                                   // e1 -> cat_0[0:16]
  for (int l = 1; l <= 4; ++l) {                                                               // e_{l+1}: Down_l (reverse), Conv_{l+1}
    const int h = H >> (l - 1), ww = W >> (l - 1);
    layer(QN_DOWN, L_DOWN + l - 1, buf(w.cat[l - 1]), 4 << (l - 1), h, ww, buf(w.t[l]), q_groups(8 << l), 0);
    float* dst = l < 4 ? buf(w.cat[l]) : buf(w.d[4]);
    block(QN_ENC, L_ENC + 3 * (l - 1), buf(w.t[l]), q_groups(8 << l), h / 2, ww / 2, buf(w.h[l]), dst, l < 4 ? 4 << l : 2 << l);
  }
  for (int l = 3; l >= 0; --l) {                                                               // d_{l+2}: Up (reverse) into cat_l's second half, Up_conv
    const int k = L_DEC + 4 * (3 - l), h = H >> l, ww = W >> l;
    layer(QN_UP, k, buf(w.d[l + 1]), 2 << (l + 1), h / 2, ww / 2, buf(w.cat[l]), 4 << l, 16 << l);
    block(QN_DEC, k + 1, buf(w.cat[l]), 4 << l, h, ww, buf(w.h[l]), buf(w.d[l]), 2 << l);
  }
  launch_conv(QN_LAST, L[L_LAST].form, mode, buf(w.d[0]), 2, 16, ga, wp(L_LAST), 3, N, D, H, W, s);
  launch_pool(QN_LAST, ga, nullptr, 1, Q_BI, y, 1, 1, 0, x, N, D, (long)H * W, s);
  return launch_status("dpx_grunet_forward");
}
