// Codec, reduced-precision decoder convolutions: dia_codec_conv_bf16 / dia_codec_convt_bf16 (DESIGN.md "Codec: bf16 modes").
// The contract is csrc/codec.hip's k_codec_conv for the decoder's forms (conv k 1 / 7, dilation 1 / 3 / 9; transposed conv as the
// two-tap phase mode; per-row lens; bias, residual and tanhf in the epilogue; nothing read or written at or beyond a row's end).
// Activations stay fp32 in HBM: only the MFMA operands are reduced.
//
// k_codec_conv_bf<MW, PLANES> runs on v_mfma_f32_32x32x16_bf16: M = output channels, N = time, K = input channels x taps.  Operand
// maps (lane l, r = l & 31, h = l >> 5): A[row r][k 8 h + j] = weight, B[k 8 h + j][col r] = input, j = 0 .. 7 in one 16-byte
// fragment; D as in k_codec_conv (column = time on the lane, channel (reg & 3) + 8 (reg >> 2) + 4 h in the 16 registers).
//
// A workgroup of 4 waves owns MT = 32 MW output channels x NT = 128 positions and walks the input channels in chunks of KC = 16: one
// MFMA k-step per tap.  Per chunk it stages, once,
//   the input   [position][plane][16 channels] bf16: loaded and Snake'd in fp32 exactly as k_codec_conv does (accurate sinf, once per
//               staged element), then hi = bf16(v) (RNE) and, for PLANES = 2, lo = bf16(v - hi) (the subtraction is exact in fp32).
//               The row stride is 32 PLANES + 16 bytes, an odd number of 16-byte slots: the 16 lanes of a ds_read_b128 group (one
//               h, 16 positions distinct mod 16) land on 16 different slots of the 256-byte bank row.  A tap is an offset on the
//               position, as in k_codec_conv, so the transposed form stays a mode;
//   the weights [plane][tap][8-channel group 0 / 1][MT][8 channels] bf16, copied in 16-byte pieces from the host's image (same order
//               with the group index running over the whole of C_in and MT over Cp; include/dia_hip.h): a lane's A fragment is one
//               16-byte read, consecutive lanes 16 bytes apart.
// Products per (chunk, tap): w_hi x_hi, then for PLANES = 2 w_hi x_lo and w_lo x_hi, in that order; w_lo x_lo (at most 2^-16 of
// sum |w| |x|, 2^-22 of it measured on the widest layers) is dropped.  Every chunk accumulates from zero and is added to the running
// total, as in k_codec_conv.  The order depends on nothing but (channel chunk, tap, product): an output element has the same bits
// wherever its tile, window or batch row lies.
//
// LDS, static: PLANES = 1: 8.5 KiB input + 14 KiB weights; PLANES = 2: 14.2 KiB + 28 KiB = 42.2 KiB, three workgroups per CU.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdarg>
#include <cstdio>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

constexpr int NT = 128;                // positions per workgroup
constexpr int KC = 16;                 // input channels per staged chunk: one k-step of the MFMA
constexpr int MAXTAPS = 7;
constexpr int MAXHALO = 54;            // k 7, dilation 9: 6 * 9
constexpr int XPOS = NT + MAXHALO;     // staged positions

struct ConvB {
  const float* x; const bf16_raw* w; const float* bias; const float* alpha; const float* inv; const float* res; float* y;
  const int* lens;
  long wplane;                         // elements between the hi and the lo image
  int T, C_in, C_out, Cp, Cg, ldx, ldy;  // Cg: 8-channel groups of the weight image (C_in rounded up to KC, / 8)
  int ntaps, tap_step, tap_off0;       // tap j reads input position n + tap_off0 + j * tap_step
  int lo, width;                       // smallest tap offset (<= 0); staged positions = NT + largest - smallest
  int ostride, phases, pad, extra;     // o = n * ostride + phase - pad; n runs over [0, len + extra)
  int tanh_out;
};

template <int MW, int PLANES>
__global__ __launch_bounds__(256) void k_codec_conv_bf(ConvB p) {
  constexpr int MT = 32 * MW, WAVES_N = 4 / MW, WN = NT / WAVES_N, NACC = WN / 32;
  constexpr int XSB = 32 * PLANES + 16;                          // bytes per staged position
  static_assert((XSB / 16) % 2 == 1, "an odd number of 16-byte slots per position");
  __shared__ __attribute__((aligned(16))) unsigned char xs[XPOS * XSB];
  __shared__ __attribute__((aligned(16))) bf16x8 ws[PLANES * MAXTAPS * 2 * MT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave % MW, wn = wave / MW;
  const int b = blockIdx.z / p.phases, ph = blockIdx.z - b * p.phases;
  const int len = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;    // positions of this row
  const int n0 = blockIdx.x * NT;
  if (n0 >= len + p.extra) return;                               // workgroup-uniform
  const int co0 = blockIdx.y * MT;
  const float* xb = p.x + (long)b * p.C_in * p.ldx;
  const bf16_raw* wp = p.w + (long)ph * p.ntaps * p.Cg * p.Cp * 8;

  f32x16 tot[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i)
    for (int e = 0; e < 16; ++e) tot[i][e] = 0.f;

  for (int c0 = 0; c0 < p.C_in; c0 += KC) {
    __syncthreads();                                             // the previous chunk's reads are done
    // input: a task is 4 channels of one position (lanes along time), stored as one 8-byte piece per plane
    for (int e = tid; e < (KC / 4) * p.width; e += 256) {
      const int q = e / p.width, c = e - q * p.width;
      const int i = n0 + p.lo + c;
      const bool pos = i >= 0 && i < len;
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cg = c0 + q * 4 + u;
        v[u] = 0.f;
        if (pos && cg < p.C_in) {
          float t = xb[(long)cg * p.ldx + i];
          if (p.alpha) {
            const float s = sinf(p.alpha[cg] * t);               // accurate sinf: alpha x is not range-limited
            t = t + s * s * p.inv[cg];
          }
          v[u] = t;
        }
      }
      bf16x4 hi, lo;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma clang fp contract(off)
        hi[u] = (__bf16)v[u];
        lo[u] = (__bf16)(v[u] - (float)hi[u]);
      }
      *reinterpret_cast<bf16x4*>(xs + c * XSB + q * 8) = hi;
      if (PLANES == 2) *reinterpret_cast<bf16x4*>(xs + c * XSB + 32 + q * 8) = lo;
    }
    // weights: PLANES * ntaps * 2 runs of MT 16-byte pieces
    for (int e = tid; e < PLANES * p.ntaps * 2 * MT; e += 256) {
      const int m = e % MT, rw = e / MT;
      const int g = rw & 1, j = (rw >> 1) % p.ntaps, pl = (rw >> 1) / p.ntaps;
      const int gg = c0 / 8 + g, co = co0 + m;
      bf16x8 v;
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = (__bf16)0.f;
      if (gg < p.Cg && co < p.Cp) v = *reinterpret_cast<const bf16x8*>(wp + pl * p.wplane + (((long)j * p.Cg + gg) * p.Cp + co) * 8);
      ws[e] = v;
    }
    __syncthreads();

    f32x16 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    for (int j = 0; j < p.ntaps; ++j) {
      const bf16x8 whi = ws[(j * 2 + h) * MT + wm * 32 + r];
      bf16x8 wlo = whi;
      if (PLANES == 2) wlo = ws[((p.ntaps + j) * 2 + h) * MT + wm * 32 + r];
      const unsigned char* xa = xs + (wn * WN + r + (p.tap_off0 + j * p.tap_step - p.lo)) * XSB + h * 16;
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        const bf16x8 xhi = *reinterpret_cast<const bf16x8*>(xa + i * 32 * XSB);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, xhi, acc[i], 0, 0, 0);
        if (PLANES == 2) {
          const bf16x8 xlo = *reinterpret_cast<const bf16x8*>(xa + i * 32 * XSB + 32);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, xlo, acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, xhi, acc[i], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NACC; ++i) tot[i] += acc[i];
  }

  const long out_len = (long)len * p.ostride;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int n = n0 + wn * WN + i * 32 + r;
    const long o = (long)n * p.ostride + ph - p.pad;
    const bool col = n < len + p.extra && o >= 0 && o < out_len;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int co = co0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (col && co < p.C_out) {
        const long at = ((long)b * p.C_out + co) * p.ldy + o;
        float v = tot[i][e] + p.bias[co];
        if (p.res) v += p.res[at];
        if (p.tanh_out) v = tanhf(v);
        p.y[at] = v;
      }
    }
  }
}

int bf_fail(const char* fmt, ...) {
  char buf[224];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

// dia_codec_conv's / dia_codec_convt's own checks (csrc/codec.hip conv_common), plus planes; 0 when clean
int bf_common(const dia_codec_conv_args* a, int planes, const char* fn, int phases) {
  if (!a) return bf_fail("%s: null argument", fn);
  if (planes != 1 && planes != 2) return bf_fail("%s: planes = %d is not 1 (bf16) or 2 (bf16x2)", fn, planes);
  if (!a->x || !a->w || !a->bias || !a->y) return bf_fail("%s: null pointer (x, w, bias and y are required)", fn);
  if ((a->alpha == nullptr) != (a->inv == nullptr)) return bf_fail("%s: alpha and inv go together", fn);
  if ((const void*)a->x == (const void*)a->y) return bf_fail("%s: y must not be x", fn);
  if (((uintptr_t)a->w & 15) != 0) return bf_fail("%s: w must be 16-byte aligned", fn);
  if (a->C_in < 1 || a->C_in > DIA_CODEC_MAX_CHANNELS || a->C_out < 1 || a->C_out > DIA_CODEC_MAX_CHANNELS)
    return bf_fail("%s: C_in = %d / C_out = %d outside [1, %d]", fn, a->C_in, a->C_out, DIA_CODEC_MAX_CHANNELS);
  if (a->T < 1 || a->T > DIA_CODEC_MAX_T) return bf_fail("%s: T = %d outside [1, %d]", fn, a->T, DIA_CODEC_MAX_T);
  if (a->B < 1 || (long)a->B * phases > 65535) return bf_fail("%s: B = %d outside [1, %d]", fn, a->B, 65535 / phases);
  if (a->ldx < a->T) return bf_fail("%s: ldx = %d below T = %d", fn, a->ldx, a->T);
  if ((long)a->ldy < (long)a->T * phases) return bf_fail("%s: ldy = %d below the output length %ld", fn, a->ldy, (long)a->T * phases);
  if (a->tanh_out != 0 && a->tanh_out != 1) return bf_fail("%s: tanh_out = %d is not 0 or 1", fn, a->tanh_out);
  return 0;
}

int bf_launch(const dia_codec_conv_args* a, ConvB k, int planes, void* stream, const char* name) {
  k.x = a->x; k.w = reinterpret_cast<const bf16_raw*>(a->w); k.bias = a->bias; k.alpha = a->alpha; k.inv = a->inv; k.res = a->res;
  k.y = a->y; k.lens = a->lens;
  k.T = a->T; k.C_in = a->C_in; k.C_out = a->C_out; k.Cp = (a->C_out + 31) / 32 * 32; k.Cg = (a->C_in + KC - 1) / KC * (KC / 8);
  k.ldx = a->ldx; k.ldy = a->ldy; k.tanh_out = a->tanh_out;
  k.wplane = (long)k.phases * k.ntaps * k.Cg * k.Cp * 8;
  const int nb = (a->T + k.extra + NT - 1) / NT;
  const dim3 g1(nb, 1, a->B * k.phases), g2(nb, (a->C_out + 63) / 64, a->B * k.phases);
  hipStream_t st = (hipStream_t)stream;
  if (a->C_out <= 32) {
    if (planes == 1) dia_launch<k_codec_conv_bf<1, 1>>(g1, dim3(256), 0, st, k);
    else dia_launch<k_codec_conv_bf<1, 2>>(g1, dim3(256), 0, st, k);
  } else {
    if (planes == 1) dia_launch<k_codec_conv_bf<2, 1>>(g2, dim3(256), 0, st, k);
    else dia_launch<k_codec_conv_bf<2, 2>>(g2, dim3(256), 0, st, k);
  }
  return dia_check_launch(name);
}

}  // namespace

extern "C" int dia_codec_conv_bf16(const dia_codec_conv_args* a, int planes, void* stream) {
  if (int rc = bf_common(a, planes, "dia_codec_conv_bf16", 1)) return rc;
  if (a->k != 1 && a->k != 7) return bf_fail("dia_codec_conv_bf16: kernel size %d is not 1 or 7", a->k);
  if (a->dilation != 1 && a->dilation != 3 && a->dilation != 9) return bf_fail("dia_codec_conv_bf16: dilation %d is not 1, 3 or 9", a->dilation);
  if (a->k == 1 && a->dilation != 1) return bf_fail("dia_codec_conv_bf16: kernel size 1 takes dilation 1, not %d", a->dilation);
  if (a->stride != 0) return bf_fail("dia_codec_conv_bf16: stride = %d belongs to dia_codec_convt_bf16; it must be 0 here", a->stride);
  ConvB k = {};
  const int half = (a->k / 2) * a->dilation;
  k.ntaps = a->k; k.tap_step = a->dilation; k.tap_off0 = -half; k.lo = -half; k.width = NT + 2 * half;
  k.ostride = 1; k.phases = 1; k.pad = 0; k.extra = 0;
  return bf_launch(a, k, planes, stream, "k_codec_conv_bf");
}

extern "C" int dia_codec_convt_bf16(const dia_codec_conv_args* a, int planes, void* stream) {
  const int s = a ? a->stride : 2;
  if (a && s != 2 && s != 4 && s != 8) return bf_fail("dia_codec_convt_bf16: stride %d is not 2, 4 or 8", s);
  if (int rc = bf_common(a, planes, "dia_codec_convt_bf16", s)) return rc;
  if (a->k != 0 && a->k != 2 * s) return bf_fail("dia_codec_convt_bf16: kernel size %d is not 2 * stride = %d", a->k, 2 * s);
  if (a->dilation != 0 && a->dilation != 1) return bf_fail("dia_codec_convt_bf16: dilation %d is not supported", a->dilation);
  if (a->res) return bf_fail("dia_codec_convt_bf16: a residual is not supported");
  ConvB k = {};
  k.ntaps = 2; k.tap_step = -1; k.tap_off0 = 0; k.lo = -1; k.width = NT + 1;
  k.ostride = s; k.phases = s; k.pad = s / 2; k.extra = 1;
  return bf_launch(a, k, planes, stream, "k_codec_conv_bf (transposed)");
}
