// Codec, reduced-precision decoder convolutions: dia_codec_conv_bf16 / dia_codec_convt_bf16 (DESIGN.md "Codec: bf16 modes").
// The contract is csrc/codec.hip's k_codec_conv for the decoder's forms, by construction: the argument checks and the geometry
// (conv_form / convt_form), the row prologue (conv_row), the Snake step (snake) and the epilogue (conv_epilogue) are the functions of
// csrc/codec_conv.hpp that k_codec_conv calls.  Activations stay fp32 in HBM: only the MFMA operands are reduced.
//
// k_codec_conv_bf<MW, PLANES> runs on v_mfma_f32_32x32x16_bf16: M = output channels, N = time, K = input channels x taps.  Operand
// maps (lane l, r = l & 31, h = l >> 5): A[row r][k 8 h + j] = weight, B[k 8 h + j][col r] = input, j = 0 .. 7 in one 16-byte
// fragment; D is a 32x32 tile as in k_codec_conv, which is why conv_epilogue serves both.
//
// A workgroup of 4 waves owns MT = 32 MW output channels x NT = 128 positions and walks the input channels in chunks of KC = 16: one
// MFMA k-step per tap.  Per chunk it stages, once,
//   the input   [position][plane][16 channels] bf16: loaded in fp32, zero outside [0, len), snake() once per staged element, then
//               hi = bf16(v) (RNE) and, for PLANES = 2, lo = bf16(v - hi) (the subtraction is exact in fp32).
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
#include "codec_conv.hpp"
#include "launch.hpp"

namespace {

using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

constexpr int XPOS = NT + MAXHALO;     // staged positions

struct ConvB : ConvArgs {
  const bf16_raw* w;
  long wplane;                         // elements between the hi and the lo image
  int Cg;                              // 8-channel groups of the weight image (C_in rounded up to KC, / 8)
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
  const ConvRow row = conv_row(p);
  const int b = row.b, ph = row.ph, len = row.len;               // len: positions of this row
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
          v[u] = xb[(long)cg * p.ldx + i];
          if (p.alpha) v[u] = snake(v[u], p.alpha[cg], p.inv[cg]);
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

  conv_epilogue(p, tot, row, len, n0 + wn * WN + r, co0 + wm * 32, h);
}

int bf_launch(const dia_codec_conv_args* a, ConvB k, int planes, void* stream, const char* name) {
  conv_fill(a, k);
  k.w = reinterpret_cast<const bf16_raw*>(a->w);
  k.Cg = (a->C_in + KC - 1) / KC * (KC / 8);
  k.wplane = (long)k.phases * k.ntaps * k.Cg * k.Cp * 8;
  const dim3 grid = conv_grid(a, k, a->T);
  hipStream_t st = (hipStream_t)stream;
  if (conv_narrow(a)) {
    if (planes == 1) dia_launch<k_codec_conv_bf<1, 1>>(grid, dim3(256), 0, st, k);
    else dia_launch<k_codec_conv_bf<1, 2>>(grid, dim3(256), 0, st, k);
  } else {
    if (planes == 1) dia_launch<k_codec_conv_bf<2, 1>>(grid, dim3(256), 0, st, k);
    else dia_launch<k_codec_conv_bf<2, 2>>(grid, dim3(256), 0, st, k);
  }
  return dia_check_launch(name);
}

}  // namespace

extern "C" int dia_codec_conv_bf16(const dia_codec_conv_args* a, int planes, void* stream) {
  ConvB k = {};
  if (int rc = conv_form(a, "dia_codec_conv_bf16", "dia_codec_convt_bf16", k, planes)) return rc;
  return bf_launch(a, k, planes, stream, "k_codec_conv_bf");
}

extern "C" int dia_codec_convt_bf16(const dia_codec_conv_args* a, int planes, void* stream) {
  ConvB k = {};
  if (int rc = convt_form(a, "dia_codec_convt_bf16", k, planes)) return rc;
  return bf_launch(a, k, planes, stream, "k_codec_conv_bf (transposed)");
}
