// Codec: what the fp32 convolution kernel (csrc/codec.hip, k_codec_conv) and the bf16 one (csrc/codec_bf16.hip, k_codec_conv_bf)
// share.  Host side: the argument checks of every entry point, the tap geometry of every form, the kernel-argument fill and the
// grid.  Device side: the row prologue, the Snake step and the epilogue of a 32x32 MFMA output tile.  The staging loops, the LDS
// layouts and the MFMA loops differ and stay with their kernels.  Everything here is file-local to the including source.
#pragma once
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include <cstdarg>
#include <cstdio>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int NT = 128;                // positions per workgroup
constexpr int KC = 16;                 // input channels per staged chunk
constexpr int MAXTAPS = 7;
constexpr int MAXHALO = 54;            // k 7, dilation 9: 6 * 9

// the kernel arguments both kernels read; ConvK / ConvB add their weight pointer and what goes with it
struct ConvArgs {
  const float* x; const float* bias; const float* alpha; const float* inv; const float* res; float* y;
  const int* lens;
  int T, C_in, C_out, Cp, ldx, ldy;
  int ntaps, tap_step, tap_off0;       // tap j reads input position n + tap_off0 + j * tap_step
  int lo, width;                       // smallest tap offset (<= 0); staged positions per row = NT + largest - smallest
  int ostride, phases, pad, extra;     // o = n * ostride + phase - pad; n runs over [0, len + extra)
  int tanh_out;
};

// ---------------------------------------------------------------------------------------------- device side
struct ConvRow { int b, ph, len; };    // batch row, launch phase, input positions of the row (lens clamped to [0, T])

__device__ __forceinline__ ConvRow conv_row(const ConvArgs& p) {
  const int b = blockIdx.z / p.phases;
  return {b, (int)blockIdx.z - b * p.phases, p.lens ? min(max(p.lens[b], 0), p.T) : p.T};
}

__device__ __forceinline__ float snake(float v, float al, float iv) {
  const float s = sinf(al * v);                                  // accurate sinf: alpha x is not range-limited
  return v + s * s * iv;
}

// D registers of NACC 32x32 tiles -> y: column n_lane + 32 i (time) on the lane, channel co_wave + (reg & 3) + 8 (reg >> 2) + 4 h in
// the 16 registers; `len` counts the positions n of the row.  Nothing is written at or beyond a row's end.
template <int NACC>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& p, const f32x16 (&tot)[NACC], const ConvRow& row, int len, int n_lane,
                                              int co_wave, int h) {
  const long out_len = (long)len * p.ostride;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int n = n_lane + i * 32;
    const long o = (long)n * p.ostride + row.ph - p.pad;
    const bool col = n < len + p.extra && o >= 0 && o < out_len;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int co = co_wave + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (col && co < p.C_out) {
        const long at = ((long)row.b * p.C_out + co) * p.ldy + o;
        float v = tot[i][e] + p.bias[co];
        if (p.res) v += p.res[at];
        if (p.tanh_out) v = tanhf(v);
        p.y[at] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- host side
int codec_fail(const char* fmt, ...) {
  char buf[224];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

// what every convolution entry point checks; 0 when clean.  planes: the bf16 entry points' own argument, 1 for the fp32 ones
int conv_common(const dia_codec_conv_args* a, const char* fn, int phases, int out_per_in, int in_per_out = 1, int planes = 1) {
  if (!a) return codec_fail("%s: null argument", fn);
  if (planes != 1 && planes != 2) return codec_fail("%s: planes = %d is not 1 (bf16) or 2 (bf16x2)", fn, planes);
  if (!a->x || !a->w || !a->bias || !a->y) return codec_fail("%s: null pointer (x, w, bias and y are required)", fn);
  if ((a->alpha == nullptr) != (a->inv == nullptr)) return codec_fail("%s: alpha and inv go together", fn);
  if ((const void*)a->x == (const void*)a->y) return codec_fail("%s: y must not be x", fn);
  if (((uintptr_t)a->w & 15) != 0) return codec_fail("%s: w must be 16-byte aligned", fn);
  if (a->C_in < 1 || a->C_in > DIA_CODEC_MAX_CHANNELS || a->C_out < 1 || a->C_out > DIA_CODEC_MAX_CHANNELS)
    return codec_fail("%s: C_in = %d / C_out = %d outside [1, %d]", fn, a->C_in, a->C_out, DIA_CODEC_MAX_CHANNELS);
  if (a->T < 1 || a->T > DIA_CODEC_MAX_T) return codec_fail("%s: T = %d outside [1, %d]", fn, a->T, DIA_CODEC_MAX_T);
  if (a->B < 1 || (long)a->B * phases > 65535) return codec_fail("%s: B = %d outside [1, %d]", fn, a->B, 65535 / phases);
  if (a->ldx < a->T) return codec_fail("%s: ldx = %d below T = %d", fn, a->ldx, a->T);
  if ((long)a->ldy < (long)a->T * out_per_in / in_per_out)
    return codec_fail("%s: ldy = %d below the output length %ld", fn, a->ldy, (long)a->T * out_per_in / in_per_out);
  if (a->tanh_out != 0 && a->tanh_out != 1) return codec_fail("%s: tanh_out = %d is not 0 or 1", fn, a->tanh_out);
  return 0;
}

// One function per form: every check of entry point `fn`, then the form's geometry into k.  0 when clean.
// conv, k 1 / 7, dilation 1 / 3 / 9; fnt names the transposed entry point a stride belongs to
int conv_form(const dia_codec_conv_args* a, const char* fn, const char* fnt, ConvArgs& k, int planes = 1) {
  if (int rc = conv_common(a, fn, 1, 1, 1, planes)) return rc;
  if (a->k != 1 && a->k != 7) return codec_fail("%s: kernel size %d is not 1 or 7", fn, a->k);
  if (a->dilation != 1 && a->dilation != 3 && a->dilation != 9) return codec_fail("%s: dilation %d is not 1, 3 or 9", fn, a->dilation);
  if (a->k == 1 && a->dilation != 1) return codec_fail("%s: kernel size 1 takes dilation 1, not %d", fn, a->dilation);
  if (a->stride != 0) return codec_fail("%s: stride = %d belongs to %s; it must be 0 here", fn, a->stride, fnt);
  const int half = (a->k / 2) * a->dilation;
  k.ntaps = a->k; k.tap_step = a->dilation; k.tap_off0 = -half; k.lo = -half; k.width = NT + 2 * half;
  k.ostride = 1; k.phases = 1; k.pad = 0; k.extra = 0;
  return 0;
}

// transposed, k = 2 s: one launch phase per output residue, two taps (x[m], x[m - 1])
int convt_form(const dia_codec_conv_args* a, const char* fn, ConvArgs& k, int planes = 1) {
  const int s = a ? a->stride : 2;
  if (a && s != 2 && s != 4 && s != 8) return codec_fail("%s: stride %d is not 2, 4 or 8", fn, s);
  if (int rc = conv_common(a, fn, s, s, 1, planes)) return rc;
  if (a->k != 0 && a->k != 2 * s) return codec_fail("%s: kernel size %d is not 2 * stride = %d", fn, a->k, 2 * s);
  if (a->dilation != 0 && a->dilation != 1) return codec_fail("%s: dilation %d is not supported", fn, a->dilation);
  if (a->res) return codec_fail("%s: a residual is not supported", fn);
  k.ntaps = 2; k.tap_step = -1; k.tap_off0 = 0; k.lo = -1; k.width = NT + 1;
  k.ostride = s; k.phases = s; k.pad = s / 2; k.extra = 1;
  return 0;
}

// the k-3 form (stride 0) and the strided form (k = 2 s: two taps over the C_in s residue rows); xstride = 0 / s.  fp32 only
int convs_form(const dia_codec_conv_args* a, const char* fn, ConvArgs& k, int& xstride) {
  const int s = a ? a->stride : 0;
  if (a && s != 0 && s != 2 && s != 4 && s != 8) return codec_fail("%s: stride %d is not 0 (the k-3 form), 2, 4 or 8", fn, s);
  if (int rc = conv_common(a, fn, 1, 1, s ? s : 1)) return rc;
  if (a->dilation != 0 && a->dilation != 1) return codec_fail("%s: dilation %d is not supported", fn, a->dilation);
  if (a->res) return codec_fail("%s: a residual is not supported", fn);
  if (s == 0 && a->k != 3) return codec_fail("%s: kernel size %d is not 3 (stride 0) or 2 * stride", fn, a->k);
  if (s != 0 && a->k != 0 && a->k != 2 * s) return codec_fail("%s: kernel size %d is not 2 * stride = %d", fn, a->k, 2 * s);
  if (s != 0 && a->T % s != 0) return codec_fail("%s: T = %d is not a multiple of stride %d", fn, a->T, s);
  k.ntaps = s ? 2 : 3; k.tap_step = 1; k.tap_off0 = s ? 0 : -1; k.lo = k.tap_off0; k.width = NT + k.ntaps - 1;
  k.ostride = 1; k.phases = 1; k.pad = 0; k.extra = 0;
  xstride = s;
  return 0;
}

// the entry point's arguments into the kernel's block, beside the geometry its form has set
void conv_fill(const dia_codec_conv_args* a, ConvArgs& k) {
  k.x = a->x; k.bias = a->bias; k.alpha = a->alpha; k.inv = a->inv; k.res = a->res; k.y = a->y; k.lens = a->lens;
  k.T = a->T; k.C_in = a->C_in; k.C_out = a->C_out; k.Cp = (a->C_out + 31) / 32 * 32; k.ldx = a->ldx; k.ldy = a->ldy;
  k.tanh_out = a->tanh_out;
}

// C_out <= 32 runs the MW = 1 kernel (one 32-channel block, 4 waves along time), anything wider MW = 2 (64-channel blocks)
bool conv_narrow(const dia_codec_conv_args* a) { return a->C_out <= 32; }

// positions: the row's positions n at full length (T, or T / s for the strided form)
dim3 conv_grid(const dia_codec_conv_args* a, const ConvArgs& k, int positions) {
  return dim3((positions + k.extra + NT - 1) / NT, conv_narrow(a) ? 1 : (a->C_out + 63) / 64, a->B * k.phases);
}

}  // namespace
