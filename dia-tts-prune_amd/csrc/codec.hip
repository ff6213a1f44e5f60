// Codec: the Descript Audio Codec decoder in exact fp32 (dia_codec_embed / dia_codec_conv / dia_codec_convt, DESIGN.md "Codec").
//
// One implicit-GEMM kernel serves every convolution of the decoder.  M = output channels, N = time, K = input channels x taps, on
// v_mfma_f32_32x32x2_f32: f32 operands, f32 accumulate, bit for bit an fmaf chain, so no plane splitting is needed for reference
// accuracy.  Operand maps (lane l, r = l & 31, h = l >> 5): A[row r][k h] = weight, B[k h][col r] = input; D has the column (time)
// on the lane and row (reg & 3) + 8 (reg >> 2) + 4 h (channel) in the 16 registers, so a store of one register is 32 consecutive
// floats of one channel.
//
// A workgroup of 4 waves owns MT = 32 MW output channels x NT = 128 positions and walks the input channels in chunks of KC = 16.
// Per chunk it stages, once, the input rows [KC][NT + halo] (zero outside [0, len), Snake applied here: one sinf per staged element,
// not per tap) and the weights [taps][KC][MT], then issues taps x KC / 2 MFMAs per accumulator.  A tap is only an offset into the
// staged row: tap j reads position n + tap_off0 + j * tap_step.  That covers
//   conv, k 7 / 1, dilation d:  tap_step = d, tap_off0 = -(k / 2) d, output o = n
//   transposed conv, k = 2 s:   one launch phase r per output residue, two taps (x[m], x[m - 1]), output o = m s + r - s / 2
// Every chunk accumulates from zero and is then added to the running total: the sum over K is blocked (112 products, then the
// chunks), which keeps the rounding error of the 5376-term sums of the 768-channel layers near that of a blocked CPU sum.  The
// order depends on nothing but (channel, tap), so an output element has the same bits wherever its tile, window or batch row lies.
//
// LDS: 14 KiB of input rows + 42 KiB of weights = 56 KiB static, two workgroups per CU.  Row strides are 32 mod 64 floats, so the
// two lane halves (k = 0 / 1) of one ds_read hit disjoint banks.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdarg>
#include <cstdio>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int NT = 128;                // positions per workgroup
constexpr int KC = 16;                 // input channels per staged chunk
constexpr int MAXTAPS = 7;
constexpr int MAXHALO = 54;            // k 7, dilation 9: 6 * 9
constexpr int XS = 224;                // staged input row stride: >= NT + MAXHALO, 32 mod 64
constexpr int WS = 96;                 // staged weight row stride: >= 64, 32 mod 64
static_assert(XS >= NT + MAXHALO && XS % 64 == 32 && WS >= 64 && WS % 64 == 32, "LDS strides");

struct ConvK {
  const float* x; const float* w; const float* bias; const float* alpha; const float* inv; const float* res; float* y;
  const int* lens;
  int T, C_in, C_out, Cp, ldx, ldy;
  int ntaps, tap_step, tap_off0;       // tap j reads input position n + tap_off0 + j * tap_step
  int lo, width;                       // smallest tap offset (<= 0); staged positions per row = NT + largest - smallest
  int ostride, phases, pad, extra;     // o = n * ostride + phase - pad; n runs over [0, len + extra)
  int tanh_out;
};

template <int MW>
__global__ __launch_bounds__(256) void k_codec_conv(ConvK p) {
  constexpr int MT = 32 * MW, WAVES_N = 4 / MW, WN = NT / WAVES_N, NACC = WN / 32;
  __shared__ __attribute__((aligned(16))) float xs[KC * XS];
  __shared__ __attribute__((aligned(16))) float ws[MAXTAPS * KC * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave % MW, wn = wave / MW;
  const int b = blockIdx.z / p.phases, ph = blockIdx.z - b * p.phases;
  const int len = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;
  const int n0 = blockIdx.x * NT;
  if (n0 >= len + p.extra) return;                               // workgroup-uniform
  const int co0 = blockIdx.y * MT;
  const float* xb = p.x + (long)b * p.C_in * p.ldx;
  const float* wp = p.w + (long)ph * p.ntaps * p.C_in * p.Cp;

  f32x16 tot[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i)
    for (int e = 0; e < 16; ++e) tot[i][e] = 0.f;

  for (int c0 = 0; c0 < p.C_in; c0 += KC) {
    __syncthreads();                                             // the previous chunk's reads are done
    // input rows: wave w stages channels 4 w .. 4 w + 3, lanes along time
#pragma unroll
    for (int kk = 0; kk < KC / 4; ++kk) {
      const int ci = wave * (KC / 4) + kk, cg = c0 + ci;
      const bool row = cg < p.C_in;
      const float al = (row && p.alpha) ? p.alpha[cg] : 0.f;
      const float iv = (row && p.alpha) ? p.inv[cg] : 0.f;
      const float* xr = xb + (long)(row ? cg : 0) * p.ldx;
      for (int c = lane; c < p.width; c += 64) {
        const int i = n0 + p.lo + c;
        float v = 0.f;
        if (row && i >= 0 && i < len) {
          v = xr[i];
          if (p.alpha) {
            const float s = sinf(al * v);                        // accurate sinf: alpha x is not range-limited
            v = v + s * s * iv;
          }
        }
        xs[ci * XS + c] = v;
      }
    }
    // weights: ntaps * KC rows of MT floats
    for (int e = tid; e < p.ntaps * KC * (MT / 4); e += 256) {
      const int q = e % (MT / 4), rw = e / (MT / 4);
      const int ci = rw % KC, j = rw / KC;
      const int cg = c0 + ci, co = co0 + q * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cg < p.C_in && co < p.Cp) v = *reinterpret_cast<const float4*>(wp + ((long)j * p.C_in + cg) * p.Cp + co);
      *reinterpret_cast<float4*>(ws + (j * KC + ci) * WS + q * 4) = v;
    }
    __syncthreads();

    f32x16 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    for (int j = 0; j < p.ntaps; ++j) {
      const float* wa = ws + (j * KC + h) * WS + wm * 32 + r;
      const float* xa = xs + h * XS + wn * WN + r + (p.tap_off0 + j * p.tap_step - p.lo);
#pragma unroll
      for (int pp = 0; pp < KC / 2; ++pp) {
        const float a = wa[pp * 2 * WS];
#pragma unroll
        for (int i = 0; i < NACC; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xa[pp * 2 * XS + i * 32], acc[i], 0, 0, 0);
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

constexpr int ET = 16;                 // frames per embedding workgroup

struct EmbK {
  const int* codes; const int* lens; const float* tables; const float* bias; float* z;
  int T, n_cb, cb_size, latent, ld_codes, ldz;
};

// nine row gathers, their sum and the summed bias; the tile goes through LDS so that reads run along the channel and writes along time
__global__ __launch_bounds__(256) void k_codec_embed(EmbK p) {
  __shared__ float s[ET][257];
  __shared__ int ids[DIA_CODEC_MAX_CODEBOOKS][ET];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int len = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;
  const int t0 = blockIdx.x * ET;
  if (t0 >= len) return;
  for (int e = tid; e < p.n_cb * ET; e += 256) {
    const int i = e / ET, tt = e - i * ET, t = t0 + tt;
    const int id = t < len ? p.codes[((long)b * p.n_cb + i) * p.ld_codes + t] : 0;
    ids[i][tt] = min(max(id, 0), p.cb_size - 1);
  }
  __syncthreads();
  const int c = blockIdx.y * 256 + tid;
  if (c < p.latent) {
    const float bs = p.bias[c];
    for (int tt = 0; tt < ET; ++tt) {
      float v = bs;
      for (int i = 0; i < p.n_cb; ++i) v += p.tables[((long)i * p.cb_size + ids[i][tt]) * p.latent + c];
      s[tt][tid] = v;
    }
  }
  __syncthreads();
  for (int e = tid; e < ET * 256; e += 256) {
    const int tt = e % ET, cc = e / ET;
    const int t = t0 + tt, co = blockIdx.y * 256 + cc;
    if (t < len && co < p.latent) p.z[((long)b * p.latent + co) * p.ldz + t] = s[tt][cc];
  }
}

int codec_fail(const char* fmt, ...) {
  char buf[224];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

// what dia_codec_conv and dia_codec_convt share; 0 when clean
int conv_common(const dia_codec_conv_args* a, const char* fn, int phases, int out_per_in) {
  if (!a) return codec_fail("%s: null argument", fn);
  if (!a->x || !a->w || !a->bias || !a->y) return codec_fail("%s: null pointer (x, w, bias and y are required)", fn);
  if ((a->alpha == nullptr) != (a->inv == nullptr)) return codec_fail("%s: alpha and inv go together", fn);
  if ((const void*)a->x == (const void*)a->y) return codec_fail("%s: y must not be x", fn);
  if (((uintptr_t)a->w & 15) != 0) return codec_fail("%s: w must be 16-byte aligned", fn);
  if (a->C_in < 1 || a->C_in > DIA_CODEC_MAX_CHANNELS || a->C_out < 1 || a->C_out > DIA_CODEC_MAX_CHANNELS)
    return codec_fail("%s: C_in = %d / C_out = %d outside [1, %d]", fn, a->C_in, a->C_out, DIA_CODEC_MAX_CHANNELS);
  if (a->T < 1 || a->T > DIA_CODEC_MAX_T) return codec_fail("%s: T = %d outside [1, %d]", fn, a->T, DIA_CODEC_MAX_T);
  if (a->B < 1 || (long)a->B * phases > 65535) return codec_fail("%s: B = %d outside [1, %d]", fn, a->B, 65535 / phases);
  if (a->ldx < a->T) return codec_fail("%s: ldx = %d below T = %d", fn, a->ldx, a->T);
  if ((long)a->ldy < (long)a->T * out_per_in) return codec_fail("%s: ldy = %d below the output length %ld", fn, a->ldy, (long)a->T * out_per_in);
  if (a->tanh_out != 0 && a->tanh_out != 1) return codec_fail("%s: tanh_out = %d is not 0 or 1", fn, a->tanh_out);
  return 0;
}

int conv_launch(const dia_codec_conv_args* a, ConvK k, void* stream, const char* name) {
  k.x = a->x; k.w = a->w; k.bias = a->bias; k.alpha = a->alpha; k.inv = a->inv; k.res = a->res; k.y = a->y; k.lens = a->lens;
  k.T = a->T; k.C_in = a->C_in; k.C_out = a->C_out; k.Cp = (a->C_out + 31) / 32 * 32; k.ldx = a->ldx; k.ldy = a->ldy;
  k.tanh_out = a->tanh_out;
  const int nb = (a->T + k.extra + NT - 1) / NT;
  if (a->C_out <= 32)
    dia_launch<k_codec_conv<1>>(dim3(nb, 1, a->B * k.phases), dim3(256), 0, (hipStream_t)stream, k);
  else
    dia_launch<k_codec_conv<2>>(dim3(nb, (a->C_out + 63) / 64, a->B * k.phases), dim3(256), 0, (hipStream_t)stream, k);
  return dia_check_launch(name);
}

}  // namespace

extern "C" int dia_codec_conv(const dia_codec_conv_args* a, void* stream) {
  if (int rc = conv_common(a, "dia_codec_conv", 1, 1)) return rc;
  if (a->k != 1 && a->k != 7) return codec_fail("dia_codec_conv: kernel size %d is not 1 or 7", a->k);
  if (a->dilation != 1 && a->dilation != 3 && a->dilation != 9) return codec_fail("dia_codec_conv: dilation %d is not 1, 3 or 9", a->dilation);
  if (a->k == 1 && a->dilation != 1) return codec_fail("dia_codec_conv: kernel size 1 takes dilation 1, not %d", a->dilation);
  if (a->stride != 0) return codec_fail("dia_codec_conv: stride = %d belongs to dia_codec_convt; it must be 0 here", a->stride);
  ConvK k = {};
  const int half = (a->k / 2) * a->dilation;
  k.ntaps = a->k; k.tap_step = a->dilation; k.tap_off0 = -half; k.lo = -half; k.width = NT + 2 * half;
  k.ostride = 1; k.phases = 1; k.pad = 0; k.extra = 0;
  return conv_launch(a, k, stream, "k_codec_conv");
}

extern "C" int dia_codec_convt(const dia_codec_conv_args* a, void* stream) {
  const int s = a ? a->stride : 2;
  if (a && s != 2 && s != 4 && s != 8) return codec_fail("dia_codec_convt: stride %d is not 2, 4 or 8", s);
  if (int rc = conv_common(a, "dia_codec_convt", s, s)) return rc;
  if (a->k != 0 && a->k != 2 * s) return codec_fail("dia_codec_convt: kernel size %d is not 2 * stride = %d", a->k, 2 * s);
  if (a->dilation != 0 && a->dilation != 1) return codec_fail("dia_codec_convt: dilation %d is not supported", a->dilation);
  if (a->res) return codec_fail("dia_codec_convt: a residual is not supported");
  ConvK k = {};
  k.ntaps = 2; k.tap_step = -1; k.tap_off0 = 0; k.lo = -1; k.width = NT + 1;
  k.ostride = s; k.phases = s; k.pad = s / 2; k.extra = 1;
  return conv_launch(a, k, stream, "k_codec_conv (transposed)");
}

extern "C" int dia_codec_embed(const dia_codec_embed_args* a, void* stream) {
  if (!a) return codec_fail("dia_codec_embed: null argument");
  if (!a->codes || !a->tables || !a->bias || !a->z) return codec_fail("dia_codec_embed: null pointer (codes, tables, bias and z are required)");
  if (a->n_codebooks < 1 || a->n_codebooks > DIA_CODEC_MAX_CODEBOOKS)
    return codec_fail("dia_codec_embed: n_codebooks = %d outside [1, %d]", a->n_codebooks, DIA_CODEC_MAX_CODEBOOKS);
  if (a->codebook_size < 1) return codec_fail("dia_codec_embed: codebook_size = %d", a->codebook_size);
  if (a->latent_dim < 1 || a->latent_dim > DIA_CODEC_MAX_CHANNELS)
    return codec_fail("dia_codec_embed: latent_dim = %d outside [1, %d]", a->latent_dim, DIA_CODEC_MAX_CHANNELS);
  if (a->T < 1 || a->T > DIA_CODEC_MAX_T) return codec_fail("dia_codec_embed: T = %d outside [1, %d]", a->T, DIA_CODEC_MAX_T);
  if (a->B < 1 || a->B > 65535) return codec_fail("dia_codec_embed: B = %d outside [1, 65535]", a->B);
  if (a->ld_codes < a->T || a->ldz < a->T) return codec_fail("dia_codec_embed: ld_codes = %d / ldz = %d below T = %d", a->ld_codes, a->ldz, a->T);
  EmbK k = {};
  k.codes = a->codes; k.lens = a->lens; k.tables = a->tables; k.bias = a->bias; k.z = a->z;
  k.T = a->T; k.n_cb = a->n_codebooks; k.cb_size = a->codebook_size; k.latent = a->latent_dim; k.ld_codes = a->ld_codes; k.ldz = a->ldz;
  dia_launch<k_codec_embed>(dim3((a->T + ET - 1) / ET, (a->latent_dim + 255) / 256, a->B), dim3(256), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_codec_embed");
}
