// Codec: the Descript Audio Codec in exact fp32.  Decoder: dia_codec_embed / dia_codec_conv / dia_codec_convt (DESIGN.md "Codec");
// encoder: the same dia_codec_conv plus dia_codec_convs (strided and k-3 forms) and dia_codec_quantize, the residual VQ search
// (DESIGN.md "Codec: encode side").  The argument checks, the geometry of every form, the row prologue, the Snake step and the
// epilogue are csrc/codec_conv.hpp's, shared with csrc/codec_bf16.hip.
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
//   conv, k 3:                  tap_step = 1, tap_off0 = -1, output o = n
//   strided conv, k = 2 s:      tap j = r + t s, y[o] = sum_{r, t} w[r + t s] x[(o + t) s + r - s / 2]: the s residues r of every input
//                               channel are staged as s rows of their own, row (ci, r) holding x[ci][i s + r - s / 2] at position i
//                               (every input element lands in exactly one of them), and the layer is a two-tap convolution
//                               (offsets 0 and 1) over K = C_in s rows, output o = n (template flag STRIDED: the staging gather)
// Every chunk accumulates from zero and is then added to the running total: the sum over K is blocked (112 products, then the
// chunks), which keeps the rounding error of the 5376-term sums of the 768-channel layers near that of a blocked CPU sum.  The
// order depends on nothing but (channel, tap), so an output element has the same bits wherever its tile, window or batch row lies.
//
// LDS: 14 KiB of input rows + 42 KiB of weights = 56 KiB static, two workgroups per CU.  Row strides are 32 mod 64 floats, so the
// two lane halves (k = 0 / 1) of one ds_read hit disjoint banks.
#include "codec_conv.hpp"
#include "launch.hpp"

namespace {

constexpr int XS = 224;                // staged input row stride: >= NT + MAXHALO, 32 mod 64
constexpr int WS = 96;                 // staged weight row stride: >= 64, 32 mod 64
static_assert(XS >= NT + MAXHALO && XS % 64 == 32 && WS >= 64 && WS % 64 == 32, "LDS strides");

struct ConvK : ConvArgs {
  const float* w;
  int xstride;                         // STRIDED only: s; C_in then counts the staged rows, C_in of the layer x s
};

template <int MW, bool STRIDED = false>
__global__ __launch_bounds__(256) void k_codec_conv(ConvK p) {
  constexpr int MT = 32 * MW, WAVES_N = 4 / MW, WN = NT / WAVES_N, NACC = WN / 32;
  __shared__ __attribute__((aligned(16))) float xs[KC * XS];
  __shared__ __attribute__((aligned(16))) float ws[MAXTAPS * KC * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave % MW, wn = wave / MW;
  const ConvRow row = conv_row(p);
  const int b = row.b, ph = row.ph, lin = row.len;               // lin: input positions of this row
  const int len = STRIDED ? lin / p.xstride : lin;               // positions n of this row
  const int n0 = blockIdx.x * NT;
  if (n0 >= len + p.extra) return;                               // workgroup-uniform
  const int co0 = blockIdx.y * MT;
  const float* xb = p.x + (long)b * (STRIDED ? p.C_in / p.xstride : p.C_in) * p.ldx;
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
      const int ch = STRIDED ? cg / p.xstride : cg;              // the layer's input channel
      const float al = (row && p.alpha) ? p.alpha[ch] : 0.f;
      const float iv = (row && p.alpha) ? p.inv[ch] : 0.f;
      const float* xr = xb + (long)(row ? ch : 0) * p.ldx;
      const int roff = STRIDED ? cg - ch * p.xstride - p.xstride / 2 : 0;
      for (int c = lane; c < p.width; c += 64) {
        const int i = STRIDED ? (n0 + p.lo + c) * p.xstride + roff : n0 + p.lo + c;
        float v = 0.f;
        if (row && i >= 0 && i < lin) {
          v = xr[i];
          if (p.alpha) v = snake(v, al, iv);
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

  conv_epilogue(p, tot, row, len, n0 + wn * WN + r, co0 + wm * 32, h);
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

constexpr int QF = 8;                  // frames per quantiser workgroup: two per wave, one after the other
constexpr int QMAXDIM = 32;

struct QuantK {
  const float* z; const int* lens; const float* in_w; const float* in_b; const float* cb; const float* cb2; const float* tables;
  const float* bias; int* codes;
  int T, n_cb, cb_size, dim, latent, ldz, ld_codes;
};

// sum over the 64 lanes by an xor butterfly: every lane ends with the same bits (a + b == b + a), in an order that is fixed
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The residual VQ search, all stages in one launch.  A wave owns a frame from its latent column to its last code: the column sits
// in LDS (res), is never written back, and nothing a wave computes depends on which frames share its workgroup.  Per stage:
// z_e = in_proj(res) (lanes along the latent, butterfly sum), e = z_e / max(|z_e|, 1e-12), the rows of the normalised codebook
// spread over the lanes (row j on lane j % 64, ascending per lane, strict <), then a butterfly arg-min on (distance, index): the
// smaller distance wins and, on equal distances, the smaller index -- whatever the lane order.  Control flow is uniform over the
// workgroup (frames past a row's end are searched on zeros and not written), so the barriers are plain __syncthreads().
__global__ __launch_bounds__(256) void k_codec_quantize(QuantK p) {
  extern __shared__ __attribute__((aligned(16))) float qres[];   // [QF][latent]
  __shared__ float ze[4][QMAXDIM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * QF;
  const int len = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;
  if (t0 >= len) return;                                         // workgroup-uniform
  const float* zb = p.z + (long)b * p.latent * p.ldz;
  for (int e = tid; e < p.latent * QF; e += 256) {
    const int c = e / QF, tt = e - c * QF, t = t0 + tt;
    qres[tt * p.latent + c] = t < len ? zb[(long)c * p.ldz + t] : 0.f;
  }
  __syncthreads();
  for (int f = 0; f < QF / 4; ++f) {
    const int tt = wave * (QF / 4) + f, t = t0 + tt;
    float* res = qres + tt * p.latent;
    for (int i = 0; i < p.n_cb; ++i) {
      const float* wi = p.in_w + (long)i * p.dim * p.latent;
      for (int d = 0; d < p.dim; ++d) {
        float s = 0.f;
        for (int c = lane; c < p.latent; c += 64) s = fmaf(wi[(long)d * p.latent + c], res[c], s);
        s = wave_sum(s) + p.in_b[i * p.dim + d];
        if (lane == 0) ze[wave][d] = s;
      }
      __syncthreads();
      float n2 = 0.f;
      for (int d = 0; d < p.dim; ++d) n2 = fmaf(ze[wave][d], ze[wave][d], n2);
      const float rn = 1.f / fmaxf(sqrtf(n2), 1e-12f);
      float e2 = 0.f;
      for (int d = 0; d < p.dim; ++d) { const float v = ze[wave][d] * rn; e2 = fmaf(v, v, e2); }
      float best = __builtin_inff();
      int idx = 0x7fffffff;
      const float* cbi = p.cb + (long)i * p.cb_size * p.dim;
      for (int j = lane; j < p.cb_size; j += 64) {
        float dot = 0.f;
        for (int d = 0; d < p.dim; ++d) dot = fmaf(ze[wave][d] * rn, cbi[(long)j * p.dim + d], dot);
        const float dist = e2 - 2.f * dot + p.cb2[i * p.cb_size + j];
        if (dist < best) { best = dist; idx = j; }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
      }
      idx = min(idx, p.cb_size - 1);                             // a column of NaN finds nothing: stay inside the table
      const float* tab = p.tables + ((long)i * p.cb_size + idx) * p.latent;
      const float* bs = p.bias + (long)i * p.latent;
      for (int c = lane; c < p.latent; c += 64) res[c] -= tab[c] + bs[c];
      if (lane == 0 && t < len) p.codes[((long)b * p.n_cb + i) * p.ld_codes + t] = idx;
      __syncthreads();                                           // ze is rewritten by the next stage
    }
  }
}

// k: the geometry its form has set; xstride != 0: the strided form, where K runs over C_in x s staged rows and n over the T / s outputs
int conv_launch(const dia_codec_conv_args* a, ConvK k, int xstride, void* stream, const char* name) {
  conv_fill(a, k);
  k.w = a->w; k.xstride = xstride;
  if (xstride) k.C_in = a->C_in * xstride;
  const dim3 grid = conv_grid(a, k, xstride ? a->T / xstride : a->T);
  hipStream_t st = (hipStream_t)stream;
  if (xstride) {
    if (conv_narrow(a)) dia_launch<k_codec_conv<1, true>>(grid, dim3(256), 0, st, k);
    else dia_launch<k_codec_conv<2, true>>(grid, dim3(256), 0, st, k);
  } else {
    if (conv_narrow(a)) dia_launch<k_codec_conv<1>>(grid, dim3(256), 0, st, k);
    else dia_launch<k_codec_conv<2>>(grid, dim3(256), 0, st, k);
  }
  return dia_check_launch(name);
}

}  // namespace

extern "C" int dia_codec_conv(const dia_codec_conv_args* a, void* stream) {
  ConvK k = {};
  if (int rc = conv_form(a, "dia_codec_conv", "dia_codec_convt", k)) return rc;
  return conv_launch(a, k, 0, stream, "k_codec_conv");
}

extern "C" int dia_codec_convt(const dia_codec_conv_args* a, void* stream) {
  ConvK k = {};
  if (int rc = convt_form(a, "dia_codec_convt", k)) return rc;
  return conv_launch(a, k, 0, stream, "k_codec_conv (transposed)");
}

extern "C" int dia_codec_convs(const dia_codec_conv_args* a, void* stream) {
  ConvK k = {};
  int s = 0;
  if (int rc = convs_form(a, "dia_codec_convs", k, s)) return rc;
  return conv_launch(a, k, s, stream, s ? "k_codec_conv (strided)" : "k_codec_conv (k 3)");
}

extern "C" int dia_codec_quantize(const dia_codec_quantize_args* a, void* stream) {
  if (!a) return codec_fail("dia_codec_quantize: null argument");
  if (!a->z || !a->in_w || !a->in_b || !a->codebook || !a->codebook_sq || !a->tables || !a->bias || !a->codes)
    return codec_fail("dia_codec_quantize: null pointer (z, in_w, in_b, codebook, codebook_sq, tables, bias and codes are required)");
  if (a->n_codebooks < 1 || a->n_codebooks > DIA_CODEC_MAX_CODEBOOKS)
    return codec_fail("dia_codec_quantize: n_codebooks = %d outside [1, %d]", a->n_codebooks, DIA_CODEC_MAX_CODEBOOKS);
  if (a->codebook_size < 1 || a->codebook_size > DIA_CODEC_MAX_CODEBOOK_SIZE)
    return codec_fail("dia_codec_quantize: codebook_size = %d outside [1, %d]", a->codebook_size, DIA_CODEC_MAX_CODEBOOK_SIZE);
  if (a->codebook_dim < 1 || a->codebook_dim > QMAXDIM)
    return codec_fail("dia_codec_quantize: codebook_dim = %d outside [1, %d]", a->codebook_dim, QMAXDIM);
  if (a->latent_dim < 1 || a->latent_dim > DIA_CODEC_MAX_CHANNELS)
    return codec_fail("dia_codec_quantize: latent_dim = %d outside [1, %d]", a->latent_dim, DIA_CODEC_MAX_CHANNELS);
  if (a->T < 1 || a->T > DIA_CODEC_MAX_T) return codec_fail("dia_codec_quantize: T = %d outside [1, %d]", a->T, DIA_CODEC_MAX_T);
  if (a->B < 1 || a->B > 65535) return codec_fail("dia_codec_quantize: B = %d outside [1, 65535]", a->B);
  if (a->ldz < a->T || a->ld_codes < a->T) return codec_fail("dia_codec_quantize: ldz = %d / ld_codes = %d below T = %d", a->ldz, a->ld_codes, a->T);
  QuantK k = {};
  k.z = a->z; k.lens = a->lens; k.in_w = a->in_w; k.in_b = a->in_b; k.cb = a->codebook; k.cb2 = a->codebook_sq; k.tables = a->tables;
  k.bias = a->bias; k.codes = a->codes;
  k.T = a->T; k.n_cb = a->n_codebooks; k.cb_size = a->codebook_size; k.dim = a->codebook_dim; k.latent = a->latent_dim;
  k.ldz = a->ldz; k.ld_codes = a->ld_codes;
  dia_launch<k_codec_quantize>(dim3((a->T + QF - 1) / QF, a->B), dim3(256), (size_t)QF * a->latent_dim * sizeof(float), (hipStream_t)stream, k);
  return dia_check_launch("k_codec_quantize");
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
