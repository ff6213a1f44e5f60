// Audio distance: the windowed DFT of one resolution as a GEMM, its magnitudes, the mel rows and the L1 terms between two batches
// of rows: dia_spectral (DESIGN.md "Audio distance").
//
// The DFT is frames [F x W] times a basis [W x 2 (W / 2 + 1)] (the periodic Hann window folded in, built by the host in float64
// and rounded once) on v_mfma_f32_32x32x2_f32: f32 operands, f32 accumulate.  Every MFMA step starts from zero: its result is the
// fp32 sum of two products, and the steps are added in float64 in ascending n; the magnitude is the float64 square root of the two
// sums.  Longer fp32 chains are cheaper and not good enough: a bin whose sum nearly cancels (|X| of 2e-3 where sum |x w| is 60)
// keeps the chain's absolute error, its logarithm moves by 1e-3, and that one element was the whole error of a distance: 5 x the
// float32 FFT's with chains of 16 samples, 3.7 x with 4, 0.55 x with 2 (which also says why no blocked or compensated
// fp32 scheme stands between the MFMA and the float64 add: an ill-conditioned bin keeps the error of the longest fp32 chain in its
// sum).  No FFT: W <= 2048, and the direct form has one summation order whatever the row, the tile or the batch.  Operand maps (lane
// l, r = l & 31, h = l >> 5): A[row r][k h] = basis[n = 2 p + h][bin k0 + r] (read from global memory: the basis is shared by
// every workgroup through L2), B[k h][col r] = sample n of column r's frame (from LDS); D has the column on the lane and bin (reg
// & 3) + 8 (reg >> 2) + 4 h in the 16 registers.  Two accumulators, real and imaginary, for the same 32 bins.
//
// A workgroup of 4 waves owns one row and 32 columns.  With b (distance) the columns are 16 consecutive frames of a, then the same
// 16 frames of b; without b (spectra only) they are 32 consecutive frames of a, the second 16 staged as their own half.  A half's
// input span, 15 H + W samples (H = W / 4: frames overlap 4 x), is staged in LDS once, zero outside [0, len).  Lanes that differ in
// frame read at stride H, a multiple of 32 words from W = 128 on, so the span is skewed by one word per hop: sample i sits at i +
// i / H, frame f's sample n at f (H + 1) + n + n / H, and the second half starts 16 mod 32 words after the first: the 32 lanes of
// a ds_read_b32 group land in 32 banks at every W.
//
// The bins are walked in groups of 128, wave w taking bins [32 w, 32 w + 32) of the group.  The magnitudes of a group go through
// LDS ([128][32 + 1]) as fp32; with n_mels == 0 the terms |a - b| and |log a - log b| are taken in registers from the float64
// magnitudes, lane r against lane r ^ 16 (spectra only: the magnitudes are written out from LDS, bins along the lanes); with
// n_mels > 0, thread (m, column) extends its mel row's fma chain by the group's bins, in ascending k, and the terms are taken over
// the mel rows after the last group.  The terms are formed and added in float64 (the difference of two floats is exact there), per
// thread in a fixed order, then over the workgroup by a fixed tree: one pair of partials per (row, frame tile), written with plain
// stores.  No atomics, no order between workgroups.
//
// LDS at W = 2048, n_mels = 320: 4 KiB of tree + 2 x 38.2 KiB of span + 16.5 KiB of magnitudes + 41.3 KiB of mel rows = 138 KiB.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int THREADS = 256;
constexpr int HF = DIA_SPECTRAL_TILE_FRAMES;   // frames of one half
constexpr int COLS = 2 * HF;                   // MFMA columns
constexpr int GB = 128;                        // bins of one group: 32 per wave
constexpr int MS = COLS + 1;                   // row stride of the magnitude and mel buffers
constexpr int UNR = 8;                         // MFMA steps (2 samples each) of one basis prefetch
constexpr int RED_BYTES = 2 * THREADS * (int)sizeof(double);
static_assert(COLS == 32 && GB == 32 * (THREADS / 64), "one MFMA tile of columns, one bin tile per wave");

// floats of one staged half: the skewed span, rounded up to 16 mod 32
__host__ __device__ constexpr int span_floats(int W) {
  const int H = W / 4, need = (HF - 1) * H + W + (HF - 1) + 4;
  return (need + 15) / 32 * 32 + 16;
}

size_t lds_bytes(int W, int n_mels) { return RED_BYTES + sizeof(float) * (2 * (size_t)span_floats(W) + GB * MS + (size_t)n_mels * MS); }

struct SpecK {
  const float* a; const float* b; const float* basis; const float* fb; const int* fb_range; double* partial; float* out;
  double eps;
  int ld, W, logH, nbin, n_mels, tiles, out_frames, power;
  int len[DIA_SPECTRAL_MAX_ROWS];
};

__global__ __launch_bounds__(THREADS) void k_spectral(SpecK P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);
  float* span = reinterpret_cast<float*>(smem + RED_BYTES);
  const int W = P.W, H = W >> 2, logH = P.logH, nbin = P.nbin, n_mels = P.n_mels;
  const int sps = span_floats(W);
  float* magb = span + 2 * sps;
  float* mel = magb + GB * MS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int row = blockIdx.y;
  const int L = P.len[row], F = 1 + L / H;
  const bool dist = P.b != nullptr;
  const int f0 = blockIdx.x * (dist ? HF : COLS);
  if (f0 >= F) return;                                           // workgroup-uniform

  // the two halves' spans, skewed by one word per hop
  for (int half = 0; half < 2; ++half) {
    const float* src = ((half && dist) ? P.b : P.a) + (long)row * P.ld;
    const int s0 = (f0 + ((half && !dist) ? HF : 0)) * H - W / 2;
    float* sp = span + half * sps;
    for (int i = tid; i < (HF - 1) * H + W; i += THREADS) {
      const int s = s0 + i;
      sp[i + (i >> logH)] = (s >= 0 && s < L) ? src[s] : 0.f;
    }
  }
  for (int e = tid; e < n_mels * MS; e += THREADS) mel[e] = 0.f;
  __syncthreads();

  const float* xp = span + (r >> 4) * sps + (r & (HF - 1)) * (H + 1) + h;
  double s_mag = 0.0, s_log = 0.0;
  const double pw = (double)P.power;

  for (int g0 = 0; g0 < nbin; g0 += GB) {
    const int k0 = g0 + wave * 32;
    double tr[16], ti[16];                                       // the sums over n: every MFMA step's pair of products, added here
#pragma unroll
    for (int e = 0; e < 16; ++e) { tr[e] = 0.0; ti[e] = 0.0; }
    if (k0 < nbin) {                                             // wave-uniform
      // bins past the last read the last bin's column and are zeroed below
      const float* bp = P.basis + (long)h * 2 * nbin + min(k0 + r, nbin - 1);
      const long step = 4L * nbin;                               // two samples on
      float cr[UNR], ci[UNR], nr[UNR], ni[UNR];
      f32x16 zero;
#pragma unroll
      for (int e = 0; e < 16; ++e) zero[e] = 0.f;
#pragma unroll
      for (int u = 0; u < UNR; ++u) { cr[u] = bp[u * step]; ci[u] = bp[u * step + nbin]; }
      for (int p = 0; p < W / 2; p += UNR) {                     // UNR steps: the next ones' basis is requested first
        bp += UNR * step;
        const bool more = p + UNR < W / 2;
        if (more) {
#pragma unroll
          for (int u = 0; u < UNR; ++u) { nr[u] = bp[u * step]; ni[u] = bp[u * step + nbin]; }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {                          // every step from zero: two products, then the float64 add
          const int n = 2 * (p + u);
          const float x = xp[n + (n >> logH)];
          const f32x16 re = __builtin_amdgcn_mfma_f32_32x32x2f32(cr[u], x, zero, 0, 0, 0);
          const f32x16 im = __builtin_amdgcn_mfma_f32_32x32x2f32(ci[u], x, zero, 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 16; ++e) { tr[e] += (double)re[e]; ti[e] += (double)im[e]; }
        }
        if (more) {
#pragma unroll
          for (int u = 0; u < UNR; ++u) { cr[u] = nr[u]; ci[u] = ni[u]; }
        }
      }
    }
    const bool in_regs = dist && n_mels == 0;                    // the STFT terms: from the float64 magnitudes, before they are rounded
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int bl = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const double m = sqrt(tr[e] * tr[e] + ti[e] * ti[e]);
      magb[bl * MS + r] = g0 + bl < nbin ? (float)m : 0.f;
      if (in_regs) {                                             // workgroup-uniform; column r ^ 16 is the same frame of the other row
        const double o = __shfl_xor(m, HF, 64);
        if (r < HF && g0 + bl < nbin && f0 + r < F) {
          s_mag += fabs(m - o);
          s_log += pw * fabs(log10(fmax(m, P.eps)) - log10(fmax(o, P.eps)));
        }
      }
    }
    __syncthreads();

    const int gn = min(GB, nbin - g0);                           // live bins of this group
    if (n_mels > 0) {
      // thread (m, column) owns its mel element through every group: no barrier between its updates
      for (int e = tid; e < n_mels * COLS; e += THREADS) {
        const int c = e & (COLS - 1), m = e >> 5;
        const int lo = max(max(P.fb_range[2 * m], 0), g0), hi = min(min(P.fb_range[2 * m + 1], nbin), g0 + gn);
        if (lo < hi) {
          const float* fr = P.fb + (long)m * nbin;
          float v = mel[m * MS + c];
          for (int k = lo; k < hi; ++k) v = fmaf(fr[k], magb[(k - g0) * MS + c], v);
          mel[m * MS + c] = v;
        }
      }
    } else if (dist) {
      // done in registers above
    } else {
      for (int e = tid; e < GB * COLS; e += THREADS) {
        const int bl = e & (GB - 1), c = e >> 7;
        if (bl < gn && f0 + c < F) P.out[((long)row * P.out_frames + f0 + c) * nbin + g0 + bl] = magb[bl * MS + c];
      }
    }
    __syncthreads();                                             // the next group rewrites magb
  }

  if (n_mels > 0) {
    if (dist) {
      for (int e = tid; e < n_mels * HF; e += THREADS) {
        const int fr = e & (HF - 1), m = e >> 4;
        if (f0 + fr < F) {
          const double sa = mel[m * MS + fr], sb = mel[m * MS + HF + fr];
          s_mag += fabs(sa - sb);
          s_log += pw * fabs(log10(fmax(sa, P.eps)) - log10(fmax(sb, P.eps)));
        }
      }
    } else {
      for (int e = tid; e < n_mels * COLS; e += THREADS) {
        const int m = e % n_mels, c = e / n_mels;
        if (f0 + c < F) P.out[((long)row * P.out_frames + f0 + c) * n_mels + m] = mel[m * MS + c];
      }
    }
  }
  if (!dist) return;

  red[tid] = s_mag;
  red[THREADS + tid] = s_log;
  __syncthreads();
  for (int s = THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[THREADS + tid] += red[THREADS + tid + s];
    }
    __syncthreads();
  }
  if (tid < 2) P.partial[((long)row * P.tiles + blockIdx.x) * 2 + tid] = red[tid * THREADS];
}

int spectral_fail(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

}  // namespace

extern "C" int dia_spectral(const dia_spectral_args* a, void* stream) {
  if (!a) return spectral_fail("dia_spectral: null argument");
  if (!a->a || !a->basis || !a->len) return spectral_fail("dia_spectral: null pointer (a, basis and the host array len are required)");
  const int W = a->window;
  if (W < DIA_SPECTRAL_MIN_WINDOW || W > DIA_SPECTRAL_MAX_WINDOW || (W & (W - 1)))
    return spectral_fail("dia_spectral: window = %d is not a power of two in [%d, %d]", W, DIA_SPECTRAL_MIN_WINDOW, DIA_SPECTRAL_MAX_WINDOW);
  if (a->n_mels < 0 || a->n_mels > DIA_SPECTRAL_MAX_MELS) return spectral_fail("dia_spectral: n_mels = %d outside [0, %d]", a->n_mels, DIA_SPECTRAL_MAX_MELS);
  if (a->n_mels > 0 && (!a->fb || !a->fb_range)) return spectral_fail("dia_spectral: n_mels = %d needs fb and fb_range", a->n_mels);
  if (a->B < 1 || a->B > DIA_SPECTRAL_MAX_ROWS) return spectral_fail("dia_spectral: B = %d outside [1, %d]", a->B, DIA_SPECTRAL_MAX_ROWS);
  if (a->ld < 1 || a->ld > DIA_SPECTRAL_MAX_T) return spectral_fail("dia_spectral: ld = %d outside [1, %d]", a->ld, DIA_SPECTRAL_MAX_T);
  if (a->power != 1 && a->power != 2) return spectral_fail("dia_spectral: power = %d is neither 1 nor 2", a->power);
  if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return spectral_fail("dia_spectral: eps = %g is not positive", a->eps);
  const int H = W / 4;
  int most = 0;
  for (int b = 0; b < a->B; ++b) {
    if (a->len[b] < 1 || a->len[b] > a->ld) return spectral_fail("dia_spectral: row %d: len = %d outside [1, ld = %d]", b, a->len[b], a->ld);
    if (a->len[b] > most) most = a->len[b];
  }
  const int F = 1 + most / H;
  const int per = a->b ? HF : COLS, tiles = (F + per - 1) / per;
  if (a->b) {
    if (!a->partial) return spectral_fail("dia_spectral: a distance (b given) needs partial");
    if (a->tiles < tiles) return spectral_fail("dia_spectral: tiles = %d below the %d frame tiles of the longest row", a->tiles, tiles);
  } else {
    if (!a->out) return spectral_fail("dia_spectral: spectra only (no b) needs out");
    if (a->out_frames < F) return spectral_fail("dia_spectral: out_frames = %d below the %d frames of the longest row", a->out_frames, F);
  }
  SpecK k = {};
  k.a = a->a; k.b = a->b; k.basis = a->basis; k.fb = a->fb; k.fb_range = a->fb_range; k.partial = a->partial; k.out = a->out;
  k.eps = a->eps;
  k.ld = a->ld; k.W = W; k.nbin = W / 2 + 1; k.n_mels = a->n_mels; k.tiles = a->tiles; k.out_frames = a->out_frames; k.power = a->power;
  k.logH = 0;
  while ((1 << k.logH) < H) ++k.logH;
  for (int b = 0; b < a->B; ++b) k.len[b] = a->len[b];
  dia_launch<k_spectral>(dim3(tiles, a->B), dim3(THREADS), lds_bytes(W, a->n_mels), (hipStream_t)stream, k);
  return dia_check_launch("k_spectral");
}
