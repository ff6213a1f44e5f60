// Speed factor: time-scaling by linear interpolation or by WSOLA, dia_timescale (DESIGN.md "Speed factor").
//
// k_ts_interp   the reference application's method: output j reads the signal at pos_j = j (N - 1) / (M - 1), evaluated in float64
//               and rounded once.  One thread per output, plain VALU, bound by launch and memory.
// k_ts_search   WSOLA's search, sequential in the frame index by construction (frame k's template is the continuation of frame
//               k - 1's segment): ONE workgroup of 256 threads per row walks the row's frames.  Per frame it stages the template
//               (W floats) and the candidate span (W + 2 D floats) in LDS, zero where the window has no sample, which is also what
//               keeps a NaN behind a row's length out of the sums.  Thread t then owns the R = 5 adjacent offsets
//               e = 5 t .. 5 t + 4 (e = delta + D; further passes of 1280 offsets when 2 D + 1 > 1280): five independent fmaf
//               chains from 0 in ascending n.  Four template values come as one ds_read_b128 broadcast, the candidate window
//               slides by four words per four steps (eight values in registers, statically indexed: the loop is unrolled so that
//               no register is indexed dynamically), and a lane stride of 5 words keeps the candidate reads free of bank conflicts.
//               The arg-max (largest corr, then smallest |delta|, then the negative one; NaN never wins) is reduced through the
//               wave by shuffles and over the four waves through LDS; every thread redoes the last four-way step, which saves a
//               barrier per frame.  At the defaults (W 1024, D 512) a frame is 1025 x 1024 fma on one CU.
// k_ts_synth    the two-term overlap-add, parallel over rows x tiles of 1024 outputs: y[m] = fmaf(w[nb], x[..], w[na] * x[..]).
//
// Every index into x is formed in 64 bits and tested against [0, n_valid) before the load: whatever centre[] and delta hold,
// nothing outside a row's window is read.  The rows' 64-bit absolute indices come in HOST arrays and are reduced here.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdarg>
#include <cstdio>

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TILE = 4 * THREADS;      // outputs of one workgroup of k_ts_interp / k_ts_synth
constexpr int R = 5;                   // adjacent offsets of one thread of k_ts_search
constexpr int PASS = THREADS * R;
constexpr int PAD = 8;                 // floats behind the candidate span that the last threads' windows slide over
constexpr int NO_DELTA = 1 << 30;      // "no candidate yet": loses every tie

struct RowW {
  int n_valid;                         // window samples that exist: [0, n_valid) of x[b]
  int nk;                              // frames to search
  int first;                           // k0 == 0: the row's first frame is frame 0, delta 0 without a search
  int dprev;                           // delta of frame k0 - 1
  int m0;                              // out_start - (k0 - 1) * Hs: output t of the row lies m0 + t behind the centre of frame k0 - 1
  int n_out;
};

struct WsolaK {
  const float* x; float* y; const float* win; const int* centre; int* delta;
  int ldx, ldy, ldk, W, D, lgHs;
  RowW row[DIA_TS_MAX_ROWS];
};

struct RowI {
  long N, M;                           // samples and outputs of the whole signal
  long out0, in0;                      // absolute index of y[b][0] and x[b][0]
  int n_valid, n_out;
};

struct InterpK {
  const float* x; float* y;
  int ldx, ldy;
  RowI row[DIA_TS_MAX_ROWS];
};

__device__ __forceinline__ float ts_load(const float* x, long i, int n_valid) { return (i >= 0 && i < n_valid) ? x[i] : 0.f; }

__global__ __launch_bounds__(THREADS) void k_ts_interp(InterpK P) {
  const int b = blockIdx.y;
  const RowI r = P.row[b];
  const float* x = P.x + (long)b * P.ldx;
  float* y = P.y + (long)b * P.ldy;
#pragma unroll
  for (int u = 0; u < TILE / THREADS; ++u) {
    const int t = blockIdx.x * TILE + u * THREADS + threadIdx.x;
    if (t >= r.n_out) return;
    const long j = r.out0 + t;
    if (r.N == 1) { y[t] = ts_load(x, -r.in0, r.n_valid); continue; }
    double pos = 0.0;
    if (r.M > 1) pos = j == r.M - 1 ? (double)(r.N - 1) : (double)(j * (r.N - 1)) / (double)(r.M - 1);
    long i = (long)floor(pos);
    if (i > r.N - 2) i = r.N - 2;
    const double x0 = ts_load(x, i - r.in0, r.n_valid), x1 = ts_load(x, i + 1 - r.in0, r.n_valid);
    y[t] = (float)((x1 - x0) * (pos - (double)i) + x0);
  }
}

// (c1, d1) beats (c2, d2): the larger correlation, then the smaller |delta|, then the negative delta
__device__ __forceinline__ bool ts_better(float c1, int d1, float c2, int d2) {
  if (c1 > c2) return true;
  if (!(c1 == c2)) return false;
  const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
  return a1 < a2 || (a1 == a2 && d1 < d2);
}

__global__ __launch_bounds__(THREADS) void k_ts_search(WsolaK P) {
  // all LDS is dynamic, every carve a multiple of 16 bytes: the wave maxima [2][WAVES], the template [W], candidates [W + 2 D + PAD]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* red_c = lds;
  int* red_d = reinterpret_cast<int*>(lds + WAVES);
  const int b = blockIdx.x;
  const RowW r = P.row[b];
  if (r.nk == 0) return;
  const int tid = threadIdx.x;
  const int W = P.W, D = P.D, Hs = W >> 1, nd = 2 * D + 1, span = W + 2 * D;
  float* tpl = lds + 2 * WAVES;
  float* cand = tpl + W;
  const float* x = P.x + (long)b * P.ldx;
  const int* centre = P.centre + (long)b * (P.ldk + 1);
  int* dout = P.delta + (long)b * P.ldk;
  int dprev = r.dprev;

  for (int i = 0; i < r.nk; ++i) {
    if (i == 0 && r.first) {           // frame 0
      dprev = 0;
      if (tid == 0) dout[0] = 0;
      continue;
    }
    const long tpos = (long)centre[i] + dprev;                   // p_{k-1} + Hs
    const long cpos = (long)centre[i + 1] - D - Hs;              // tap 0 of the candidate at delta = -D
    for (int n = tid; n < W; n += THREADS) tpl[n] = ts_load(x, tpos + n, r.n_valid);
    for (int n = tid; n < span + PAD; n += THREADS) cand[n] = n < span ? ts_load(x, cpos + n, r.n_valid) : 0.f;
    __syncthreads();

    float bc = -INFINITY;
    int bd = NO_DELTA;
    for (int e0 = tid * R; e0 < nd; e0 += PASS) {
      const float* c = cand + e0;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
      float v0 = c[0], v1 = c[1], v2 = c[2], v3 = c[3];
#pragma unroll 2
      for (int n = 0; n < W; n += 4) {
        const float4 t = *reinterpret_cast<const float4*>(tpl + n);
        const float v4 = c[n + 4], v5 = c[n + 5], v6 = c[n + 6], v7 = c[n + 7];
        a0 = fmaf(t.x, v0, a0); a1 = fmaf(t.x, v1, a1); a2 = fmaf(t.x, v2, a2); a3 = fmaf(t.x, v3, a3); a4 = fmaf(t.x, v4, a4);
        a0 = fmaf(t.y, v1, a0); a1 = fmaf(t.y, v2, a1); a2 = fmaf(t.y, v3, a2); a3 = fmaf(t.y, v4, a3); a4 = fmaf(t.y, v5, a4);
        a0 = fmaf(t.z, v2, a0); a1 = fmaf(t.z, v3, a1); a2 = fmaf(t.z, v4, a2); a3 = fmaf(t.z, v5, a3); a4 = fmaf(t.z, v6, a4);
        a0 = fmaf(t.w, v3, a0); a1 = fmaf(t.w, v4, a1); a2 = fmaf(t.w, v5, a2); a3 = fmaf(t.w, v6, a3); a4 = fmaf(t.w, v7, a4);
        v0 = v4; v1 = v5; v2 = v6; v3 = v7;
      }
      const int d0 = e0 - D;
      if (ts_better(a0, d0, bc, bd)) { bc = a0; bd = d0; }
      if (e0 + 1 < nd && ts_better(a1, d0 + 1, bc, bd)) { bc = a1; bd = d0 + 1; }
      if (e0 + 2 < nd && ts_better(a2, d0 + 2, bc, bd)) { bc = a2; bd = d0 + 2; }
      if (e0 + 3 < nd && ts_better(a3, d0 + 3, bc, bd)) { bc = a3; bd = d0 + 3; }
      if (e0 + 4 < nd && ts_better(a4, d0 + 4, bc, bd)) { bc = a4; bd = d0 + 4; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float oc = __shfl_xor(bc, s);
      const int od = __shfl_xor(bd, s);
      if (ts_better(oc, od, bc, bd)) { bc = oc; bd = od; }
    }
    if ((tid & 63) == 0) { red_c[tid >> 6] = bc; red_d[tid >> 6] = bd; }
    __syncthreads();                   // also: every read of tpl / cand of this frame lies before the next frame's staging
    bc = red_c[0]; bd = red_d[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      if (ts_better(red_c[w], red_d[w], bc, bd)) { bc = red_c[w]; bd = red_d[w]; }
    dprev = bd == NO_DELTA ? 0 : bd;
    if (tid == 0) dout[i] = dprev;
  }
}

__global__ __launch_bounds__(THREADS) void k_ts_synth(WsolaK P) {
  const int b = blockIdx.y;
  const RowW r = P.row[b];
  const int Hs = P.W >> 1;
  const float* x = P.x + (long)b * P.ldx;
  float* y = P.y + (long)b * P.ldy;
  const int* centre = P.centre + (long)b * (P.ldk + 1);
  const int* delta = P.delta + (long)b * P.ldk;
#pragma unroll
  for (int u = 0; u < TILE / THREADS; ++u) {
    const int t = blockIdx.x * TILE + u * THREADS + threadIdx.x;
    if (t >= r.n_out) return;
    const int mm = r.m0 + t;
    const int j = mm >> P.lgHs;        // frame ka = k0 - 1 + j; the host checked j + 1 <= nk
    const int nb = mm & (Hs - 1), na = nb + Hs;
    const int da = j == 0 ? r.dprev : delta[j - 1];
    const int ca = (j == 0 && r.first) ? 0 : centre[j];
    const long pa = (long)ca + da - Hs, pb = (long)centre[j + 1] + delta[j] - Hs;
    const float ya = P.win[na] * ts_load(x, pa + na, r.n_valid);
    y[t] = fmaf(P.win[nb], ts_load(x, pb + nb, r.n_valid), ya);
  }
}

int ts_fail(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

}  // namespace

extern "C" int dia_timescale(const dia_timescale_args* a, void* stream) {
  if (!a) return ts_fail("dia_timescale: null argument");
  if (!a->x || !a->y) return ts_fail("dia_timescale: null pointer (x and y are required)");
  if (!a->in_start || !a->out_start || !a->total || !a->in_count || !a->out_count)
    return ts_fail("dia_timescale: null pointer (the host arrays in_start, out_start, total, in_count and out_count are required)");
  if (a->mode != DIA_TS_INTERP && a->mode != DIA_TS_WSOLA) return ts_fail("dia_timescale: mode = %d is neither DIA_TS_INTERP nor DIA_TS_WSOLA", a->mode);
  if ((const void*)a->x == (const void*)a->y) return ts_fail("dia_timescale: y must not be x");
  if (a->B < 1 || a->B > DIA_TS_MAX_ROWS) return ts_fail("dia_timescale: B = %d outside [1, %d]", a->B, DIA_TS_MAX_ROWS);
  if (a->ldx < 1 || a->ldx > DIA_TS_MAX_T || a->ldy < 1 || a->ldy > DIA_TS_MAX_T)
    return ts_fail("dia_timescale: ldx = %d / ldy = %d outside [1, %d]", a->ldx, a->ldy, DIA_TS_MAX_T);
  const bool wsola = a->mode == DIA_TS_WSOLA;
  int lgHs = 0;
  if (wsola) {
    if (!a->win || !a->centre || !a->delta || !a->k0 || !a->k1 || !a->delta_prev)
      return ts_fail("dia_timescale: null pointer (DIA_TS_WSOLA needs win, centre, delta and the host arrays k0, k1 and delta_prev)");
    if (a->window < DIA_TS_MIN_WINDOW || a->window > DIA_TS_MAX_WINDOW || (a->window & (a->window - 1)))
      return ts_fail("dia_timescale: window = %d is not a power of two in [%d, %d]", a->window, DIA_TS_MIN_WINDOW, DIA_TS_MAX_WINDOW);
    if (a->tolerance < 0 || a->tolerance > a->window) return ts_fail("dia_timescale: tolerance = %d outside [0, window = %d]", a->tolerance, a->window);
    if (a->ldk < 1 || a->ldk > DIA_TS_MAX_T) return ts_fail("dia_timescale: ldk = %d outside [1, %d]", a->ldk, DIA_TS_MAX_T);
    while ((2 << lgHs) < a->window) ++lgHs;
  } else if (!a->out_total) {
    return ts_fail("dia_timescale: null pointer (DIA_TS_INTERP needs the host array out_total)");
  }
  const long Hs = wsola ? a->window / 2 : 0;
  WsolaK kw = {};
  InterpK ki = {};
  int most = 0, most_k = 0;
  for (int b = 0; b < a->B; ++b) {
    const long in0 = a->in_start[b], out0 = a->out_start[b], tot = a->total[b];
    if (in0 < 0 || out0 < 0) return ts_fail("dia_timescale: row %d: in_start = %ld / out_start = %ld is negative", b, in0, out0);
    if (tot < 0 && tot != DIA_TS_OPEN) return ts_fail("dia_timescale: row %d: total = %ld is neither a length nor DIA_TS_OPEN", b, tot);
    if (a->in_count[b] < 0 || a->in_count[b] > a->ldx) return ts_fail("dia_timescale: row %d: in_count = %d outside [0, ldx = %d]", b, a->in_count[b], a->ldx);
    if (a->out_count[b] < 0 || a->out_count[b] > a->ldy) return ts_fail("dia_timescale: row %d: out_count = %d outside [0, ldy = %d]", b, a->out_count[b], a->ldy);
    long valid = a->in_count[b];
    if (tot != DIA_TS_OPEN && tot - in0 < valid) valid = tot - in0 > 0 ? tot - in0 : 0;
    const int cnt = a->out_count[b];
    if (wsola) {
      const long k0 = a->k0[b], k1 = a->k1[b];
      if (k0 < 0 || k1 < k0) return ts_fail("dia_timescale: row %d: frames [%ld, %ld) are not a range", b, k0, k1);
      if (k1 - k0 > a->ldk) return ts_fail("dia_timescale: row %d: %ld frames exceed ldk = %d", b, k1 - k0, a->ldk);
      if (k1 > (1L << 40)) return ts_fail("dia_timescale: row %d: frame %ld is out of range", b, k1);
      const long m0 = out0 - (k0 - 1) * Hs;
      if (cnt > 0 && (m0 < 0 || m0 + cnt > (k1 - k0) * Hs))
        return ts_fail("dia_timescale: row %d: outputs [%ld, %ld) lie outside [%ld, %ld), the range of frames [%ld, %ld)", b, out0, out0 + cnt,
                       (k0 - 1) * Hs, (k1 - 1) * Hs, k0 - 1, k1);
      RowW& r = kw.row[b];
      r.n_valid = (int)valid; r.nk = (int)(k1 - k0); r.first = k0 == 0; r.dprev = k0 == 0 ? 0 : a->delta_prev[b];
      r.m0 = cnt > 0 ? (int)m0 : 0; r.n_out = cnt;
      if (r.nk > most_k) most_k = r.nk;
    } else {
      const long M = a->out_total[b];
      if (tot == DIA_TS_OPEN || tot < 1 || tot > (1L << 31)) return ts_fail("dia_timescale: row %d: DIA_TS_INTERP needs a total in [1, 2^31], not %ld", b, tot);
      if (M < 1 || M > (1L << 31)) return ts_fail("dia_timescale: row %d: out_total = %ld outside [1, 2^31]", b, M);
      if (out0 + cnt > M) return ts_fail("dia_timescale: row %d: outputs [%ld, %ld) lie beyond out_total = %ld", b, out0, out0 + cnt, M);
      RowI& r = ki.row[b];
      r.N = tot; r.M = M; r.out0 = out0; r.in0 = in0; r.n_valid = (int)valid; r.n_out = cnt;
    }
    if (cnt > most) most = cnt;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (!wsola) {
    if (most == 0) return 0;
    ki.x = a->x; ki.y = a->y; ki.ldx = a->ldx; ki.ldy = a->ldy;
    dia_launch<k_ts_interp>(dim3((most + TILE - 1) / TILE, a->B), dim3(THREADS), 0, st, ki);
    return dia_check_launch("k_ts_interp");
  }
  kw.x = a->x; kw.y = a->y; kw.win = a->win; kw.centre = a->centre; kw.delta = a->delta;
  kw.ldx = a->ldx; kw.ldy = a->ldy; kw.ldk = a->ldk; kw.W = a->window; kw.D = a->tolerance; kw.lgHs = lgHs;
  if (most_k > 0) {
    const size_t smem = (size_t)(2 * WAVES + 2 * a->window + 2 * a->tolerance + PAD) * sizeof(float);
    dia_launch<k_ts_search>(dim3(a->B), dim3(THREADS), smem, st, kw);
    if (int rc = dia_check_launch("k_ts_search")) return rc;
  }
  if (most == 0) return 0;
  dia_launch<k_ts_synth>(dim3((most + TILE - 1) / TILE, a->B), dim3(THREADS), 0, st, kw);
  return dia_check_launch("k_ts_synth");
}
