// Loudness: the sample arithmetic of an ITU-R BS.1770-4 meter and a gain, dia_loudness (DESIGN.md "Loudness").
//
// The K-weighting is two biquads in cascade with a float64 state (the high-pass has a double pole at 0.995).  A recursion is
// sequential in the sample index, but it is linear: with the 4 x 4 zero-input transition A of the state over one sample, the state
// after n samples is A^n s + (the zero-state response), so a row is cut into chunks that run in parallel and are joined by a carry.
// The grid is absolute and never straddles a 100 ms step: one workgroup (ONE wave) owns one step, one lane one chunk of it.
//
// k_loud_ends   tile t of row b = samples [t step, (t + 1) step), staged through LDS with a halo by coalesced loads (zero outside
//               the row).  (a) Peaks, over every sample of the row, whole step or not: lane l takes samples l, l + 64, ...; the four
//               oversampled values behind a sample are fp32 fmaf chains from 0 in ascending tap over the 1 -> 4 bank (LDS, broadcast
//               reads); max |.| is exact in any order, so the wave reduces it by shuffles.  (b) When the step is whole, lane c runs
//               chunk c from the ZERO state and leaves its end state e_c in LDS; then every lane walks z_0 = 0,
//               z_{c+1} = A^chunk z_c + e_c (uniform, e_c a broadcast read) and keeps z of its own chunk: the chunk's initial state had
//               the step started from zero.  z goes to the workspace, and so does the step's zero-state end state E.
// k_loud_carry  one wave per row: lane 0 walks the steps, init_0 = 0, init_{s+1} = A^step init_s + E_s; all lanes reduce the tiles'
//               peaks.
// k_loud_sums   step s of row b again: lane c starts from z_c + A^(c chunk) init_s, the true state, and adds the squares of its
//               outputs in float64 in ascending sample order; lane 0 adds the chunks' sums in ascending chunk order.
// k_loud_apply  y = (float)((double)x * gain), one thread per output.
//
// A lane reads LDS at a stride of `chunk` words; the plan (dia_hip/loudness.py) keeps chunk odd, so the 64 lanes hit 64 banks.
// Every index into x is tested against [0, len) before the load.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace {

constexpr int LANES = 64;
constexpr int APPLY_THREADS = 256;
constexpr int APPLY_TILE = 4 * APPLY_THREADS;
constexpr int T_COEF = 0, T_CHUNK = 10, T_STEP = 26, T_POW = 42;      // offsets into dia_loudness_args.table

struct MeasK {
  const float* x; double* steps; float* peaks; double* ws; const double* table; const float* bank;
  int ldx, ld_steps, step, chunk, chunks, nt, halo;
  int first[4];
  int len[DIA_LOUD_MAX_ROWS];
};

struct ApplyK {
  const float* x; float* y;
  int ldx, ldy;
  int in_off[DIA_LOUD_MAX_ROWS];
  int out_count[DIA_LOUD_MAX_ROWS];
  double gain[DIA_LOUD_MAX_ROWS];
};

// the workspace of row b: E [ld_steps][4], init [ld_steps][4], z [ld_steps][chunks][4], tile peaks [ld_steps + 1] (two floats each)
struct RowWs { double* E; double* init; double* z; float2* pk; };
__device__ __forceinline__ RowWs row_ws(const MeasK& P, int b) {
  const long per = (long)P.ld_steps * (8 + 4 * P.chunks) + P.ld_steps + 1;
  double* w = P.ws + (long)b * per;
  RowWs r;
  r.E = w;
  r.init = w + (long)P.ld_steps * 4;
  r.z = w + (long)P.ld_steps * 8;
  r.pk = reinterpret_cast<float2*>(w + (long)P.ld_steps * (8 + 4 * P.chunks));
  return r;
}

struct Coef { double b0, b1, b2, a1, a2; };
__device__ __forceinline__ Coef load_coef(const double* t) { return Coef{t[0], t[1], t[2], t[3], t[4]}; }

// one sample through one biquad (transposed direct form II); the chain from sample to sample is y -> s1: two fma
__device__ __forceinline__ double biquad(const Coef& c, double x, double& s1, double& s2) {
  const double y = fma(c.b0, x, s1);
  s1 = fma(-c.a1, y, fma(c.b1, x, s2));
  s2 = fma(c.b2, x, -c.a2 * y);
  return y;
}

// out = M v + add, M row-major; each row one fma chain in ascending column
__device__ __forceinline__ void matvec(const double* M, const double v[4], const double add[4], double out[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s = add[r];
#pragma unroll
    for (int k = 0; k < 4; ++k) s = fma(M[4 * r + k], v[k], s);
    out[r] = s;
  }
}

__global__ __launch_bounds__(LANES) void k_loud_ends(MeasK P) {
  // dynamic LDS: end states [chunks][4] float64, then the bank [4 nt], then the tile [step + 2 halo]
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* es = lds_d;
  float* bank = reinterpret_cast<float*>(es + 4 * P.chunks);
  float* xs = bank + 4 * P.nt;
  const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
  const int n = P.len[b];
  const long t0 = (long)t * P.step;
  if (t0 >= n) return;
  const float* x = P.x + (long)b * P.ldx;
  const int H = P.halo, S = P.step;
  for (int i = lane; i < S + 2 * H; i += LANES) {
    const long at = t0 - H + i;
    xs[i] = (at >= 0 && at < n) ? x[at] : 0.f;
  }
  for (int i = lane; i < 4 * P.nt; i += LANES) bank[i] = P.bank[i];
  __syncthreads();

  const int cnt = (n - t0 < S) ? (int)(n - t0) : S;
  float sp = 0.f, tp = 0.f;
  for (int q = lane; q < cnt; q += LANES) {
    sp = fmaxf(sp, fabsf(xs[H + q]));
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float* c = xs + H + q + P.first[p];
      const float* h = bank + p * P.nt;
      float acc = 0.f;
      for (int k = 0; k < P.nt; ++k) acc = fmaf(h[k], c[k], acc);
      tp = fmaxf(tp, fabsf(acc));
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    sp = fmaxf(sp, __shfl_xor(sp, s));
    tp = fmaxf(tp, __shfl_xor(tp, s));
  }
  RowWs w = row_ws(P, b);
  if (lane == 0) w.pk[t] = make_float2(sp, fmaxf(sp, tp));
  if (cnt < S) return;                                     // not a whole step: no sums (uniform)

  const Coef ca = load_coef(P.table + T_COEF), cb = load_coef(P.table + T_COEF + 5);
  const int C = P.chunks, L = P.chunk;
  if (lane < C) {
    const int i0 = lane * L, i1 = (i0 + L < S) ? i0 + L : S;
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0;
    for (int i = i0; i < i1; ++i) biquad(cb, biquad(ca, (double)xs[H + i], s1a, s2a), s1b, s2b);
    es[4 * lane + 0] = s1a; es[4 * lane + 1] = s2a; es[4 * lane + 2] = s1b; es[4 * lane + 3] = s2b;
  }
  __syncthreads();
  double ML[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) ML[i] = P.table[T_CHUNK + i];
  double z[4] = {0.0, 0.0, 0.0, 0.0}, mine[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c + 1 < C; ++c) {                        // z_{c+1} from z_c: the last chunk's end is not needed here
    double e[4] = {es[4 * c], es[4 * c + 1], es[4 * c + 2], es[4 * c + 3]}, nz[4];
    matvec(ML, z, e, nz);
#pragma unroll
    for (int r = 0; r < 4; ++r) { z[r] = nz[r]; if (c + 1 == lane) mine[r] = nz[r]; }
  }
  if (lane < C) {
    double* zo = w.z + ((long)t * C + lane) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) zo[r] = mine[r];
  }
  if (lane == C - 1) {
    // the step's zero-state end state: the last chunk run on from z_{C-1}.  Its length differs from `chunk`, so instead of a
    // second matrix the lane simply runs its samples again from z
    const int i0 = lane * L;
    double s1a = mine[0], s2a = mine[1], s1b = mine[2], s2b = mine[3];
    for (int i = i0; i < S; ++i) biquad(cb, biquad(ca, (double)xs[H + i], s1a, s2a), s1b, s2b);
    double* E = w.E + (long)t * 4;
    E[0] = s1a; E[1] = s2a; E[2] = s1b; E[3] = s2b;
  }
}

__global__ __launch_bounds__(LANES) void k_loud_carry(MeasK P) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = P.len[b];
  const int ns = n / P.step, tiles = (n + P.step - 1) / P.step;
  RowWs w = row_ws(P, b);
  float sp = 0.f, tp = 0.f;
  for (int t = lane; t < tiles; t += LANES) {
    const float2 v = w.pk[t];
    sp = fmaxf(sp, v.x);
    tp = fmaxf(tp, v.y);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    sp = fmaxf(sp, __shfl_xor(sp, s));
    tp = fmaxf(tp, __shfl_xor(tp, s));
  }
  if (lane != 0) return;
  P.peaks[2 * b] = sp;
  P.peaks[2 * b + 1] = tp;
  double MS[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) MS[i] = P.table[T_STEP + i];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < ns; ++s) {
    double* o = w.init + (long)s * 4;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    const double* Es = w.E + (long)s * 4;
    double e[4] = {Es[0], Es[1], Es[2], Es[3]}, nv[4];
    matvec(MS, v, e, nv);
    v[0] = nv[0]; v[1] = nv[1]; v[2] = nv[2]; v[3] = nv[3];
  }
}

__global__ __launch_bounds__(LANES) void k_loud_sums(MeasK P) {
  // dynamic LDS: the chunks' sums [chunks] float64, then the step [step]
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* sums = lds_d;
  float* xs = reinterpret_cast<float*>(sums + P.chunks);
  const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
  const int n = P.len[b], S = P.step;
  if (t >= n / S) return;
  const float* x = P.x + (long)b * P.ldx + (long)t * S;    // [t S, (t + 1) S) lies inside [0, n)
  for (int i = lane; i < S; i += LANES) xs[i] = x[i];
  __syncthreads();
  const Coef ca = load_coef(P.table + T_COEF), cb = load_coef(P.table + T_COEF + 5);
  const int C = P.chunks, L = P.chunk;
  RowWs w = row_ws(P, b);
  if (lane < C) {
    const double* zi = w.z + ((long)t * C + lane) * 4;
    const double* in = w.init + (long)t * 4;
    const double z[4] = {zi[0], zi[1], zi[2], zi[3]}, v[4] = {in[0], in[1], in[2], in[3]};
    double s[4];
    matvec(P.table + T_POW + 16 * lane, v, z, s);
    const int i0 = lane * L, i1 = (i0 + L < S) ? i0 + L : S;
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
      const double y = biquad(cb, biquad(ca, (double)xs[i], s[0], s[1]), s[2], s[3]);
      acc = fma(y, y, acc);
    }
    sums[lane] = acc;
  }
  __syncthreads();
  if (lane == 0) {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) acc += sums[c];
    P.steps[(long)b * P.ld_steps + t] = acc;
  }
}

__global__ __launch_bounds__(APPLY_THREADS) void k_loud_apply(ApplyK P) {
  const int b = blockIdx.y;
  const int cnt = P.out_count[b];
  const double g = P.gain[b];
  const float* x = P.x + (long)b * P.ldx + P.in_off[b];
  float* y = P.y + (long)b * P.ldy;
#pragma unroll
  for (int u = 0; u < APPLY_TILE / APPLY_THREADS; ++u) {
    const int i = blockIdx.x * APPLY_TILE + u * APPLY_THREADS + threadIdx.x;
    if (i >= cnt) return;
    y[i] = (float)((double)x[i] * g);
  }
}

int ld_fail(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

}  // namespace

extern "C" int dia_loudness(const dia_loudness_args* a, void* stream) {
  if (!a) return ld_fail("dia_loudness: null argument");
  if (!a->x || !a->len) return ld_fail("dia_loudness: null pointer (x and the host array len are required)");
  if (a->mode != DIA_LOUD_MEASURE && a->mode != DIA_LOUD_APPLY)
    return ld_fail("dia_loudness: mode = %d is neither DIA_LOUD_MEASURE nor DIA_LOUD_APPLY", a->mode);
  if (a->B < 1 || a->B > DIA_LOUD_MAX_ROWS) return ld_fail("dia_loudness: B = %d outside [1, %d]", a->B, DIA_LOUD_MAX_ROWS);
  if (a->ldx < 1 || a->ldx > DIA_LOUD_MAX_T) return ld_fail("dia_loudness: ldx = %d outside [1, %d]", a->ldx, DIA_LOUD_MAX_T);
  for (int b = 0; b < a->B; ++b)
    if (a->len[b] < 0 || a->len[b] > a->ldx) return ld_fail("dia_loudness: row %d: len = %d outside [0, ldx = %d]", b, a->len[b], a->ldx);
  const hipStream_t st = (hipStream_t)stream;

  if (a->mode == DIA_LOUD_APPLY) {
    if (!a->y || !a->in_off || !a->out_count || !a->gain)
      return ld_fail("dia_loudness: null pointer (DIA_LOUD_APPLY needs y and the host arrays in_off, out_count and gain)");
    if ((const void*)a->x == (const void*)a->y) return ld_fail("dia_loudness: y must not be x");
    if (a->ldy < 1 || a->ldy > DIA_LOUD_MAX_T) return ld_fail("dia_loudness: ldy = %d outside [1, %d]", a->ldy, DIA_LOUD_MAX_T);
    ApplyK k = {};
    int most = 0;
    for (int b = 0; b < a->B; ++b) {
      const int off = a->in_off[b], cnt = a->out_count[b];
      if (off < 0) return ld_fail("dia_loudness: row %d: in_off = %d is negative", b, off);
      if (cnt < 0 || cnt > a->ldy) return ld_fail("dia_loudness: row %d: out_count = %d outside [0, ldy = %d]", b, cnt, a->ldy);
      if ((long)off + cnt > a->len[b]) return ld_fail("dia_loudness: row %d: samples [%d, %ld) lie beyond len = %d", b, off, (long)off + cnt, a->len[b]);
      if (!std::isfinite(a->gain[b])) return ld_fail("dia_loudness: row %d: the gain is not finite", b);
      k.in_off[b] = off; k.out_count[b] = cnt; k.gain[b] = a->gain[b];
      if (cnt > most) most = cnt;
    }
    if (most == 0) return 0;
    k.x = a->x; k.y = a->y; k.ldx = a->ldx; k.ldy = a->ldy;
    dia_launch<k_loud_apply>(dim3((most + APPLY_TILE - 1) / APPLY_TILE, a->B), dim3(APPLY_THREADS), 0, st, k);
    return dia_check_launch("k_loud_apply");
  }

  if (!a->steps || !a->peaks || !a->ws || !a->table || !a->bank || !a->first)
    return ld_fail("dia_loudness: null pointer (DIA_LOUD_MEASURE needs steps, peaks, ws, table, bank and the host array first)");
  if (a->step < DIA_LOUD_MIN_STEP || a->step > DIA_LOUD_MAX_STEP)
    return ld_fail("dia_loudness: step = %d outside [%d, %d]", a->step, DIA_LOUD_MIN_STEP, DIA_LOUD_MAX_STEP);
  if (a->chunk < 1 || a->chunk > a->step) return ld_fail("dia_loudness: chunk = %d outside [1, step = %d]", a->chunk, a->step);
  if (a->chunks != (a->step + a->chunk - 1) / a->chunk || a->chunks > DIA_LOUD_MAX_CHUNKS)
    return ld_fail("dia_loudness: chunks = %d is not ceil(step / chunk) = %d, or above %d", a->chunks, (a->step + a->chunk - 1) / a->chunk,
                   DIA_LOUD_MAX_CHUNKS);
  if (a->nt < 1 || a->nt > DIA_LOUD_MAX_TAPS) return ld_fail("dia_loudness: nt = %d outside [1, %d]", a->nt, DIA_LOUD_MAX_TAPS);
  if (a->ld_steps < 1) return ld_fail("dia_loudness: ld_steps = %d below 1", a->ld_steps);
  MeasK k = {};
  int halo = 0;
  for (int p = 0; p < 4; ++p) {
    const int lo = a->first[p], hi = a->first[p] + a->nt - 1;
    if (lo < -DIA_LOUD_MAX_TAPS || hi > DIA_LOUD_MAX_TAPS)
      return ld_fail("dia_loudness: phase %d reads x[q + %d .. q + %d], outside [-%d, %d]", p, lo, hi, DIA_LOUD_MAX_TAPS, DIA_LOUD_MAX_TAPS);
    if (-lo > halo) halo = -lo;
    if (hi > halo) halo = hi;
    k.first[p] = lo;
  }
  int most = 0;
  for (int b = 0; b < a->B; ++b) {
    if (a->len[b] / a->step > a->ld_steps)
      return ld_fail("dia_loudness: row %d: %d whole steps exceed ld_steps = %d", b, a->len[b] / a->step, a->ld_steps);
    k.len[b] = a->len[b];
    if (a->len[b] > most) most = a->len[b];
  }
  const long need = DIA_LOUD_WS_DOUBLES(a->B, a->ld_steps, a->chunks);
  if (a->ws_doubles < need) return ld_fail("dia_loudness: ws_doubles = %ld below the %ld this launch needs", (long)a->ws_doubles, need);
  k.x = a->x; k.steps = a->steps; k.peaks = a->peaks; k.ws = a->ws; k.table = a->table; k.bank = a->bank;
  k.ldx = a->ldx; k.ld_steps = a->ld_steps; k.step = a->step; k.chunk = a->chunk; k.chunks = a->chunks; k.nt = a->nt; k.halo = halo;
  const int tiles = (most + a->step - 1) / a->step, whole = most / a->step;
  if (tiles > 0) {
    const size_t smem = (size_t)4 * a->chunks * sizeof(double) + (size_t)(4 * a->nt + a->step + 2 * halo) * sizeof(float);
    dia_launch<k_loud_ends>(dim3(tiles, a->B), dim3(LANES), smem, st, k);
    if (int rc = dia_check_launch("k_loud_ends")) return rc;
  }
  dia_launch<k_loud_carry>(dim3(a->B), dim3(LANES), 0, st, k);
  if (int rc = dia_check_launch("k_loud_carry")) return rc;
  if (whole == 0) return 0;
  const size_t smem = (size_t)a->chunks * sizeof(double) + (size_t)a->step * sizeof(float);
  dia_launch<k_loud_sums>(dim3(whole, a->B), dim3(LANES), smem, st, k);
  return dia_check_launch("k_loud_sums");
}
