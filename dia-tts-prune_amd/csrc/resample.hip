// Resampler: polyphase sample-rate conversion, dia_resample (DESIGN.md "Resampler").
//
// Output m = q n + p of a row is sum_k bank[k][p] * x[q o + first[p] + k] over the nt compact taps of phase p: an fp32 fmaf chain
// from 0 in ascending k, whatever the row, the tile or the window, so that cutting a signal into windows, chunks or batch rows
// changes no bit of it.  About 2 nt flops against 4 (1 + o / n) bytes per output: a VALU kernel bound by launch and memory.
//
// A workgroup of 256 threads owns TILE = 1024 consecutive outputs of one row.  first[] is nondecreasing along the outputs, so the
// taps of the tile cover one contiguous input span, from tap 0 of its first output to tap nt - 1 of its last: at most
// ceil((TILE - 1) o / n) + 2 + nt samples.  They are staged in LDS once, zero where the window has no sample (before 0, at or
// beyond the signal's end, which is also what keeps a NaN behind a row's length out of the sums).  Lane l then takes outputs
// l, l + 256, l + 512, l + 768 of the tile: the four chains are independent, stores are coalesced, and the bank is tap-major
// ([nt][n]), so lanes of consecutive phase read consecutive floats of it through the vector cache.  LDS reads of a wave are
// consecutive outputs' taps: the same or the next address when upsampling (broadcast, no conflict), a stride of o / n floats
// when downsampling (44100 -> 16000: 2.76, up to 3 lanes of a 32-lane group on one bank).
//
// The rows' windows come as 64-bit absolute indices in HOST arrays; they are reduced here to (phase of the first output, 32-bit
// offset of its period in the window, samples valid in the window) and travel in the kernel's arguments, at most 64 rows a launch.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdarg>
#include <cstdio>

namespace {

constexpr int TILE = DIA_RESAMPLE_TILE;
constexpr int THREADS = 256;
constexpr int PER = TILE / THREADS;    // outputs per thread

struct RowK {
  int n_out;                           // outputs of this row
  int p0;                              // phase of output 0 of the row
  int xoff;                            // window index of the input sample at (period of output 0) * o
  int n_valid;                         // window samples that exist: [0, n_valid) of x[b]
};

struct ResK {
  const float* x; float* y; const float* bank; const int* first;
  int ldx, ldy, o, n, nt, cap;         // cap: floats of dynamic LDS
  RowK row[DIA_RESAMPLE_MAX_ROWS];
};

__global__ __launch_bounds__(THREADS) void k_resample(ResK P) {
  extern __shared__ float xs[];
  const int b = blockIdx.y;
  const RowK r = P.row[b];
  const int tile0 = blockIdx.x * TILE;
  if (tile0 >= r.n_out) return;
  const int tid = threadIdx.x;
  const int cnt = min(TILE, r.n_out - tile0);
  const int n = P.n, o = P.o, nt = P.nt;

  // the staged span: tap 0 of the tile's first output .. tap nt - 1 of its last
  const int t0 = r.p0 + tile0, q0 = t0 / n, pp0 = t0 - q0 * n;
  const int t1 = t0 + cnt - 1, q1 = t1 / n, pp1 = t1 - q1 * n;
  const int lo = q0 * o + P.first[pp0] + r.xoff;
  int span = q1 * o + P.first[pp1] + r.xoff + nt - lo;
  span = min(max(span, nt), P.cap);                              // a malformed first[] cannot lead outside the LDS
  const float* x = P.x + (long)b * P.ldx;
  for (int i = tid; i < span; i += THREADS) {
    const int rel = lo + i;
    xs[i] = (rel >= 0 && rel < r.n_valid) ? x[rel] : 0.f;
  }
  __syncthreads();

  const int qs = THREADS / n, rs = THREADS - qs * n;             // the step between a lane's outputs, in periods and phases
  int t = t0 + tid, q = t / n, p = t - q * n;
  int ph[PER], at[PER];
  float acc[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const bool live = tid + i * THREADS < cnt;
    ph[i] = live ? p : 0;
    at[i] = live ? min(max(q * o + P.first[ph[i]] + r.xoff - lo, 0), span - nt) : 0;
    acc[i] = 0.f;
    p += rs; q += qs;
    if (p >= n) { p -= n; ++q; }
  }
  const float* bank = P.bank;
#pragma unroll 2
  for (int k = 0; k < nt; ++k) {
#pragma unroll
    for (int i = 0; i < PER; ++i) acc[i] = fmaf(bank[ph[i]], xs[at[i] + k], acc[i]);
    bank += n;
  }
  float* y = P.y + (long)b * P.ldy + tile0;
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (tid + i * THREADS < cnt) y[tid + i * THREADS] = acc[i];
}

int resample_fail(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

}  // namespace

extern "C" int dia_resample(const dia_resample_args* a, void* stream) {
  if (!a) return resample_fail("dia_resample: null argument");
  if (!a->x || !a->y || !a->bank || !a->first) return resample_fail("dia_resample: null pointer (x, y, bank and first are required)");
  if (!a->in_start || !a->out_start || !a->total || !a->in_count || !a->out_count)
    return resample_fail("dia_resample: null pointer (the host arrays in_start, out_start, total, in_count and out_count are required)");
  if ((const void*)a->x == (const void*)a->y) return resample_fail("dia_resample: y must not be x");
  if (a->B < 1 || a->B > DIA_RESAMPLE_MAX_ROWS) return resample_fail("dia_resample: B = %d outside [1, %d]", a->B, DIA_RESAMPLE_MAX_ROWS);
  if (a->o < 1 || a->o > DIA_RESAMPLE_MAX_T || a->n < 1 || a->n > DIA_RESAMPLE_MAX_T)
    return resample_fail("dia_resample: o = %d / n = %d outside [1, %d]", a->o, a->n, DIA_RESAMPLE_MAX_T);
  if (a->nt < 1 || a->nt > DIA_RESAMPLE_MAX_TAPS) return resample_fail("dia_resample: nt = %d outside [1, %d]", a->nt, DIA_RESAMPLE_MAX_TAPS);
  if (a->ldx < 1 || a->ldx > DIA_RESAMPLE_MAX_T || a->ldy < 1 || a->ldy > DIA_RESAMPLE_MAX_T)
    return resample_fail("dia_resample: ldx = %d / ldy = %d outside [1, %d]", a->ldx, a->ldy, DIA_RESAMPLE_MAX_T);
  const long cap = ((long)(TILE - 1) * a->o + a->n - 1) / a->n + 2 + a->nt;
  if (cap > DIA_RESAMPLE_MAX_TILE_FLOATS)
    return resample_fail("dia_resample: o = %d, n = %d, nt = %d: a workgroup's input tile of %ld floats exceeds %d", a->o, a->n, a->nt, cap,
                         DIA_RESAMPLE_MAX_TILE_FLOATS);
  ResK k = {};
  k.x = a->x; k.y = a->y; k.bank = a->bank; k.first = a->first;
  k.ldx = a->ldx; k.ldy = a->ldy; k.o = a->o; k.n = a->n; k.nt = a->nt; k.cap = (int)cap;
  int most = 0;
  for (int b = 0; b < a->B; ++b) {
    const long in0 = a->in_start[b], out0 = a->out_start[b], tot = a->total[b];
    if (in0 < 0 || out0 < 0) return resample_fail("dia_resample: row %d: in_start = %ld / out_start = %ld is negative", b, in0, out0);
    if (tot < 0 && tot != DIA_RESAMPLE_OPEN) return resample_fail("dia_resample: row %d: total = %ld is neither a length nor DIA_RESAMPLE_OPEN", b, tot);
    if (a->in_count[b] < 0 || a->in_count[b] > a->ldx) return resample_fail("dia_resample: row %d: in_count = %d outside [0, ldx = %d]", b, a->in_count[b], a->ldx);
    if (a->out_count[b] < 0 || a->out_count[b] > a->ldy) return resample_fail("dia_resample: row %d: out_count = %d outside [0, ldy = %d]", b, a->out_count[b], a->ldy);
    const long xoff = out0 / a->n * a->o - in0;
    // every index the kernel forms stays below 2^31: |xoff| + (periods of a row + 2) * o + nt
    if (xoff < -(1L << 29) || xoff > (1L << 29) || ((long)a->out_count[b] / a->n + 2) * a->o > (1L << 29))
      return resample_fail("dia_resample: row %d: the window [%ld, +%d) lies too far from output %ld (o = %d, n = %d)", b, in0, a->in_count[b], out0, a->o, a->n);
    long valid = a->in_count[b];
    if (tot != DIA_RESAMPLE_OPEN && tot - in0 < valid) valid = tot - in0 > 0 ? tot - in0 : 0;
    k.row[b].n_out = a->out_count[b];
    k.row[b].p0 = (int)(out0 % a->n);
    k.row[b].xoff = (int)xoff;
    k.row[b].n_valid = (int)valid;
    if (a->out_count[b] > most) most = a->out_count[b];
  }
  if (most == 0) return 0;
  dia_launch<k_resample>(dim3((most + TILE - 1) / TILE, a->B), dim3(THREADS), (size_t)cap * sizeof(float), (hipStream_t)stream, k);
  return dia_check_launch("k_resample");
}
