// Activation statistics for activation-aware pruning (dia_act_stats, DESIGN.md "Activation statistics").
//
// Wanda ranks a weight by |W[k][n]| * ||x_k||_2, the norm of input channel k over a calibration set.  Every GEMM input of the
// decode step and of the encoder already lies on the device as an activation plane set (common.hpp); this kernel adds the squares
// of one plane set's counted rows into one double per channel:
//   acc[k] += sum over counted rows m, in ascending m, of (double)v * (double)v,   v = fl32(x[m][k] * scale[m])
// The reference has no counterpart: its pruning looks at the weights alone (offline_prune.py:82-156).
//
// One thread owns a fragment of 8 consecutive channels (the 32- or 16-byte fragment of the plane layout) and walks the rows in
// order: no atomics, no cross-thread reduction, so a channel's sum does not depend on how the rows are spread over launches
// or on eager against graph replay.  Rows are taken in chunks of 64: lane i of each workgroup forms the gate and the scale of
// row 64 * chunk + i once and hands them over in LDS.
//
// fp contraction is OFF in this file: v is the product rounded to fp32, and the scale is the expression of the header,
// rounding by rounding.
#pragma clang fp contract(off)
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdio>

namespace {

constexpr int CHUNK = 64;             // rows per hand-over = threads per workgroup

struct CalibK {
  const void* x; long plane_stride; int ktiles, kt_used, M, act_f32;
  const float* ssq_in; int ssq_in_n, ssq_ld; float inv_d, eps;
  const uint8_t* row_mask;
  const int* cur; const int* first_step; const int* fsm; int T, rows_per_slot;
  double* acc; long long* counter;
};

__global__ __launch_bounds__(CHUNK) void k_act_stats(CalibK p) {
  __shared__ float sc[CHUNK];          // the row's scale ...
  __shared__ int cnt[CHUNK];           // ... and whether the row counts
  const int tid = threadIdx.x;
  const int frag = blockIdx.x * CHUNK + tid;          // 8 channels k0 .. k0 + 7
  const bool own = frag < p.kt_used * 4;
  const int k0 = frag * 8;
  double a[8];
  if (own) {
    const double2* ap = reinterpret_cast<const double2*>(p.acc + k0);
#pragma unroll
    for (int j = 0; j < 4; ++j) { const double2 t = ap[j]; a[2 * j] = t.x; a[2 * j + 1] = t.y; }
  }
  long long counted = 0;
  for (int m0 = 0; m0 < p.M; m0 += CHUNK) {
    const int m = m0 + tid;
    float s = 1.0f;
    bool on = false;
    if (m < p.M) {
      on = p.row_mask ? p.row_mask[m] != 0 : true;
      if (p.rows_per_slot > 0) {       // k_score's gate: prompt replay rows, a finished utterance, a row outside the buffer
        const int b = m / p.rows_per_slot;
        const int t = p.cur[b];
        const int first = p.first_step ? p.first_step[b] : 1;
        const bool done = p.fsm ? p.fsm[b * 8 + 3] != 0 : false;
        on = on && t >= first && t >= 0 && t < p.T && !done;
      }
      if (on && p.ssq_in) {
        float q = 0.f;
        for (int i = 0; i < p.ssq_in_n; ++i) q += p.ssq_in[(long)i * p.ssq_ld + m];
        s = 1.0f / sqrtf(q * p.inv_d + p.eps);
      }
    }
    __syncthreads();                   // the previous chunk has been read
    sc[tid] = s; cnt[tid] = on ? 1 : 0;
    __syncthreads();
    const int n = min(CHUNK, p.M - m0);
    for (int r = 0; r < n; ++r) {
      if (!cnt[r]) continue;           // (uniform over the workgroup)
      const float s_r = sc[r];
      ++counted;
      if (!own) continue;
      const long off = plane_frag_off(m0 + r, k0, p.ktiles);
      float v[8];
      if (p.act_f32) {
        KVElem<float>::load8(reinterpret_cast<const float*>(p.x) + off, v);
      } else {
        const bf16_raw* P = reinterpret_cast<const bf16_raw*>(p.x) + off;
        float mi[8], lo[8];
        KVElem<bf16_raw>::load8(P, v);
        KVElem<bf16_raw>::load8(P + p.plane_stride, mi);
        KVElem<bf16_raw>::load8(P + 2 * p.plane_stride, lo);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (v[j] + mi[j]) + lo[j];       // exact: split3
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float w = v[j] * s_r;
        a[j] += (double)w * (double)w;
      }
    }
  }
  if (own) {
    double2* ap = reinterpret_cast<double2*>(p.acc + k0);
#pragma unroll
    for (int j = 0; j < 4; ++j) ap[j] = double2{a[2 * j], a[2 * j + 1]};
  }
  if (frag == 0) *p.counter += counted;
}

}  // namespace

// the argument checks of dia_act_stats; dia_engine_set_calib runs them on every tap's arguments before any step exists
int dia_act_stats_validate(const dia_act_stats_args* a, const char* who) {
  char msg[200];
  const char* why = nullptr;
  if (!a) why = "null argument";
  else if (!a->x) why = "null plane";
  else if (!a->acc) why = "null acc";
  else if (!a->counter) why = "null counter";
  else if (a->ktiles <= 0) why = "ktiles <= 0";
  else if (a->ktiles_used < 0 || a->ktiles_used > a->ktiles) why = "ktiles_used outside [0, ktiles]";
  else if (a->rows_pad <= 0 || a->rows_pad % 16 != 0) why = "rows_pad must be a positive multiple of 16";
  else if (a->M <= 0 || a->M > a->rows_pad) why = "M <= 0 or beyond the plane's rows (rows_pad)";
  else if (!a->act_f32 && a->plane_stride < (int64_t)a->rows_pad * a->ktiles * 32) why = "plane_stride smaller than one bf16 plane";
  else if (a->ssq_in && a->ssq_in_n <= 0) why = "ssq_in without ssq_in_n > 0";
  else if (a->ssq_in && a->ssq_ld < a->M) why = "ssq_ld smaller than M";
  else if (a->rows_per_slot != 0 && a->rows_per_slot != 2) why = "rows_per_slot must be 0 (no gate) or 2 (the decode step's row pairs)";
  else if (a->rows_per_slot != 0 && !a->cur) why = "the gate (rows_per_slot) without cur";
  else if (a->rows_per_slot != 0 && a->T <= 0) why = "the gate (rows_per_slot) without T > 0";
  else if ((reinterpret_cast<uintptr_t>(a->x) & 15) || (reinterpret_cast<uintptr_t>(a->acc) & 15) || (reinterpret_cast<uintptr_t>(a->counter) & 7))
    why = "x and acc must be 16-byte aligned, counter 8-byte aligned";
  if (!why) return DIA_OK;
  snprintf(msg, sizeof msg, "%s: %s", who, why);
  return dia_fail(DIA_E_ARG, msg);
}

extern "C" int dia_act_stats(const dia_act_stats_args* a, void* stream) {
  const int rc = dia_act_stats_validate(a, "dia_act_stats");
  if (rc) return rc;
  CalibK k;
  k.x = a->x; k.plane_stride = (long)a->plane_stride; k.ktiles = a->ktiles; k.kt_used = a->ktiles_used > 0 ? a->ktiles_used : a->ktiles;
  k.M = a->M; k.act_f32 = a->act_f32 ? 1 : 0;
  k.ssq_in = a->ssq_in; k.ssq_in_n = a->ssq_in_n; k.ssq_ld = a->ssq_ld; k.inv_d = a->inv_d; k.eps = a->eps;
  k.row_mask = a->row_mask;
  k.cur = a->cur; k.first_step = a->first_step; k.fsm = a->fsm; k.T = a->T; k.rows_per_slot = a->rows_per_slot;
  k.acc = a->acc; k.counter = reinterpret_cast<long long*>(a->counter);
  const int frags = k.kt_used * 4;
  dia_launch<k_act_stats>(dim3((frags + CHUNK - 1) / CHUNK), dim3(CHUNK), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_act_stats");
}
