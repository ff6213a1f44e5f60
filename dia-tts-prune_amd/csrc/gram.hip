// Gram matrices of the GEMM inputs for error-compensated quantisation (dia_act_gram, DESIGN.md "Gram matrices and GPTQ").
//
// GPTQ (Frantar et al. 2022) pushes every element's rounding error into the weights it has not rounded yet and needs, per
// matrix, the Hessian of the layer's output error, H = X^T X / rows: the full Gram matrix of the GEMM's input rows.  This
// kernel is dia_act_stats (calib.hip) with an outer product in place of the square: it reads the same plane set, forms the
// same gate and the same row scale, and adds
//   G[i][j] += sum over counted rows m, in ascending m, of (double)v[m][i] * (double)v[m][j],   v = fl32(x[m][k] * scale[m])
// into a packed lower triangle of 32 x 32 tiles.  The reference has no counterpart: offline_quantize.py rounds to nearest.
//
// One workgroup owns one tile (ti, tj), tj <= ti; one thread owns 4 consecutive doubles of one tile row and walks the rows
// in order: no atomics, no cross-thread sums, so G has the same bits however the rows are spread over launches that keep their
// order, and under graph replay as eager.  The product of two widened floats is exact in double, so an element takes one
// rounding per counted row, and fma gives the bits of multiply-then-add: the diagonal is dia_act_stats's acc bit for bit.
// The VALU fma is used on purpose: the f64 MFMA adds four products per step in an order nobody has pinned.
//
// Rows are taken in chunks of 64: thread i < 64 forms the gate and the scale of row 64 * chunk + i once (as k_act_stats), then
// the workgroup stages the chunk's counted rows of the two 32-channel column blocks, scaled, in LDS (16 KiB).  Every launch
// reads and writes all of G — at the decode step's 2..16 rows that traffic is the whole cost — so the tile is loaded only
// once a chunk holds a counted row: a workgroup that finds none (prompt replay, a finished batch) returns without touching G.
// A thread's 32 bytes and its 7 neighbours' make one 256-byte tile row; a workgroup streams 8 KiB in and 8 KiB out.
//
// fp contraction is OFF in this file: v is the product rounded to fp32, and the scale is the expression of the header,
// rounding by rounding.
#pragma clang fp contract(off)
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdio>

int dia_act_stats_validate(const dia_act_stats_args* a, const char* who);

namespace {

constexpr int CHUNK = 64;             // rows per staging round
constexpr int NT = 256;               // threads per workgroup: 32 tile rows x 8 threads of 4 doubles

struct GramK {
  const void* x; long plane_stride; int ktiles, kt_used, M, act_f32;
  const float* ssq_in; int ssq_in_n, ssq_ld; float inv_d, eps;
  const uint8_t* row_mask;
  const int* cur; const int* first_step; const int* fsm; int T, rows_per_slot;
  double* gram; long long* counter;
};

// 8 consecutive channels of row m from k0, times the row's scale, each product rounded to fp32
__device__ __forceinline__ void stage8(const GramK& p, int m, int k0, float s, float* dst) {
  const long off = plane_frag_off(m, k0, p.ktiles);
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
  for (int j = 0; j < 8; ++j) dst[j] = v[j] * s;
}

__global__ __launch_bounds__(NT) void k_act_gram(GramK p) {
  __shared__ float vi[CHUNK][32];      // the chunk's scaled rows, channels of tile row ti ...
  __shared__ float vj[CHUNK][32];      // ... and of tile column tj
  __shared__ float sc[CHUNK];
  __shared__ int cnt[CHUNK];
  const int tid = threadIdx.x;
  // block -> (ti, tj) of the packed lower triangle: block = ti (ti + 1) / 2 + tj
  const int blk = blockIdx.x;
  int ti = (int)((sqrtf(8.0f * (float)blk + 1.0f) - 1.0f) * 0.5f);
  while (ti * (ti + 1) / 2 > blk) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= blk) ++ti;
  const int tj = blk - ti * (ti + 1) / 2;
  const int i = tid >> 3, j0 = (tid & 7) * 4;           // this thread's patch: G[32 ti + i][32 tj + j0 .. + 3]
  double* gp = p.gram + ((long)blk * 1024 + i * 32 + j0);
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  bool loaded = false;
  long long counted = 0;
  for (int m0 = 0; m0 < p.M; m0 += CHUNK) {
    float s = 1.0f;
    bool on = false;
    const int m = m0 + tid;
    if (tid < CHUNK && m < p.M) {
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
        for (int n = 0; n < p.ssq_in_n; ++n) q += p.ssq_in[(long)n * p.ssq_ld + m];
        s = 1.0f / sqrtf(q * p.inv_d + p.eps);
      }
    }
    __syncthreads();                   // the previous chunk has been read
    if (tid < CHUNK) { sc[tid] = s; cnt[tid] = on ? 1 : 0; }
    const int any = __syncthreads_or(on ? 1 : 0);
    if (!any) continue;                // (uniform over the workgroup)
    if (!loaded) {
      const double2 t0 = *reinterpret_cast<const double2*>(gp), t1 = *reinterpret_cast<const double2*>(gp + 2);
      a0 = t0.x; a1 = t0.y; a2 = t1.x; a3 = t1.y;
      loaded = true;
    }
    const int n = min(CHUNK, p.M - m0);
    {                                  // stage: thread -> (row r, fragment q of 8 channels) of both column blocks
      const int r = tid & (CHUNK - 1), q = tid >> 6;
      if (r < n && cnt[r]) {
        const float s_r = sc[r];
        stage8(p, m0 + r, ti * 32 + q * 8, s_r, &vi[r][q * 8]);
        stage8(p, m0 + r, tj * 32 + q * 8, s_r, &vj[r][q * 8]);
      }
    }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
      if (!cnt[r]) continue;           // (uniform over the workgroup)
      ++counted;
      const double u = (double)vi[r][i];
      const float4 w = *reinterpret_cast<const float4*>(&vj[r][j0]);
      a0 = fma(u, (double)w.x, a0);
      a1 = fma(u, (double)w.y, a1);
      a2 = fma(u, (double)w.z, a2);
      a3 = fma(u, (double)w.w, a3);
    }
  }
  if (loaded) {
    *reinterpret_cast<double2*>(gp) = double2{a0, a1};
    *reinterpret_cast<double2*>(gp + 2) = double2{a2, a3};
  }
  if (blk == 0 && tid == 0) *p.counter += counted;
}

}  // namespace

// the argument checks of dia_act_gram: everything dia_act_stats refuses, and the matrix; dia_engine_set_gram runs them on every tap
int dia_act_gram_validate(const dia_act_gram_args* a, const char* who) {
  char msg[200];
  const char* why = nullptr;
  if (!a) why = "null argument";
  else if (!a->gram) why = "null gram";
  else if (reinterpret_cast<uintptr_t>(a->gram) & 15) why = "gram must be 16-byte aligned";
  else if (a->ktiles_used > 2048 || (a->ktiles_used == 0 && a->ktiles > 2048)) why = "more than 2048 k-tiles";
  if (why) {
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return dia_fail(DIA_E_ARG, msg);
  }
  dia_act_stats_args s = {};
  s.x = a->x; s.plane_stride = a->plane_stride; s.ktiles = a->ktiles; s.ktiles_used = a->ktiles_used; s.M = a->M; s.rows_pad = a->rows_pad;
  s.act_f32 = a->act_f32; s.ssq_in_n = a->ssq_in_n; s.ssq_in = a->ssq_in; s.ssq_ld = a->ssq_ld; s.inv_d = a->inv_d; s.eps = a->eps;
  s.rows_per_slot = a->rows_per_slot; s.row_mask = a->row_mask; s.cur = a->cur; s.first_step = a->first_step; s.fsm = a->fsm; s.T = a->T;
  s.acc = a->gram; s.counter = a->counter;
  return dia_act_stats_validate(&s, who);
}

extern "C" int dia_act_gram(const dia_act_gram_args* a, void* stream) {
  const int rc = dia_act_gram_validate(a, "dia_act_gram");
  if (rc) return rc;
  GramK k;
  k.x = a->x; k.plane_stride = (long)a->plane_stride; k.ktiles = a->ktiles; k.kt_used = a->ktiles_used > 0 ? a->ktiles_used : a->ktiles;
  k.M = a->M; k.act_f32 = a->act_f32 ? 1 : 0;
  k.ssq_in = a->ssq_in; k.ssq_in_n = a->ssq_in_n; k.ssq_ld = a->ssq_ld; k.inv_d = a->inv_d; k.eps = a->eps;
  k.row_mask = a->row_mask;
  k.cur = a->cur; k.first_step = a->first_step; k.fsm = a->fsm; k.T = a->T; k.rows_per_slot = a->rows_per_slot;
  k.gram = a->gram; k.counter = reinterpret_cast<long long*>(a->counter);
  const long tiles = (long)k.kt_used * (k.kt_used + 1) / 2;
  dia_launch<k_act_gram>(dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_act_gram");
}
