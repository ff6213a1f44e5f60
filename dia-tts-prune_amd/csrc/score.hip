// Teacher-forced scoring: what the model says about tokens that are already known (dia_score, DESIGN.md "Scoring").
//
// A teacher-forced step at row t = cur[b] has produced the logits that predict token row t, and that row already holds the forced
// token.  Per channel this kernel reduces the two logit rows of the utterance to three numbers:
//   lp_cond  log-softmax of the conditional row at the target           (no guidance, no constraints)
//   lp_cfg   log-softmax of the guided, constrained row at the target   (what k_sample draws from at temperature 1, no top-k / top-p)
//   H_cfg    entropy of that guided distribution, in nats
// The reference has no counterpart: it only ever samples (dia/model.py:447-488).
//
// k_sample's decomposition: one workgroup per utterance, one wave per channel, every lane 17 of the <= 1088 logits in registers.
// Wave reductions only, no LDS, no atomics; lane 0 of each wave stores the three results.  Reads cur[] and writes no state, so it
// sits between the logits GEMM and the sampler, which advances cur.
//
// fp contraction is OFF in this file as in sample.hip: the guided logit is the sampler's expression, rounding by rounding.
#pragma clang fp contract(off)
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdio>

namespace {

constexpr int NV = 17;                 // 64 * 17 = 1088 logits per wave, as the sampler
constexpr int VCAP = NV * 64;
constexpr int MAXC_SCORE = 12;         // the sampler's channel bound

struct ScoreK {
  const float* logits; int ld_logits; int B, T, C, V;
  float cfg_scale; const float* cfg_scales;
  int eos, pad, bos;
  const int* tokens; const int* cur; const int* first_step; const int* fsm;
  float* out;
};

__global__ __launch_bounds__(MAXC_SCORE * 64) void k_score(ScoreK p) {
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
  const int b = blockIdx.x;
  // the logits depend on no device-side state: requested first, on clamped indices (k_sample's scheme)
  const float* un = p.logits + (long)(2 * b) * p.ld_logits + c * p.V;
  const float* co = p.logits + (long)(2 * b + 1) * p.ld_logits + c * p.V;
  float cv[NV], uv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = min(lane + 64 * i, p.V - 1);
    cv[i] = co[v]; uv[i] = un[v];
  }
  const int t = p.cur[b];
  const int first = p.first_step ? p.first_step[b] : 1;
  const bool done = p.fsm ? p.fsm[b * 8 + 3] != 0 : false;
  const float s = p.cfg_scales ? p.cfg_scales[b] : p.cfg_scale;
  // audio-prompt replay rows, a finished utterance, a row outside the buffer: nothing is written (uniform over the workgroup)
  if (t < first || t < 0 || t >= p.T || done) return;
  const long pos = ((long)b * p.T + t) * p.C + c;
  const int tok = p.tokens[pos];

  float g[NV];
  float mc = -INFINITY, mg = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = lane + 64 * i;
    const float d = cv[i] - uv[i];
    float x = cv[i] + s * d;                                                              // model.py:457, as k_sample forms it
    if (v >= p.V || v == p.pad || v == p.bos || (c > 0 && v == p.eos)) x = -INFINITY;     // model.py:462-472
    if (v >= p.V) cv[i] = -INFINITY;
    g[i] = x;
    mc = fmaxf(mc, cv[i]); mg = fmaxf(mg, x);
  }
  mc = wave_max(mc); mg = wave_max(mg);
  // z = sum exp(l - m); a = sum exp(l - m) * (l - m) over the terms with p > 0: H = log z - a / z
  float zc = 0.f, zg = 0.f, ag = 0.f;
  float lc_t = 0.f, lg_t = 0.f;        // the target's logits, in the lane that holds them
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float dc = cv[i] - mc, dg = g[i] - mg;
    zc += expf(dc);
    const float eg = expf(dg);
    zg += eg;
    if (eg > 0.f) ag += eg * dg;
    if (lane + 64 * i == tok) { lc_t = dc; lg_t = dg; }
  }
  zc = wave_sum(zc); zg = wave_sum(zg); ag = wave_sum(ag);
  lc_t = __shfl(lc_t, tok & 63, 64); lg_t = __shfl(lg_t, tok & 63, 64);
  if (lane == 0) {
    const float lzg = logf(zg);
    float r0 = lc_t - logf(zc), r1 = lg_t - lzg, r2 = lzg - ag / zg;
    if (tok < 0 || tok >= p.V) r0 = r1 = r2 = __builtin_nanf("");
    float* o = p.out + pos * 3;
    o[0] = r0; o[1] = r1; o[2] = r2;
  }
}

}  // namespace

// the argument checks of dia_score; dia_engine_set_score runs them on the arguments it is handed, before any step exists
int dia_score_validate(const dia_score_args* a, const char* who) {
  char msg[160];
  const char* why = nullptr;
  if (!a || !a->logits || !a->tokens || !a->cur || !a->out) why = "null argument";
  else if (a->C > MAXC_SCORE || a->C <= 0) why = "channels outside [1, 12] (one wave per channel, the sampler's bound)";
  else if (a->V > VCAP || a->V <= 0) why = "vocabulary outside [1, 1088] (17 logits per lane)";
  else if (a->B <= 0 || a->T <= 0) why = "empty shape";
  else if ((long)a->ld_logits < (long)a->C * a->V) why = "ld_logits is narrower than C * V";
  if (!why) return DIA_OK;
  snprintf(msg, sizeof msg, "%s: %s", who, why);
  return dia_fail(DIA_E_ARG, msg);
}

extern "C" int dia_score(const dia_score_args* a, void* stream) {
  const int rc = dia_score_validate(a, "dia_score");
  if (rc) return rc;
  ScoreK k;
  k.logits = a->logits; k.ld_logits = a->ld_logits; k.B = a->B; k.T = a->T; k.C = a->C; k.V = a->V;
  k.cfg_scale = a->cfg_scale; k.cfg_scales = a->cfg_scales; k.eos = a->eos; k.pad = a->pad; k.bos = a->bos;
  k.tokens = a->tokens; k.cur = a->cur; k.first_step = a->first_step; k.fsm = a->fsm; k.out = a->out;
  dia_launch<k_score>(dim3(a->B), dim3(a->C * 64), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_score");
}
