// Frame streaming: final codec frames out of running slots, between two decode steps (dia_emit_frames, DESIGN.md "Frame streaming").
//
// The sampler writes token row `cur` of an utterance and never rewrites an earlier row, and the codec's frame t reads row
// first_step + t + delay[c] of channel c (the delay pattern undone, reference dia/audio.py:88-163).  So frame t is final as soon
// as row first_step + t + max_delay exists: with W = finished ? last + 1 : cur, the frames below ready = W - first_step - max_delay.
// The host states the rule in dia_hip/tokens.py (ready_frames / frames_window); this kernel computes the same per slot, gathers
// the frames that became final since its last visit into a per-slot staging area, and keeps its own count of what it handed out.
//
// One workgroup per listed slot, the slot numbers as kernel arguments (k_slot_admit's scheme).  Plain vector loads and stores;
// stream order is the only ordering: the counter is read by every lane, then a barrier, then lane 0 writes it.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <algorithm>
#include <cstdarg>
#include <cstdio>

namespace {

constexpr int MAXC = 16;               // channels (the embedding kernels' bound)

struct EmitK {
  int T, C, max_delay, codebook_size, cap, reset;
  const int* tokens; const int* cur; const int* fsm; const int* first_step; const int* delay;
  int* emitted; int* out; int* state;
  int slot[DIA_SLOTS_PER_CALL];
};

__global__ __launch_bounds__(256) void k_emit_frames(EmitK p) {
  const int b = p.slot[blockIdx.x];
  const int tid = threadIdx.x;
  int* st = p.state + b * 4;
  if (p.reset) {
    if (tid == 0) {
      p.emitted[b] = 0;
      st[0] = 0; st[1] = 0; st[2] = -1; st[3] = 0;
    }
    return;
  }
  // workgroup-uniform state of the slot
  const int cur = p.cur[b];
  const int finished = p.fsm[b * 8 + 3] != 0;
  const int last = p.fsm[b * 8 + 4];
  const int fs = p.first_step ? p.first_step[b] : 1;
  const int em = p.emitted[b];
  const int W = finished ? last + 1 : cur;                       // rows [fs, W) are written for good
  const int ready = max(0, W - fs - p.max_delay);
  const int n = min(max(ready - em, 0), p.cap);
  const int* tok = p.tokens + (long)b * p.T * p.C;
  int* out = p.out + (long)b * p.cap * p.C;
  const int base = fs + em;
  for (int j = tid; j < n * p.C; j += 256) {                     // j = t * C + c: consecutive lanes, consecutive words of out
    const int t = j / p.C, c = j - t * p.C;
    // <= W - 1 <= T - 1 by the rule; the clamp keeps a corrupted state (counter, delay table) inside the slot's rows
    const int row = min(max(base + t + p.delay[c], 0), p.T - 1);
    const int v = tok[(long)row * p.C + c];
    out[j] = (v < 0 || v > p.codebook_size - 1) ? 0 : v;
  }
  __syncthreads();                                               // every lane has read emitted[b]
  if (tid == 0) {
    p.emitted[b] = em + n;
    st[0] = em; st[1] = n; st[2] = finished ? ready : -1; st[3] = finished;
  }
}

}  // namespace

static int emit_fail(const char* fmt, ...) {
  char buf[192];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return dia_fail(DIA_E_ARG, buf);
}

extern "C" int dia_emit_frames(const dia_emit_args* a, void* stream) {
  if (!a || !a->slot || !a->emitted || !a->state) return emit_fail("dia_emit_frames: null argument");
  const bool reset = (a->flags & DIA_EMIT_RESET) != 0;
  if (!reset && (!a->tokens || !a->cur || !a->fsm || !a->delay || !a->out)) return emit_fail("dia_emit_frames: null argument");
  if (a->flags & ~DIA_EMIT_RESET) return emit_fail("dia_emit_frames: unknown flags %d", a->flags);
  if (a->B <= 0 || a->n < 1 || a->n > DIA_SLOTS_PER_CALL)
    return emit_fail("dia_emit_frames: n must be in [1, %d] and B positive", DIA_SLOTS_PER_CALL);
  if (a->C < 1 || a->C > MAXC) return emit_fail("dia_emit_frames: C = %d outside [1, %d]", a->C, MAXC);
  if (a->cap < 1) return emit_fail("dia_emit_frames: cap = %d, at least one frame per slot and call", a->cap);
  if (a->T < 1 || a->max_delay < 0 || a->max_delay >= a->T)
    return emit_fail("dia_emit_frames: max_delay = %d outside [0, T = %d)", a->max_delay, a->T);
  if ((long)a->cap * a->C > (1L << 30)) return emit_fail("dia_emit_frames: cap * C too large");
  EmitK k = {};
  k.T = a->T; k.C = a->C; k.max_delay = a->max_delay; k.codebook_size = a->codebook_size; k.cap = a->cap; k.reset = reset ? 1 : 0;
  k.tokens = a->tokens; k.cur = a->cur; k.fsm = a->fsm; k.first_step = a->first_step; k.delay = a->delay;
  k.emitted = a->emitted; k.out = a->out; k.state = a->state;
  for (int i = 0; i < a->n; ++i) {
    k.slot[i] = a->slot[i];
    if (k.slot[i] < 0 || k.slot[i] >= a->B) return emit_fail("dia_emit_frames: slot %d outside [0, B = %d)", k.slot[i], a->B);
    for (int j = 0; j < i; ++j)
      if (k.slot[j] == k.slot[i]) return emit_fail("dia_emit_frames: slot %d listed twice", k.slot[i]);
  }
  dia_launch<k_emit_frames>(dim3(a->n), dim3(256), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_emit_frames");
}
