// Decode-step sequencer: chains the kernels of one autoregressive step (reference
// Decoder.decode_step, dia/layers.py:671-720, driven by the loop at dia/model.py:748-807) on one HIP
// stream and replays it as a hipGraph.  The engine allocates nothing: every buffer comes from the
// caller (PyTorch-ROCm tensors used as storage).  All per-step variables (current step, KV length,
// EOS state) live in device memory, so the captured graph is static and the host never syncs
// inside the loop.
#include "common.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include "tuning.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <algorithm>
#include <utility>

struct dia_engine {
  dia_engine_desc d;
  std::vector<dia_dec_layer> layers;
  hipStream_t stream = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int launches = 0;
  bool seg = false;               // the step runs persistent MLP segments (dia_seg_mlp)
  std::vector<const void*> seg_w;
  int mlp_fused = -1;             // -1 not tried yet, 1 the MLP runs as one fused launch, 0 two launches
  int wo_defer = -1;              // -1 not tried yet, 1 wo's split-K slices are merged by the launch behind it, 0 inside wo (dia_gemm_wo_deferred refused)
  float* x_alt = nullptr;         // dia_engine_set_x_alt: the residual stream of odd layers while wo_defer is in force
  std::vector<dia_mxfp4_layer> f4;      // dia_engine_set_mxfp4: the MXFP4 streams per layer (empty: none) ...
  const void* f4_logits = nullptr;      // ... and of the logits head
  std::vector<dia_us_layer> us;         // dia_engine_set_usparse: the unstructured sparse streams per layer (empty: none) ...
  dia_us_mat us_logits = {};            // ... and of the logits head
  bool score_on = false;                // dia_engine_set_score: every step scores the forced row between the logits GEMM and the sampler
  dia_score_args score = {};
  bool calib_on = false;                // dia_engine_set_calib: every step accumulates the activation statistics of each GEMM input in front of the GEMM
  std::vector<double*> calib_acc;       // ... per tap (6 * l + m, the logits head last): the accumulator,
  std::vector<int32_t> calib_kt;        // ... its k-tiles
  int64_t* calib_counters = nullptr;    // ... and the device row counters
  bool gram_on = false;                 // dia_engine_set_gram: the same taps with dia_act_gram, at the taps that have a matrix
  std::vector<double*> gram_ptr;        // ... per tap: the packed Gram matrix or nullptr (no launch),
  std::vector<int32_t> gram_kt;         // ... its k-tiles
  int64_t* gram_counters = nullptr;     // ... and the device row counters
  std::vector<dia_lora_layer> lora;     // dia_engine_set_lora: the adapter tables of the two decode sites per layer (empty: no LoRA launches)
  const int32_t* lora_slot = nullptr;   // ... and the device array adapter_of_slot [B]
  int lora_adapters = 0;
  std::vector<dia_kv_fp8_ptrs> f8kv;    // dia_engine_set_cross_fp8: the e4m3 copy of every layer's cross caches (empty: the bf16 caches)
  std::vector<dia_kv_fp8_ptrs> f8self;  // dia_engine_set_self_fp8: the e4m3 self caches of every layer (empty: the bf16 caches k_self / v_self)
  std::vector<hipEvent_t> prof;   // when non-empty: one event recorded after every launch (profile step)
  // weight prefetch beside the chain (graph mode): launch i+lookahead's weights are pulled into the
  // Infinity Cache by a side stream as soon as launch i has been issued
  int pf_lookahead = 0;
  bool pf_capturing = false;
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> pf_ev;
  std::vector<std::pair<const void*, long>> pf_w;   // per launch: weight pointer and bytes (null for attention)
};

int dia_prefetch_launch(const void* ptr, long nbytes, int nblocks, hipStream_t st);
int dia_score_validate(const dia_score_args* a, const char* who);
int dia_lora_validate(const dia_lora_args* a, const char* who);
int dia_act_stats_validate(const dia_act_stats_args* a, const char* who);
int dia_act_gram_validate(const dia_act_gram_args* a, const char* who);
static int ensure_sink();
static int dia_lora_noop(void* st);

static inline void mark(dia_engine* e, int i) {
  if (!e->prof.empty() && i + 1 < (int)e->prof.size()) (void)hipEventRecord(e->prof[i + 1], e->stream);
  if (e->pf_capturing) {
    const int j = i + e->pf_lookahead;
    if (j < (int)e->pf_w.size() && e->pf_w[j].first != nullptr) {
      (void)hipEventRecord(e->pf_ev[i], e->stream);
      (void)hipStreamWaitEvent(e->side, e->pf_ev[i], 0);
      const long bytes = e->pf_w[j].second;
      const int nb = (int)std::min<long>(512, std::max<long>(32, bytes / (256 * 16 * 8)));
      (void)dia_prefetch_launch(e->pf_w[j].first, bytes, nb, e->side);
    }
  }
}

// MXFP8 default policy (DESIGN.md "MXFP8 weight stream"): a launch class streams MXFP8 at a row range only where its in-step time
// was below the dense launch's in every repetition of the A/B (profiles/r05_mxfp8_speed.txt): wi, wo and the logits head at
// <= 4 rows, wi and the logits head at 5..16 rows.  The 128..192-strip projections are bound by their fixed cost and lost
// (+1..6 %), wo at 5..16 rows lost to the dense strip-pair split-K form (+1..4 %)
constexpr int MXFP8_DEFAULT = (1 << DIA_MAT_WI | 1 << DIA_MAT_WO | 1 << DIA_MAT_LOGITS) | (1 << DIA_MAT_WI | 1 << DIA_MAT_LOGITS) << 8;
static_assert(MXFP8_DEFAULT == 0x5070 && DIA_MAT_COUNT <= 8, "the knob mxfp8 holds one byte of class bits per row range");
extern "C" int dia_mxfp8_classes(int rows) {
  if (rows <= 0 || rows > 16) return 0;
  const int knob = dia_tune(DIA_TUNE_MXFP8);
  const int mask = knob >= 0 ? knob : MXFP8_DEFAULT;
  return (rows <= 4 ? mask : mask >> 8) & ((1 << DIA_MAT_COUNT) - 1);
}

// MXFP4: not measured yet — the classes MXFP8 streams by default, until profiles/ holds an A/B of its own (DESIGN.md "MXFP4 weight stream")
constexpr int MXFP4_DEFAULT = (1 << DIA_MAT_WI | 1 << DIA_MAT_WO | 1 << DIA_MAT_LOGITS) | (1 << DIA_MAT_WI | 1 << DIA_MAT_LOGITS) << 8;
static_assert(MXFP4_DEFAULT == 0x5070, "the knob mxfp4 holds one byte of class bits per row range");
extern "C" int dia_mxfp4_classes(int rows) {
  if (rows <= 0 || rows > 16) return 0;
  const int knob = dia_tune(DIA_TUNE_MXFP4);
  const int mask = knob >= 0 ? knob : MXFP4_DEFAULT;
  return (rows <= 4 ? mask : mask >> 8) & ((1 << DIA_MAT_COUNT) - 1);
}

// Unstructured sparse streams: opt-in by the knob usparse.  No class won a repetition of the in-step A/B (profiles/r21_usparse_speed.txt,
// scratch/usparse_speed.py: 3-23 % fewer frames/s per class), so none streams by default (DESIGN.md "Unstructured sparse weight stream"); <= 4 rows only (the kernel's range)
constexpr int USPARSE_DEFAULT = 0;
extern "C" int dia_usparse_classes(int rows) {
  if (rows <= 0 || rows > 4) return 0;
  const int knob = dia_tune(DIA_TUNE_USPARSE);
  return (knob >= 0 ? knob : USPARSE_DEFAULT) & ((1 << DIA_MAT_COUNT) - 1);
}

// The step's GEMM launches, one row per dia_step_mat (the row index is also the MXFP8 class bit): where the matrix and its streams live in
// dia_dec_layer (the logits head: dia_engine_desc, see mat_weights), its epilogue, the planes it reads and emits, what it writes
enum { PL_NONE = -1, PL_X, PL_A, PL_H };                // activation planes: the normed residual stream, attention output, MLP hidden
enum { OUT_NONE, OUT_QKV, OUT_QC, OUT_LOGITS, OUT_X };  // SCALE_STORE: an fp32 buffer; RESID_EMIT: the residual stream
struct step_mat_row {
  int mat;
  const void* dia_dec_layer::*w; int32_t dia_dec_layer::*kt; int32_t dia_dec_layer::*ns;      // dense tiles, kt * ns * 1024 bytes
  const void* dia_dec_layer::*w24; const void* dia_dec_layer::*wf8;                            // 2:4 and MXFP8 streams
  const void* dia_mxfp4_layer::*wf4;                                                           // MXFP4 stream (dia_engine_set_mxfp4)
  dia_us_mat dia_us_layer::*wus;                                                               // unstructured sparse stream (dia_engine_set_usparse)
  int epi, in, out, emit;
  const int32_t* dia_dec_layer::*cmap;                  // RESID_EMIT: the consumer's compaction map and norm weight (null: the next
  const float* dia_dec_layer::*gnext;                   // layer's g_sa, or the final norm)
};
#define MAT(M, m) DIA_MAT_##M, &dia_dec_layer::w_##m, &dia_dec_layer::kt_##m, &dia_dec_layer::ns_##m, &dia_dec_layer::w_##m##_24, &dia_dec_layer::w_##m##_f8, &dia_mxfp4_layer::w_##m, &dia_us_layer::w_##m
constexpr step_mat_row STEP_MATS[DIA_MAT_COUNT] = {
  {MAT(QKV, qkv), DIA_EPI_SCALE_STORE, PL_X, OUT_QKV, PL_NONE, nullptr, nullptr},      // q/k/v projection of the pre-SA-normed row (layers.py:541, 273-275)
  {MAT(O, o), DIA_EPI_RESID_EMIT, PL_A, OUT_X, PL_X, &dia_dec_layer::cmap_ca, &dia_dec_layer::g_ca},       // o_proj + residual; emits the pre-CA-normed planes (layers.py:341-343, 555, 560)
  {MAT(CQ, cq), DIA_EPI_SCALE_STORE, PL_X, OUT_QC, PL_NONE, nullptr, nullptr},         // cross-attention query (layers.py:273, 278)
  {MAT(CO, co), DIA_EPI_RESID_EMIT, PL_A, OUT_X, PL_X, &dia_dec_layer::cmap_mlp, &dia_dec_layer::g_mlp},   // cross o_proj + residual; emits the pre-MLP-normed planes
  {MAT(WI, wi), DIA_EPI_SWIGLU_EMIT, PL_X, OUT_NONE, PL_H, nullptr, nullptr},          // SwiGLU MLP (layers.py:95-104)
  {MAT(WO, wo), DIA_EPI_RESID_EMIT, PL_H, OUT_X, PL_X, &dia_dec_layer::cmap_next, nullptr},
  {DIA_MAT_LOGITS, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, DIA_EPI_SCALE_STORE, PL_X, OUT_LOGITS, PL_NONE, nullptr, nullptr},   // final norm + logits (layers.py:714-717)
};
#undef MAT
constexpr bool rows_in_order(int m = 0) { return m == DIA_MAT_COUNT || (STEP_MATS[m].mat == m && rows_in_order(m + 1)); }
static_assert(rows_in_order(), "row m of STEP_MATS describes matrix m of dia_step_mat");

struct mat_w { const void* w; int kt, ns; const void *w24, *wf8, *wf4; const dia_us_mat* wus; };
static mat_w mat_weights(const dia_engine* e, int l, int m) {
  const dia_engine_desc& d = e->d;
  if (m == DIA_MAT_LOGITS) return {d.w_logits, d.kt_logits, d.ns_logits, d.w_logits_24, d.w_logits_f8, e->f4_logits, e->us_logits.stream ? &e->us_logits : nullptr};
  const dia_dec_layer& L = e->layers[l];
  const step_mat_row& r = STEP_MATS[m];
  return {L.*r.w, L.*r.kt, L.*r.ns, L.*r.w24, L.*r.wf8, e->f4.empty() ? nullptr : e->f4[l].*r.wf4,
          (e->us.empty() || !(e->us[l].*r.wus).stream) ? nullptr : &(e->us[l].*r.wus)};
}

// The launches of one step, in order: launch(layer, what) for every one, `what` a dia_step_mat or one of the launches below.
// enqueue_step issues them; the prefetch list and dia_engine_launches_per_step walk the same sequence.
// CALIB + m: dia_engine_set_calib's tap in front of matrix m (a dia_act_stats over the planes m is about to read)
// GRAM + m: dia_engine_set_gram's tap in the same place (a dia_act_gram), issued only where the tap has a matrix
enum { ATTN_SELF = DIA_MAT_COUNT, ATTN_CROSS, SEG_MLP, SAMPLER, SCORE, LORA_QKV, LORA_CQ, CALIB, GRAM = CALIB + DIA_MAT_COUNT };
static inline int tap_index(const dia_engine* e, int l, int m) { return l < e->d.n_layer ? 6 * l + m : 6 * e->d.n_layer; }
template <class Launch>
static int step_sequence(const dia_engine* e, bool with_sampler, Launch&& launch) {
  int rc = DIA_OK;                   // the first failure ends the sequence
  auto run = [&](int l, std::initializer_list<int> seq) {
    for (int what : seq) {
      if (!rc && e->calib_on && what < DIA_MAT_COUNT) rc = launch(l, CALIB + what);
      if (!rc && e->gram_on && what < DIA_MAT_COUNT && e->gram_ptr[tap_index(e, l, what)]) rc = launch(l, GRAM + what);
      if (!rc) rc = launch(l, what);
    }
  };
  for (int l = 0; l < e->d.n_layer; ++l) {
    if (!e->seg || l == 0) run(l, {DIA_MAT_QKV});
    if (e->lora.empty()) run(l, {ATTN_SELF, DIA_MAT_O, DIA_MAT_CQ, ATTN_CROSS});
    else run(l, {LORA_QKV, ATTN_SELF, DIA_MAT_O, DIA_MAT_CQ, LORA_CQ, ATTN_CROSS});     // dia_engine_set_lora: the adapters' corrections of qkv / qc
    if (e->seg) run(l, {SEG_MLP});     // persistent MLP segment: co, wi, wo and the next layer's qkv in one launch
    else run(l, {DIA_MAT_CO, DIA_MAT_WI, DIA_MAT_WO});
  }
  run(e->d.n_layer, {DIA_MAT_LOGITS});
  if (with_sampler && e->score_on) run(e->d.n_layer, {SCORE});      // reads cur[] before the sampler advances it
  if (with_sampler) run(e->d.n_layer, {SAMPLER});
  return rc;
}

// wo's cross-workgroup split-K: sets g.sk / spw / nw and the scratch that goes with them; returns wo_pair (17..128 rows split K per m-tile)
static bool wo_split_k(const dia_engine_desc& d, const dia_dec_layer& L, int R, dia_gemm_args& g) {
  // K = 8192 over only D/16 = 128 strips: cross-workgroup split-K (fence-free slab hand-off) streams the
  // matrix from more CUs.  M <= 4: two workgroups per strip, 12.4 -> 11.2 us per launch.  5..16 rows: four
  // per strip, which also brings the per-wave K range down to what k_gemm16 keeps in registers (23.2 ->
  // 18.4 us in the step at batch 8).  Shapes without a split kernel fall back to one workgroup per strip.
  int wo_sk = (R <= 4 && L.kt_wo % 2 == 0) ? 2 : ((R <= 16 && L.kt_wo % 4 == 0) ? 4 : 1);
  int wo_spw = 0;
  if (R > 4 && R <= 16) {
    // 5..16 rows: K ranges of 64 k-tiles (8 waves x 8 k-tiles keep their A fragments in registers: 160 VGPRs, one
    // workgroup per CU) and as many strips per workgroup as it takes to stay at one round of <= 256 workgroups —
    // dense wo (K 8192 x 128 strips): 4 ranges x 64 strip PAIRS, both tiles of a pair handed over together
    // (14.3 -> 11.7 us); the 50 %-pruned wo (K 4096): 2 ranges x 128 strips
    if (L.kt_wo % 64 == 0 && L.kt_wo / 64 >= 2 && L.kt_wo / 64 <= 8) wo_sk = L.kt_wo / 64;
    if (wo_sk > 1 && L.ns_wo * wo_sk >= 512 && L.ns_wo % 2 == 0) wo_spw = 2;
  }
  // two-plane weights (kt_wo counts hi and lo tiles): the tuned forms take 128 weight k-tiles per workgroup, so K splits into
  // kt_wo / 128 ranges at every row count (dense wo: 4); other hidden widths run unsplit on the generic kernel
  const int w2_sk = (d.w_planes == 2 && L.kt_wo % 128 == 0 && L.kt_wo / 128 <= 8) ? L.kt_wo / 128 : 1;
  if (d.w_planes == 2) { wo_sk = w2_sk; wo_spw = 0; }
  if (dia_tune(DIA_TUNE_WO_SK) >= 1 && dia_tune(DIA_TUNE_WO_SK) <= 8 && L.kt_wo % dia_tune(DIA_TUNE_WO_SK) == 0) wo_sk = dia_tune(DIA_TUNE_WO_SK);
  g.sk = wo_sk; g.sk_scratch = wo_sk > 1 ? d.sk_scratch : nullptr; g.sk_tickets = wo_sk > 1 ? d.sk_tickets : nullptr;
  bool wo_pair = false;
  if (R > 16 && R <= 128) {     // 2..8 m-tiles: split-K 4 over every m-tile (k_gemm16 with gridDim.z) when the scratch covers
    g.sk_scratch = d.sk_scratch; g.sk_tickets = d.sk_tickets;    // it, else dia_gemm splits K by itself (two m-tiles: k_gemm32)
    g.sk_scratch_floats = d.sk_scratch_floats > 0 ? d.sk_scratch_floats : (int64_t)(d.D / 16) * 4 * 512;
    wo_pair = L.kt_wo % 4 == 0 && g.sk_scratch_floats >= (int64_t)((R + 15) / 16) * L.ns_wo * 4 * 256 &&
              dia_tune(DIA_TUNE_WO_PAIR) != 0;
    g.sk = wo_pair ? 4 : 1;
    if (d.w_planes == 2) {
      wo_pair = w2_sk > 1 && g.sk_scratch_floats >= (int64_t)((R + 15) / 16) * L.ns_wo * w2_sk * 256;
      g.sk = wo_pair ? w2_sk : 1;
    }
  }
  if (dia_tune(DIA_TUNE_WO_NW) > 0) g.nw = dia_tune(DIA_TUNE_WO_NW);
  g.spw = wo_spw;
  if (dia_tune(DIA_TUNE_WO_SPW) > 0) g.spw = dia_tune(DIA_TUNE_WO_SPW);
  return wo_pair;
}

// the dia_lora_apply of one decode site: q / k / v of layer l into d.qkv (cross = false) or its cross-attention query into d.qc, from the
// residual rows `x` the projection consumed
static dia_lora_args lora_site(const dia_engine* e, int l, bool cross, const float* x) {
  const dia_engine_desc& d = e->d;
  const dia_lora_layer& A = e->lora[l];
  dia_lora_args a = {};
  a.x = x; a.ldx = d.D; a.D = d.D; a.gain = cross ? e->layers[l].g_ca : e->layers[l].g_sa; a.eps = d.eps; a.M = 2 * d.B;
  a.rows_per_slot = 2; a.n_slots = d.B; a.adapter_of_slot = e->lora_slot; a.n_adapters = e->lora_adapters;
  if (cross) {
    a.out = d.qc; a.ldo = d.cq_heads * 128;
    if (A.cq.n_cols > 0) a.seg[a.n_segs++] = A.cq;
  } else {
    a.out = d.qkv; a.ldo = (d.q_heads + 2 * d.kv_heads) * 128;
    for (const dia_lora_seg* s : {&A.q, &A.k, &A.v}) if (s->n_cols > 0) a.seg[a.n_segs++] = *s;
  }
  return a;
}

static int enqueue_step(dia_engine* e, bool with_sampler) {
  const dia_engine_desc& d = e->d;
  void* st = (void*)e->stream;
  const int R = 2 * d.B;
  const int xkt = d.D / 32;                                       // k-tiles of the x planes
  const int akt = (max(d.q_heads, d.cq_heads) * 128) / 32;        // k-tiles of the attention planes
  const int hkt = d.F / 32;
  const long mt = d.rows_pad / 16;
  const struct { void* p; long stride; int kt; } planes[] = {     // indexed by PL_*; plane strides in elements
    {d.planes_x, mt * xkt * 512, xkt}, {d.planes_a, mt * akt * 512, akt}, {d.planes_h, mt * hkt * 512, hkt}};
  const int nqkv = (d.q_heads + 2 * d.kv_heads) * 128;
  // activation format of every producer -> consumer edge (common.hpp): fp32 tiles from 5 rows on, three planes below
  const int F = d.act_f32 ? 1 : 0;
  // 17..32 rows: every GEMM may split K inside dia_gemm (k_gemm32 / k_gemm32m) when it is handed the scratch
  const bool two_tiles = R > 16 && R <= 32 && d.sk_scratch && d.sk_tickets && d.sk_scratch_floats > 0;   // (k_gemm32 / k_gemm32m / blk32 only)

  const bool seg = e->seg;            // persistent MLP segments: co, wi, wo and the next layer's qkv in one launch
  // <= 4 rows, OPT-IN (knob wo_diag=1; measured, not adopted): wo from its diagonal layout (256 workgroups with the whole K each, no
  // split-K hand-off: 9.4 -> 8.8 us); it leaves one sum of squares per 8-column half strip, so what consumes x after a wo (the
  // following q/k/v projection, the logits head) adds D / 8 partials — and their 16 extra dependent loads cost more than wo gains
  // (qkv 4.7 -> 8.7 us, logits 8.1 -> 12.8: batch 1 1 039 -> 969 frames/s, profiles/r03_wo_diag_ab.txt)
  bool diag = (R <= 2 || (R <= 4 && d.F <= 4096)) && d.act_f32 && d.w_planes <= 1 && dia_tune(DIA_TUNE_WO_DIAG) == 1 && !seg;     // (the image of 3-4 rows x 8192 does not fit LDS)
  for (int l = 0; l < d.n_layer && diag; ++l) diag = e->layers[l].w_wo_diag != nullptr && e->layers[l].cmap_next == nullptr;
  const int xn_wo = diag ? d.D / 8 : d.D / 16;
  // 2:4 sparse weight streams (dia_dec_layer.w_*_24): at <= 4 rows (batch 1-2) every matrix that has one.  From 5 rows on the dense
  // k_gemm16 forms are as fast or faster in the step (wo 10.9 vs 11.7 us at 16 rows, profiles/r04_sparse24_speed.txt): dense tiles
  auto sparse24 = [&](dia_gemm_args& g, const void* w24) {
    if (!w24 || !F || d.w_planes > 1 || R > 4) return;
    g.W = w24; g.KT /= 2; g.w_format = DIA_W_SPARSE24; g.nw = 0; g.spw = 0;
    int sk = g.sk > 1 ? g.sk : 1;                 // split-K over whole stream groups (8 sparse k-tiles per workgroup and split)
    while (sk > 1 && g.KT % (8 * sk) != 0) sk /= 2;
    g.sk = sk;
    if (sk == 1) { g.sk_scratch = nullptr; g.sk_tickets = nullptr; }
  };
  // MXFP8 / MXFP4 weight streams (dia_dec_layer.w_*_f8 / dia_engine_set_mxfp4): at <= 16 rows (batch 1-8) the launch classes of
  // dia_mxfp8_classes / dia_mxfp4_classes.  K splits over whole stream groups of 16 k-tiles with at most 128 per workgroup; the kernel
  // picks its own waves and strips per workgroup
  const bool mx_ok = F && d.w_planes <= 1 && !seg && !diag;
  const int f8_mask = mx_ok ? dia_mxfp8_classes(R) : 0, f4_mask = mx_ok ? dia_mxfp4_classes(R) : 0;
  auto mx = [&](dia_gemm_args& g, const void* ws, int format, int mask, int cls) {      // true: the launch takes this stream
    if (!ws || !(mask >> cls & 1) || g.cmap || g.strip_map || g.KT % 16 != 0) return false;
    int sk = g.sk > 1 ? g.sk : 1;
    while (sk > 1 && g.KT % (16 * sk) != 0) sk /= 2;
    while (g.KT / sk > 128 && g.KT % (32 * sk) == 0 && d.sk_scratch && d.sk_tickets && sk < 4) sk *= 2;
    if (g.KT / sk > 128) return false;            // (no split that fits: dense tiles)
    g.W = ws; g.w_format = format; g.nw = 0; g.spw = 0;
    g.sk = sk;
    if (sk == 1) { g.sk_scratch = nullptr; g.sk_tickets = nullptr; }
    else { g.sk_scratch = d.sk_scratch; g.sk_tickets = d.sk_tickets; }
    return true;
  };
  // unstructured sparse streams (dia_engine_set_usparse): at <= 4 rows the launch classes of dia_usparse_classes, K split as for the MX
  // streams.  W is the engine's own copy of the dia_us_mat, which outlives the descriptor
  const int us_mask = mx_ok ? dia_usparse_classes(R) : 0;
  auto us = [&](dia_gemm_args& g, const dia_us_mat* m, int cls) {
    if (!m || g.w_format != DIA_W_DENSE) return false;
    return mx(g, m, DIA_W_USPARSE, us_mask, cls);
  };
  bool wo_pair = false;             // of the wo descriptor built last
  // <= 4 rows: wo's two K slices merged by the launch behind it (the next layer's q/k/v projection, the logits head) while it stages
  // its row, instead of wo's ticket hand-off (dia_gemm_wo_deferred) — decided below, once every descriptor can be looked at.
  // That launch reads the whole old residual row and writes the new one: the stream alternates between x and x_alt by layer
  bool defer = false;
  const int64_t slice_floats = (int64_t)d.rows_pad * d.D;
  auto xbuf = [&](int l) { return (defer && (l & 1)) ? e->x_alt : d.x; };
  // the descriptor of matrix m of layer l (the logits head: l = n_layer) from its row of STEP_MATS
  auto step_gemm = [&](int l, int m) {
    const step_mat_row& r = STEP_MATS[m];
    const dia_dec_layer* L = l < d.n_layer ? &e->layers[l] : nullptr;
    const mat_w w = mat_weights(e, l, m);
    dia_gemm_args g = {};
    g.A = planes[r.in].p; g.a_plane_stride = planes[r.in].stride; g.a_ktiles = planes[r.in].kt; g.M = R;
    g.W = w.w; g.KT = w.kt; g.nstrips = w.ns; g.epi = r.epi; g.ssq_ld = d.rows_pad;
    if (r.in == PL_X) {             // the normed stream: scaled by the row's inverse RMS; behind a wo, x carries wo's count of partial sums
      g.ssq_in = d.ssq; g.ssq_in_n = (m == DIA_MAT_LOGITS || (m == DIA_MAT_QKV && l > 0)) ? xn_wo : d.D / 16; g.inv_d = 1.0f / d.D; g.eps = d.eps;
    }
    if (r.emit != PL_NONE) { g.P = planes[r.emit].p; g.p_plane_stride = planes[r.emit].stride; g.p_ktiles = planes[r.emit].kt; }
    switch (r.out) {
      case OUT_QKV: g.out = d.qkv; g.ldo = nqkv; g.strip_map = L->smap_qkv; break;
      case OUT_QC: g.out = d.qc; g.ldo = d.cq_heads * 128; g.strip_map = L->smap_cq; break;
      case OUT_LOGITS: g.out = d.logits; g.ldo = d.ld_logits; break;
      case OUT_X:                   // residual add; emits the planes of x * gnext in the consumer's (compacted) K order
        g.out = xbuf(l); g.ldo = d.D; g.ssq_out = d.ssq; g.cmap = L->*r.cmap;
        g.gnext = r.gnext ? L->*r.gnext : ((l + 1 < d.n_layer) ? e->layers[l + 1].g_sa : d.g_final);
        break;
    }
    g.w_planes = d.w_planes; g.act_f32 = r.epi == DIA_EPI_SCALE_STORE ? F : 3 * F;      // x read as fp32 tiles; the emitting epilogues: in and out
    if (two_tiles) { g.sk_scratch = d.sk_scratch; g.sk_tickets = d.sk_tickets; g.sk_scratch_floats = d.sk_scratch_floats; }
    if (m == DIA_MAT_WO) wo_pair = wo_split_k(d, *L, R, g);
    if (m == DIA_MAT_WO && diag) {
      g.W = L->w_wo_diag; g.w_layout = 1; g.nstrips = d.D / 8; g.sk = 1; g.sk_scratch = nullptr; g.sk_tickets = nullptr; g.nw = 0; g.spw = 0;
      return g;
    }
    sparse24(g, w.w24);
    // a matrix with both streams: the smaller one; what refuses it (class off, no K split that fits) leaves the other its turn
    if (!us(g, w.wus, m) && !mx(g, w.wf4, DIA_W_MXFP4, f4_mask, m)) mx(g, w.wf8, DIA_W_MXFP8, f8_mask, m);
    if (defer && (m == DIA_MAT_LOGITS || (m == DIA_MAT_QKV && l > 0))) g.gnext = L ? L->g_sa : d.g_final;     // the consumer norms the row itself
    return g;
  };
  // what dia_gemm_wo_deferred needs beside the descriptor; nslices == 0: this launch goes through dia_gemm
  auto step_defer = [&](int l, int m) {
    dia_wo_defer_args w = {};
    if (!defer || !(m == DIA_MAT_WO || m == DIA_MAT_LOGITS || (m == DIA_MAT_QKV && l > 0))) return w;
    w.nslices = 2; w.slices = d.sk_scratch; w.slice_stride = slice_floats;
    if (m == DIA_MAT_WO) { w.defer = 1; return w; }
    w.xold = xbuf(l - 1); w.ldx = d.D;
    w.xnew = l < d.n_layer ? xbuf(l) : nullptr;   // (nothing reads x behind the logits head: the sampler's embedding overwrites it)
    return w;
  };
  // every wo and every launch behind one in the shape the deferred kernels serve: dense one-plane tiles (no 2:4 / unstructured sparse / MXFP8 / MXFP4 stream picked),
  // K 8192 in two slices -> a row of D = 2048, no compaction map on the edge; else the whole model keeps the in-launch merge
  if (R <= 4 && F && d.w_planes <= 1 && !seg && !diag && e->wo_defer != 0 && dia_tune(DIA_TUNE_WO_DEFER) != 0 && dia_tune(DIA_TUNE_MLP_FUSE) <= 0 &&
      e->x_alt && d.sk_scratch && d.D == 2048 && (d.sk_scratch_floats > 0 ? d.sk_scratch_floats : (int64_t)(d.D / 16) * 4 * 512) >= 2 * slice_floats) {
    // (everything dia_gemm_wo_deferred checks for either role is checked here for every launch of the model: a refusal can then only
    // meet the first wo of the first step, before anything of the deferred form has been issued)
    const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    bool ok = al16(d.x) && al16(e->x_alt) && al16(d.sk_scratch) && slice_floats % 4 == 0 && slice_floats >= (int64_t)xkt * 512 && d.D % 4 == 0 &&
              dia_tune(DIA_TUNE_GEMM_SPW) <= 0;
    for (int l = 0; l < d.n_layer && ok; ++l) {
      const dia_gemm_args go = step_gemm(l, DIA_MAT_WO), gc = step_gemm(l + 1, l + 1 < d.n_layer ? DIA_MAT_QKV : DIA_MAT_LOGITS);
      const float* gcons = l + 1 < d.n_layer ? e->layers[l + 1].g_sa : d.g_final;       // the consumer's norm weight
      const int spw = gc.spw > 0 ? gc.spw : (gc.nstrips >= 1024 ? 4 : (gc.nstrips > 512 ? (gc.nstrips + 255) / 256 : 1));   // as pick_spw (gemm.hip)
      ok = go.w_format == DIA_W_DENSE && go.w_layout == 0 && go.sk == 2 && go.KT == 256 && !go.cmap && go.nw == 0 && go.nstrips == d.D / 16 &&
           (go.act_f32 & 3) == 3 && go.gnext && go.nstrips * 16 <= go.p_ktiles * 32 &&
           gc.w_format == DIA_W_DENSE && gc.w_layout == 0 && gc.KT == 64 && gc.nw == 0 && gc.sk <= 1 && !gc.cmap && (gc.act_f32 & 1) && gcons && al16(gcons) &&
           (l + 1 == d.n_layer || (gc.nstrips + spw - 1) / spw >= d.D / 16);                 // x_new: 16 columns from each of D/16 workgroups
    }
    defer = ok;
  }

  // dia_engine_set_calib: the statistics of the rows matrix m of layer l is about to contract with, scaled as m scales them
  auto step_tap = [&](int l, int m) {
    const dia_gemm_args g = step_gemm(l, m);
    const int i = l < d.n_layer ? 6 * l + m : 6 * d.n_layer;
    dia_act_stats_args a = {};
    a.x = g.A; a.plane_stride = g.a_plane_stride; a.ktiles = g.a_ktiles; a.ktiles_used = e->calib_kt[i]; a.M = R; a.rows_pad = d.rows_pad;
    a.act_f32 = F; a.ssq_in = g.ssq_in; a.ssq_in_n = g.ssq_in_n; a.ssq_ld = g.ssq_ld; a.inv_d = g.inv_d; a.eps = g.eps;
    a.rows_per_slot = 2; a.cur = d.sample.cur; a.first_step = d.sample.first_step; a.fsm = d.sample.fsm; a.T = d.T;
    a.acc = e->calib_acc[i]; a.counter = e->calib_counters + i;
    return a;
  };
  // dia_engine_set_gram: the same rows, into the tap's packed Gram matrix
  auto step_gram = [&](int l, int m) {
    const dia_gemm_args g = step_gemm(l, m);
    const int i = tap_index(e, l, m);
    dia_act_gram_args a = {};
    a.x = g.A; a.plane_stride = g.a_plane_stride; a.ktiles = g.a_ktiles; a.ktiles_used = e->gram_kt[i]; a.M = R; a.rows_pad = d.rows_pad;
    a.act_f32 = F; a.ssq_in = g.ssq_in; a.ssq_in_n = g.ssq_in_n; a.ssq_ld = g.ssq_ld; a.inv_d = g.inv_d; a.eps = g.eps;
    a.rows_per_slot = 2; a.cur = d.sample.cur; a.first_step = d.sample.first_step; a.fsm = d.sample.fsm; a.T = d.T;
    a.gram = e->gram_ptr[i]; a.counter = e->gram_counters + i;
    return a;
  };
  if (e->gram_on && e->launches == 0 && !e->exec) {       // as below: checked before the first launch of the first step
    for (int l = 0; l <= d.n_layer; ++l)
      for (int m = (l < d.n_layer ? 0 : DIA_MAT_LOGITS); m < (l < d.n_layer ? DIA_MAT_LOGITS : DIA_MAT_COUNT); ++m) {
        if (!e->gram_ptr[tap_index(e, l, m)]) continue;
        const dia_act_gram_args a = step_gram(l, m);
        const int vrc = dia_act_gram_validate(&a, "dia_engine_set_gram");
        if (vrc) return vrc;
      }
  }
  if (e->calib_on && e->launches == 0 && !e->exec) {      // every tap's descriptor is checked before the first launch of the first step
    for (int l = 0; l <= d.n_layer; ++l)
      for (int m = (l < d.n_layer ? 0 : DIA_MAT_LOGITS); m < (l < d.n_layer ? DIA_MAT_LOGITS : DIA_MAT_COUNT); ++m) {
        const dia_act_stats_args a = step_tap(l, m);
        const int vrc = dia_act_stats_validate(&a, "dia_engine_set_calib");
        if (vrc) return vrc;
      }
  }

  int n = 0;
  bool fused = false;         // the wi launch of this layer ran wo as well
  const int rc = step_sequence(e, with_sampler, [&](int l, int what) -> int {
    int rc = DIA_OK;
    if (what == ATTN_SELF || what == ATTN_CROSS) {
      const dia_dec_layer& L = e->layers[l];
      dia_attn_args a = {};
      a.kv_dtype = d.kv_dtype; a.cur = d.sample.cur; a.v_blocked = d.v_blocked; a.cos_t = d.cos_t; a.sin_t = d.sin_t;
      a.P = planes[PL_A].p; a.p_plane_stride = planes[PL_A].stride; a.p_ktiles = akt;
      a.scratch = d.attn_scratch; a.tickets = d.attn_tickets; a.act_f32 = F;
      if (what == ATTN_SELF) {
        a.mode = DIA_ATTN_SELF; a.n_kv_heads = d.kv_heads; a.group = d.q_heads / d.kv_heads; a.n_rows = R; a.kv_cap = d.T;
        a.q = d.qkv; a.ldq = nqkv; a.k_off = d.q_heads * 128; a.v_off = (d.q_heads + d.kv_heads) * 128; a.rope_rows = d.T + 1;
        a.kc = L.k_self; a.vc = L.v_self; a.head_map = L.hmap_self; a.kv_plane_stride = d.kv_plane_self;
      } else {
        a.mode = DIA_ATTN_CROSS; a.n_kv_heads = d.cq_heads; a.group = 1; a.n_rows = d.B; a.kv_cap = d.S;
        a.q = d.qc; a.ldq = d.cq_heads * 128; a.len = d.text_len;
        a.kc = L.k_cross; a.vc = L.v_cross; a.head_map = L.hmap_cross; a.kv_plane_stride = d.kv_plane_cross;
      }
      if (what == ATTN_CROSS && !e->f8kv.empty()) rc = dia_attn_cross_fp8(&a, &e->f8kv[l], st);
      else if (what == ATTN_SELF && !e->f8self.empty()) rc = dia_attn_self_fp8(&a, &e->f8self[l], st);
      else rc = dia_attn(&a, st);
    } else if (what == SEG_MLP) {
      dia_seg_args sa = {};
      sa.a_in = (const float*)d.planes_a; sa.a_ktiles = akt; sa.M = R; sa.W = e->seg_w[l];
      sa.has_qkv = l + 1 < d.n_layer; sa.nslots = dia_seg_slots(sa.has_qkv); sa.D = d.D; sa.F = d.F;
      sa.x = d.x; sa.ldx = d.D; sa.g_mlp = e->layers[l].g_mlp; sa.g_next = (l + 1 < d.n_layer) ? e->layers[l + 1].g_sa : d.g_final;
      sa.qkv_out = d.qkv; sa.ldq = nqkv; sa.planes_x = (float*)d.planes_x; sa.xkt = xkt; sa.ssq = d.ssq; sa.ssq_ld = d.rows_pad;
      sa.eps = d.eps; sa.ws = d.seg_ws;
      rc = dia_seg_mlp(&sa, st);
    } else if (what == SAMPLER) {
      rc = dia_sample(&d.sample, st);
    } else if (what == SCORE) {
      rc = dia_score(&e->score, st);
    } else if (what >= GRAM) {
      const dia_act_gram_args ga = step_gram(l, what - GRAM);
      rc = dia_act_gram(&ga, st);
    } else if (what >= CALIB) {
      const dia_act_stats_args ca = step_tap(l, what - CALIB);
      rc = dia_act_stats(&ca, st);
    } else if (what == LORA_QKV || what == LORA_CQ) {
      // the rows the projection read: layer l's residual stream — under deferral the q/k/v launch of layer l > 0 has just written it (xnew)
      const dia_lora_args la = lora_site(e, l, what == LORA_CQ, xbuf(l));
      rc = la.n_segs ? dia_lora_apply(&la, st) : dia_lora_noop(st);
    } else if (what == DIA_MAT_WO && fused) {
      fused = false;                             // (the fused launch counts as two)
    } else {
      dia_gemm_args g = step_gemm(l, what);
      // opt-in (tuning knob mlp_fuse, EXPERIMENTS=1 builds), batch 1: wi and wo in one persistent launch (dia_mlp_fused).  Anything it refuses
      // (rows, shapes, CU count) takes the two launches.
      if (what == DIA_MAT_WI && e->mlp_fused != 0 && R <= 2 && d.mlp_barrier && !e->layers[l].cmap_mlp && d.w_planes <= 1 && !d.act_f32) {
        dia_gemm_args go = step_gemm(l, DIA_MAT_WO);
        go.sk = 2; go.sk_scratch = d.sk_scratch; go.sk_tickets = d.sk_tickets; go.nw = 0; go.spw = 0;
        rc = dia_mlp_fused(&g, &go, d.mlp_barrier, st);
        if (rc != DIA_OK && rc != DIA_E_ARG) return rc;
        fused = rc == DIA_OK;
        e->mlp_fused = fused ? 1 : 0;            // 0: not available for this model, do not try again
      }
      const dia_wo_defer_args wd = step_defer(l, what);
      if (!fused) rc = wd.nslices ? dia_gemm_wo_deferred(&g, &wd, st, nullptr) : dia_gemm(&g, st);
      if (rc == DIA_OK && wd.defer) e->wo_defer = 1;
      if (rc == DIA_E_ARG && wd.nslices) {
        // dia_gemm_wo_deferred cannot serve the deferred form of this model: from now on the in-launch merge.  The first wo of a step is the
        // first launch that asks for it, so nothing of this step has been issued in the other form yet — issue it again here
        const bool first = what == DIA_MAT_WO && l == 0 && e->wo_defer < 0;
        e->wo_defer = 0;
        if (!first) return rc;
        defer = false;
        g = step_gemm(l, what);
        rc = dia_gemm(&g, st);
      }
      if (what == DIA_MAT_WO && rc == DIA_E_ARG && g.sk > 1) {
        g.sk = 1;
        if (!wo_pair) { g.sk_scratch = nullptr; g.sk_tickets = nullptr; }     // two m-tiles keep the lent scratch
        rc = dia_gemm(&g, st);
      }
    }
    if (!rc) mark(e, n++);
    return rc;
  });
  if (!rc) e->launches = n;
  return rc;
}

extern "C" int dia_engine_create(const dia_engine_desc* d, void* stream, dia_engine** out) {
  if (!d || !out || !d->layers) return dia_fail(DIA_E_ARG, "dia_engine_create: null argument");
  if (d->n_layer <= 0 || d->B <= 0) return dia_fail(DIA_E_ARG, "dia_engine_create: empty model");
  if (d->D % 32 != 0 || d->F % 32 != 0) return dia_fail(DIA_E_ARG, "dia_engine_create: D and F must be multiples of 32");
  if (d->rows_pad < 2 * d->B || d->rows_pad % 16 != 0) return dia_fail(DIA_E_ARG, "dia_engine_create: rows_pad must be 16*ceil(2B/16)");
  if (d->q_heads % d->kv_heads != 0) return dia_fail(DIA_E_ARG, "dia_engine_create: q_heads % kv_heads != 0");
  if (d->act_f32 && !d->sample.embed.act_f32)
    return dia_fail(DIA_E_ARG, "dia_engine_create: act_f32 needs an embedding that writes fp32 tiles too");
  if (!d->act_f32 && d->sample.embed.act_f32) return dia_fail(DIA_E_ARG, "dia_engine_create: the embedding writes fp32 tiles but the engine reads planes");
  if (!d->x || !d->planes_x || !d->planes_a || !d->planes_h || !d->ssq || !d->qkv || !d->qc || !d->logits || !d->cos_t ||
      !d->sin_t || !d->text_len || !d->w_logits || !d->g_final || !d->attn_scratch || !d->attn_tickets)
    return dia_fail(DIA_E_ARG, "dia_engine_create: missing buffer");
  dia_engine* e = new dia_engine();
  e->d = *d;
  e->layers.assign(d->layers, d->layers + d->n_layer);
  e->d.layers = e->layers.data();
  e->stream = (hipStream_t)stream;
  if (d->seg_w && d->seg_ws) {
    const int nqkv = (d->q_heads + 2 * d->kv_heads) * 128;
    if (2 * d->B > 4 || !d->act_f32 || d->w_planes > 1 || !dia_seg_supported(d->D, d->F, max(d->q_heads, d->cq_heads) * 128, nqkv) ||
        d->cq_heads * 128 != 2048) {
      delete e;
      return dia_fail(DIA_E_ARG, "dia_engine_create: persistent segments need <= 4 rows, fp32 activation tiles, one weight plane, Dia-1.6B decoder shapes and 256 CUs");
    }
    for (int l = 0; l < d->n_layer; ++l) {
      const dia_dec_layer& L = d->layers[l];
      if (!d->seg_w[l] || L.cmap_mlp || L.cmap_next || L.smap_qkv) { delete e; return dia_fail(DIA_E_ARG, "dia_engine_create: persistent segments take dense (uncompacted) layers only"); }
    }
    e->seg_w.assign(d->seg_w, d->seg_w + d->n_layer);
    e->d.seg_w = e->seg_w.data();
    e->seg = true;
  }
  // measured: 37 us fused vs 27 us as two launches (batch 1, full size) — the write-through stores of the hidden
  // planes are acknowledged late under the weight stream (up to 10 us), the barrier and the coherent re-read add
  // 3.5 us each.  Kept as an opt-in experiment.
  e->mlp_fused = dia_tune(DIA_TUNE_MLP_FUSE) > 0 ? -1 : 0;
  *out = e;
  return DIA_OK;
}

extern "C" int dia_engine_destroy(dia_engine* e) {
  if (!e) return DIA_OK;
  // replays may still be queued: the executable graph (and the kernarg blocks it owns) must outlive them
  hipError_t he = hipSuccess;
  if (e->stream) he = hipStreamSynchronize(e->stream);
  if (e->side) { hipError_t h2 = hipStreamSynchronize(e->side); if (he == hipSuccess) he = h2; }
  if (e->exec) (void)hipGraphExecDestroy(e->exec);
  if (e->graph) (void)hipGraphDestroy(e->graph);
  for (auto& ev : e->pf_ev) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : e->prof) if (ev) (void)hipEventDestroy(ev);
  if (e->side) (void)hipStreamDestroy(e->side);
  delete e;
  return he == hipSuccess ? DIA_OK : dia_fail_hip(he, "dia_engine_destroy: hipStreamSynchronize");
}

extern "C" int dia_engine_decode(dia_engine* e, int n_steps, int use_graph) {
  if (!e || n_steps < 0) return dia_fail(DIA_E_ARG, "dia_engine_decode: bad argument");
  if (!use_graph) {
    for (int i = 0; i < n_steps; ++i) {
      int rc = enqueue_step(e, true);
      if (rc) return rc;
    }
    return DIA_OK;
  }
  if (!e->exec) {
    if (e->stream == nullptr) return dia_fail(DIA_E_STATE, "dia_engine_decode: graph capture needs a non-default stream");
    if (e->pf_lookahead > 0) {
      int rc0 = ensure_sink();
      if (rc0) return rc0;
      e->pf_w.clear();
      (void)step_sequence(e, true, [&](int l, int what) {
        const mat_w w = what < DIA_MAT_COUNT ? mat_weights(e, l, what) : mat_w{};      // (attention, the sampler, a segment, a tap: nothing)
        e->pf_w.push_back({w.w, (long)w.kt * w.ns * 1024});
        return DIA_OK;
      });
      if (!e->side && hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) != hipSuccess) return dia_fail(DIA_E_HIP, "hipStreamCreate(side)");
      e->pf_ev.assign(e->pf_w.size() + 2, nullptr);
      for (auto& ev : e->pf_ev)
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return dia_fail(DIA_E_HIP, "hipEventCreate(prefetch)");
    }
    hipError_t he = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    if (he != hipSuccess) return dia_fail_hip(he, "hipStreamBeginCapture");
    if (e->pf_lookahead > 0) {       // fork the side stream into the capture
      (void)hipEventRecord(e->pf_ev[e->pf_w.size()], e->stream);
      (void)hipStreamWaitEvent(e->side, e->pf_ev[e->pf_w.size()], 0);
      e->pf_capturing = true;
    }
    int rc = enqueue_step(e, true);
    if (e->pf_lookahead > 0) {       // join
      e->pf_capturing = false;
      (void)hipEventRecord(e->pf_ev[e->pf_w.size() + 1], e->side);
      (void)hipStreamWaitEvent(e->stream, e->pf_ev[e->pf_w.size() + 1], 0);
    }
    he = hipStreamEndCapture(e->stream, &e->graph);
    if (rc) return rc;
    if (he != hipSuccess) return dia_fail_hip(he, "hipStreamEndCapture");
    he = hipGraphInstantiate(&e->exec, e->graph, nullptr, nullptr, 0);
    if (he != hipSuccess) return dia_fail_hip(he, "hipGraphInstantiate");
  }
  for (int i = 0; i < n_steps; ++i) {
    hipError_t he = hipGraphLaunch(e->exec, e->stream);
    if (he != hipSuccess) return dia_fail_hip(he, "hipGraphLaunch");
  }
  return DIA_OK;
}

extern "C" int dia_engine_step_logits_only(dia_engine* e) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_step_logits_only: null engine");
  return enqueue_step(e, false);
}

// bounded device-side wait (wall clock, 100 MHz): lets the host run ahead of the stream
__global__ void k_delay(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

extern "C" int dia_engine_profile_step(dia_engine* e, float* ms, int cap) {
  if (!e || !ms) return dia_fail(DIA_E_ARG, "dia_engine_profile_step: null argument");
  const int n = dia_engine_launches_per_step(e);
  if (cap < n) return dia_fail(DIA_E_ARG, "dia_engine_profile_step: output array too small");
  e->prof.resize(n + 1);
  for (auto& ev : e->prof) {
    hipError_t he = hipEventCreate(&ev);
    if (he != hipSuccess) return dia_fail_hip(he, "hipEventCreate");
  }
  // Events inside a captured graph cannot be read back with hipEventElapsedTime on ROCm 7.2, so the
  // step is launched eagerly BEHIND a ~3 ms device-side delay kernel: by the time the delay ends the
  // host has queued every launch and event, and the intervals are device-side kernel time + the
  // in-queue dependency gap (what a graph replay pays), not host launch latency.
  int rc = DIA_OK;
  dia_launch<k_delay>(dim3(1), dim3(64), 0, e->stream, 300000LL /* 100 MHz ticks = 3 ms */);
  (void)hipEventRecord(e->prof[0], e->stream);
  rc = enqueue_step(e, true);
  {
    hipError_t he = hipStreamSynchronize(e->stream);
    if (rc == DIA_OK && he != hipSuccess) rc = dia_fail_hip(he, "hipStreamSynchronize");
  }
  if (rc == DIA_OK)
    for (int i = 0; i < n; ++i)
      if (hipEventElapsedTime(&ms[i], e->prof[i], e->prof[i + 1]) != hipSuccess) { ms[i] = -1.f; (void)hipGetLastError(); }
  for (auto& ev : e->prof) (void)hipEventDestroy(ev);
  e->prof.clear();
  return rc;
}

// One eager step behind the same device-side delay, every kernel bracketed by its own dispatch-level start / stop
// events (launch.hpp): ms[i] = duration of the i-th kernel of the step, in launch order, as rocprofv3 would report it.
extern "C" int dia_engine_time_step(dia_engine* e, float* ms, float* interval_ms, int cap) {
  if (!e || !ms) return dia_fail(DIA_E_ARG, "dia_engine_time_step: null argument");
  const int n = dia_engine_launches_per_step(e);
  if (cap < n) return dia_fail(DIA_E_ARG, "dia_engine_time_step: output array too small");
  dia_launch<k_delay>(dim3(1), dim3(64), 0, e->stream, 300000LL /* 100 MHz ticks = 3 ms */);
  dia_recorder_arm();
  int rc = enqueue_step(e, true);
  const int got = dia_recorder_collect(ms, cap, interval_ms);
  hipError_t he = hipStreamSynchronize(e->stream);
  if (rc != DIA_OK) return rc;
  if (he != hipSuccess) return dia_fail_hip(he, "dia_engine_time_step: hipStreamSynchronize");
  return got;      // kernels launched (n, or n - 1 when the MLP ran fused), or a negative DIA_E_*
}

// kernel instantiation name ("k_gemv_small<8, 8, 2, false>") of the i-th launch of this thread's last timed step / launch
extern "C" const char* dia_timed_kernel_name(int i) { return dia_recorder_label(i); }

extern "C" int dia_engine_mlp_fused(const dia_engine* e) { return e && e->mlp_fused == 1; }

extern "C" int dia_engine_launches_per_step(const dia_engine* e) {
  if (!e) return dia_fail(DIA_E_ARG, "null engine");
  int n = 0;
  (void)step_sequence(e, true, [&](int, int) { return ++n, DIA_OK; });
  return n;
}

// ------------------------------------------------------------------------------------------------
// Weight prefetch into the die-level Infinity Cache (256 MiB): a pure read pass, no output.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_prefetch(const uint4* __restrict__ p, long n16, unsigned* sink) {
  uint4 acc = {0, 0, 0, 0};
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const uint4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
    acc.x ^= a.x ^ b.x ^ c.x ^ d.x; acc.y ^= a.y ^ b.y ^ c.y ^ d.y;
    acc.z ^= a.z ^ b.z ^ c.z ^ d.z; acc.w ^= a.w ^ b.w ^ c.w ^ d.w;
  }
  for (; i < n16; i += stride) { const uint4 a = p[i]; acc.x ^= a.x; acc.y ^= a.y; acc.z ^= a.z; acc.w ^= a.w; }
  // data-dependent, practically never true: keeps the loads alive without writing anything
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9E3779B9u && sink) *sink = 1;
}

static unsigned* g_sink = nullptr;
static int ensure_sink() {
  if (!g_sink) {
    hipError_t e = hipMalloc(&g_sink, 4);
    if (e != hipSuccess) return dia_fail_hip(e, "hipMalloc(sink)");
  }
  return DIA_OK;
}

int dia_prefetch_launch(const void* ptr, long nbytes, int nblocks, hipStream_t st) {
  dia_launch<k_prefetch>(dim3(nblocks), dim3(256), 0, st, (const uint4*)ptr, (long)(nbytes / 16), g_sink);
  return dia_check_launch("k_prefetch");
}

extern "C" int dia_prefetch(const void* ptr, int64_t nbytes, int nblocks, void* stream) {
  if (!ptr || nbytes <= 0 || nblocks <= 0) return dia_fail(DIA_E_ARG, "dia_prefetch: bad argument");
  int rc = ensure_sink();
  if (rc) return rc;
  return dia_prefetch_launch(ptr, (long)nbytes, nblocks, (hipStream_t)stream);
}

extern "C" int dia_engine_set_x_alt(dia_engine* e, float* x_alt) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_x_alt: null engine");
  if (e->exec || e->wo_defer == 1) return dia_fail(DIA_E_STATE, "dia_engine_set_x_alt: a step has already been issued or captured");
  e->x_alt = x_alt;
  return DIA_OK;
}

extern "C" int dia_engine_set_mxfp4(dia_engine* e, const dia_mxfp4_streams* s) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_mxfp4: null engine");
  if (e->exec || e->launches > 0) return dia_fail(DIA_E_STATE, "dia_engine_set_mxfp4: a step has already been issued or captured");
  if (s && (s->n_layer != e->d.n_layer || !s->layers)) return dia_fail(DIA_E_ARG, "dia_engine_set_mxfp4: one dia_mxfp4_layer per decoder layer");
  e->f4.clear();
  if (s) e->f4.assign(s->layers, s->layers + s->n_layer);
  e->f4_logits = s ? s->w_logits : nullptr;
  return DIA_OK;
}

extern "C" int dia_engine_set_usparse(dia_engine* e, const dia_us_streams* s) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_usparse: null engine");
  if (e->exec || e->launches > 0) return dia_fail(DIA_E_STATE, "dia_engine_set_usparse: a step has already been issued or captured");
  if (s && (s->n_layer != e->d.n_layer || !s->layers)) return dia_fail(DIA_E_ARG, "dia_engine_set_usparse: one dia_us_layer per decoder layer");
  const auto bad = [](const dia_us_mat& m) { return m.stream && m.rate != 4 && m.rate != 2; };
  if (s) {
    bool ok = !bad(s->w_logits);
    for (int l = 0; l < s->n_layer && ok; ++l) {
      const dia_us_layer& L = s->layers[l];
      ok = !bad(L.w_qkv) && !bad(L.w_o) && !bad(L.w_cq) && !bad(L.w_co) && !bad(L.w_wi) && !bad(L.w_wo);
    }
    if (!ok) return dia_fail(DIA_E_ARG, "dia_engine_set_usparse: a stream's rate must be 4 or 2");
  }
  e->us.clear();
  if (s) e->us.assign(s->layers, s->layers + s->n_layer);
  e->us_logits = s ? s->w_logits : dia_us_mat{};
  return DIA_OK;
}

extern "C" int dia_engine_set_score(dia_engine* e, const dia_score_args* a) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_score: null engine");
  if (e->exec || e->launches > 0) return dia_fail(DIA_E_STATE, "dia_engine_set_score: a step has already been issued or captured");
  if (a) {
    const dia_sample_args& sp = e->d.sample;
    if (!sp.teacher) return dia_fail(DIA_E_ARG, "dia_engine_set_score: scoring needs a teacher-forced engine (sample.teacher)");
    if (sp.slot_cfg_scale || sp.slot_temperature || sp.slot_top_p || sp.slot_top_k || sp.slot_max_tokens)
      return dia_fail(DIA_E_ARG, "dia_engine_set_score: scoring is for closed batches, this sampler has per-slot state");
    const int rc = dia_score_validate(a, "dia_engine_set_score");
    if (rc) return rc;
    if (a->B != e->d.B) return dia_fail(DIA_E_ARG, "dia_engine_set_score: B differs from the engine's");
    e->score = *a;
  }
  e->score_on = a != nullptr;
  return DIA_OK;
}

// what a tapped step needs of its engine, for dia_engine_set_calib and dia_engine_set_gram alike; cap[i]: the k-tiles of tap i's plane set
static int tap_preconditions(const dia_engine* e, const char* who, int n_layer, bool have_arrays, std::vector<int>* cap) {
  char msg[256];
  auto fail = [&](const char* why) { snprintf(msg, sizeof msg, "%s: %s", who, why); return dia_fail(DIA_E_ARG, msg); };
  const dia_engine_desc& d = e->d;
  const dia_sample_args& sp = d.sample;
  if (n_layer != d.n_layer || !have_arrays) return fail("n_layer differs from the engine's, or a null array");
  if (!sp.teacher) return fail("calibration needs a teacher-forced engine (sample.teacher)");
  if (sp.slot_cfg_scale || sp.slot_temperature || sp.slot_top_p || sp.slot_top_k || sp.slot_max_tokens)
    return fail("calibration is for closed batches, this sampler has per-slot state");
  if (!sp.cur) return fail("the gate needs sample.cur");
  if (e->seg) return fail("the persistent MLP segments keep the inputs of co, wi, wo and q/k/v inside their launch (seg must be off)");
  if (dia_tune(DIA_TUNE_MLP_FUSE) > 0) return fail("the knob mlp_fuse keeps wo's input inside the fused launch");
  if (dia_tune(DIA_TUNE_WO_DIAG) == 1) return fail("the knob wo_diag changes the partial sums behind wo");
  if (sp.embed.cmap) return fail("compacted checkpoint (compaction map on the first layer's q/k/v input)");
  for (int l = 0; l < d.n_layer; ++l) {
    const dia_dec_layer& L = e->layers[l];
    if (L.cmap_ca || L.cmap_mlp || L.cmap_next || L.smap_qkv || L.smap_cq)
      return fail("compacted checkpoint (strip or compaction map on an edge of the step)");
  }
  const int n = 6 * d.n_layer + 1;
  const int akt = (max(d.q_heads, d.cq_heads) * 128) / 32;
  cap->resize(n);
  for (int i = 0; i < n; ++i) {
    const int m = i < 6 * d.n_layer ? i % 6 : DIA_MAT_LOGITS;
    const int in = STEP_MATS[m].in;
    (*cap)[i] = in == PL_X ? d.D / 32 : (in == PL_A ? akt : d.F / 32);
  }
  return DIA_OK;
}

extern "C" int dia_engine_set_calib(dia_engine* e, const dia_calib_args* a) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_calib: null engine");
  if (e->exec || e->launches > 0) return dia_fail(DIA_E_STATE, "dia_engine_set_calib: a step has already been issued or captured");
  if (!a) { e->calib_on = false; e->calib_acc.clear(); e->calib_kt.clear(); e->calib_counters = nullptr; return DIA_OK; }
  std::vector<int> cap;
  const int rc = tap_preconditions(e, "dia_engine_set_calib", a->n_layer, a->acc && a->kt && a->counters, &cap);
  if (rc) return rc;
  if (e->gram_on) return dia_fail(DIA_E_ARG, "dia_engine_set_calib: the engine already has dia_engine_set_gram, whose diagonals are these statistics");
  const int n = (int)cap.size();
  for (int i = 0; i < n; ++i)
    if (!a->acc[i] || a->kt[i] <= 0 || a->kt[i] > cap[i]) return dia_fail(DIA_E_ARG, "dia_engine_set_calib: a tap without acc, or k-tiles outside (0, k-tiles of its plane set]");
  e->calib_acc.assign(a->acc, a->acc + n);
  e->calib_kt.assign(a->kt, a->kt + n);
  e->calib_counters = a->counters;
  e->calib_on = true;
  e->wo_defer = 0;            // the in-launch merge: every q/k/v input reaches planes_x
  return DIA_OK;
}

extern "C" int dia_engine_set_gram(dia_engine* e, const dia_gram_args* a) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_gram: null engine");
  if (e->exec || e->launches > 0) return dia_fail(DIA_E_STATE, "dia_engine_set_gram: a step has already been issued or captured");
  if (!a) { e->gram_on = false; e->gram_ptr.clear(); e->gram_kt.clear(); e->gram_counters = nullptr; return DIA_OK; }
  std::vector<int> cap;
  const int rc = tap_preconditions(e, "dia_engine_set_gram", a->n_layer, a->gram && a->kt && a->counters, &cap);
  if (rc) return rc;
  if (e->calib_on) return dia_fail(DIA_E_ARG, "dia_engine_set_gram: the engine already has dia_engine_set_calib (the Gram's diagonal is the same statistic)");
  const int n = (int)cap.size();
  for (int i = 0; i < n; ++i) {
    if (a->kt[i] <= 0 || a->kt[i] > cap[i]) return dia_fail(DIA_E_ARG, "dia_engine_set_gram: a tap's k-tiles outside (0, k-tiles of its plane set]");
    if (reinterpret_cast<uintptr_t>(a->gram[i]) & 15) return dia_fail(DIA_E_ARG, "dia_engine_set_gram: a tap's gram is not 16-byte aligned");
  }
  e->gram_ptr.assign(a->gram, a->gram + n);
  e->gram_kt.assign(a->kt, a->kt + n);
  e->gram_counters = a->counters;
  e->gram_on = true;
  e->wo_defer = 0;            // the in-launch merge: every q/k/v input reaches planes_x
  return DIA_OK;
}

// a site no adapter of the bank touches keeps its place in the sequence (the launch count does not depend on the bank's contents)
__global__ void k_lora_none() {}
static int dia_lora_noop(void* st) {
  dia_launch<k_lora_none>(dim3(1), dim3(64), 0, (hipStream_t)st);
  return dia_check_launch("k_lora_none");
}

extern "C" int dia_engine_set_lora(dia_engine* e, const dia_lora_step* s) {
  if (!e) return dia_fail(DIA_E_ARG, "dia_engine_set_lora: null engine");
  if (e->exec || e->launches > 0) return dia_fail(DIA_E_STATE, "dia_engine_set_lora: a step has already been issued or captured");
  if (!s) { e->lora.clear(); e->lora_slot = nullptr; e->lora_adapters = 0; return DIA_OK; }
  const dia_engine_desc& d = e->d;
  if (s->n_layer != d.n_layer || !s->layers) return dia_fail(DIA_E_ARG, "dia_engine_set_lora: one dia_lora_layer per decoder layer");
  if (!s->adapter_of_slot || s->n_adapters <= 0) return dia_fail(DIA_E_ARG, "dia_engine_set_lora: adapter_of_slot and at least one adapter");
  if (e->seg) return dia_fail(DIA_E_ARG, "dia_engine_set_lora: the persistent MLP segments run the q/k/v projection inside their launch (seg must be off)");
  if (d.sample.embed.cmap) return dia_fail(DIA_E_ARG, "dia_engine_set_lora: compacted checkpoint (compaction map on the first layer's q/k/v input)");
  for (int l = 0; l < d.n_layer; ++l) {
    const dia_dec_layer& L = e->layers[l];
    if (L.smap_qkv || L.smap_cq || L.cmap_ca || L.cmap_next)
      return dia_fail(DIA_E_ARG, "dia_engine_set_lora: compacted checkpoint (strip or compaction map on an adapted projection)");
  }
  e->lora.assign(s->layers, s->layers + s->n_layer);
  e->lora_slot = s->adapter_of_slot; e->lora_adapters = s->n_adapters;
  for (int l = 0; l < d.n_layer; ++l) {        // every site's descriptor, on either residual buffer, is checked before a step exists
    for (int site = 0; site < 4; ++site) {
      const float* x = (site & 2) ? e->x_alt : d.x;
      if (!x) continue;
      const dia_lora_args a = lora_site(e, l, (site & 1) != 0, x);
      const int rc = a.n_segs ? dia_lora_validate(&a, "dia_engine_set_lora") : DIA_OK;
      if (rc) { e->lora.clear(); e->lora_slot = nullptr; e->lora_adapters = 0; return rc; }
    }
  }
  return DIA_OK;
}

// dia_engine_set_cross_fp8 / dia_engine_set_self_fp8: the e4m3 caches of every layer, over a capacity (S or T) of whole 32-key granules
static int set_kv_fp8(const char* who, dia_engine* e, const dia_kv_fp8_ptrs* layers, char cap_name, int32_t dia_engine_desc::*cap,
                      std::vector<dia_kv_fp8_ptrs> dia_engine::*into) {
  auto fail = [&](int code, const std::string& what) { return dia_fail(code, (std::string(who) + ": " + what).c_str()); };
  if (!e) return fail(DIA_E_ARG, "null engine");
  if (e->exec || e->launches > 0) return fail(DIA_E_STATE, "a step has already been issued or captured");
  if (!layers) { (e->*into).clear(); return DIA_OK; }
  const dia_engine_desc& d = e->d;
  if (d.kv_dtype != DIA_KV_BF16 || !d.v_blocked || d.*cap <= 0 || d.*cap % 32 != 0)
    return fail(DIA_E_ARG, std::string("the engine needs bf16 K/V (DIA_KV_BF16) with the blocked V layout and ") + cap_name + " % 32 == 0");
  for (int l = 0; l < d.n_layer; ++l)
    if (!layers[l].k8 || !layers[l].v8 || !layers[l].ks || !layers[l].vs) return fail(DIA_E_ARG, "null buffer in a layer");
  (e->*into).assign(layers, layers + d.n_layer);
  return DIA_OK;
}

extern "C" int dia_engine_set_cross_fp8(dia_engine* e, const dia_kv_fp8_ptrs* layers) {
  return set_kv_fp8("dia_engine_set_cross_fp8", e, layers, 'S', &dia_engine_desc::S, &dia_engine::f8kv);
}

extern "C" int dia_engine_set_prefetch(dia_engine* e, int lookahead) {
  if (!e || lookahead < 0) return dia_fail(DIA_E_ARG, "dia_engine_set_prefetch: bad argument");
  if (e->exec) return dia_fail(DIA_E_STATE, "dia_engine_set_prefetch: the step graph is already captured");
  e->pf_lookahead = lookahead;
  return DIA_OK;
}

extern "C" int dia_engine_set_self_fp8(dia_engine* e, const dia_kv_fp8_ptrs* layers) {
  return set_kv_fp8("dia_engine_set_self_fp8", e, layers, 'T', &dia_engine_desc::T, &dia_engine::f8self);
}
