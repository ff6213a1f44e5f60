/* libdia_hip.so — C ABI of the MI355X-native Dia decode path.
 *
 * The reference (babybirdprd/dia-tts-prune) has no native code and no FFI seam: its hot path is
 * PyTorch ops called from dia/layers.py and dia/model.py.  This header therefore DEFINES the
 * boundary a maintainer would bind (ctypes stub in INTEGRATION.md); every entry point names the
 * reference call site whose arithmetic it replaces.  All pointers are raw device pointers unless
 * marked "host"; no torch types cross this boundary.  Every function returns 0 on success and a
 * negative DIA_E_* code on failure; dia_last_error() gives the message (thread-local).
 *
 * One engine per device / stream; an engine is not re-entrant (the reference's Dia object is not
 * either: SURVEY.md §8b "Threading").
 */
#ifndef DIA_HIP_H
#define DIA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The version stays 8 although dia_embed_args / dia_sample_args grew at their tails and dia_slot_admit / dia_slot_retire were added
 * (continuous batching): zero-filled tails behave as before, and a binding of the older layout fails the sizeof / export checks.
 * dia_emit_frames / dia_emit_args (frame streaming) are a new entry point and a new struct: nothing older changed. */
#define DIA_ABI_VERSION 8

#define DIA_OK 0
#define DIA_E_ARG (-1)     /* bad argument / unsupported shape */
#define DIA_E_HIP (-2)     /* HIP runtime error */
#define DIA_E_STATE (-3)   /* call order violated */

#define DIA_KV_F32 0       /* parity mode: K/V caches in float32 */
#define DIA_KV_BF16 1      /* perf mode (reference GPU bf16 path, state.py:142-151) */
#define DIA_KV_BF16X2 2    /* every K / V value as hi + lo bf16 (16 significand bits) in two planes of the bf16 layouts, `kv_plane_stride`
                            * elements apart: the bytes of the fp32 caches, the MFMA attention kernel, logits within 1e-3 of the fp32 path */

/* GEMM epilogues */
#define DIA_EPI_SCALE_STORE 0  /* out[m][n] = acc * inv_rms[m]                      (q/k/v, cross-q, logits) */
#define DIA_EPI_RESID_EMIT 1   /* x[m][n] += acc; emit planes(x*g_next), strip ssq   (o_proj, wo)             */
#define DIA_EPI_SWIGLU_EMIT 2  /* h = silu(gate*inv)* (up*inv); emit planes(h)       (wi_fused)               */
#define DIA_EPI_CROSSKV 3      /* K = RoPE(acc*inv) , V = acc*inv -> cross caches    (precompute_cross_attn_cache) */

/* weight formats of dia_gemm_args.w_format */
#define DIA_W_DENSE 0      /* bf16 tiles [nstrips][KT][64][8], KT = K/32 */
#define DIA_W_SPARSE24 1   /* 2:4 sparse stream (dia_hip/layout.py tile_weight_24), KT = K/64 */
#define DIA_W_MXFP8 2      /* OCP MX e4m3 stream (dia_hip/layout.py tile_weight_fp8), KT = K/32 */
#define DIA_W_MXFP4 4      /* OCP MX e2m1 stream (dia_hip/layout.py tile_weight_fp4), KT = K/32.  (3 is not assigned: dia_gemm keeps
                            * refusing it as an unknown format, as callers and tests written against the previous header expect) */

#define DIA_W_USPARSE 5    /* lane-local fixed-rate stream of an unstructured-pruned bf16 matrix (dia_hip/layout.py tile_weight_us), KT = K/32;
                            * W is a HOST pointer to a dia_us_mat (below) */

/* attention modes */
#define DIA_ATTN_SELF 0   /* decoder self-attention over the growing cache (layers.py:541-555) */
#define DIA_ATTN_CROSS 1  /* decoder cross-attention over encoder K/V, cond rows (layers.py:560-574) */
#define DIA_ATTN_ENC 2    /* encoder bidirectional self-attention over L packed tokens (layers.py:396-404) */

const char* dia_last_error(void);
int dia_abi_version(void);
/* number of visible HIP devices, or a negative error */
int dia_device_count(void);
/* Tuning / debug overrides of the launch heuristics (process-wide; csrc/tuning.hpp lists the knobs, e.g. "attn_nz",
 * "gemm_spw", "wo_sk").  value < 0 clears a knob.  The DIA_TUNE variable ("name=value,...") is read once, at the
 * first knob lookup (this call, dia_get_tuning or a launch heuristic); settings made here override it.  The reference
 * has no counterpart (its only switches are torch.compile / dtype, model.py:631-647). */
int dia_set_tuning(const char* name, int value);
int dia_get_tuning(const char* name);
/* 1 when the library was built with EXPERIMENTS=1 (measured-and-rejected kernels: dia_mlp_fused, the sparse weight
 * stream of dia_gemm_args.sp_blocks, earlier two-m-tile GEMM forms); 0 for the product build, in which those entry
 * points fail with DIA_E_ARG */
int dia_has_experiments(void);

/* ------------------------------------------------------------------------------------------------
 * Kernel-level entry points (unit parity tests call these; the engine below chains them).
 * `stream` is a hipStream_t passed as void*.
 * ------------------------------------------------------------------------------------------------ */

/* out[M][N] = X[M][K] . W[K][N] with X given as three bf16 planes and W as bf16 tiles.
 * Replaces DenseGeneral.forward = torch.tensordot (layers.py:55-66) and, through its epilogues, the
 * surrounding RMSNorm scale (layers.py:541,560,579,714), residual adds (555,574,582), the SwiGLU
 * gate (layers.py:95-101) and the cross K/V RoPE + cache write (layers.py:652-663). */
typedef struct {
  const void* A;            /* planes base, bf16 */
  int64_t a_plane_stride;   /* elements between planes */
  int32_t a_ktiles;         /* K/32 of the plane layout */
  int32_t M;                /* valid rows */
  const void* W;            /* weight tiles, bf16 [nstrips][KT][64][8] */
  int32_t KT;               /* K/32 */
  int32_t nstrips;          /* N/16 */
  int32_t epi;              /* DIA_EPI_* */
  int32_t nw;               /* waves per workgroup (4, 8 or 16); 0 = choose */
  /* row scale = rsqrt(sum_i ssq_in[i][m] * inv_d + eps); ssq_in == NULL -> scale 1 */
  const float* ssq_in;
  int32_t ssq_in_n;
  int32_t ssq_ld;           /* row stride of ssq arrays (padded row count) */
  float inv_d;
  float eps;
  float* out;               /* SCALE_STORE: [M][ldo]; RESID_EMIT: x in/out [M][ldo] */
  int32_t ldo;
  int32_t spw;              /* strips per workgroup for the M <= 4 kernel; 0 = choose */
  const float* gnext;       /* RESID_EMIT: norm weight of the consumer (NULL -> 1) */
  void* P;                  /* emitted planes (RESID_EMIT, SWIGLU_EMIT) */
  int64_t p_plane_stride;
  int32_t p_ktiles;
  int32_t _pad1;
  float* ssq_out;           /* RESID_EMIT: [nstrips][ssq_ld] */
  /* CROSSKV */
  void* kc;                 /* K cache of one layer, [kv_batch][heads][kv_cap][128] */
  void* vc;
  int32_t kv_dtype;
  int32_t kv_heads;
  int32_t kv_cap;
  int32_t kv_batch_index;
  const float* cos_t;       /* [npos][64] */
  const float* sin_t;
  /* structured-pruned (compacted) checkpoints — all optional, NULL = dense:
   * cmap      RESID_EMIT: int32 [N]; column n of the residual stream is emitted at plane position
   *           cmap[n] (the consumer's compacted K order) or dropped when cmap[n] < 0;
   * strip_map SCALE_STORE / CROSSKV: int32 [nstrips]; compact strip s holds the 16 output columns
   *           of original strip strip_map[s] (whole heads dropped by a later o_proj). */
  const int32_t* cmap;
  const int32_t* strip_map;
  /* cross-workgroup split-K (long K, few strips; one m-tile only): sk_scratch holds nstrips*sk*256 floats,
   * sk_tickets nstrips int32 zeroed once by the caller (the kernel re-zeroes them).  sk: 0 or 1 = off,
   * n > 1 = n workgroups per strip (opt-in: measured slower than 1 on the decode shapes).  With 17..32 rows
   * (two m-tiles) both sizes double and sk_scratch_floats must state the capacity. */
  float* sk_scratch;
  int32_t* sk_tickets;
  int32_t sk;
  int32_t kv_vblocked;      /* CROSSKV: 1 = write V in the blocked layout of dia_attn_args.v_blocked (kv_cap % 32 == 0) */
  /* CROSSKV over a packed prefill batch: row m belongs to utterance row_b[m] (-1 = padding, skipped) at text
   * position m - seg_off[row_b[m]]; both NULL = one utterance, kv_batch_index, position m. */
  const int32_t* row_b;
  const int32_t* seg_off;
  /* capacity of sk_scratch in floats (0 = not stated: only the explicit `sk` split-K, nstrips * sk * 256 floats, is
   * assumed).  With 17..32 rows and K > 2048 dia_gemm splits K by itself when nstrips * (KT / 64) * 512 floats fit;
   * the column-block form (k_gemm_blk32, debug knob) needs nstrips * (KT / 8) * 512 floats. */
  int64_t sk_scratch_floats;
  /* zero-skipping weight stream of an unstructured-pruned matrix (dia_hip.layout.sparse_tile_weight) instead of W:
   * sp_blocks = concatenated tile blocks, sp_toff[strip * KT + ktile] = (block offset / 16) << 8 | chunks.
   * M <= 4, KT in {16, 32, 64}, no split-K; results are bit-identical to the dense tiles of the same matrix. */
  const void* sp_blocks;
  const uint32_t* sp_toff;
  /* fp32 ACTIVATION TILES: bit 0 = A is, bit 1 = P receives the fragment order of one plane ([mtile][ktile][lane][8]) with 4-byte
   * elements — 4 bytes per value instead of the 6 of three planes (a_plane_stride / p_plane_stride unused; a buffer sized for three
   * planes holds them).  The 5..128-row kernel is instantiated per format and splits each value into its planes in registers: same
   * arithmetic bit for bit, a third less activation traffic per workgroup.  Both bits (or bit 0 alone when nothing is emitted):
   * the M <= 4 GEMV (splits while staging its image through LDS) and the 8-wave forms of the 5..128-row kernel; a mixed-format
   * call runs the generic kernel.  Not available in the tiled prefill kernel. */
  int32_t act_f32;
  /* 0 / 1: W holds one bf16 tile set (exact for bf16-representable checkpoints).  3: W holds THREE tile sets back to back, the
   * hi / mid / lo bf16 planes of fp32 weights (hi + mid + lo == w exactly; plane stride = KT * nstrips * 512 elements): the
   * products of a genuine fp32 checkpoint, exact like the activations' — through the generic kernel only (no split-K, no
   * persistent forms): the parity configuration for checkpoints that bf16 cannot hold, not a fast path.
   * 2: W holds the hi = bf16(w) and lo = bf16(w - hi) planes of fp32 weights (16 significand bits, relative error <= 2^-17),
   * INTERLEAVED per k-tile inside one tile set (dia_hip/layout.py tile_weight_bf16x2): weight k-tile j of a strip is plane j & 1
   * of activation k-tile j >> 1, so KT counts hi and lo tiles (KT == 2 * K/32, a_ktiles >= KT/2) and every strip is one
   * sequential stream of twice the bytes.  The decode step's shapes (fp32 tiles in and out, 128 weight k-tiles per workgroup,
   * i.e. K = 2048 or split-K slices of it) run the tuned M <= 4 GEMV and 5..128-row kernels; every other shape the generic one.
   * Not with w_layout = 1 or the sparse stream. */
  int32_t w_planes;
  int64_t kv_plane_stride;  /* CROSSKV with kv_dtype DIA_KV_BF16X2: elements between the hi and the lo plane of kc / vc.  Must be positive
                             * and a multiple of 8 then (dia_attn's rule for the same caches), else DIA_E_ARG; so is a kv_dtype outside 0..2. */
  int32_t w_layout;         /* 0: 16-column strips (above); 1: diagonal tiles of 4-column groups (dia_hip/layout.py diag_tile_weight): W = bf16
                             * [N/4][K/128][64][8], `nstrips` = N/8 (8-column half strips, one workgroup each, the whole K, no split-K);
                             * M <= 4, DIA_EPI_RESID_EMIT, fp32 tiles in and out; ssq_out receives N/8 partials per row */
  /* CROSSKV for SEVERAL decoder layers in one launch (the prefill's cross-K/V projections share their input): kv_layer_strips > 0 =
   * original strips per layer (kv_heads * 16); strip s (after strip_map, whose entries then count layer * kv_layer_strips + strip)
   * belongs to layer s / kv_layer_strips and is written kv_layer_stride ELEMENTS behind kc / vc per layer.  W = the layers' tile
   * sets back to back, nstrips = their sum.  0 = one layer (above). */
  int32_t kv_layer_strips;
  int64_t kv_layer_stride;
  /* DIA_W_DENSE (0): W as above.  DIA_W_SPARSE24: W is the 2:4 sparse stream of a matrix with at most 2 non-zeros in every
   * group of 4 consecutive K of a column (dia_hip/layout.py tile_weight_24: per strip, groups of 8 sparse k-tiles of 64 K, each
   * a 1 KiB index block followed by 8 KiB of kept values, the A operand of v_smfmac_f32_16x16x64_bf16) and KT counts sparse
   * k-tiles (K/64, a multiple of 8 per workgroup).  M <= 16, fp32 activation tiles in and out (act_f32 = 3; bit 0 alone when
   * nothing is emitted), SCALE_STORE / RESID_EMIT (with gnext) / SWIGLU_EMIT, split-K through sk; not with w_planes > 1,
   * w_layout = 1, sp_blocks, CROSSKV or the compaction maps — those return DIA_E_ARG.
   * DIA_W_MXFP8: W is the MXFP8 stream of a matrix whose every value is an e4m3 element times the power-of-two scale of its
   * block of 32 consecutive K of a column (dia_hip/quant.py; dia_hip/layout.py tile_weight_fp8: per strip, groups of 16 k-tiles,
   * each a 256-byte block of E8M0 scales followed by 8 KiB of e4m3 elements, expanded to the bf16 B operand of
   * v_mfma_f32_16x16x32_bf16 in registers) and KT = K/32, a multiple of 16 and at most 128 per workgroup (KT / sk).  Same
   * restrictions as DIA_W_SPARSE24; results equal the dense tiles of the same matrix up to summation order.
   * DIA_W_MXFP4: the same with e2m1 elements (dia_hip/layout.py tile_weight_fp4: the scale block followed by 4 KiB of elements, two
   * per byte); same shapes, restrictions and results as DIA_W_MXFP8.
   * DIA_W_USPARSE: W points to a dia_us_mat in HOST memory (read during the call only) that names the stream of an unstructured-pruned
   * matrix and its rate; KT = K/32 as for the MX streams (a multiple of 16, at most 128 per workgroup).  M <= 4 only; otherwise the
   * restrictions of DIA_W_SPARSE24.  Lossless: results equal the dense tiles of the same matrix up to summation order. */
  int32_t w_format;
  int32_t _pad2;
} dia_gemm_args;
int dia_gemm(const dia_gemm_args* a, void* stream);
/* One matrix as an unstructured sparse stream (dia_gemm_args.w_format = DIA_W_USPARSE; dia_hip/layout.py tile_weight_us(w, rate)).
 * With ns = nstrips, G = KT / 16 groups of 16 k-tiles and R = rate the device bytes at `stream` are, back to back:
 *   1. fixed part [ns][G][1024 + 2048 R]: per group a 1 KiB mask block [64 lanes][16 bytes] (byte i of lane l: bit j = element j of
 *      the lane's dense B-operand fragment of k-tile i, W[32 t + 8 (l >> 4) + j][16 strip + (l & 15)], is non-zero), then value slots
 *      of 1 KiB [64 lanes][16 bytes]: a lane's window of a k-tile = its first R non-zeros in element order as bf16 (R = 4: slot p
 *      holds the 8-byte windows of k-tiles 2p, 2p + 1; R = 2: the 4-byte windows of k-tiles 4p .. 4p + 3);
 *   2. run table uint32 [ns * G * 16 + 1], padded to 16 bytes: entry (strip * G + g) * 16 + c = index of the first overflow entry of
 *      column c of group g of the strip, the last entry the total;
 *   3. overflow entries uint32 (k within the group | bf16 bits << 16) ordered by (strip, group, column, k): the non-zeros beyond the
 *      windows; padded to 16 bytes plus 16 zero bytes.
 * stream == NULL: the matrix has no stream (the engine keeps its dense tiles). */
typedef struct {
  const void* stream;       /* device, 16-byte aligned */
  int32_t rate;             /* 4 or 2 */
  int32_t _pad;
} dia_us_mat;
/* wo's cross-workgroup split-K merged by the launch that FOLLOWS it instead of inside it (M <= 4, dense one-plane weights, fp32
 * activation tiles, no cmap; anything else returns DIA_E_ARG and the caller keeps the in-launch merge through dia_gemm).  The
 * launch is described by a dia_gemm_args as for dia_gemm, plus:
 * Producer (defer = 1; RESID_EMIT with gnext, KT = 256, sk = 2): K slice s stores the valid rows of its partial tile to
 * slices + s * slice_stride in the fp32 tile order of P (p_ktiles, nstrips * 16 <= p_ktiles * 32) and returns: no ticket, no
 * merge; out, P, ssq_out, sk_scratch and sk_tickets are validated as for dia_gemm but not touched.
 * Consumer (defer = 0; SCALE_STORE, KT = 64, i.e. a row of D = 2048): instead of A and ssq_in its prologue reads the slices,
 * (2 x 64 * 512 floats), the old residual rows xold [M][ldx >= 2048] and its own norm weight a->gnext [2048] (A must still be a
 * valid pointer, it is not read; ssq_in is ignored), and rebuilds bit for bit what the in-launch form
 * leaves: x_new = x_old + (s_0 + s_1), the row's sum of squares, the image x_new * gnext.  xnew (may be NULL; != xold, every
 * workgroup reads the whole old row) receives x_new, 16 columns from each of the first D/16 workgroups.
 * ms_out != NULL: timed as dia_gemm_timed (synchronises; dia_timed_kernel_name(0) names the kernel). */
typedef struct {
  float* slices;
  int64_t slice_stride;     /* floats between two slices: at least one m-tile of P (p_ktiles * 512; the consumer: 64 * 512) */
  int32_t nslices;          /* 2 */
  int32_t defer;
  const float* xold;
  float* xnew;
  int32_t ldx;
  int32_t _pad0;
} dia_wo_defer_args;
int dia_gemm_wo_deferred(const dia_gemm_args* a, const dia_wo_defer_args* w, void* stream, float* ms_out);
/* same launch, bracketed by dispatch-level start/stop events (hipExtLaunchKernelGGL); returns the
 * kernel's own duration in milliseconds and synchronises on its end */
/* Fused SwiGLU MLP for 1-2 rows (batch 1): wi (DIA_EPI_SWIGLU_EMIT into planes P) and wo (DIA_EPI_RESID_EMIT reading
 * those planes, with sk_scratch / sk_tickets for a split-K of 2) in one persistent launch with a grid barrier
 * between the phases (MlpBlock.forward, layers.py:92-105).  `barrier`: two int32 on the device, zeroed by the
 * caller once per session; barrier[1] != 0 afterwards means a workgroup gave up waiting (results invalid).
 * Returns DIA_E_ARG when the shapes do not chain, no instantiation exists or 2 * wo->nstrips exceeds the CU
 * count (every workgroup must be resident) — callers then issue the two dia_gemm launches instead. */
int dia_mlp_fused(const dia_gemm_args* wi, const dia_gemm_args* wo, int32_t* barrier, void* stream);
/* same, bracketed by dispatch-level start/stop events; *ms_out = kernel duration (blocks until it finished) */
int dia_mlp_fused_timed(const dia_gemm_args* wi, const dia_gemm_args* wo, int32_t* barrier, void* stream, float* ms_out);


int dia_gemm_timed(const dia_gemm_args* a, void* stream, float* ms_out);

/* Single-query attention (decode) and the encoder's bidirectional attention on the same kernel.
 * Replaces RotaryEmbedding.forward (layers.py:135-173), KVCache.update (state.py:99-103),
 * repeat_interleave (layers.py:319-320) and F.scaled_dot_product_attention (layers.py:329-337). */
typedef struct {
  int32_t mode;             /* DIA_ATTN_* */
  int32_t kv_dtype;
  int32_t n_kv_heads;       /* grid.x */
  int32_t group;            /* q heads per kv head: 4 (self), 1 (cross, enc) */
  int32_t n_rows;           /* SELF: R = 2B rows; CROSS: B utterances; ENC: L tokens */
  int32_t kv_cap;           /* cache capacity per head (audio_length / text capacity) */
  const float* q;           /* fp32 [rows][ldq]; q head h at column q_off + h*128 */
  int32_t ldq;
  int32_t q_off;
  int32_t k_off;            /* SELF: new k of kv head h at k_off + h*128, new v at v_off + h*128 */
  int32_t v_off;
  void* kc;                 /* [kv rows][n_kv_heads][kv_cap][128] */
  void* vc;
  const int32_t* cur;       /* SELF/CROSS: per-utterance current step (device) */
  const int32_t* len;       /* CROSS: per-utterance text length (device); ENC: unused */
  int32_t enc_len;          /* ENC: L (== n_rows, <= kv_cap) */
  int32_t rope_rows;        /* rows of cos_t / sin_t, or 0 = not stated.  When stated, dia_attn refuses shapes whose RoPE
                             * position could leave the tables (SELF: kv_cap + 1 rows needed, ENC: enc_len) */
  const float* cos_t;
  const float* sin_t;
  void* P;                  /* output planes [3][mtiles][p_ktiles][64][8] */
  int64_t p_plane_stride;
  int32_t p_ktiles;
  int32_t _pad1;
  /* split-key partials: required when more than 128 keys are possible (kv_cap, or enc_len for ENC).
   * scratch: dia_attn_scratch_floats(pairs_rows, n_kv_heads, kv_cap) floats, pairs_rows = n_rows;
   * tickets: n_rows*n_kv_heads int32, zero before the first launch (the kernel re-zeroes them). */
  float* scratch;
  int32_t* tickets;
  /* int32 [n_kv_heads*group] or NULL: query head h is emitted at head position head_map[h] of the
   * (compacted) o_proj input; < 0 = head pruned, nothing emitted */
  const int32_t* head_map;
  /* 1: bf16 caches with V stored blocked as [key/32][128 dims][32 keys] (K stays [key][128]) -> the MFMA
   * attention kernel; 0: V stored [key][128] -> the VALU kernel (required for fp32 caches and ENC) */
  int32_t v_blocked;
  int32_t act_f32;          /* 1: P receives fp32 activation tiles (dia_gemm_args.act_f32) instead of three planes */
  int64_t kv_plane_stride;  /* DIA_KV_BF16X2: elements between the hi and the lo plane of kc / vc */
} dia_attn_args;
int dia_attn(const dia_attn_args* a, void* stream);
int dia_attn_scratch_floats(int n_rows, int n_kv_heads, int kv_cap);

/* Encoder self-attention of a PACKED prefill batch (Encoder.forward, layers.py:385-462, for every utterance
 * at once): utterance b owns packed rows [seg_off[b], seg_off[b] + seg_len[b]), seg_off a multiple of 32;
 * row_b[m] = utterance of packed row m or -1 for padding.  Launches the K/V plane preparation and the
 * MFMA attention; all arithmetic fp32-exact (three bf16 planes per operand).  kp / vp are scratch:
 * 3 * heads * rows * 128 bf16 each. */
typedef struct {
  const float* qkv;         /* [rows][ldq] fp32: q head h at q_off + h*128, k at k_off + h*128, v at v_off + h*128 */
  int32_t ldq, q_off, k_off, v_off;
  int32_t heads;
  int32_t rows;             /* packed rows, multiple of 32 */
  const int32_t* row_b;     /* [rows] */
  const int32_t* seg_off;   /* [B] */
  const int32_t* seg_len;   /* [B] */
  const float* cos_t;       /* [npos][64] */
  const float* sin_t;
  void* kp;                 /* scratch K planes */
  void* vp;                 /* scratch V planes (blocked) */
  void* P;                  /* output planes [3][rows/16][p_ktiles][64][8]; padding rows are not written */
  int64_t p_plane_stride;
  int32_t p_ktiles;
  int32_t _pad0;
} dia_enc_attn_args;
int dia_enc_attn(const dia_enc_attn_args* a, void* stream);

/* Decoder prefill over an audio prompt, batched (Decoder.forward in prefill mode, layers.py:722-766, with the
 * replay semantics of DESIGN.md §8: token row r -> cache slot r at RoPE position r + 1).  All prompt rows of all
 * utterances, both CFG rows, are packed: segment s = (utterance b, CFG row c) owns packed rows
 * [seg_off[s], seg_off[s] + seg_len[s]), seg_off a multiple of 32; row_seg[m] = segment of packed row m or -1;
 * seg_row[s] = 2b + c (the self-cache row; b = seg_row >> 1 indexes tokens, cross caches and text_len).
 * bf16 caches with blocked V only.  The dense layers between these three calls are dia_gemm over the packed rows. */
typedef struct {
  const int32_t* row_seg; const int32_t* seg_off; const int32_t* seg_len; const int32_t* seg_row;
  int32_t rows;             /* packed rows, multiple of 32 */
  int32_t _pad0;
  /* dia_dec_prefill_embed: x[m] = sum_c emb[c][tokens[b][r][c]], planes(x * g), strip ssq */
  const int32_t* tokens;    /* [B][T][C] */
  int32_t T, C, V, D;
  const float* emb;         /* [C][V][D] */
  const float* g;           /* first layer's pre-SA norm weight */
  float* x;                 /* [rows][D] */
  void* P; int64_t p_plane_stride; int32_t p_ktiles; int32_t ssq_ld;   /* embed: x planes; attn: output planes */
  float* ssq;               /* [D/16][ssq_ld] */
  /* dia_dec_prefill_kv (self K/V append of every packed row) and dia_dec_prefill_attn */
  const float* q;           /* fp32 [rows][ldq]: q head h at q_off + h*128 (kv: k at k_off, v at v_off) */
  int32_t ldq, q_off, k_off, v_off;
  int32_t q_heads, kv_heads, kv_cap;
  int32_t causal;           /* attn: 1 = self (keys 0..r of the segment's cache row), 0 = cross (text keys of the cond segment; uncond -> 0) */
  void* kc; void* vc;       /* bf16 caches [cache row][kv_heads][kv_cap][128], V blocked [.. kv_cap/32][128][32] */
  const float* cos_t; const float* sin_t;
  const int32_t* text_len;  /* cross: [B] */
} dia_dec_prefill_args;
int dia_dec_prefill_embed(const dia_dec_prefill_args* a, void* stream);
int dia_dec_prefill_kv(const dia_dec_prefill_args* a, void* stream);
int dia_dec_prefill_attn(const dia_dec_prefill_args* a, void* stream);

/* Encoder helper: RoPE(k) and v of all L tokens from the qkv rows into an fp32 [heads][cap][128]
 * scratch "cache" (layers.py:274-279,306-307 for the encoder). */
int dia_enc_kv_prep(const float* qkv, int ldq, int k_off, int v_off, int heads, int L, int cap,
                    const float* cos_t, const float* sin_t, float* kc, float* vc, void* stream);

/* x[m][:] = table[ids[m]][:] for the text encoder (layers.py:452), plus planes(x*g) and strip ssq.
 * cmap: as dia_gemm_args.cmap (first encoder layer's q/k/v input order of a compacted checkpoint) or NULL. */
int dia_embed_text(const int32_t* ids, int L, const float* table, int D, const float* g, float* x,
                   void* P, int64_t p_plane_stride, int p_ktiles, float* ssq, int ssq_ld, const int32_t* cmap, void* stream);

/* Decoder input embedding: x[2b..2b+1][:] = sum_c emb_c[tokens[b][cur[b]-1][c]] (layers.py:691-696). */
typedef struct {
  const int32_t* tokens;    /* [B][T][C] */
  const int32_t* cur;       /* [B] */
  int32_t B, T, C, V, D;
  int32_t act_f32;          /* 1: P receives fp32 activation tiles (dia_gemm_args.act_f32) instead of three planes */
  const float* emb;         /* [C][V][D] fp32 */
  const float* g;           /* first pre_sa_norm weight */
  float* x;                 /* [rows][D] */
  void* P;
  int64_t p_plane_stride;
  int32_t p_ktiles;
  int32_t ssq_ld;
  float* ssq;               /* [D/16][ssq_ld] */
  const int32_t* cmap;      /* as dia_gemm_args.cmap (first layer's q/k/v input order) or NULL */
  /* device int32 [n_slots] or NULL: embed the rows of these utterances only (an admission into a running session must not
   * touch the rows of the live ones); NULL = all B, as before.  Ignored by the sampler's own next-step embedding. */
  const int32_t* slots;
  int32_t n_slots;
  int32_t _pad0;
} dia_embed_args;
int dia_embed_tokens(const dia_embed_args* a, void* stream);

/* CFG + constraints + temperature / top-k / top-p / multinomial + EOS/delay state machine + token
 * write + next-step embedding.  Replaces Dia._decoder_step (model.py:447-488), _sample_next_token
 * (model.py:32-82) and the loop body at model.py:771-807 (device-side, no host sync). */
typedef struct {
  const float* logits;      /* [rows][ld_logits], channel c at column c*V */
  int32_t ld_logits;
  int32_t B;
  int32_t T;                /* token buffer rows = audio_length */
  int32_t C;                /* 1..12: the sampler keeps 13056 bytes of LDS scratch per channel, and 13 channels pass the 160 KiB of a
                             * CU; refused before any launch (the embedding calls above take up to 16) */
  int32_t V;                /* 1..1088 */
  int32_t max_tokens;
  float cfg_scale, temperature, top_p;
  int32_t top_k;
  int32_t eos, pad, bos;
  int32_t max_delay;
  int32_t ignore_eos;       /* perf runs: natural EOS does not start the countdown */
  int32_t teacher;          /* parity runs: record samples in `pred`, leave `tokens` untouched */
  const int32_t* delay;     /* [C] device */
  const float* noise;       /* [B][noise_steps][C][V] Exp(1) variates; step index = cur - first_step[b] */
  int32_t noise_steps;
  int32_t _pad0;
  int32_t* tokens;          /* [B][T][C] */
  int32_t* pred;            /* [B][T][C] raw samples per step (row cur) */
  int32_t* cur;             /* [B] in/out */
  int32_t* fsm;             /* [B][8]: eos_detected, eos_countdown, bos_countdown, done, last_step, 3 unused */
  /* audio prompt (model.py:311-353, 406-422): first_step[b] = 1 + prompt frames = the first step that is
   * sampled.  Steps cur < first_step[b] REPLAY rows already in the token buffer: nothing is sampled or
   * written, the state machine does not move, only cur advances and the next row is embedded; the noise
   * row of step cur is cur - first_step[b].  NULL = no prompt anywhere (first_step 1). */
  const int32_t* first_step;
  dia_embed_args embed;     /* next-step embedding; embed.tokens/cur are taken from above */
  /* per-slot sampling state of a continuously batched session (device arrays [B], written by dia_slot_admit): all five or
   * none.  NULL = the scalars above for every utterance, the kernel instantiation of a closed batch.  With them, utterance b
   * samples with slot_*[b] (its own instantiation of the kernel: the values are workgroup-uniform, so the route choice stays
   * a uniform branch), `max_tokens` above is the session's capacity (noise_steps >= max_tokens - 1) and `noise` is required;
   * a slot whose temperature is 0 does not read it. */
  const float* slot_cfg_scale;
  const float* slot_temperature;
  const float* slot_top_p;
  const int32_t* slot_top_k;
  const int32_t* slot_max_tokens;
} dia_sample_args;
int dia_sample(const dia_sample_args* a, void* stream);

/* Continuous batching: (re)initialise the device state of `n` slots (utterance indices) of a running session in ONE launch, in
 * stream order between two decode steps / graph replays.  For slot[i]: token rows [0, T) = the first prefix_rows[i] rows of
 * prefix[i] (the BOS / PAD prefill or the delayed audio-prompt rows the host prepared), -1 behind them; pred rows -1;
 * cur = 1; fsm = {0, -1, max_delay, 0, 0, 0, 0, 0}; first_step, text_len and the five per-slot sampling values.  Replaces
 * what the reference does per call in Dia._prepare_generation (model.py:355-427) and DecoderInferenceState / DecoderOutput
 * construction (state.py:178-208) for ONE utterance of a batch.  Caches are NOT cleared: keys at and beyond a slot's length
 * are weighted by exactly 0 and only have to be finite, which the previous utterance's values are (DESIGN.md
 * "Continuous batching").  The per-slot HOST arrays are read during the call (they travel as kernel arguments); at most
 * DIA_SLOTS_PER_CALL slots per call.
 * dia_slot_retire parks slots (reads n, slot, B and the cur / fsm / text_len pointers only): fsm[3] = 1 (done), cur = 1,
 * text_len = 0 — an empty slot then costs one self-attention key and no cross-attention key per step. */
#define DIA_SLOTS_PER_CALL 64
typedef struct {
  int32_t B, T, C, S;          /* session shape: slots, token rows, channels, text capacity of the cross caches */
  int32_t max_delay;
  int32_t n;                   /* slots in this call, 1..DIA_SLOTS_PER_CALL */
  const int32_t* slot;         /* host [n], distinct, each < B */
  const int32_t* text_len;     /* host [n], each <= S */
  const int32_t* first_step;   /* host [n], 1 + prompt frames, each in [1, T] */
  const int32_t* prefix_rows;  /* host [n], each in [1, prefix_ld] and <= T */
  const int32_t* max_tokens;   /* host [n], each in [2, T] */
  const float* cfg_scale;      /* host [n] */
  const float* temperature;    /* host [n] */
  const float* top_p;          /* host [n] */
  const int32_t* top_k;        /* host [n] */
  const int32_t* prefix;       /* DEVICE int32 [n][prefix_ld][C] */
  int32_t prefix_ld;
  int32_t _pad0;
  /* device state of the session, as in dia_sample_args / dia_engine_desc */
  int32_t* tokens;             /* [B][T][C] */
  int32_t* pred;               /* [B][T][C] */
  int32_t* cur;                /* [B] */
  int32_t* fsm;                /* [B][8] */
  int32_t* d_first_step;       /* [B] */
  int32_t* d_text_len;         /* [B] */
  float* slot_cfg_scale;       /* [B] ... */
  float* slot_temperature;
  float* slot_top_p;
  int32_t* slot_top_k;
  int32_t* slot_max_tokens;
} dia_slot_admit_args;
int dia_slot_admit(const dia_slot_admit_args* a, void* stream);
int dia_slot_retire(const dia_slot_admit_args* a, void* stream);

/* Frame streaming: take the codec frames that have become FINAL out of running slots, in ONE launch, in stream order between two
 * decode steps / graph replays (csrc/stream.hip; DESIGN.md "Frame streaming").  A step writes token row cur and no later step
 * rewrites it, so with W = fsm[3] ? fsm[4] + 1 : cur the rows [first_step, W) of a slot belong to its output slice for good, and
 * frame t — what the reference's codec input holds at [t] after the delay pattern is undone and the last max_delay rows are
 * dropped (dia/audio.py:88-163, model.py:498-533) — is final exactly when t < ready = max(0, W - first_step - max_delay).
 * For every listed slot b: n = min(ready - emitted[b], cap) frames [emitted[b], emitted[b] + n) go to out[b][0..n)[C] as
 * tokens[b][first_step + t + delay[c]][c], ids outside [0, codebook_size) -> 0; state[b] = {start = emitted[b], n,
 * total = finished ? ready : -1, finished}; emitted[b] += n.  A slot has been taken out completely when start + n == total.
 * Reads tokens / cur / fsm / first_step / delay and writes none of them; rows [n, cap) of out[b] and slots that are not listed are
 * left alone.  Plain loads and stores, no atomics: stream order is the only ordering.
 * flags = DIA_EMIT_RESET: the listed slots start over instead — emitted[b] = 0, state[b] = {0, 0, -1, 0} — to be enqueued behind
 * dia_slot_admit for the same slots (reads n, slot, the shape and the emitted / state pointers only).
 * The slot list is a HOST array read during the call (it travels as kernel arguments); at most DIA_SLOTS_PER_CALL slots per call. */
#define DIA_EMIT_RESET 1
typedef struct {
  int32_t B, T, C;             /* session shape: slots, token rows, channels (1..16) */
  int32_t max_delay;           /* largest entry of delay, in [0, T) */
  int32_t codebook_size;
  int32_t cap;                 /* frames per slot and call = depth of out, >= 1 */
  int32_t n;                   /* slots in this call, 1..DIA_SLOTS_PER_CALL */
  int32_t flags;               /* 0 or DIA_EMIT_RESET */
  const int32_t* slot;         /* host [n], distinct, each < B */
  /* device state of the session, as in dia_sample_args (read only) */
  const int32_t* tokens;       /* [B][T][C] */
  const int32_t* cur;          /* [B] */
  const int32_t* fsm;          /* [B][8] */
  const int32_t* first_step;   /* [B], NULL = 1 everywhere */
  const int32_t* delay;        /* [C] */
  /* streaming state (device) */
  int32_t* emitted;            /* [B] frames taken out of the slot's utterance so far */
  int32_t* out;                /* [B][cap][C] staging, frame-major */
  int32_t* state;              /* [B][4] start, n, total, finished of the last call */
} dia_emit_args;
int dia_emit_frames(const dia_emit_args* a, void* stream);

/* Teacher-forced scoring (csrc/score.hip; DESIGN.md "Scoring"): the log-probability the model gives to tokens that are already in
 * the token buffer, ONE launch, in stream order behind the logits GEMM of a step and before its sampler (cur not yet advanced).
 * The reference has no counterpart (it only samples: model.py:447-488).  For every utterance b with t = cur[b], first_step[b] <= t
 * < T and fsm[b][3] == 0, and every channel c, with tok = tokens[b][t][c], un / co = logits rows 2b / 2b + 1 at columns
 * [c * V, c * V + V) and g = co + s * (co - un) under the sampler's constraints (-inf on EOS for channels >= 1, on PAD and BOS
 * everywhere; the expression and rounding of dia_sample):
 *   out[b][t][c][0] = log_softmax(co)[tok]                    no guidance, no constraints
 *   out[b][t][c][1] = log_softmax(g)[tok]                     -inf for a masked target
 *   out[b][t][c][2] = -sum p * log p of softmax(g), in nats   terms with p == 0 count 0
 * fp32: m = max, z = sum expf(l - m), lp = (l_tok - m) - logf(z).  A target outside [0, V) writes NaN to all three; every other
 * utterance (prompt replay rows, finished, t outside [0, T)) writes nothing.  Reads only, apart from out: no state moves.
 * One workgroup per utterance, one wave per channel: C <= 12, V <= 1088, ld_logits >= C * V, else DIA_E_ARG before any launch. */
typedef struct {
  const float* logits;         /* [2B rows][ld_logits], channel c at column c*V (dia_sample_args.logits) */
  int32_t ld_logits;
  int32_t B;
  int32_t T;                   /* token buffer rows */
  int32_t C;                   /* 1..12 */
  int32_t V;                   /* 1..1088 */
  float cfg_scale;             /* s of every utterance, unless ... */
  const float* cfg_scales;     /* ... device float [B] or NULL: s per utterance */
  int32_t eos, pad, bos;
  int32_t _pad0;
  const int32_t* tokens;       /* [B][T][C]: row cur[b] holds the target */
  const int32_t* cur;          /* [B] */
  const int32_t* first_step;   /* [B] or NULL = 1 everywhere: rows below it are audio-prompt replay */
  const int32_t* fsm;          /* [B][8] as dia_sample_args.fsm or NULL: an utterance with fsm[b][3] != 0 (done) is left alone */
  float* out;                  /* [B][T][C][3] */
} dia_score_args;
int dia_score(const dia_score_args* a, void* stream);

/* Read-only pass over [ptr, ptr+nbytes) that pulls it into the 256 MiB Infinity Cache ahead of its
 * consumer (weights of the next kernels of the decode chain); writes nothing. */
int dia_prefetch(const void* ptr, int64_t nbytes, int nblocks, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Persistent MLP segment (csrc/seg.hip): cross o_proj -> wi_fused + SwiGLU -> wo (-> the NEXT layer's q/k/v projection)
 * of one decoder layer in ONE launch, for M <= 4 rows (batch 1-2) of a dense Dia-1.6B-shaped decoder.  Replaces the
 * launches co, wi, wo (and the following layer's qkv) of the step = reference DecoderLayer.forward layers.py:574-584
 * (+ layers.py:541, 273-275 of the next layer).  256 workgroups, one per CU, all resident together; the weights come in
 * the "ring layout" (dia_hip/layout.py seg_ring): per CU one contiguous run of 16 KiB slots in consumption order.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* a_in;        /* cross-attention output, fp32 activation tiles [ktile][64][8] of m-tile 0 (act_f32 format) */
  int32_t a_ktiles;         /* its K/32 (= 64) */
  int32_t M;                /* valid rows, 1..4 */
  const void* W;            /* ring arena of this layer: bf16 [256][nslots][16][64][8] */
  int32_t nslots;           /* dia_seg_slots(has_qkv): 29 with the next layer's q/k/v, 26 without */
  int32_t has_qkv;
  int32_t D, F;             /* 2048, 8192 (checked) */
  float* x;                 /* residual stream [rows][ldx], updated in place */
  int32_t ldx;
  const float* g_mlp;       /* pre_mlp_norm weight [D] */
  const float* g_next;      /* next consumer's norm weight [D]: the next layer's pre_sa_norm, or the final norm */
  float* qkv_out;           /* [rows][ldq] q|k|v of the next layer (has_qkv) */
  int32_t ldq;
  float* planes_x;          /* fp32 activation tiles of x * g_next, as DIA_EPI_RESID_EMIT leaves them (launched consumers read these) */
  int32_t xkt;
  float* ssq;               /* [D/16][ssq_ld] strip sums of squares of x */
  int32_t ssq_ld;
  float eps;
  void* ws;                 /* dia_seg_workspace_bytes() bytes; the first dia_seg_workspace_control_bytes() zeroed ONCE by the caller
                             * (and again after any failed launch) */
  int32_t timeout_us;       /* bound of every in-kernel wait; 0 = 20 ms */
  void* stamps;             /* debug: int64 [256][16] wall-clock (100 MHz) stamps of every workgroup's sync wave; NULL = off */
} dia_seg_args;
int dia_seg_mlp(const dia_seg_args* a, void* stream);
int64_t dia_seg_workspace_bytes(void);
int64_t dia_seg_workspace_control_bytes(void);
int32_t dia_seg_slots(int with_qkv);
/* 1 when the shapes (D, F, attention width = heads * 128, q/k/v width) have a segment kernel and the device has the CUs */
int dia_seg_supported(int D, int F, int attn_width, int nqkv);
/* after a stream sync: 0, or the code of the in-kernel wait that timed out (1 x1, 2 hidden, 3 wo partials, 4 x2) */
int dia_seg_error(const void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Engine: owns nothing but the launch sequence.  All memory is allocated by the caller.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  const void *w_qkv, *w_o, *w_cq, *w_co, *w_wi, *w_wo;   /* weight tiles */
  const void* w_wo_diag;                                 /* NULL, or wo once more in the diagonal layout (dia_gemm_args.w_layout = 1): used at <= 4 rows */
  const float *g_sa, *g_ca, *g_mlp;                      /* RMSNorm weights [D] */
  void *k_self, *v_self;                                 /* [R][kv_heads][T][128] */
  void *k_cross, *v_cross;                               /* [B][cq_heads][S][128] */
  int32_t kt_qkv, ns_qkv, kt_o, ns_o, kt_cq, ns_cq, kt_co, ns_co, kt_wi, ns_wi, kt_wo, ns_wo;
  /* compaction maps (device int32, NULL = dense): */
  const int32_t* cmap_ca;     /* emitted by self o_proj for the cross-q input order */
  const int32_t* cmap_mlp;    /* emitted by cross o_proj for the wi_fused input order */
  const int32_t* cmap_next;   /* emitted by wo for the next layer's q/k/v input order (or the logits head's) */
  const int32_t* smap_qkv;    /* strip map of the q/k/v output */
  const int32_t* smap_cq;     /* strip map of the cross-q output */
  const int32_t* hmap_self;   /* head map of self-attention */
  const int32_t* hmap_cross;  /* head map of cross-attention */
  /* 2:4 sparse streams of the same matrices (dia_gemm_args.w_format = DIA_W_SPARSE24, KT = kt_* / 2), NULL = dense only.  A step
   * of at most 4 rows (batch 1-2) streams every matrix that has one; more rows (the dense forms are as fast there), planes between
   * the kernels (act_f32 = 0), two- or three-plane weights and the wo_diag / segment / mlp_fused experiments use the dense tiles */
  const void *w_qkv_24, *w_o_24, *w_cq_24, *w_co_24, *w_wi_24, *w_wo_24;
  /* MXFP8 streams of the same matrices (dia_gemm_args.w_format = DIA_W_MXFP8, KT = kt_*), NULL = dense only.  A step of at most 16
   * rows (batch 1-8) streams the matrices that have one and that the knob mxfp8 (csrc/tuning.hpp) enables for its row range;
   * more rows, planes between the kernels, two- or three-plane weights and the experiments use the dense tiles */
  const void *w_qkv_f8, *w_o_f8, *w_cq_f8, *w_co_f8, *w_wi_f8, *w_wo_f8;
} dia_dec_layer;

typedef struct {
  int32_t n_layer, D, F, q_heads, kv_heads, cq_heads, C, V;
  int32_t B;                /* utterances; rows R = 2B */
  int32_t T;                /* audio_length (self cache capacity, token buffer rows) */
  int32_t S;                /* text capacity of the cross caches */
  int32_t kv_dtype;
  int32_t rows_pad;         /* 16 * ceil(R/16) */
  int32_t ld_logits;        /* 16 * ceil(C*V/16) */
  float eps;
  int32_t v_blocked;        /* 1: V caches in the blocked layout (bf16 only) -> MFMA attention */
  const dia_dec_layer* layers;   /* host array [n_layer] */
  const void* w_logits;
  int32_t kt_logits, ns_logits;
  const float* g_final;
  /* scratch (device) */
  float* x;                 /* [rows_pad][D] */
  void* planes_x;           /* [3][rows_pad/16][D/32][64][8] */
  void* planes_a;           /* attention output planes, width q_heads*128 */
  void* planes_h;           /* MLP hidden planes, width F */
  float* ssq;               /* [D/16][rows_pad] */
  float* qkv;               /* [rows_pad][(q_heads+2*kv_heads)*128] */
  float* qc;                /* [rows_pad][cq_heads*128] */
  float* logits;            /* [rows_pad][ld_logits] */
  const float* cos_t;       /* [T+1][64] */
  const float* sin_t;
  const int32_t* text_len;  /* [B] */
  float* sk_scratch;        /* split-K slabs: at least (D/16)*4*512 floats; with 17..128 rows (batch 9-64) also
                             * ceil(rows/16) * (D/16) * 4 * 256 (wo splits K four ways for every m-tile) */
  int32_t* sk_tickets;      /* max(max strips, 8 * D/16) int32, zeroed by the caller once */
  float* attn_scratch;      /* max over self/cross of dia_attn_scratch_floats(...) floats */
  int32_t* attn_tickets;    /* max(R*kv_heads, B*cq_heads) int32, zeroed by the caller once */
  int64_t sk_scratch_floats;/* capacity of sk_scratch in floats (0 = the minimum above) */
  int32_t* mlp_barrier;     /* 2 int32 zeroed by the caller once: dia_mlp_fused's barrier words (NULL = never fuse) */
  int32_t act_f32;          /* 1: planes_x / planes_a / planes_h carry fp32 activation tiles (dia_gemm_args.act_f32); needs
                             * sample.embed.act_f32 == 1 */
  int32_t w_planes;         /* 0 / 1, 2: every weight pointer holds interleaved hi / lo bf16 planes of fp32 weights and every kt_* counts
                             * both (2 * K/32), or 3: three bf16 planes back to back (dia_gemm_args.w_planes) */
  dia_sample_args sample;   /* sampler + FSM + embedding parameters */
  /* persistent MLP segments (NULL / 0 = the eight-launch layer): host array [n_layer] of ring arenas (layer l's arena holds
   * co, wi, wo of layer l and, for l + 1 < n_layer, qkv of layer l + 1), used when 2B <= 4 */
  const void* const* seg_w;
  void* seg_ws;             /* workspace of dia_seg_mlp */
  int64_t kv_plane_self, kv_plane_cross;   /* DIA_KV_BF16X2: plane strides (elements) of the self / cross caches */
  const void* w_logits_24;  /* 2:4 sparse stream of the logits head (as dia_dec_layer.w_*_24: used at <= 4 rows), NULL = dense only */
  const void* w_logits_f8;  /* MXFP8 stream of the logits head (as dia_dec_layer.w_*_f8), NULL = dense only */
} dia_engine_desc;

/* The weight matrices a decode step streams, in launch order: the six of a decoder layer (each layer: qkv, self-attention, o, cq,
 * cross-attention, co, wi, wo), then the logits head (then the sampler).  The one definition of that order: the engine's launch
 * table is indexed by it, and bit m of dia_mxfp8_classes / the knob "mxfp8" is matrix m. */
enum dia_step_mat { DIA_MAT_QKV, DIA_MAT_O, DIA_MAT_CQ, DIA_MAT_CO, DIA_MAT_WI, DIA_MAT_WO, DIA_MAT_LOGITS, DIA_MAT_COUNT };

typedef struct dia_engine dia_engine;
int dia_engine_create(const dia_engine_desc* d, void* stream, dia_engine** out);
int dia_engine_destroy(dia_engine* e);
/* 1 when the engine's decode step runs the MLP as one fused launch (dia_mlp_fused: batch 1, shapes with an instantiation) */
int dia_engine_mlp_fused(const dia_engine* e);
/* enqueue `n_steps` decode steps; use_graph != 0 replays a captured hipGraph of one step */
int dia_engine_decode(dia_engine* e, int n_steps, int use_graph);
/* before the first graph decode: prefetch the weights of launch i+lookahead into the Infinity Cache
 * on a side branch of the step graph as soon as launch i has been issued (0 = off) */
int dia_engine_set_prefetch(dia_engine* e, int lookahead);
/* before the first step: a second residual buffer [rows_pad][D].  With it a step of at most 4 rows over dense one-plane weights
 * merges wo's two K slices in the launch behind it (dia_gemm_wo_deferred; knob wo_defer=0: never): the slices lie in sk_scratch
 * (2 * rows_pad * D floats), and the residual stream alternates between x (even layers) and x_alt (odd layers), because that
 * launch reads the whole old row while it writes the new one.  NULL = the in-launch merge */
int dia_engine_set_x_alt(dia_engine* e, float* x_alt);
/* enqueue ONE decode step stopping after the logits GEMM (no sampling); for per-kernel timing */
int dia_engine_step_logits_only(dia_engine* e);
/* run ONE eager decode step with a HIP event recorded on the engine's stream after every launch and
 * return the elapsed milliseconds of each launch (launch order: dia_step_mat).  Synchronises the stream. */
int dia_engine_profile_step(dia_engine* e, float* ms_per_launch, int cap);
/* run ONE eager decode step with every kernel bracketed by dispatch-level start / stop events (timestamps of the
 * dispatch packet itself): ms_per_kernel[i] = begin -> end of the i-th launch (pure execution), interval_ms[i] (may be
 * NULL) = end of launch i-1 -> end of launch i = what the launch costs inside the dependent chain, boundary included —
 * the quantity rocprofv3 --kernel-trace reports as a kernel's duration in a replayed graph (begin[i] == end[i-1] there).
 * Same order as dia_engine_profile_step.  Returns the number of kernels launched or a negative DIA_E_*.  Synchronises. */
int dia_engine_time_step(dia_engine* e, float* ms_per_kernel, float* interval_ms, int cap);
/* kernel instantiation name (as rocprofv3 prints it, without the namespace) of the i-th launch of the calling thread's
 * last dia_engine_time_step / dia_gemm_timed; "" when out of range */
const char* dia_timed_kernel_name(int i);
/* Launch classes of a decode step of `rows` rows that stream MXFP8 when the model carries the streams (dia_dec_layer.w_*_f8,
 * dia_engine_desc.w_logits_f8): bit m = matrix m of dia_step_mat.  0 above 16 rows.  The knob "mxfp8" overrides the measured
 * default (bits 0-6: at most 4 rows, bits 8-14: 5..16 rows). */
int dia_mxfp8_classes(int rows);
/* MXFP4 streams of the matrices a decode step streams (dia_gemm_args.w_format = DIA_W_MXFP4, KT = kt_* of dia_dec_layer /
 * kt_logits), handed to an engine beside its description: the description structs stay as they are.  NULL = dense only. */
typedef struct {
  const void *w_qkv, *w_o, *w_cq, *w_co, *w_wi, *w_wo;
} dia_mxfp4_layer;
typedef struct {
  int32_t n_layer;                  /* must equal dia_engine_desc.n_layer */
  int32_t _pad;
  const dia_mxfp4_layer* layers;    /* host array [n_layer], copied */
  const void* w_logits;
} dia_mxfp4_streams;
/* before the first step: a step of at most 16 rows then streams MXFP4 for the matrices that have a stream here and that
 * dia_mxfp4_classes enables, under the conditions of the MXFP8 streams (an MXFP4 stream goes before an MXFP8 one of the same
 * matrix).  NULL streams = none.  The streams hold the same numbers as the dense tiles. */
int dia_engine_set_mxfp4(dia_engine* e, const dia_mxfp4_streams* s);
/* as dia_mxfp8_classes for the MXFP4 streams and the knob "mxfp4" */
int dia_mxfp4_classes(int rows);
/* Unstructured sparse streams of the matrices a decode step streams (dia_gemm_args.w_format = DIA_W_USPARSE, KT = kt_* of
 * dia_dec_layer / kt_logits), handed to an engine beside its description as the MXFP4 streams are.  stream == NULL = dense only. */
typedef struct {
  dia_us_mat w_qkv, w_o, w_cq, w_co, w_wi, w_wo;
} dia_us_layer;
typedef struct {
  int32_t n_layer;                  /* must equal dia_engine_desc.n_layer */
  int32_t _pad;
  const dia_us_layer* layers;       /* host array [n_layer], copied */
  dia_us_mat w_logits;
} dia_us_streams;
/* before the first step (DIA_E_STATE afterwards): a step of at most 4 rows then streams the matrices that have a stream here and that
 * dia_usparse_classes enables, under the conditions of the MX streams; a 2:4 stream of the same matrix goes first, an MX stream
 * after.  NULL = none.  The streams hold the same numbers as the dense tiles. */
int dia_engine_set_usparse(dia_engine* e, const dia_us_streams* s);
/* as dia_mxfp8_classes for the unstructured sparse streams and the knob "usparse": bits 0-6 = matrices of dia_step_mat; 0 above 4 rows */
int dia_usparse_classes(int rows);
/* before the first step (DIA_E_STATE afterwards): every step then issues dia_score(a) between its logits GEMM and its sampler, eager
 * and in the captured graph, and dia_engine_launches_per_step reports one more; dia_engine_step_logits_only still ends at the
 * logits.  *a is copied; its pointers must stay valid while the engine steps.  NULL = the step without it, launch for launch.
 * Scoring is for closed teacher-forced batches: DIA_E_ARG when the engine's sample.teacher == 0 or its sampler has per-slot state,
 * and for everything dia_score refuses. */
int dia_engine_set_score(dia_engine* e, const dia_score_args* a);

/* ------------------------------------------------------------------------------------------------
 * Activation statistics for activation-aware pruning (csrc/calib.hip; DESIGN.md "Activation statistics").  The reference prunes by
 * weight magnitude alone (offline_prune.py:82-156); Wanda ranks by |W[k][n]| * ||x_k||_2 and needs, per matrix, the sum of
 * squares of every input channel over a calibration set.  One launch, for one activation plane set:
 *   acc[k] += sum over counted rows m, in ascending m, of (double)v * (double)v      k in [0, 32 * ktiles_used)
 *   v       = fl32( x[m][k] * scale[m] )
 * x[m][k] is read from fp32 tiles (act_f32 = 1: [mtile][ktile][lane][8]) or from three bf16 planes (act_f32 = 0: x = (hi + mid) + lo
 * in fp32, exact by construction).  scale[m] = 1 without ssq_in, else the row's inverse RMS as the GEMV consumers form it, in
 * fp32 with contraction off:
 *   q = 0;  for i = 0 .. ssq_in_n - 1, ascending:  q = fl32(q + ssq_in[i * ssq_ld + m]);
 *   scale[m] = 1.0f / sqrtf( fl32( fl32(q * inv_d) + eps ) )          (division and square root correctly rounded)
 * A row counts iff  (row_mask == NULL or row_mask[m] != 0)  and, with rows_per_slot == 2, the gate of dia_score holds for
 * utterance b = m / 2:  first_step[b] <= cur[b] < T, cur[b] >= 0 and fsm[b][3] == 0.  Rows m >= M (tile padding) are never read.
 * *counter advances by the number of counted rows (one thread).  One thread owns 8 consecutive channels and walks the rows in
 * order; there are no atomics and no cross-thread sums, so acc[k] has the same bits however the rows are spread over launches that
 * keep their order, and under graph replay as eager.  Nothing but acc and counter is written.
 * DIA_E_ARG with a message, before any HIP call: a null x, acc or counter; ktiles <= 0; ktiles_used outside [0, ktiles]; rows_pad
 * not a positive multiple of 16; M <= 0 or M > rows_pad; three planes with plane_stride < rows_pad * ktiles * 32; ssq_in without
 * ssq_in_n > 0 or with ssq_ld < M; rows_per_slot other than 0 and 2; the gate without cur or without T > 0; x or acc not
 * 16-byte aligned. */
typedef struct {
  const void* x;               /* plane set: fp32 tiles, or three bf16 planes plane_stride elements apart */
  int64_t plane_stride;        /* elements between the bf16 planes (act_f32 = 0) */
  int32_t ktiles;              /* k-tiles (32 channels) per m-tile of the plane set: its row pitch */
  int32_t ktiles_used;         /* k-tiles to accumulate, from 0; 0 = ktiles */
  int32_t M;                   /* rows */
  int32_t rows_pad;            /* rows the plane set holds: 16 * its m-tiles */
  int32_t act_f32;
  int32_t ssq_in_n;            /* partial sums per row */
  const float* ssq_in;         /* [ssq_in_n][ssq_ld] strip partial sums of squares, or NULL: scale 1 */
  int32_t ssq_ld;
  float inv_d;
  float eps;
  int32_t rows_per_slot;       /* 0: no gate; 2: rows 2b and 2b + 1 belong to utterance b (M <= 2 * entries of cur) */
  const uint8_t* row_mask;     /* device [M] or NULL */
  const int32_t* cur;          /* device [B] (the gate) */
  const int32_t* first_step;   /* [B] or NULL = 1 everywhere */
  const int32_t* fsm;          /* [B][8] or NULL = nobody is done */
  int32_t T;
  int32_t _pad0;
  double* acc;                 /* device [32 * ktiles_used], read and written */
  int64_t* counter;            /* device, one per call site */
} dia_act_stats_args;
int dia_act_stats(const dia_act_stats_args* a, void* stream);

/* The taps of a calibrating engine, in the order a step issues them: for layer l = 0 .. n_layer - 1 one per matrix of
 * dia_step_mat (index 6 * l + m: qkv, o, cq, co, wi, wo), then the logits head's (index 6 * n_layer).  Each is one dia_act_stats on
 * the plane set its matrix is about to contract with (PL_X with the row scale its consumer uses, PL_A, PL_H), gated as dia_score. */
typedef struct {
  int32_t n_layer;             /* must equal dia_engine_desc.n_layer */
  int32_t _pad0;
  double* const* acc;          /* host array [6 * n_layer + 1] of device arrays, copied; acc[i] holds 32 * kt[i] doubles */
  const int32_t* kt;           /* host array [6 * n_layer + 1]: k-tiles of every tap (the matrix's K / 32), copied */
  int64_t* counters;           /* device [6 * n_layer + 1] */
} dia_calib_args;
/* before the first step (DIA_E_STATE afterwards): every step then issues one dia_act_stats in front of each of its GEMMs, eager and
 * in the captured graph: 6 * n_layer + 1 more launches, which dia_engine_launches_per_step, the prefetch list and the profile walk
 * see.  A calibrating engine keeps wo's in-launch merge (under deferral the q/k/v input of layers > 0 never reaches planes_x; the
 * two forms are bit-identical).  NULL = the step without them, launch for launch.  DIA_E_ARG: an engine that is not teacher-forced
 * or whose sampler has per-slot state, compaction or strip maps on any edge, persistent segments, the knobs mlp_fuse and wo_diag,
 * a tap wider than its plane set, and everything dia_act_stats refuses for a tap. */
int dia_engine_set_calib(dia_engine* e, const dia_calib_args* a);

/* ------------------------------------------------------------------------------------------------
 * Gram matrices for error-compensated quantisation (csrc/gram.hip; DESIGN.md "Gram matrices and GPTQ").  GPTQ needs, per matrix,
 * H = X^T X / rows over the calibration rows of the GEMM's input.  One launch, for one activation plane set, read exactly as
 * dia_act_stats reads it (the same x, planes, row scale rounding by rounding, row rule; rows m >= M are never read):
 *   v[m][k]  = fl32( x[m][k] * scale[m] )
 *   G[i][j] += sum over counted rows m, in ascending m, of (double)v[m][i] * (double)v[m][j]       for j's tile <= i's tile
 * The product of two widened floats is exact in double: one rounding per element and counted row, by a VALU fma (no f64 MFMA).
 * G is packed as the lower triangle of 32 x 32 tiles, T = ktiles_used (0 = ktiles): tile (ti, tj), tj <= ti, lies at index
 * ti (ti + 1) / 2 + tj, each tile 1024 doubles row-major, G[32 ti + r][32 tj + c] at r * 32 + c.  Diagonal tiles are stored whole
 * and are symmetric bit for bit.  gram holds T (T + 1) / 2 * 1024 doubles; nothing outside them, *counter aside, is written.
 * One thread owns its patch of G and walks the rows in order: no atomics, no cross-thread sums, so G has the same bits however the
 * rows are spread over launches that keep their order, and under graph replay as eager; its diagonal is dia_act_stats's acc bit for
 * bit.  A launch that counts no row leaves G untouched (and unread).
 * DIA_E_ARG with a message, before any HIP call: everything dia_act_stats refuses (gram in the place of acc), a null gram, a gram
 * that is not 16-byte aligned, and more than 2048 k-tiles (the tile index is decoded in 32-bit arithmetic). */
typedef struct {
  const void* x;               /* the fields of dia_act_stats_args, with the same meaning ... */
  int64_t plane_stride;
  int32_t ktiles;
  int32_t ktiles_used;
  int32_t M;
  int32_t rows_pad;
  int32_t act_f32;
  int32_t ssq_in_n;
  const float* ssq_in;
  int32_t ssq_ld;
  float inv_d;
  float eps;
  int32_t rows_per_slot;
  const uint8_t* row_mask;
  const int32_t* cur;
  const int32_t* first_step;
  const int32_t* fsm;
  int32_t T;
  int32_t _pad0;
  double* gram;                /* ... and the packed matrix: device [T (T + 1) / 2][32][32], read and written */
  int64_t* counter;            /* device, one per call site */
} dia_act_gram_args;
int dia_act_gram(const dia_act_gram_args* a, void* stream);

/* The counterpart of dia_engine_set_calib for Gram matrices: the same taps in the same order (6 * l + m, the logits head last).  At
 * every tap whose gram[i] is non-NULL the step issues one dia_act_gram where a calibrating engine issues dia_act_stats; a NULL entry
 * means no launch for that tap, so a caller bounds memory by layer (kt[i] is still read and checked). */
typedef struct {
  int32_t n_layer;             /* must equal dia_engine_desc.n_layer */
  int32_t _pad0;
  double* const* gram;         /* host array [6 * n_layer + 1] of device arrays or NULL, copied; gram[i] holds kt[i] (kt[i] + 1) / 2 tiles */
  const int32_t* kt;           /* host array [6 * n_layer + 1]: k-tiles of every tap (the matrix's K / 32), copied */
  int64_t* counters;           /* device [6 * n_layer + 1] */
} dia_gram_args;
/* before the first step (DIA_E_STATE afterwards): one more launch per non-NULL tap, eager and in the captured graph, which
 * dia_engine_launches_per_step, the prefetch list and the profile walk see; wo's in-launch merge is kept.  NULL = the step without
 * them, launch for launch.  DIA_E_ARG: everything dia_engine_set_calib refuses, an engine that already has dia_engine_set_calib (the
 * Gram's diagonal is the same statistic, bit for bit), and everything dia_act_gram refuses for a tap. */
int dia_engine_set_gram(dia_engine* e, const dia_gram_args* a);
/* number of kernel launches in one decode step */
int dia_engine_launches_per_step(const dia_engine* e);

/* ------------------------------------------------------------------------------------------------
 * Per-request LoRA adapters, unmerged (csrc/lora.hip; DESIGN.md "Per-request adapters").  The reference wraps the model with
 * PEFT for ONE adapter per process (cli.py:166-174); here several adapters stay resident beside the base weights and every row
 * of a projection's output receives the correction of the adapter its slot selected:
 *   out[m][col_off + n] += scale[a] * sum_j B_a[j][n] * sum_k A_a[j][k] * xn[m][k],   a = adapter_of_slot[slot(m)],
 * nothing for a < 0.  xn[m] = x[m] * gain * rsqrt(mean(x[m]^2) + eps) is rebuilt from the fp32 residual row, so the call does not
 * depend on the activation format between the GEMMs.  Everything below is appended: no existing struct or entry point changed.
 * ------------------------------------------------------------------------------------------------ */
#define DIA_LORA_MAX_RANK 64
#define DIA_LORA_MAX_SEGS 3
/* One adapted module = one column range of the output.  The tables are DEVICE arrays indexed by adapter: A[a] -> fp32
 * [rank[a]][D] (PEFT's lora_A.weight), B[a] -> fp32 [rank[a]][n_cols] (lora_B.weight transposed: the DenseGeneral order
 * [in, out]), both 16-byte aligned, NULL or rank 0 = this adapter leaves the module alone; scale[a] = lora_alpha / r. */
typedef struct {
  int32_t col_off;             /* first output column, a multiple of 4 */
  int32_t n_cols;              /* width, a multiple of 4 */
  const float* const* A;       /* device [n_adapters] of device pointers */
  const float* const* B;
  const int32_t* rank;         /* device [n_adapters], each 0..DIA_LORA_MAX_RANK */
  const float* scale;          /* device [n_adapters] */
  int32_t max_rank;            /* the caller's statement of the largest entry of rank[]: above DIA_LORA_MAX_RANK -> DIA_E_ARG (the
                                * kernel skips such an entry) */
  int32_t _pad0;
} dia_lora_seg;
/* The SCALE_STORE sites (q/k/v of the decoder's and the encoder's self-attention, the cross-attention query): ONE launch, in
 * stream order behind the projection's dia_gemm and before whatever reads `out`.  One workgroup per (row, segment); segments must
 * not overlap.  D a multiple of 256, at most 2048.  DIA_E_ARG with a message for everything else that is refused. */
typedef struct {
  const float* x;              /* fp32 residual rows [M][ldx] the projection's input was normed from */
  int32_t ldx;
  int32_t D;
  const float* gain;           /* the consumer's RMSNorm weight [D] */
  float eps;
  int32_t M;                   /* rows */
  const int32_t* row_slot;     /* device [M]: slot (utterance) of row m, < 0 = skipped; NULL: slot = m / rows_per_slot */
  int32_t rows_per_slot;       /* 2 for the decode step's rows 2b + {0, 1} */
  int32_t n_slots;
  const int32_t* adapter_of_slot;   /* device [n_slots]: adapter index or < 0 = base model */
  int32_t n_adapters;
  int32_t n_segs;              /* 1..DIA_LORA_MAX_SEGS */
  dia_lora_seg seg[DIA_LORA_MAX_SEGS];
  float* out;                  /* [M][ldo], updated in place */
  int32_t ldo;
  int32_t _pad0;
} dia_lora_args;
int dia_lora_apply(const dia_lora_args* a, void* stream);
/* The cross K/V projections (DIA_EPI_CROSSKV stored RoPE(K) and V into the caches): adds RoPE(dK) and dV to the cache rows of the
 * packed rows' utterances, in stream order behind that dia_gemm.  The cache arguments are dia_gemm_args' (one layer); row m belongs
 * to utterance row_b[m] (< 0 = skipped) at position m - seg_off[row_b[m]], both NULL = utterance kv_batch_index, position m; the
 * adapter is adapter_of_slot[utterance].  f32: read, add, store; bf16: read, add in fp32, round once; bf16x2: hi + lo, add, split
 * again.  k / v: the segments (col_off unused, n_cols = kv_heads * 128, columns in checkpoint order [head][128]). */
typedef struct {
  const float* x;              /* encoder output rows before the final norm [M][ldx] */
  int32_t ldx;
  int32_t D;
  const float* gain;           /* encoder.norm weight [D] */
  float eps;
  int32_t M;
  const int32_t* row_b;
  const int32_t* seg_off;
  const int32_t* adapter_of_slot;   /* device [n_slots] */
  int32_t n_slots;
  int32_t n_adapters;
  dia_lora_seg k, v;
  void* kc;
  void* vc;
  int32_t kv_dtype, kv_heads, kv_cap, kv_batch_index;
  int32_t kv_vblocked;
  int32_t rope_rows;           /* rows of cos_t / sin_t (positions at or beyond it are skipped) */
  int64_t kv_plane_stride;
  const float* cos_t;
  const float* sin_t;
} dia_lora_crosskv_args;
int dia_lora_crosskv(const dia_lora_crosskv_args* a, void* stream);
/* The two decode-step sites of one decoder layer: self-attention q / k / v (column ranges of dia_engine_desc.qkv) and the
 * cross-attention query (dia_engine_desc.qc); n_cols == 0 = module not adapted by any adapter of the bank. */
typedef struct {
  dia_lora_seg q, k, v, cq;
} dia_lora_layer;
typedef struct {
  int32_t n_layer;                   /* must equal dia_engine_desc.n_layer */
  int32_t n_adapters;
  const dia_lora_layer* layers;      /* host array [n_layer], copied */
  const int32_t* adapter_of_slot;    /* device int32 [B]: written by the caller in stream order (admission / retirement), read by every step */
} dia_lora_step;
/* before the first step (DIA_E_STATE afterwards): every step then issues one dia_lora_apply behind each layer's q/k/v projection
 * (before self-attention) and one behind its cross-query projection (before cross-attention), eager and in the captured graph;
 * dia_engine_launches_per_step reports 2 * n_layer more, and the prefetch walk and dia_engine_profile_step follow.  The rows read
 * are the residual stream the projection consumed (x, or x_alt on odd layers while wo's merge is deferred) with g_sa / g_ca.
 * DIA_E_ARG for a compacted model (strip or compaction maps on either site), persistent segments and everything dia_lora_apply
 * refuses.  NULL = the step without it, launch for launch. */
int dia_engine_set_lora(dia_engine* e, const dia_lora_step* s);

/* ------------------------------------------------------------------------------------------------
 * FP8 cross K/V (csrc/attn.hip; DESIGN.md "FP8 cross K/V").  The cross caches are written once per request and read on every
 * step: a second, OCP e4m3 copy of them (finite max 448) with one power-of-two scale per key and head halves what the step reads.
 * The bf16 cross caches stay as they are (the cross-K/V GEMM, dia_lora_crosskv and the prompt prefill keep writing / reading
 * them); the copy is made from them by dia_kv_quantize_fp8 and read by dia_attn_cross_fp8.  The reference has no counterpart
 * (its cross caches are bf16 or fp32 tensors, state.py:142-151).  Everything below is appended: no existing struct or entry point
 * changed.
 *   k8  uint8 [B][heads][S][128]          row layout of the bf16 K cache
 *   v8  uint8 [B][heads][S/32][128][32]   the blocked V layout (dia_attn_args.v_blocked)
 *   ks, vs  float [B][heads][S]           scale of key s: the smallest 2^e (e >= -126) with amax / 2^e <= 448 over the key's 128
 *                                         values, 1 for an all-zero key; value = e4m3(byte) * scale, rounded to nearest even
 * All four zero-initialised once by the caller (a zero byte times any finite scale is 0).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  void* k8;
  void* v8;
  float* ks;
  float* vs;
} dia_kv_fp8_ptrs;
/* ONE launch quantises the bf16 cross K and V of the listed cache rows (utterances / slots), in stream order behind whatever wrote
 * them: row[i] gets len[i] keys, always in WHOLE 32-key granules — keys from len[i] to the end of its last granule receive zero
 * bytes and scale 1, so a masked key of a re-used slot never contributes a stale NaN pattern.  Granules behind that and rows that
 * are not listed are not touched.  n_layer > 1: the same rows of n_layer layers whose caches lie kv_layer_stride ELEMENTS apart
 * (kc / vc) and f8_layer_stride elements apart (k8 / v8; ks / vs: f8_layer_stride / 128 floats).  The row and length lists are
 * HOST arrays read during the call (they travel as kernel arguments); at most DIA_SLOTS_PER_CALL rows per call. */
typedef struct {
  const void* kc;              /* bf16 [B][heads][S][128] */
  const void* vc;              /* bf16 [B][heads][S/32][128][32] */
  dia_kv_fp8_ptrs out;         /* (of the first layer) */
  int32_t B, heads, S;         /* S a multiple of 32 */
  int32_t n;                   /* rows in this call, 1..DIA_SLOTS_PER_CALL */
  const int32_t* row;          /* host [n], distinct, each < B */
  const int32_t* len;          /* host [n], each in [0, S] */
  int32_t n_layer;             /* 0 or 1: one layer */
  int32_t _pad0;
  int64_t kv_layer_stride;     /* n_layer > 1: at least B * heads * S * 128, a multiple of 8 */
  int64_t f8_layer_stride;     /* n_layer > 1: at least B * heads * S * 128, a multiple of 2048 */
} dia_kv_fp8_args;
int dia_kv_quantize_fp8(const dia_kv_fp8_args* a, void* stream);
/* dia_attn for DIA_ATTN_CROSS over the e4m3 copy: the MFMA kernel of the one-plane bf16 caches with 8-byte K and V fragments
 * expanded to bf16 in registers and the scales folded in behind the MFMAs (score * ks before the softmax scale, p * vs before p is
 * split for P.V) — bit for bit what dia_attn computes over bf16 caches holding the dequantised values, with the same key split.
 * *a describes the launch as for dia_attn (kc / vc: the bf16 caches, validated, not read).  Refused with DIA_E_ARG: anything but
 * mode == DIA_ATTN_CROSS, group == 1, v_blocked, kv_dtype == DIA_KV_BF16 and kv_cap % 32 == 0, and what dia_attn refuses. */
int dia_attn_cross_fp8(const dia_attn_args* a, const dia_kv_fp8_ptrs* p, void* stream);
/* before the first step (DIA_E_STATE afterwards): the step's cross-attention launch of layer l is dia_attn_cross_fp8 over
 * layers[l] from then on, launch for launch in the place of dia_attn.  DIA_E_ARG unless the engine has bf16 K/V with blocked V
 * and S % 32 == 0.  NULL = dia_attn over the bf16 caches, as without the call. */
int dia_engine_set_cross_fp8(dia_engine* e, const dia_kv_fp8_ptrs* layers /* host [n_layer], copied */);

/* ------------------------------------------------------------------------------------------------
 * FP8 self K/V (csrc/attn.hip; DESIGN.md "FP8 self K/V").  The self caches are the K/V traffic that grows with every step and the
 * largest allocation of a session.  In this mode a layer's self cache IS four buffers in the format above with the self shapes —
 * there is no bf16 cache beside them:
 *   k8  uint8 [R][kv_heads][T][128]         v8  uint8 [R][kv_heads][T/32][128][32]         ks, vs  float [R][kv_heads][T]
 * (0.516 of the bf16 bytes), all four zero-initialised once by the caller.  The step's new key is quantised as it is appended, by
 * the rule of dia_kv_quantize_fp8 applied to the fp32 RoPE(k) and the fp32 v.  Every byte the append writes is a finite e4m3 value,
 * so a key that is masked (not yet written, or left over from an earlier request in a re-used slot) contributes 0 x finite.  The
 * reference has no counterpart (its self caches are bf16 or fp32 tensors, state.py:99-103).  Appended: no existing struct or entry
 * point changed.
 * ------------------------------------------------------------------------------------------------ */
/* dia_attn for DIA_ATTN_SELF over e4m3 self caches: the MFMA kernel of the one-plane bf16 caches with the 8-byte fragments and
 * folded-in scales of dia_attn_cross_fp8, for 1, 2 or 4 query heads per kv head.  The wave that owns slot cur - 1 ropes the new k,
 * quantises k and v and writes 128 + 128 bytes and two scales (and patches its own fragments, bytes and scales, from a copy in
 * LDS).  With a new key that quantises to itself the outputs equal dia_attn's over bf16 caches holding the dequantised values bit
 * for bit, with the same key split.  *a describes the launch as for dia_attn; kc / vc are not read and may be NULL.  Refused with
 * DIA_E_ARG: anything but mode == DIA_ATTN_SELF, kv_dtype == DIA_KV_BF16, v_blocked, kv_cap % 32 == 0, a cur, group 1 / 2 / 4,
 * k8 / v8 aligned to 8 bytes and ks / vs to 4, scratch and tickets when kv_cap > 128, and what dia_attn refuses. */
int dia_attn_self_fp8(const dia_attn_args* a, const dia_kv_fp8_ptrs* p, void* stream);
/* before the first step (DIA_E_STATE afterwards): the step's self-attention launch of layer l is dia_attn_self_fp8 over layers[l]
 * from then on, launch for launch in the place of dia_attn; dia_dec_layer.k_self / v_self are not read and may be NULL.
 * DIA_E_ARG unless the engine has one-plane bf16 K/V (DIA_KV_BF16) with blocked V and T % 32 == 0.  Independent of
 * dia_engine_set_cross_fp8: either, both or neither.  NULL = dia_attn over the bf16 caches, as without the call. */
int dia_engine_set_self_fp8(dia_engine* e, const dia_kv_fp8_ptrs* layers /* host [n_layer], copied */);
/* The batched prompt prefill onto e4m3 self caches (csrc/prefill.hip; DESIGN.md "Prompt prefill at admission and onto fp8 caches"):
 * dia_dec_prefill_kv / dia_dec_prefill_attn (causal) with *p in the place of kc / vc, same packing (row_seg / seg_off / seg_len /
 * seg_row, rows % 32 == 0).  dia_dec_prefill_kv_fp8 appends every packed row r of a segment to key slot r of the segment's cache row,
 * quantised by the step's own arithmetic (fp32 RoPE(k) at position r + 1 and fp32 v, amax over the 128 dims, power-of-two scale,
 * e4m3 bytes held finite): the bytes and scales dia_attn_self_fp8 would have written at cur = r + 1 for the same qkv row.  No
 * byte or scale outside key slots [0, seg_len) of the listed cache rows changes; padding rows write nothing.
 * dia_dec_prefill_attn_fp8 is the causal dia_dec_prefill_attn with 8-byte fragments and the scales folded in behind the MFMAs:
 * bit for bit its output over bf16 caches holding the dequantised values.  The cross call of a prefill stays
 * dia_dec_prefill_attn (the cross caches are bf16 under either cache mode).  Refused with DIA_E_ARG before any launch: a NULL
 * argument or fp8 pointer, kc / vc not NULL, causal == 0, kv_cap % 32 != 0, k8 / v8 not aligned to 16 bytes or ks / vs to 4, and
 * what dia_dec_prefill_kv / _attn refuse.  Appended: no struct grew. */
int dia_dec_prefill_kv_fp8(const dia_dec_prefill_args* a, const dia_kv_fp8_ptrs* p, void* stream);
int dia_dec_prefill_attn_fp8(const dia_dec_prefill_args* a, const dia_kv_fp8_ptrs* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Codec (csrc/codec.hip; DESIGN.md "Codec"): the Descript Audio Codec decoder, codes [B, 9, T] -> waveform, in exact fp32 on the
 * f32-input MFMA (reference dia/audio.py:166-185: quantizer.from_codes, then decode).  Three new entry points and two new structs;
 * nothing older changed.  Activations are fp32 [B][C][ld] with time contiguous; the batch stride is C * ld.  Every row b carries
 * its own length lens[b] (device int32, clamped to [0, T]; NULL = T for every row): positions at or beyond it read as zero padding
 * and are not written, so a row of a batch comes out bit for bit as when launched alone.
 *
 * Weights are prepared by the host (dia_hip/codec.py, weight norm folded in float64), TAP-MAJOR with the output channel contiguous:
 *   dia_codec_conv   w float [k][C_in][Cp]        w[j][ci][co] = weight[co][ci][j];             Cp = C_out rounded up to 32, zero-filled
 *   dia_codec_convt  w float [s][2][C_in][Cp]     w[r][0][ci][co] = weight[ci][co][r], w[r][1][ci][co] = weight[ci][co][r + s]
 * Snake on the INPUT, x + sin(alpha x)^2 * inv, is applied once per staged element when `alpha` is set; `inv` holds
 * 1 / (alpha + 1e-9) per input channel (both or neither).
 * ------------------------------------------------------------------------------------------------ */
#define DIA_CODEC_MAX_CHANNELS 4096
#define DIA_CODEC_MAX_T (1 << 24)
#define DIA_CODEC_MAX_CODEBOOKS 16
typedef struct {
  const int32_t* codes;        /* [B][n_codebooks][ld_codes]; ids are clamped into [0, codebook_size) */
  const int32_t* lens;         /* device [B] or NULL */
  int32_t B, T;
  int32_t n_codebooks, codebook_size, latent_dim, ld_codes;
  const float* tables;         /* [n_codebooks][codebook_size][latent_dim]: out_proj_i(codebook_i[id]) without its bias */
  const float* bias;           /* [latent_dim]: the out_proj biases summed */
  float* z;                    /* [B][latent_dim][ldz] */
  int32_t ldz, _pad0;
} dia_codec_embed_args;
/* z[b][c][t] = bias[c] + sum_i tables[i][codes[b][i][t]][c] for t < lens[b] */
int dia_codec_embed(const dia_codec_embed_args* a, void* stream);

typedef struct {
  const float* x;              /* [B][C_in][ldx] */
  const float* w;              /* layout above */
  const float* bias;           /* [C_out] */
  const float* alpha;          /* [C_in] or NULL: Snake on the input */
  const float* inv;            /* [C_in], with alpha */
  const float* res;            /* [B][C_out][ldy] or NULL: added in the epilogue; may be y itself (dia_codec_conv only) */
  float* y;                    /* [B][C_out][ldy]; never x */
  const int32_t* lens;         /* device [B] or NULL: INPUT lengths */
  int32_t B, T;                /* T: input positions per row (grid extent and clamp of lens) */
  int32_t C_in, C_out, ldx, ldy;
  int32_t k, dilation;         /* dia_codec_conv: k 1 (dilation 1) or 7 (dilation 1, 3, 9), "same" padding */
  int32_t stride;              /* dia_codec_convt: 2, 4 or 8 (kernel 2 * stride, padding stride / 2: output length T * stride); else 0 */
  int32_t tanh_out;            /* tanh behind bias and residual */
} dia_codec_conv_args;
/* y[b][co][t] = bias[co] + sum_{ci, j} w[j][ci][co] * f(x[b][ci][t + (j - k / 2) * dilation]) (+ res) (tanh), t < lens[b] */
int dia_codec_conv(const dia_codec_conv_args* a, void* stream);
/* y[b][co][o] = bias[co] + sum_{ci} w[r][0][ci][co] * f(x[b][ci][m]) + w[r][1][ci][co] * f(x[b][ci][m - 1]),
 * o + stride / 2 = m * stride + r, o < lens[b] * stride.  res must be NULL. */
int dia_codec_convt(const dia_codec_conv_args* a, void* stream);

/* Encode side (DESIGN.md "Codec: encode side"): waveform -> codes [B, 9, T].  Two more entry points and one more struct; the three
 * above are unchanged.  The encoder's k-7 and 1x1 layers are dia_codec_conv; its two other forms are dia_codec_convs, over the same
 * dia_codec_conv_args and the same rules for `lens`:
 *   stride 2, 4 or 8 (k = 0 or 2 * stride, padding stride / 2): T and lens count INPUT positions, T % stride == 0, the output row
 *     has lens[b] / stride positions;  w float [2][C_in * stride][Cp], w[t][ci * stride + r][co] = weight[co][ci][r + t * stride]:
 *     y[b][co][o] = bias[co] + sum_{ci, r, t} w[t][ci * stride + r][co] * f(x[b][ci][(o + t) * stride + r - stride / 2])
 *   stride 0, k = 3 (padding 1): w float [3][C_in][Cp] as for dia_codec_conv.
 * dilation is 0 or 1, res must be NULL, tanh_out as above. */
int dia_codec_convs(const dia_codec_conv_args* a, void* stream);

#define DIA_CODEC_MAX_CODEBOOK_SIZE 4096
typedef struct {
  const float* z;              /* [B][latent_dim][ldz]: the encoder's latent */
  const int32_t* lens;         /* device [B] or NULL: frames per row */
  int32_t B, T;
  int32_t n_codebooks, codebook_size, codebook_dim /* 1..32 */, latent_dim;
  int32_t ldz, ld_codes;
  const float* in_w;           /* [n_codebooks][codebook_dim][latent_dim]: in_proj, weight norm folded */
  const float* in_b;           /* [n_codebooks][codebook_dim] */
  const float* codebook;       /* [n_codebooks][codebook_size][codebook_dim]: rows L2-normalised (eps 1e-12) */
  const float* codebook_sq;    /* [n_codebooks][codebook_size]: |normalised row|^2 */
  const float* tables;         /* [n_codebooks][codebook_size][latent_dim]: as dia_codec_embed's */
  const float* bias;           /* [n_codebooks][latent_dim]: out_proj bias PER codebook */
  int32_t* codes;              /* [B][n_codebooks][ld_codes]; frames at or beyond lens[b] are not written */
} dia_codec_quantize_args;
/* the residual VQ search, all stages in one launch; per frame, residual = z[b][:][t], and for i in 0 .. n_codebooks - 1:
 *   z_e = in_w[i] residual + in_b[i];  e = z_e / max(|z_e|, 1e-12);  codes[b][i][t] = argmin_j |e|^2 - 2 e . codebook[i][j] +
 *   codebook_sq[i][j], the LOWEST j among equal distances;  residual -= tables[i][j] + bias[i].
 * The residual stays on chip between the stages. */
int dia_codec_quantize(const dia_codec_quantize_args* a, void* stream);

/* Reduced-precision decoder convolutions (csrc/codec_bf16.hip; DESIGN.md "Codec: bf16 modes").  Two more entry points; no struct
 * grew and nothing older changed.  dia_codec_conv_bf16 / dia_codec_convt_bf16 are dia_codec_conv / dia_codec_convt over the same
 * dia_codec_conv_args (fp32 activations in and out, the same `lens` rules, bias, residual, tanh) on v_mfma_f32_32x32x16_bf16:
 * only the MFMA operands are reduced.  planes = 1 ("bf16"): weight and staged input (after Snake, computed in fp32 as above) are
 * rounded to bf16, round-to-nearest-even, and one product w_hi x_hi is formed.  planes = 2 ("bf16x2"): both operands also carry
 * lo = bf16(v - hi) (the subtraction is exact in fp32) and the products w_hi x_hi, w_hi x_lo, w_lo x_hi are accumulated in that
 * order per (16-channel chunk, tap); w_lo x_lo is dropped: at most 2^-16 of sum |w| |x| (a lo is at most 2^-8 of its value), measured
 * 2^-17.6 of it for sums of a dozen terms down to 2^-22 for the 5376 of the widest layers.  Accumulation is fp32.  The order depends on nothing
 * but (channel chunk, tap, product), so rows, windows and streamed chunks are bitwise reproducible within a mode.
 *
 * a->w points at a bf16 image the host prepares from the float64-folded fp32 weight (dia_hip/codec.py conv_layout_bf16 /
 * convt_layout_bf16), 16-byte aligned; Ci = C_in rounded up to 16, Cp = C_out rounded up to 32, both zero-filled; 8 input channels
 * contiguous per (tap, output channel), so that a lane's A fragment is one 16-byte read:
 *   dia_codec_conv_bf16   w bf16 [planes][k][Ci / 8][Cp][8]       w[p][j][g][co][u] = plane_p(weight[co][8 g + u][j])
 *   dia_codec_convt_bf16  w bf16 [planes][s][2][Ci / 8][Cp][8]    w[p][r][t][g][co][u] = plane_p(weight[8 g + u][co][r + t s])
 * plane_0 = hi, plane_1 = lo.  Refused with DIA_E_ARG before any launch: planes not 1 or 2, and what dia_codec_conv /
 * dia_codec_convt refuse. */
int dia_codec_conv_bf16(const dia_codec_conv_args* a, int planes, void* stream);
int dia_codec_convt_bf16(const dia_codec_conv_args* a, int planes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Resampler (csrc/resample.hip; DESIGN.md "Resampler"): polyphase sample-rate conversion of a batch of rows in ONE launch.  One
 * new entry point and one new struct; nothing older changed.
 *
 * The rates are reduced to o : n (input : output samples per period).  Output m = q * n + p of a signal x of `total` samples is
 *   y[m] = sum_{k = 0 .. nt - 1} bank[k][p] * x[q * o + first[p] + k],      x = 0 outside [0, total)
 * an fp32 fma chain from 0 in ascending k: the order depends on (o, n, nt, first, bank) alone, never on the row, the tile or the
 * window, so an output has the same bits however the signal is cut into rows, windows and launches.
 *
 * A row is a WINDOW of a longer signal: it holds input samples [in_start, in_start + in_count) at x[b][0 ..] and receives
 * outputs [out_start, out_start + out_count) at y[b][0 ..].  Absolute indices are 64-bit and stay on the host: the kernel gets
 * them reduced to (q, p) of the first output and a 32-bit offset.  A tap outside the window reads as ZERO (that is right outside
 * [0, total); the caller sees to it that no tap inside the signal falls outside the window — dia_hip/resample.py checks before it
 * launches); memory outside x[b][0 .. in_count) is never read, memory outside y[b][0 .. out_count) never written.
 * ------------------------------------------------------------------------------------------------ */
#define DIA_RESAMPLE_MAX_ROWS 64           /* rows of one launch */
#define DIA_RESAMPLE_MAX_T (1 << 24)       /* ldx, ldy */
#define DIA_RESAMPLE_MAX_TAPS 4096         /* nt */
#define DIA_RESAMPLE_TILE 1024             /* consecutive outputs of one workgroup */
#define DIA_RESAMPLE_MAX_TILE_FLOATS 16000 /* its staged input span, ceil((TILE - 1) * o / n) + 2 + nt floats of LDS: DIA_E_ARG above */
#define DIA_RESAMPLE_OPEN (-1)             /* total[b] of a running stream: the signal has no end yet */
typedef struct {
  const float* x;              /* device [B][ldx] */
  float* y;                    /* device [B][ldy]; never x */
  const float* bank;           /* device [nt][n]: tap-major, the phase contiguous */
  const int32_t* first;        /* device [n]: tap 0 of phase p sits at input q * o + first[p]; nondecreasing, first[n - 1] <= first[0] + o */
  int32_t B, ldx, ldy;
  int32_t o, n, nt;
  const int64_t* in_start;     /* HOST [B], read during the call (as the four below): absolute index of x[b][0], >= 0 */
  const int64_t* out_start;    /* HOST [B]: absolute index of y[b][0], >= 0 */
  const int64_t* total;        /* HOST [B]: the signal's length, or DIA_RESAMPLE_OPEN */
  const int32_t* in_count;     /* HOST [B]: 0 .. ldx */
  const int32_t* out_count;    /* HOST [B]: 0 .. ldy */
} dia_resample_args;
int dia_resample(const dia_resample_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Audio distance (csrc/spectral.hip; DESIGN.md "Audio distance"): the magnitude spectrogram or the mel spectrogram of ONE
 * resolution of a ragged batch of rows in ONE launch, and the L1 terms between two batches.  One new entry point and one new
 * struct; nothing older changed.
 *
 * A row of len >= 1 samples has F = 1 + len / H frames, H = window / 4.  Frame f is centred at sample f * H; samples outside
 * [0, len) read as ZERO (torch.stft(center=True, pad_mode="constant")).  With nbin = window / 2 + 1,
 *   X[f][k]   = sum_n basis[n][0][k] * x[f H - window / 2 + n]  +  i sum_n basis[n][1][k] * x[...]      k = 0 .. window / 2
 *   mag[f][k] = |X[f][k]|
 *   mel[f][m] = sum_k fb[m][k] * mag[f][k]        an fp32 fma chain from 0 over k in [fb_range[m][0], fb_range[m][1]), ascending
 * The basis holds the window: basis[n][0][k] = w[n] cos(2 pi n k / window), basis[n][1][k] = -w[n] sin(2 pi n k / window).  The
 * sums over n run on the exact-fp32 MFMA: two samples to a step, each step's fp32 sum of two products added in float64 in
 * ascending n; mag is the float64 root of the two sums, rounded to fp32.  S = mag when n_mels == 0, else mel.
 *
 * b != NULL (distance): partial[r][t] receives, for tile t of DIA_SPECTRAL_TILE_FRAMES consecutive frames of row r,
 *   [0] sum |Sa - Sb|    [1] sum power * |log10 max(Sa, eps) - log10 max(Sb, eps)|
 * over the tile's frames < F and all bins (or mels), in float64 and in an order that depends on the tile alone.  The caller adds
 * the tiles of a row in its own fixed order and divides by F * (nbin or n_mels).  Tiles at or beyond a row's last are not written.
 * b == NULL (spectra only): out[r][f][.] receives S of row r, f < F; nothing else of out is written.
 * Either way an element has the same bits whichever row of whichever batch it is computed in.
 *
 * Refused with DIA_E_ARG before any HIP call: a null args / a / basis / len; window not a power of two in [32, 2048]; n_mels
 * outside [0, 320], or > 0 without fb and fb_range; B outside [1, 64]; ld outside [1, 1 << 24]; a len outside [1, ld]; power not
 * 1 or 2; eps not positive; b without partial, or tiles below the tiles of the longest row; no b and no out, or out_frames below
 * the frames of the longest row.
 * ------------------------------------------------------------------------------------------------ */
#define DIA_SPECTRAL_MAX_ROWS 64           /* rows (row pairs) of one launch */
#define DIA_SPECTRAL_MAX_T (1 << 24)       /* ld */
#define DIA_SPECTRAL_MIN_WINDOW 32
#define DIA_SPECTRAL_MAX_WINDOW 2048
#define DIA_SPECTRAL_MAX_MELS 320
#define DIA_SPECTRAL_TILE_FRAMES 16        /* frames of one partial */
typedef struct {
  const float* a;              /* device [B][ld] */
  const float* b;              /* device [B][ld], or NULL: spectra only */
  const float* basis;          /* device [window][2][window / 2 + 1] */
  const float* fb;             /* device [n_mels][window / 2 + 1]; unused when n_mels == 0 */
  const int32_t* fb_range;     /* device [n_mels][2]: the bins [lo, hi) outside which row m of fb is zero (clamped to [0, nbin]) */
  double* partial;             /* device [B][tiles][2]; required with b */
  float* out;                  /* device [B][out_frames][window / 2 + 1 or n_mels]; required without b */
  int32_t B, ld, window, n_mels;
  int32_t tiles;               /* second extent of partial: at least ceil(F / DIA_SPECTRAL_TILE_FRAMES) of the longest row */
  int32_t out_frames;          /* second extent of out: at least F of the longest row */
  int32_t power;               /* 1 or 2: the p of log10(max(S, eps)^p) */
  int32_t _pad0;
  double eps;
  const int32_t* len;          /* HOST [B], read during the call: 1 .. ld */
} dia_spectral_args;
int dia_spectral(const dia_spectral_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Speed factor (csrc/timescale.hip; DESIGN.md "Speed factor"): time-scaling of a batch of rows, by linear interpolation (the
 * reference application's np.interp over np.linspace, which moves the pitch) or by WSOLA (waveform-similarity overlap-add, which
 * keeps it).  One new entry point and one new struct; nothing older changed.
 *
 * A row is a WINDOW of a longer signal x of `total` samples, as in dia_resample_args: it holds input samples
 * [in_start, in_start + in_count) at x[b][0 ..] and receives outputs [out_start, out_start + out_count) at y[b][0 ..].  x reads as
 * ZERO outside [0, total) and outside the window (the caller sees to it that nothing inside the signal that the row needs lies
 * outside the window: dia_hip/timescale.py checks before it launches); memory outside x[b][0 .. in_count) is never read, memory
 * outside y[b][0 .. out_count) and delta[b][0 .. k1 - k0) never written.
 *
 * DIA_TS_INTERP: the signal has N = total[b] samples and M = out_total[b] outputs.  Output j (absolute) is
 *   pos = j == M - 1 ? N - 1 : (double)(j * (N - 1)) / (M - 1)        (0 when M == 1)
 *   i   = min(floor(pos), N - 2),    y[j] = (float)(((double)x[i + 1] - x[i]) * (pos - i) + x[i])        (x[0] when N == 1)
 * total must be a length (not open); window, tolerance, win, centre, delta, k0, k1, delta_prev and ldk are not read.
 *
 * DIA_TS_WSOLA: W = window, D = tolerance, Hs = W / 2; frame k is centred at output k * Hs and nominally at input c_k.  The row
 * searches frames [k0, k1): centre[b][i] holds c_{k0 - 1 + i} - in_start for i = 0 .. k1 - k0 (entry 0 is not read when k0 == 0),
 * delta_prev[b] is delta of frame k0 - 1.  With p_k = c_k + delta_k - Hs:
 *   delta_0 = 0;  for k >= 1  delta_k = arg max over d in [-D, D] of corr(d) = sum_{n < W} x[p_{k-1} + Hs + n] * x[c_k + d - Hs + n]
 * every corr(d) ONE fp32 fma chain from 0 in ascending n, so its bits depend on the samples alone; among equal maxima the smallest
 * |d| wins, then the negative one; a NaN never wins (all NaN: 0).  delta[b][i] receives delta_{k0 + i}.  Then output m, which must
 * lie in [(k0 - 1) * Hs, (k1 - 1) * Hs), has the two frames ka = m / Hs and ka + 1:
 *   nb = m - ka * Hs, na = nb + Hs,   y[m] = fmaf(win[nb], x[p_{ka + 1} + nb], win[na] * x[p_ka + na])
 * The search of a row is sequential in k: one workgroup per row.  total[b] may be DIA_TS_OPEN; out_total is not read.
 *
 * Refused with DIA_E_ARG before any HIP call: a null args / x / y or a null host array; a mode other than the two; B outside
 * [1, 64]; ldx or ldy outside [1, 1 << 24]; in_count outside [0, ldx]; out_count outside [0, ldy]; negative in_start / out_start;
 * a total that is neither a length nor DIA_TS_OPEN.  INTERP: an open total, out_total < 1, outputs beyond out_total.  WSOLA:
 * null win / centre / delta; window not a power of two in [64, 4096]; tolerance outside [0, window]; ldk < 1; k0 < 0; k1 < k0;
 * k1 - k0 > ldk; outputs outside the frames' range.
 * ------------------------------------------------------------------------------------------------ */
#define DIA_TS_INTERP 0
#define DIA_TS_WSOLA 1
#define DIA_TS_MAX_ROWS 64                 /* rows of one launch */
#define DIA_TS_MAX_T (1 << 24)             /* ldx, ldy */
#define DIA_TS_MIN_WINDOW 64
#define DIA_TS_MAX_WINDOW 4096
#define DIA_TS_OPEN (-1)                   /* total[b] of a running stream: the signal has no end yet */
typedef struct {
  const float* x;              /* device [B][ldx] */
  float* y;                    /* device [B][ldy]; never x */
  const float* win;            /* device [window]: the periodic Hann window 0.5 - 0.5 cos(2 pi n / window), rounded once from float64 */
  const int32_t* centre;       /* device [B][ldk + 1]: c_k - in_start of frames k0 - 1 .. k1 */
  int32_t* delta;              /* device [B][ldk]: receives delta of frames k0 .. k1 - 1 */
  int32_t mode;                /* DIA_TS_INTERP / DIA_TS_WSOLA */
  int32_t B, ldx, ldy, ldk;
  int32_t window, tolerance;
  int32_t _pad0;
  const int64_t* in_start;     /* HOST [B], read during the call (as all below): absolute index of x[b][0], >= 0 */
  const int64_t* out_start;    /* HOST [B]: absolute index of y[b][0], >= 0 */
  const int64_t* total;        /* HOST [B]: the signal's length N, or DIA_TS_OPEN */
  const int64_t* out_total;    /* HOST [B]: INTERP: the number of outputs M of the whole signal */
  const int64_t* k0;           /* HOST [B]: WSOLA: the first frame to search */
  const int64_t* k1;           /* HOST [B]: WSOLA: one past the last */
  const int32_t* delta_prev;   /* HOST [B]: WSOLA: delta of frame k0 - 1 (not read when k0 == 0) */
  const int32_t* in_count;     /* HOST [B]: 0 .. ldx */
  const int32_t* out_count;    /* HOST [B]: 0 .. ldy */
} dia_timescale_args;
int dia_timescale(const dia_timescale_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loudness (csrc/loudness.hip; DESIGN.md "Loudness"): the sample arithmetic of an ITU-R BS.1770-4 meter for a ragged batch of mono
 * rows, and a gain.  One new entry point and one new struct; nothing older changed.
 *
 * DIA_LOUD_MEASURE.  Row b has len[b] samples at x[b][0 ..]; step = round(rate / 10) samples (100 ms).  The row's samples run
 * through the K-weighting, two biquads in cascade (transposed direct form II, float64 state, every product an fma):
 *   y = b0 x + s1;  s1 = b1 x + s2 - a1 y;  s2 = b2 x - a2 y        shelf, then the high-pass on y
 * and steps[b][s] receives the float64 sum of the squared outputs of samples [s step, (s + 1) step) for every WHOLE step
 * s < len[b] / step.  The recursion is evaluated as the linear system it is: a step is cut into `chunks` chunks of `chunk` samples
 * (the last one shorter: step - (chunks - 1) chunk, in [1, chunk]); every chunk's zero-state end state, a carry over the chunks
 * of a step and then over the steps of the row, and a second run of every chunk from its true initial state, whose squares are
 * added in ascending sample order per chunk and in ascending chunk order per step.  No atomics: an element has the same bits
 * whichever row of whichever batch it is computed in.
 * table (device, float64) holds what the carry needs, A being the 4 x 4 zero-input transition of the state
 * (s1, s2 of the shelf, s1, s2 of the high-pass) over one sample, matrices row-major:
 *   [0, 10)  shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2        [10, 26)  A^chunk        [26, 42)  A^step
 *   [42 + 16 c, 58 + 16 c)  A^(c chunk), c < chunks
 * peaks[b][0] receives max |x| over the row, peaks[b][1] the larger of it and max |.| over the row 4 x oversampled:
 *   output 4 q + p = sum_k bank[p][k] * x[q + first[p] + k]        q < len[b], p < 4, k < nt
 * one fp32 fmaf chain from 0 in ascending k, x zero outside [0, len[b]); bank is the library's own 1 -> 4 resampling bank.  The
 * oversampled signal is never stored.  An empty row has peaks 0 and no steps.
 * ws is scratch of at least DIA_LOUD_WS_DOUBLES(B, ld_steps, chunks) doubles, ws_doubles its size.
 *
 * DIA_LOUD_APPLY.  y[b][i] = (float)((double)x[b][in_off[b] + i] * gain[b]) for i < out_count[b]: one rounding per sample.
 * Memory outside x[b][0 .. len[b]) is never read, memory outside y[b][0 .. out_count[b]) never written.
 *
 * Refused with DIA_E_ARG before any HIP call: a null args / x / len; a mode other than the two; B outside [1, 64]; ldx outside
 * [1, 1 << 24]; a len outside [0, ldx].  MEASURE: null steps / peaks / ws / table / bank / first; step outside [8, 19200]; chunk
 * outside [1, step]; chunks != ceil(step / chunk) or above 64; nt outside [1, 32]; a first[p] + k that leaves [-32, 32];
 * ld_steps < 1 or below a row's whole steps; ws_doubles too small.  APPLY: null y / in_off / out_count / gain; y == x; ldy outside
 * [1, 1 << 24]; in_off < 0; out_count outside [0, ldy]; in_off + out_count > len; a gain that is not finite.
 * ------------------------------------------------------------------------------------------------ */
#define DIA_LOUD_MEASURE 0
#define DIA_LOUD_APPLY 1
#define DIA_LOUD_MAX_ROWS 64               /* rows of one launch */
#define DIA_LOUD_MAX_T (1 << 24)           /* ldx, ldy */
#define DIA_LOUD_MIN_STEP 8
#define DIA_LOUD_MAX_STEP 19200            /* 192 kHz: a step is staged in LDS */
#define DIA_LOUD_MAX_CHUNKS 64             /* one lane per chunk of a step */
#define DIA_LOUD_MAX_TAPS 32
#define DIA_LOUD_TABLE_DOUBLES(chunks) (42 + 16 * (chunks))
#define DIA_LOUD_WS_DOUBLES(B, ld_steps, chunks) ((int64_t)(B) * ((int64_t)(ld_steps) * (8 + 4 * (chunks)) + (ld_steps) + 1))
typedef struct {
  const float* x;              /* device [B][ldx] */
  float* y;                    /* device [B][ldy]; never x.  APPLY */
  double* steps;               /* device [B][ld_steps].  MEASURE */
  float* peaks;                /* device [B][2]: sample peak, true peak (linear).  MEASURE */
  double* ws;                  /* device [ws_doubles].  MEASURE */
  const double* table;         /* device [DIA_LOUD_TABLE_DOUBLES(chunks)].  MEASURE */
  const float* bank;           /* device [4][nt].  MEASURE */
  int64_t ws_doubles;
  int32_t mode;                /* DIA_LOUD_MEASURE / DIA_LOUD_APPLY */
  int32_t B, ldx, ldy, ld_steps;
  int32_t step, chunk, chunks, nt;
  int32_t _pad0;
  const int32_t* first;        /* HOST [4], read during the call (as all below).  MEASURE */
  const int32_t* len;          /* HOST [B]: 0 .. ldx */
  const int32_t* in_off;       /* HOST [B].  APPLY */
  const int32_t* out_count;    /* HOST [B]: 0 .. ldy.  APPLY */
  const double* gain;          /* HOST [B]: linear.  APPLY */
} dia_loudness_args;
int dia_loudness(const dia_loudness_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIA_HIP_H */
