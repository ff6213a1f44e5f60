// Per-request LoRA adapters, unmerged (dia_lora_apply, dia_lora_crosskv; DESIGN.md "Per-request adapters").
//
// The base projection has already written its output; these kernels add the low-rank correction of the adapter that the row's
// slot selected:   out[m, :] += (alpha / r) * B_a . (A_a . xn[m]),   a = adapter_of_slot[slot(m)],   nothing for a < 0.
// xn[m] is the RMS-normed input row the projection's GEMM consumed, rebuilt here from the fp32 residual row, the consumer's norm
// weight, D and eps — independent of the activation format between the GEMMs (planes, fp32 tiles), of the number of sum-of-squares
// partials and of the deferred-wo form.  The reference attaches adapters through PEFT at run time (cli.py:166-174); this is that
// arithmetic for DenseGeneral q/k/v projections, per row instead of per process.
//
// One workgroup of four waves per (row, module of this launch).  The problem is latency-bound (rank 8, D = 2048: A is 64 KB, B of
// q + k + v 80 KB, fp32), so every load that does not depend on another one is requested before the first wait: the row, the norm
// weight, two rank rows of A per wave, eight rank rows of B and the old output per thread.
//   down:  wave w reduces ranks w, w + 4, ... over the whole row (64 lanes x D / 64 elements: DPP row sums + two cross-row
//          exchanges) and knows the row's sum of squares by the same route, so u = A . xn needs no cross-wave reduction;
//   LDS:   the <= 64 values of u change hands once;
//   up:    every thread expands B . u for four consecutive output columns at a time.
// Plain vector loads and stores, no atomics, LDS for u only, no scratch.  A row whose slot has no adapter leaves after the two
// index loads that tell it so.
//
// dia_lora_crosskv is the same correction for the cross K/V projections, whose GEMM epilogue (DIA_EPI_CROSSKV) stored RoPE(K) and V
// straight into the caches: RoPE is linear, so RoPE(dK) and dV are added to what the caches hold — read, add in fp32, store through
// kv_store at the index of kv_row_index / kv_vblocked_index (gemm_common.hpp, shared with that epilogue), i.e. one rounding for bf16 and a fresh hi / lo split for bf16x2.
#include "gemm_common.hpp"
#include <cstdio>

namespace {

constexpr int LORA_NT = 256;           // four waves
constexpr int LORA_NWAVE = LORA_NT / 64;
constexpr int LORA_RMAX = 64;          // DIA_LORA_MAX_RANK
constexpr int LORA_BPRE = 8;           // rank rows of B requested ahead of the hand-over

struct LoraSegK {
  int col_off, n_cols;
  const float* const* A; const float* const* B; const int* rank; const float* scale;
};

struct LoraK {
  const float* x; int ldx; int D; const float* gain; float eps; float inv_d; int M;
  const int* row_slot; int rows_per_slot; const int* adapter_of_slot; int n_slots; int n_adapters;
  LoraSegK seg[DIA_LORA_MAX_SEGS];
  float* out; int ldo;
  // dia_lora_crosskv (seg[0] = K, seg[1] = V)
  void* kc; void* vc; int kv_dtype, kv_heads, kv_cap, kv_vblocked, kv_batch_index, rope_rows; long kv_plane_stride;
  const float* cos_t; const float* sin_t; const int* seg_off;
};

__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the adapter of workgroup-uniform slot `slot`, or -1
__device__ __forceinline__ int lora_adapter(const LoraK& p, int slot) {
  if (slot < 0 || slot >= p.n_slots) return -1;
  const int a = p.adapter_of_slot[slot];
  return a < p.n_adapters ? a : -1;
}

// both present and 16-byte aligned (float4 loads)
__device__ __forceinline__ bool lora_tables_ok(const float* A, const float* B) {
  return A && B && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0;
}

// u[j] = scale * inv_rms * sum_k A[j][k] * x[k] * gain[k] for j < r, left in `u` (LDS) for every thread: ends with the barrier.
// D = 256 * nx floats, nx <= NX: lane l of every wave holds the float4s i * 64 + l of the row.
template <int NX>
__device__ __forceinline__ void lora_down(const LoraK& p, int m, const float* __restrict__ A, int r, float scale, float* u) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nx = p.D >> 8, d4 = p.D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(p.x + (long)m * p.ldx);
  const float4* g4 = reinterpret_cast<const float4*>(p.gain);
  const float4* A4 = reinterpret_cast<const float4*>(A);
  const int j0 = min(wave, r - 1), j1 = min(wave + LORA_NWAVE, r - 1);      // (clamped: a wave without a rank of its own reads a valid row)
  float4 xv[NX], gv[NX], a0[NX], a1[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const int k = min(i, nx - 1) * 64 + lane;
    xv[i] = xr[k]; gv[i] = g4[k];
    a0[i] = A4[(long)j0 * d4 + k]; a1[i] = A4[(long)j1 * d4 + k];
  }
  float ss = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    if (i < nx) {
      ss += dot4(xv[i], xv[i]);
      xv[i] = float4{xv[i].x * gv[i].x, xv[i].y * gv[i].y, xv[i].z * gv[i].z, xv[i].w * gv[i].w};
      s0 += dot4(a0[i], xv[i]); s1 += dot4(a1[i], xv[i]);
    }
  }
  ss = wave_sum_dpp(ss); s0 = wave_sum_dpp(s0); s1 = wave_sum_dpp(s1);
  const float f = scale * rsqrtf(ss * p.inv_d + p.eps);
  if (lane == 0) {
    if (wave < r) u[wave] = s0 * f;
    if (wave + LORA_NWAVE < r) u[wave + LORA_NWAVE] = s1 * f;
  }
  for (int j = wave + 2 * LORA_NWAVE; j < r; j += LORA_NWAVE) {      // ranks above 8: one row of A per wave and round
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NX; ++i)
      if (i < nx) s += dot4(A4[(long)j * d4 + i * 64 + lane], xv[i]);
    s = wave_sum_dpp(s);
    if (lane == 0) u[j] = s * f;
  }
  lds_barrier();
}

template <int NX>
__global__ __launch_bounds__(LORA_NT) void k_lora(LoraK p) {
  __shared__ float u[LORA_RMAX];
  const int m = blockIdx.x;
  const LoraSegK& sg = p.seg[blockIdx.y];
  const int slot = p.row_slot ? p.row_slot[m] : m / p.rows_per_slot;
  const int a = lora_adapter(p, slot);
  if (a < 0) return;                                   // no adapter on this row: nothing is read, nothing written
  const int r = sg.rank[a];
  const float* A = sg.A[a];
  const float* B = sg.B[a];
  const float scale = sg.scale[a];
  if (r <= 0 || r > LORA_RMAX || !lora_tables_ok(A, B)) return;     // this adapter leaves the module alone
  // B . u: four consecutive columns per thread and round; the first round's B rows and old values are requested now
  const int nc4 = sg.n_cols >> 2;
  const float4* B4 = reinterpret_cast<const float4*>(B);
  float4* o4 = reinterpret_cast<float4*>(p.out + (long)m * p.ldo + sg.col_off);
  const int c0 = threadIdx.x;
  const bool has0 = c0 < nc4;
  const int cc = has0 ? c0 : 0;
  float4 bpre[LORA_BPRE];
#pragma unroll
  for (int j = 0; j < LORA_BPRE; ++j) bpre[j] = B4[(long)min(j, r - 1) * nc4 + cc];
  float4 acc = o4[cc];
  lora_down<NX>(p, m, A, r, scale, u);
  if (has0) {
#pragma unroll
    for (int j = 0; j < LORA_BPRE; ++j) {
      if (j < r) {
        const float uj = u[j];
        acc.x += uj * bpre[j].x; acc.y += uj * bpre[j].y; acc.z += uj * bpre[j].z; acc.w += uj * bpre[j].w;
      }
    }
    for (int j = LORA_BPRE; j < r; ++j) {
      const float uj = u[j];
      const float4 b = B4[(long)j * nc4 + c0];
      acc.x += uj * b.x; acc.y += uj * b.y; acc.z += uj * b.z; acc.w += uj * b.w;
    }
    o4[c0] = acc;
  }
  for (int c = c0 + LORA_NT; c < nc4; c += LORA_NT) {
    float4 v = o4[c];
    for (int j = 0; j < r; ++j) {
      const float uj = u[j];
      const float4 b = B4[(long)j * nc4 + c];
      v.x += uj * b.x; v.y += uj * b.y; v.z += uj * b.z; v.w += uj * b.w;
    }
    o4[c] = v;
  }
}

// what the cache holds at idx, plus d, stored again in the cache's format (kv_store: one rounding / a fresh hi + lo split)
__device__ __forceinline__ void kv_add(void* base, int dtype, long idx, float d, long plane_stride) {
  float v;
  if (dtype == DIA_KV_F32) v = reinterpret_cast<const float*>(base)[idx];
  else {
    const bf16_raw* q = reinterpret_cast<const bf16_raw*>(base);
    v = bf16_bits_to_f32(q[idx]);
    if (dtype == DIA_KV_BF16X2) v += bf16_bits_to_f32(q[idx + plane_stride]);
  }
  kv_store(base, dtype, idx, v + d, plane_stride);
}

// grid (packed rows, 2): y = 0 adds RoPE(dK) to the K cache, y = 1 dV to the V cache, at the row's (utterance, position)
template <int NX>
__global__ __launch_bounds__(LORA_NT) void k_lora_crosskv(LoraK p) {
  __shared__ float u[LORA_RMAX];
  const int m = blockIdx.x;
  const bool is_v = blockIdx.y != 0;
  const LoraSegK& sg = p.seg[blockIdx.y];
  int b = p.kv_batch_index, pos = m;
  if (p.row_slot) {                                    // packed batch: row -> (utterance, position), as the CROSSKV epilogue
    b = p.row_slot[m];
    if (b < 0 || b >= p.n_slots) return;               // (before seg_off[b]: seg_off has n_slots entries)
    pos = m - p.seg_off[b];
  }
  const int a = lora_adapter(p, b);
  if (a < 0 || pos < 0 || pos >= p.kv_cap || pos >= p.rope_rows) return;      // (rope_rows >= kv_cap is checked on the host)
  const int r = sg.rank[a];
  const float* A = sg.A[a];
  const float* B = sg.B[a];
  const float scale = sg.scale[a];
  if (r <= 0 || r > LORA_RMAX || !lora_tables_ok(A, B)) return;
  lora_down<NX>(p, m, A, r, scale, u);
  const int nc4 = sg.n_cols >> 2;                      // n_cols = kv_heads * 128
  const float4* B4 = reinterpret_cast<const float4*>(B);
  // one item = dims i .. i + 3 and i + 64 .. i + 67 of one head: the RoPE pairs (d, d + 64) of K, eight values of V
  for (int it = threadIdx.x; it < p.kv_heads * 16; it += LORA_NT) {
    const int head = it >> 4, i = (it & 15) * 4;
    const int clo = (head * 128 + i) >> 2, chi = clo + 16;
    float4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < r; ++j) {
      const float uj = u[j];
      const float4 bl = B4[(long)j * nc4 + clo], bh = B4[(long)j * nc4 + chi];
      lo.x += uj * bl.x; lo.y += uj * bl.y; lo.z += uj * bl.z; lo.w += uj * bl.w;
      hi.x += uj * bh.x; hi.y += uj * bh.y; hi.z += uj * bh.z; hi.w += uj * bh.w;
    }
    const float l[4] = {lo.x, lo.y, lo.z, lo.w}, h[4] = {hi.x, hi.y, hi.z, hi.w};
    if (!is_v) {
      const float4 c4 = *reinterpret_cast<const float4*>(p.cos_t + (long)pos * 64 + i);
      const float4 s4 = *reinterpret_cast<const float4*>(p.sin_t + (long)pos * 64 + i);
      const float c[4] = {c4.x, c4.y, c4.z, c4.w}, s[4] = {s4.x, s4.y, s4.z, s4.w};
      const long base = kv_row_index(b, p.kv_heads, head, p.kv_cap, pos);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        kv_add(p.kc, p.kv_dtype, base + i + t, l[t] * c[t] - h[t] * s[t], p.kv_plane_stride);
        kv_add(p.kc, p.kv_dtype, base + i + 64 + t, l[t] * s[t] + h[t] * c[t], p.kv_plane_stride);
      }
    } else if (p.kv_vblocked) {                        // [key/32][128 dims][32 keys]
      const long blk = kv_vblocked_index(b, p.kv_heads, head, p.kv_cap, pos);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        kv_add(p.vc, p.kv_dtype, blk + (long)(i + t) * 32, l[t], p.kv_plane_stride);
        kv_add(p.vc, p.kv_dtype, blk + (long)(i + 64 + t) * 32, h[t], p.kv_plane_stride);
      }
    } else {
      const long base = kv_row_index(b, p.kv_heads, head, p.kv_cap, pos);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        kv_add(p.vc, p.kv_dtype, base + i + t, l[t], p.kv_plane_stride);
        kv_add(p.vc, p.kv_dtype, base + i + 64 + t, h[t], p.kv_plane_stride);
      }
    }
  }
}

int lora_fail(const char* who, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, why);
  return dia_fail(DIA_E_ARG, msg);
}

const char* check_seg(const dia_lora_seg& s) {
  if (s.n_cols <= 0 || s.n_cols % 4 != 0 || s.col_off < 0 || s.col_off % 4 != 0) return "segment columns must be positive multiples of 4";
  if (!s.A || !s.B || !s.rank || !s.scale) return "segment without its A / B / rank / scale tables";
  if (s.max_rank < 0 || s.max_rank > DIA_LORA_MAX_RANK) return "rank above 64 (DIA_LORA_MAX_RANK)";
  return nullptr;
}

const char* check_input(const float* x, int ldx, int D, const float* gain, int M, const int32_t* adapter_of_slot, int n_slots, int n_adapters) {
  if (!x || !gain || !adapter_of_slot) return "null argument";
  if (M <= 0 || n_slots <= 0 || n_adapters <= 0) return "empty shape";
  if (D <= 0 || D % 256 != 0 || D > 2048) return "D must be a multiple of 256, at most 2048 (64 lanes x float4 per row pass)";
  if (ldx < D || ldx % 4 != 0) return "ldx must be a multiple of 4 and at least D";
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gain)) & 15) return "x and gain must be 16-byte aligned";
  return nullptr;
}

LoraSegK seg_k(const dia_lora_seg& s) { return LoraSegK{s.col_off, s.n_cols, s.A, s.B, s.rank, s.scale}; }

}  // namespace

// the argument checks of dia_lora_apply; dia_engine_set_lora runs them on the descriptors it builds, before any step exists
int dia_lora_validate(const dia_lora_args* a, const char* who) {
  if (!a) return lora_fail(who, "null argument");
  const char* why = check_input(a->x, a->ldx, a->D, a->gain, a->M, a->adapter_of_slot, a->n_slots, a->n_adapters);
  if (!why && !a->out) why = "null argument";
  if (!why && !a->row_slot && a->rows_per_slot <= 0) why = "rows_per_slot must be positive when row_slot is NULL";
  if (!why && (a->n_segs < 1 || a->n_segs > DIA_LORA_MAX_SEGS)) why = "1..3 segments per launch";
  if (!why && (a->ldo % 4 != 0 || (reinterpret_cast<uintptr_t>(a->out) & 15))) why = "out must be 16-byte aligned and ldo a multiple of 4";
  for (int i = 0; !why && i < a->n_segs; ++i) {
    why = check_seg(a->seg[i]);
    if (!why && (long)a->seg[i].col_off + a->seg[i].n_cols > a->ldo) why = "segment columns beyond ldo";
    for (int k = 0; !why && k < i; ++k)
      if (a->seg[i].col_off < a->seg[k].col_off + a->seg[k].n_cols && a->seg[k].col_off < a->seg[i].col_off + a->seg[i].n_cols)
        why = "segments overlap (two workgroups would update the same columns)";
  }
  return why ? lora_fail(who, why) : DIA_OK;
}

static void launch_lora(bool crosskv, int D, dim3 grid, hipStream_t st, const LoraK& k) {
  const int nx = D / 256;
  if (crosskv) {
    if (nx <= 2) dia_launch<k_lora_crosskv<2>>(grid, dim3(LORA_NT), 0, st, k);
    else if (nx <= 4) dia_launch<k_lora_crosskv<4>>(grid, dim3(LORA_NT), 0, st, k);
    else dia_launch<k_lora_crosskv<8>>(grid, dim3(LORA_NT), 0, st, k);
  } else {
    if (nx <= 2) dia_launch<k_lora<2>>(grid, dim3(LORA_NT), 0, st, k);
    else if (nx <= 4) dia_launch<k_lora<4>>(grid, dim3(LORA_NT), 0, st, k);
    else dia_launch<k_lora<8>>(grid, dim3(LORA_NT), 0, st, k);
  }
}

extern "C" int dia_lora_apply(const dia_lora_args* a, void* stream) {
  const int rc = dia_lora_validate(a, "dia_lora_apply");
  if (rc) return rc;
  LoraK k = {};
  k.x = a->x; k.ldx = a->ldx; k.D = a->D; k.gain = a->gain; k.eps = a->eps; k.inv_d = 1.0f / a->D; k.M = a->M;
  k.row_slot = a->row_slot; k.rows_per_slot = a->rows_per_slot; k.adapter_of_slot = a->adapter_of_slot;
  k.n_slots = a->n_slots; k.n_adapters = a->n_adapters;
  for (int i = 0; i < a->n_segs; ++i) k.seg[i] = seg_k(a->seg[i]);
  k.out = a->out; k.ldo = a->ldo;
  launch_lora(false, a->D, dim3(a->M, a->n_segs), (hipStream_t)stream, k);
  return dia_check_launch("k_lora");
}

extern "C" int dia_lora_crosskv(const dia_lora_crosskv_args* a, void* stream) {
  const char* who = "dia_lora_crosskv";
  if (!a) return lora_fail(who, "null argument");
  const char* why = check_input(a->x, a->ldx, a->D, a->gain, a->M, a->adapter_of_slot, a->n_slots, a->n_adapters);
  if (!why && (!a->kc || !a->vc || !a->cos_t || !a->sin_t)) why = "null argument";
  if (!why && ((a->row_b == nullptr) != (a->seg_off == nullptr))) why = "row_b and seg_off go together";
  if (!why && (a->kv_dtype < DIA_KV_F32 || a->kv_dtype > DIA_KV_BF16X2)) why = "kv_dtype outside 0..2";
  if (!why && (a->kv_heads <= 0 || a->kv_cap <= 0)) why = "empty cache shape";
  if (!why && a->kv_dtype == DIA_KV_BF16X2 && (a->kv_plane_stride <= 0 || a->kv_plane_stride % 8 != 0)) why = "bf16x2 caches need a positive kv_plane_stride, a multiple of 8";
  if (!why && a->kv_vblocked && (a->kv_cap % 32 != 0 || a->kv_dtype == DIA_KV_F32)) why = "blocked V needs bf16 caches and kv_cap % 32 == 0";
  if (!why && a->rope_rows <= 0) why = "rope_rows (rows of cos_t / sin_t) must be stated";
  if (!why && a->rope_rows < a->kv_cap) why = "cos_t / sin_t must cover every cache position (rope_rows >= kv_cap): K and V are corrected together or not at all";
  if (!why && !a->row_b && (a->kv_batch_index < 0 || a->kv_batch_index >= a->n_slots || a->M > a->kv_cap)) why = "one utterance: kv_batch_index outside the slots or more rows than kv_cap";
  if (!why) why = check_seg(a->k);
  if (!why) why = check_seg(a->v);
  if (!why && (a->k.n_cols != a->kv_heads * 128 || a->v.n_cols != a->kv_heads * 128)) why = "the K and V segments must be kv_heads * 128 columns wide";
  if (why) return lora_fail(who, why);
  LoraK k = {};
  k.x = a->x; k.ldx = a->ldx; k.D = a->D; k.gain = a->gain; k.eps = a->eps; k.inv_d = 1.0f / a->D; k.M = a->M;
  k.row_slot = a->row_b; k.seg_off = a->seg_off; k.adapter_of_slot = a->adapter_of_slot; k.n_slots = a->n_slots; k.n_adapters = a->n_adapters;
  k.seg[0] = seg_k(a->k); k.seg[1] = seg_k(a->v);
  k.kc = a->kc; k.vc = a->vc; k.kv_dtype = a->kv_dtype; k.kv_heads = a->kv_heads; k.kv_cap = a->kv_cap; k.kv_vblocked = a->kv_vblocked;
  k.kv_batch_index = a->kv_batch_index; k.rope_rows = a->rope_rows; k.kv_plane_stride = a->kv_plane_stride;
  k.cos_t = a->cos_t; k.sin_t = a->sin_t;
  launch_lora(true, a->D, dim3(a->M, 2), (hipStream_t)stream, k);
  return dia_check_launch("k_lora_crosskv");
}
