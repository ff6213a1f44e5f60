// Decoder prefill over an audio prompt, batched: instead of replaying the prompt rows one
// decode step at a time (1.1 ms each), all prompt rows of all utterances — both CFG rows — run as ONE packed
// batch through the MFMA-tiled GEMMs, with the three kernels below for what is not a GEMM.  Semantics are the
// replay's (oracle.generate docstring): token row r -> cache slot r at RoPE position r + 1; the K/V written to
// the caches are rounded to the cache dtype first and attention reads them back from the caches, exactly what
// the decode steps will do afterwards.  bf16 caches with the blocked V layout (the perf configuration), or FP8 self caches
// (k_prefill_kv_f8 / k_prefill_attn_f8 below: every prompted key quantised like a generated one); fp32 caches keep the replay.
//
// Packing: segment s = (utterance b, CFG row c) owns packed rows [seg_off[s], seg_off[s] + seg_len[s]),
// seg_off a multiple of 32; row_seg[m] = segment of packed row m or -1 (padding); seg_row[s] = 2b + c.
#include "common.hpp"
#include "kv_fp8.hpp"
#include "attn_tile.hpp"
#include "../../include/dia_hip.h"
#include "errors.hpp"
#include "launch.hpp"
#include <cstdio>

namespace {

constexpr int HD = 128;

struct PrefK {
  const int* row_seg; const int* seg_off; const int* seg_len; const int* seg_row; int rows;
  // embedding
  const int* tokens; int T, C, V, D; const float* emb; const float* g; float* x;
  bf16_raw* P; long p_plane_stride; int p_ktiles; float* ssq; int ssq_ld;
  // K/V append + attention
  const float* q; int ldq, q_off, k_off, v_off;
  int q_heads, kv_heads, kv_cap;         // attention: q_heads query heads, kv_heads cache heads (group = q/kv)
  bf16_raw* kc; bf16_raw* vc;            // caches [cache row][kv_heads][kv_cap][128], V blocked
  const float* cos_t; const float* sin_t;
  int causal;                            // 1 = self (keys 0..r of the segment's own cache row), 0 = cross
  const int* text_len;                   // cross: keys of utterance b
};

// x[m] = sum_c emb[c][tokens[b][r][c]] (layers.py:691-696), planes(x * g), strip ssq — one packed row per workgroup
__global__ __launch_bounds__(256) void k_prefill_embed(PrefK p) {
  __shared__ int tok[16];
  const int m = blockIdx.x, s = p.row_seg[m];
  if (s < 0) return;
  const int r = m - p.seg_off[s], b = p.seg_row[s] >> 1;
  if (threadIdx.x < p.C) tok[threadIdx.x] = p.tokens[((long)b * p.T + r) * p.C + threadIdx.x];
  __syncthreads();
  for (int d0 = threadIdx.x * 8; d0 < p.D; d0 += 256 * 8) {
    float v[8];
    for (int c = 0; c < p.C; ++c) {          // sequential sum in channel order
      const float* e = p.emb + ((long)c * p.V + tok[c]) * p.D + d0;
      const float4 a = *reinterpret_cast<const float4*>(e), bq = *reinterpret_cast<const float4*>(e + 4);
      if (c == 0) { v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = bq.x; v[5] = bq.y; v[6] = bq.z; v[7] = bq.w; }
      else { v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += bq.x; v[5] += bq.y; v[6] += bq.z; v[7] += bq.w; }
    }
    float ss = 0.f, vg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { ss += v[j] * v[j]; vg[j] = p.g ? v[j] * p.g[d0 + j] : v[j]; }
    const float other = __shfl_xor(ss, 1, 64);
    float* xo = p.x + (long)m * p.D + d0;
    *reinterpret_cast<float4*>(xo) = float4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<float4*>(xo + 4) = float4{v[4], v[5], v[6], v[7]};
    emit_planes8(p.P, p.p_plane_stride, p.p_ktiles, m, d0, vg);
    if (((d0 >> 3) & 1) == 0) p.ssq[(long)(d0 >> 4) * p.ssq_ld + m] = ss + other;
  }
}

// K = RoPE(k, r + 1) and V of every packed row into the self caches (KVCache.update for slots 0..Tp-1)
__global__ __launch_bounds__(256) void k_prefill_kv(PrefK p) {
  const int h = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  for (int t = tid; t < 32 * 64; t += 256) {
    const int rr = t >> 6, d = t & 63, m = blk * 32 + rr;
    const int s = p.row_seg[m];
    if (s < 0) continue;
    const int r = m - p.seg_off[s], pos = r + 1;
    const float* kr = p.q + (long)m * p.ldq + p.k_off + h * HD;
    const float x1 = kr[d], x2 = kr[d + 64];
    const float c = p.cos_t[(long)pos * 64 + d], sn = p.sin_t[(long)pos * 64 + d];
    bf16_raw* ko = p.kc + (((long)p.seg_row[s] * p.kv_heads + h) * p.kv_cap + r) * HD;
    KVElem<bf16_raw>::store(ko + d, x1 * c - x2 * sn);
    KVElem<bf16_raw>::store(ko + d + 64, x1 * sn + x2 * c);
  }
  for (int t = tid; t < 32 * HD; t += 256) {
    const int rr = t & 31, d = t >> 5, m = blk * 32 + rr;
    const int s = p.row_seg[m];
    if (s < 0) continue;
    const int r = m - p.seg_off[s];
    bf16_raw* vo = p.vc + ((long)p.seg_row[s] * p.kv_heads + h) * p.kv_cap * HD + (long)(r >> 5) * HD * 32 + (long)d * 32 + (r & 31);
    KVElem<bf16_raw>::store(vo, p.q[(long)m * p.ldq + p.v_off + h * HD + d]);
  }
}

// Many-query attention over the bf16 caches: grid (query head, 16-row query tile).  q as three planes (exact),
// K / V straight from the caches as single bf16 operands, p as three planes; 4 waves split the keys in 32-key
// granules, online softmax per query row, waves merged through LDS — k_attn_enc_mfma with the caches as K/V: the
// q staging, the softmax step and the merge are the one copy in attn_tile.hpp, the K / V loads and MFMAs are here.
// causal: query row r sees keys 0..r of its own cache row; else the cond segment sees the utterance's text keys
// and the uncond segment gets exact zeros.
__global__ __launch_bounds__(256) void k_prefill_attn(PrefK p) {
  __shared__ __attribute__((aligned(16))) AttnTile tile;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = blockIdx.x, qt = blockIdx.y;
  const int arow = lane & 15, akq = lane >> 4;
  const int s = p.row_seg[qt * 16];
  if (s < 0) return;
  const int off = p.seg_off[s], len = p.seg_len[s], crow = p.seg_row[s];
  const int r0 = qt * 16 - off;                       // first prompt row of this tile
  const int group = p.q_heads / p.kv_heads;
  int nkeys; const bf16_raw* Kh; const bf16_raw* Vh;
  if (p.causal) {
    nkeys = min(len, r0 + 16);
    const long base = ((long)crow * p.kv_heads + h / group) * p.kv_cap * HD;
    Kh = p.kc + base; Vh = p.vc + base;
  } else {
    if ((crow & 1) == 0) {                            // uncond row: cross-attention output is exactly 0
      const int r = tid >> 4, d0 = (tid & 15) * 8, m = qt * 16 + r;
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (m - off < len) emit_planes8(p.P, p.p_plane_stride, p.p_ktiles, m, h * HD + d0, z);
      return;
    }
    nkeys = p.text_len[crow >> 1];
    const long base = ((long)(crow >> 1) * p.kv_heads + h / group) * p.kv_cap * HD;
    Kh = p.kc + base; Vh = p.vc + base;
  }
  {
    const int m = min(qt * 16 + (tid >> 4), off + len - 1);
    attn_tile_stage_q(tile, tid, p.q + (long)m * p.ldq + p.q_off + h * HD, (m - off) + 1, p.cos_t, p.sin_t);
  }
  __syncthreads();
  f32x4 O[8];
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) O[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun[4], lrun[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mrun[r] = -INFINITY; lrun[r] = 0.f; }
  int lim[4];                                         // keys query row 4*akq + r may see
#pragma unroll
  for (int r = 0; r < 4; ++r) lim[r] = p.causal ? min(nkeys, r0 + 4 * akq + r + 1) : nkeys;
  const int klast = max(nkeys - 1, 0);
  const int ngran = (nkeys + 31) >> 5;
  for (int g = w; g < ngran; g += AttnTile::NWV) {
    const int key0 = g << 5;
    f32x4 S[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 qa[DIA_NPLANES];
#pragma unroll
      for (int pl = 0; pl < DIA_NPLANES; ++pl) qa[pl] = *reinterpret_cast<const bf16x8*>(&tile.qf[ks][pl][arow][akq][0]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 kb = *reinterpret_cast<const bf16x8*>(Kh + (long)min(key0 + 16 * t + arow, klast) * HD + 32 * ks + 8 * akq);
#pragma unroll
        for (int pl = 0; pl < DIA_NPLANES; ++pl) S[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[pl], kb, S[t], 0, 0, 0);
      }
    }
    float alpha[4];
    attn_tile_softmax<false>(tile, w, arow, akq, S, key0, lim, nullptr, nullptr, mrun, lrun, alpha);
#pragma unroll
    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) O[nb][r] *= alpha[r];
    bf16x8 pa[DIA_NPLANES];
#pragma unroll
    for (int pl = 0; pl < DIA_NPLANES; ++pl) pa[pl] = *reinterpret_cast<const bf16x8*>(&tile.pbuf[w][pl][arow][8 * akq]);
    const bf16_raw* Vblk = Vh + (long)g * HD * 32;
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
      const bf16x8 vb = *reinterpret_cast<const bf16x8*>(Vblk + (long)(16 * nb + arow) * 32 + 8 * akq);
#pragma unroll
      for (int pl = 0; pl < DIA_NPLANES; ++pl) O[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[pl], vb, O[nb], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }
  attn_tile_merge_emit<6>(tile, tid, O, mrun, lrun, qt * 16, off + len, p.P, p.p_plane_stride, p.p_ktiles, h * HD);
}

// ---------------------------------------------------------------------------------------------------
// The same two steps onto FP8 self caches (dia_hip.h "FP8 self K/V"): k8 [row][kv_heads][T][128], v8 [row][kv_heads][T/32][128][32],
// ks / vs float [row][kv_heads][T].  The cross call keeps k_prefill_attn: the cross caches stay bf16.
struct PrefF8 { uint8_t* k8; uint8_t* v8; float* ks; float* vs; };

// grid (kv head, 32-row block), 4 waves.  seg_off is a multiple of 32, so a block is keys [r0, r0 + 32) of ONE segment: one K run of
// 32 x 128 bytes and one blocked V granule.  One wave per (row, kv head) at a time, lane l holding dims l and l + 64 of k and of v:
// RoPE, amax, scale and bytes are k_attn_self_f8's owner-wave append, spelt the same way, from the fp32 projection values.  The
// bytes are staged in LDS; a block of 32 live rows leaves as 16-byte stores, a partial one as the live keys' K rows (16-byte
// stores) and the live keys' V bytes one by one — no byte or scale outside keys [0, seg_len) of the segment's cache row changes.
__global__ __launch_bounds__(256) void k_prefill_kv_f8(PrefK p, PrefF8 f8) {
  __shared__ __attribute__((aligned(16))) uint8_t kst[32 * HD];      // [key][dim]
  __shared__ __attribute__((aligned(16))) uint8_t vst[HD * 32];      // [dim][key]: the granule as it lies in the cache
  const int h = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = p.row_seg[blk * 32];
  if (s < 0) return;                                    // (uniform) a block of padding rows
  const int off = p.seg_off[s], r0 = blk * 32 - off;
  const int nlive = min(min(32, p.seg_len[s] - r0), p.kv_cap - r0);      // live rows are the block's first nlive
  if (r0 < 0 || (r0 & 31) != 0 || nlive <= 0) return;
  const long pair_keys = ((long)p.seg_row[s] * p.kv_heads + h) * p.kv_cap;
  uint8_t* K8 = f8.k8 + (pair_keys + r0) * HD;          // this block's 32 K rows ...
  uint8_t* V8 = f8.v8 + (pair_keys + r0) * HD;          // ... and its V granule (r0 / 32 granules of 128 x 32 bytes)
  float* KS = f8.ks + pair_keys + r0;
  float* VS = f8.vs + pair_keys + r0;
  for (int rr = w; rr < nlive; rr += 4) {               // (wave-uniform trip)
    const int m = blk * 32 + rr;
    if (p.row_seg[m] != s) continue;
    const int pos = r0 + rr + 1;
    const float* qr = p.q + (long)m * p.ldq;
    const float* kh = qr + p.k_off + h * HD;
    const float* vh = qr + p.v_off + h * HD;
    const float kx1 = kh[lane], kx2 = kh[lane + 64];
    const float vx1 = vh[lane], vx2 = vh[lane + 64];
    const float rc = p.cos_t[(long)pos * 64 + lane], rs = p.sin_t[(long)pos * 64 + lane];
    const float k1 = __builtin_fmaf(kx1, rc, -mul_rn(kx2, rs)), k2 = __builtin_fmaf(kx2, rc, mul_rn(kx1, rs));
    const unsigned ksb = kv_scale_bits_f32(wave_umax(max(__float_as_uint(k1) & 0x7fffffffu, __float_as_uint(k2) & 0x7fffffffu)));
    const unsigned vsb = kv_scale_bits_f32(wave_umax(max(__float_as_uint(vx1) & 0x7fffffffu, __float_as_uint(vx2) & 0x7fffffffu)));
    const float kinv = __uint_as_float((254u << 23) - ksb), vinv = __uint_as_float((254u << 23) - vsb);      // 1 / scale, exact
    kst[rr * HD + lane] = (uint8_t)e4m3_finite(k1 * kinv); kst[rr * HD + lane + 64] = (uint8_t)e4m3_finite(k2 * kinv);
    vst[lane * 32 + rr] = (uint8_t)e4m3_finite(vx1 * vinv); vst[(lane + 64) * 32 + rr] = (uint8_t)e4m3_finite(vx2 * vinv);
    if (lane == 0) { KS[rr] = __uint_as_float(ksb); VS[rr] = __uint_as_float(vsb); }
  }
  __syncthreads();
  // live mask of the block (bit rr), the same in every thread
  unsigned live = 0;
  for (int rr = 0; rr < nlive; ++rr) live |= (p.row_seg[blk * 32 + rr] == s ? 1u : 0u) << rr;
  if ((live >> (tid >> 3)) & 1u)                        // K: thread = (key tid / 8, 16 dims)
    *reinterpret_cast<uint4*>(K8 + tid * 16) = *reinterpret_cast<const uint4*>(kst + tid * 16);
  if (live == 0xffffffffu) {                            // V: thread = (dim tid / 2, 16 keys)
    *reinterpret_cast<uint4*>(V8 + tid * 16) = *reinterpret_cast<const uint4*>(vst + tid * 16);
  } else {
    for (int t = tid; t < HD * 32; t += 256)
      if ((live >> (t & 31)) & 1u) V8[t] = vst[t];
  }
}

// k_prefill_attn (causal) over the e4m3 self caches: 8-byte K / V fragments expanded to bf16 in registers (exact), the scales folded
// in behind the MFMAs — S[key] *= ks[key] before the softmax scale and the mask, p[key] *= vs[key] before split3, lrun from the
// unscaled p.  The scales are powers of two, so every MFMA receives products equal to those of k_prefill_attn over bf16 caches
// holding the dequantised values and the output is the same bit for bit (as long as p * vs is a normal fp32): everything else that
// rounds — q staging, softmax step, wave merge — is the same attn_tile.hpp code in both kernels.  A lane holds the score
// of key key0 + 16t + arow in S[t][.], so it loads that key's two scales; the clamped re-read of klast clamps the K scale index too.
__global__ __launch_bounds__(256) void k_prefill_attn_f8(PrefK p, PrefF8 f8) {
  __shared__ __attribute__((aligned(16))) AttnTile tile;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = blockIdx.x, qt = blockIdx.y;
  const int arow = lane & 15, akq = lane >> 4;
  const int s = p.row_seg[qt * 16];
  if (s < 0) return;
  const int off = p.seg_off[s], len = min(p.seg_len[s], p.kv_cap), crow = p.seg_row[s];
  const int r0 = qt * 16 - off;                       // first prompt row of this tile
  const int group = p.q_heads / p.kv_heads;
  const int nkeys = min(len, r0 + 16);
  const long pair_keys = ((long)crow * p.kv_heads + h / group) * p.kv_cap;
  const uint8_t* K8 = f8.k8 + pair_keys * HD;
  const uint8_t* V8 = f8.v8 + pair_keys * HD;
  const float* KS = f8.ks + pair_keys;
  const float* VS = f8.vs + pair_keys;
  {
    const int m = min(qt * 16 + (tid >> 4), off + len - 1);
    attn_tile_stage_q(tile, tid, p.q + (long)m * p.ldq + p.q_off + h * HD, (m - off) + 1, p.cos_t, p.sin_t);
  }
  __syncthreads();
  f32x4 O[8];
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) O[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun[4], lrun[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mrun[r] = -INFINITY; lrun[r] = 0.f; }
  int lim[4];                                         // keys query row 4*akq + r may see
#pragma unroll
  for (int r = 0; r < 4; ++r) lim[r] = min(nkeys, r0 + 4 * akq + r + 1);
  const int klast = max(nkeys - 1, 0);
  const int ngran = (nkeys + 31) >> 5;
  for (int g = w; g < ngran; g += AttnTile::NWV) {
    const int key0 = g << 5;
    f32x4 S[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int kidx[2] = {min(key0 + arow, klast), min(key0 + 16 + arow, klast)};
    const float ksc[2] = {KS[kidx[0]], KS[kidx[1]]};
    const float vsc[2] = {VS[min(key0 + arow, p.kv_cap - 1)], VS[min(key0 + 16 + arow, p.kv_cap - 1)]};     // (inside the row: finite)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 qa[DIA_NPLANES];
#pragma unroll
      for (int pl = 0; pl < DIA_NPLANES; ++pl) qa[pl] = *reinterpret_cast<const bf16x8*>(&tile.qf[ks][pl][arow][akq][0]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 kb = expand_e4m3(*reinterpret_cast<const uint2*>(K8 + (long)kidx[t] * HD + 32 * ks + 8 * akq));
#pragma unroll
        for (int pl = 0; pl < DIA_NPLANES; ++pl) S[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[pl], kb, S[t], 0, 0, 0);
      }
    }
    float alpha[4];
    attn_tile_softmax<true>(tile, w, arow, akq, S, key0, lim, ksc, vsc, mrun, lrun, alpha);
#pragma unroll
    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) O[nb][r] *= alpha[r];
    bf16x8 pa[DIA_NPLANES];
#pragma unroll
    for (int pl = 0; pl < DIA_NPLANES; ++pl) pa[pl] = *reinterpret_cast<const bf16x8*>(&tile.pbuf[w][pl][arow][8 * akq]);
    const uint8_t* Vblk = V8 + (long)g * HD * 32;
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
      const bf16x8 vb = expand_e4m3(*reinterpret_cast<const uint2*>(Vblk + (long)(16 * nb + arow) * 32 + 8 * akq));
#pragma unroll
      for (int pl = 0; pl < DIA_NPLANES; ++pl) O[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[pl], vb, O[nb], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }
  attn_tile_merge_emit<6>(tile, tid, O, mrun, lrun, qt * 16, off + len, p.P, p.p_plane_stride, p.p_ktiles, h * HD);
}

int fill(const dia_dec_prefill_args* a, PrefK& k) {
  if (!a || !a->row_seg || !a->seg_off || !a->seg_len || !a->seg_row || a->rows <= 0 || a->rows % 32 != 0)
    return dia_fail(DIA_E_ARG, "dia_dec_prefill: packing arrays missing or rows not a multiple of 32");
  k.row_seg = a->row_seg; k.seg_off = a->seg_off; k.seg_len = a->seg_len; k.seg_row = a->seg_row; k.rows = a->rows;
  k.tokens = a->tokens; k.T = a->T; k.C = a->C; k.V = a->V; k.D = a->D; k.emb = a->emb; k.g = a->g; k.x = a->x;
  k.P = (bf16_raw*)a->P; k.p_plane_stride = a->p_plane_stride; k.p_ktiles = a->p_ktiles; k.ssq = a->ssq; k.ssq_ld = a->ssq_ld;
  k.q = a->q; k.ldq = a->ldq; k.q_off = a->q_off; k.k_off = a->k_off; k.v_off = a->v_off;
  k.q_heads = a->q_heads; k.kv_heads = a->kv_heads; k.kv_cap = a->kv_cap;
  k.kc = (bf16_raw*)a->kc; k.vc = (bf16_raw*)a->vc; k.cos_t = a->cos_t; k.sin_t = a->sin_t; k.causal = a->causal; k.text_len = a->text_len;
  return DIA_OK;
}

// what the K/V append and the attention need of the shared arguments, whatever format the caches have
bool kv_shape_ok(const dia_dec_prefill_args* a) { return a->q && a->cos_t && a->sin_t && a->kv_heads > 0; }
bool attn_shape_ok(const dia_dec_prefill_args* a) {
  return kv_shape_ok(a) && a->P && a->q_heads > 0 && a->q_heads % a->kv_heads == 0 && a->p_plane_stride % 8 == 0 &&
         (a->q_heads * 128 + 31) / 32 <= a->p_ktiles;
}

}  // namespace

extern "C" int dia_dec_prefill_embed(const dia_dec_prefill_args* a, void* stream) {
  PrefK k; int rc = fill(a, k); if (rc) return rc;
  if (!a->tokens || !a->emb || !a->x || !a->P || !a->ssq || a->C <= 0 || a->C > 16 || a->D % 16 != 0 || a->p_ktiles * 32 < a->D || a->p_plane_stride % 8 != 0)
    return dia_fail(DIA_E_ARG, "dia_dec_prefill_embed: bad argument");
  dia_launch<k_prefill_embed>(dim3(a->rows), dim3(256), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_prefill_embed");
}

extern "C" int dia_dec_prefill_kv(const dia_dec_prefill_args* a, void* stream) {
  PrefK k; int rc = fill(a, k); if (rc) return rc;
  if (!kv_shape_ok(a) || !a->kc || !a->vc || a->kv_cap % 32 != 0)
    return dia_fail(DIA_E_ARG, "dia_dec_prefill_kv: bad argument");
  dia_launch<k_prefill_kv>(dim3(a->kv_heads, a->rows / 32), dim3(256), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_prefill_kv");
}

namespace {
// what both fp8 entry points refuse before they look at anything else; `who` prefixes the message
int fill_f8(const char* who, const dia_dec_prefill_args* a, const dia_kv_fp8_ptrs* f, PrefK& k, PrefF8& f8) {
  static thread_local char msg[160];
  auto fail = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return dia_fail(DIA_E_ARG, msg); };
  if (!a || !f) return fail("null argument");
  if (!f->k8 || !f->v8 || !f->ks || !f->vs) return fail("null argument (k8 / v8 / ks / vs)");
  if (a->kc || a->vc) return fail("kc / vc must be NULL: the fp8 self caches are the only caches of this call");
  if (!a->causal) return fail("causal must be 1 (the cross caches stay bf16: dia_dec_prefill_attn serves the cross call)");
  if (a->kv_cap <= 0 || a->kv_cap % 32 != 0) return fail("kv_cap must be a positive multiple of 32");
  if (((uintptr_t)f->k8 | (uintptr_t)f->v8) % 16 != 0 || ((uintptr_t)f->ks | (uintptr_t)f->vs) % 4 != 0)
    return fail("k8 / v8 must be 16-byte aligned, ks / vs 4-byte");
  const int rc = fill(a, k);
  if (rc) return rc;
  f8 = PrefF8{(uint8_t*)f->k8, (uint8_t*)f->v8, f->ks, f->vs};
  return DIA_OK;
}
}  // namespace

extern "C" int dia_dec_prefill_kv_fp8(const dia_dec_prefill_args* a, const dia_kv_fp8_ptrs* f, void* stream) {
  PrefK k; PrefF8 f8; int rc = fill_f8("dia_dec_prefill_kv_fp8", a, f, k, f8); if (rc) return rc;
  if (!kv_shape_ok(a)) return dia_fail(DIA_E_ARG, "dia_dec_prefill_kv_fp8: bad argument");
  dia_launch<k_prefill_kv_f8>(dim3(a->kv_heads, a->rows / 32), dim3(256), 0, (hipStream_t)stream, k, f8);
  return dia_check_launch("k_prefill_kv_f8");
}

extern "C" int dia_dec_prefill_attn_fp8(const dia_dec_prefill_args* a, const dia_kv_fp8_ptrs* f, void* stream) {
  PrefK k; PrefF8 f8; int rc = fill_f8("dia_dec_prefill_attn_fp8", a, f, k, f8); if (rc) return rc;
  if (!attn_shape_ok(a)) return dia_fail(DIA_E_ARG, "dia_dec_prefill_attn_fp8: bad argument");
  dia_launch<k_prefill_attn_f8>(dim3(a->q_heads, a->rows / 16), dim3(256), 0, (hipStream_t)stream, k, f8);
  return dia_check_launch("k_prefill_attn_f8");
}

extern "C" int dia_dec_prefill_attn(const dia_dec_prefill_args* a, void* stream) {
  PrefK k; int rc = fill(a, k); if (rc) return rc;
  if (!attn_shape_ok(a) || !a->kc || !a->vc || a->kv_cap % 32 != 0 || (!a->causal && !a->text_len))
    return dia_fail(DIA_E_ARG, "dia_dec_prefill_attn: bad argument");
  dia_launch<k_prefill_attn>(dim3(a->q_heads, a->rows / 16), dim3(256), 0, (hipStream_t)stream, k);
  return dia_check_launch("k_prefill_attn");
}
