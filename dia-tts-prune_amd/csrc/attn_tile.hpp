// The many-query attention tile: a workgroup of 4 waves owns (one head, 16 packed query rows), the waves split the keys in
// 32-key granules, each keeps an online softmax per query row and the four are merged through LDS.  Three kernels run it —
// k_attn_enc_mfma (attn.hip: encoder, K / V as three bf16 planes), k_prefill_attn and k_prefill_attn_f8 (prefill.hip: decoder
// prompt over bf16 / e4m3 caches).  The stages that do not depend on where K and V come from are here, ONE spelling each, so
// that the kernels round alike by construction (test_attention_bitwise_against_the_bf16_kernel); each kernel keeps its
// prologue, its pointers and its granule loop with the K / V loads and the MFMAs.
//
// Lane roles inside a wave: arow = lane & 15, akq = lane >> 4.  A score tile S[t][r] is (query row 4*akq + r, key
// key0 + 16t + arow), an output tile O[nb][r] is (query row 4*akq + r, dim 16*nb + arow).
#pragma once
#include "common.hpp"

struct AttnTile {
  static constexpr int NWV = 4, HD = 128;
  bf16_raw qf[4][DIA_NPLANES][16][4][8];      // q planes, A-fragment order: [k-step][plane][row][akq][8]
  bf16_raw pbuf[NWV][DIA_NPLANES][16][32];    // p planes of each wave's current granule
  float part[NWV * 16 * HD];                  // each wave's O, its running maximum and its softmax sum
  float pm_s[NWV * 16], pl_s[NWV * 16];
};
static_assert(sizeof(AttnTile) == 57856, "two workgroups per CU");

// RoPE(q) of the 16 rows -> three planes in LDS: thread (row tid >> 4, 4 dim pairs), the rotation rounded as
// fma(x1, c, -(x2*s)) / fma(x2, c, x1*s).  qh = the 128 fp32 q values of this thread's row and head, pos = its RoPE position;
// the caller clamps both for rows past the segment's end (recomputed, never emitted) and follows with __syncthreads().
__device__ __forceinline__ void attn_tile_stage_q(AttnTile& t, int tid, const float* qh, int pos, const float* cos_t, const float* sin_t) {
  const int r = tid >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = (tid & 15) * 4 + i;
    const float x1 = qh[d], x2 = qh[d + 64];
    const float c = cos_t[(long)pos * 64 + d], s = sin_t[(long)pos * 64 + d];
    const float qv[2] = {__builtin_fmaf(x1, c, -mul_rn(x2, s)), __builtin_fmaf(x2, c, mul_rn(x1, s))};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int D = d + 64 * e;
      __bf16 a, bb, c3;
      split3(qv[e], a, bb, c3);
      t.qf[D >> 5][0][r][(D >> 3) & 3][D & 7] = *reinterpret_cast<const bf16_raw*>(&a);
      t.qf[D >> 5][1][r][(D >> 3) & 3][D & 7] = *reinterpret_cast<const bf16_raw*>(&bb);
      t.qf[D >> 5][2][r][(D >> 3) & 3][D & 7] = *reinterpret_cast<const bf16_raw*>(&c3);
    }
  }
}

// Online softmax of one granule's two score tiles.  lim[r] = keys that query row 4*akq + r may see (scores of keys at or
// past it are masked).  Updates mrun / lrun, returns the factors alpha[r] that O is to be rescaled by, and leaves the p planes
// in pbuf[w], readable by the whole wave on return.  SCALED (e4m3 caches): ksc[t] / vsc[t] are the power-of-two K / V scales
// of key key0 + 16t + arow — the score takes ksc before the softmax scale, p takes vsc before split3, lrun sums the unscaled p.
template <bool SCALED>
__device__ __forceinline__ void attn_tile_softmax(AttnTile& t, int w, int arow, int akq, const f32x4 (&S)[2], int key0, const int (&lim)[4],
                                                  const float* ksc, const float* vsc, float (&mrun)[4], float (&lrun)[4], float (&alpha)[4]) {
  const float scale = 0.08838834764831845f;      // 1 / sqrt(128)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool v0 = key0 + arow < lim[r], v1 = key0 + 16 + arow < lim[r];
    float s0, s1;
    if constexpr (SCALED) {
      s0 = v0 ? mul_rn(mul_rn(S[0][r], ksc[0]), scale) : -INFINITY; s1 = v1 ? mul_rn(mul_rn(S[1][r], ksc[1]), scale) : -INFINITY;
    } else {
      s0 = v0 ? S[0][r] * scale : -INFINITY; s1 = v1 ? S[1][r] * scale : -INFINITY;
    }
    const float mnew = fmaxf(mrun[r], row16_max(fmaxf(s0, s1)));
    alpha[r] = (mrun[r] == -INFINITY) ? 0.f : expf(mrun[r] - mnew);
    float p0 = (s0 == -INFINITY) ? 0.f : expf(s0 - mnew), p1 = (s1 == -INFINITY) ? 0.f : expf(s1 - mnew);
    lrun[r] = __builtin_fmaf(lrun[r], alpha[r], row16_sum(p0 + p1));
    mrun[r] = mnew;
    if constexpr (SCALED) { p0 = mul_rn(p0, vsc[0]); p1 = mul_rn(p1, vsc[1]); }
    __bf16 a, bb, c3;
    split3(p0, a, bb, c3);
    t.pbuf[w][0][4 * akq + r][arow] = *reinterpret_cast<const bf16_raw*>(&a);
    t.pbuf[w][1][4 * akq + r][arow] = *reinterpret_cast<const bf16_raw*>(&bb);
    t.pbuf[w][2][4 * akq + r][arow] = *reinterpret_cast<const bf16_raw*>(&c3);
    split3(p1, a, bb, c3);
    t.pbuf[w][0][4 * akq + r][16 + arow] = *reinterpret_cast<const bf16_raw*>(&a);
    t.pbuf[w][1][4 * akq + r][16 + arow] = *reinterpret_cast<const bf16_raw*>(&bb);
    t.pbuf[w][2][4 * akq + r][16 + arow] = *reinterpret_cast<const bf16_raw*>(&c3);
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Merge the four waves and emit: every wave leaves O / mrun / lrun in LDS, then thread (row r = tid >> 4, dims d0 = 8 * (tid & 15)..)
// sums the waves' parts at the common maximum, divides by the softmax sum and writes packed row m0 + r, columns k0 + d0.. of the
// planes P — rows at or past m_end (padding inside a segment's last tile) are not written.
// Rounding order: the softmax sum accumulates by a rounded product and a rounded add, dims 0..FUSED-1 of a thread's eight by
// fused multiply-add and the rest like the sum.  FUSED is 6 in the two prefill kernels and 8 in the encoder kernel — the
// contraction each had before the order was written down, kept so that no output bit moves.
template <int FUSED>
__device__ __forceinline__ void attn_tile_merge_emit(AttnTile& t, int tid, const f32x4 (&O)[8], const float (&mrun)[4], const float (&lrun)[4],
                                                     int m0, int m_end, bf16_raw* P, long p_plane_stride, int p_ktiles, int k0) {
  constexpr int NWV = AttnTile::NWV, HD = AttnTile::HD;
  const int lane = tid & 63, w = tid >> 6, arow = lane & 15, akq = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) t.part[(w * 16 + 4 * akq + r) * HD + 16 * nb + arow] = O[nb][r];
    if (arow == 0) { t.pm_s[w * 16 + 4 * akq + r] = mrun[r]; t.pl_s[w * 16 + 4 * akq + r] = lrun[r]; }
  }
  __syncthreads();
  const int r = tid >> 4, d0 = (tid & 15) * 8, m = m0 + r;
  if (m >= m_end) return;
  float mm = -INFINITY;
#pragma unroll
  for (int ww = 0; ww < NWV; ++ww) mm = fmaxf(mm, t.pm_s[ww * 16 + r]);
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, Ls = 0.f;
#pragma unroll
  for (int ww = 0; ww < NWV; ++ww) {
    const float pmw = t.pm_s[ww * 16 + r];
    const float f = (pmw == -INFINITY) ? 0.f : expf(pmw - mm);
    Ls = add_rn(Ls, mul_rn(t.pl_s[ww * 16 + r], f));
#pragma unroll
    for (int j = 0; j < FUSED; ++j) o[j] = __builtin_fmaf(t.part[(ww * 16 + r) * HD + d0 + j], f, o[j]);
#pragma unroll
    for (int j = FUSED; j < 8; ++j) o[j] = add_rn(o[j], mul_rn(t.part[(ww * 16 + r) * HD + d0 + j], f));
  }
  const float inv = Ls > 0.f ? 1.0f / Ls : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] *= inv;
  emit_planes8(P, p_plane_stride, p_ktiles, m, k0 + d0, o);
}
