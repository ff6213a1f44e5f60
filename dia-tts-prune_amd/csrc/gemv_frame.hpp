// The frame of the decode weight-stream kernels: k_gemv24 (gemm_sparse.hip), k_gemm_mx (gemm_mx.hip) and k_gemm_us (gemm_us.hip).
// One workgroup owns a 16-column strip (persistent form: several), its waves split K, and around each kernel's own inner loop
// (weight addressing, load_strip, fragment expansion, MFMAs) all three do the same things, kept here once:
//   LDS prefix     wave partial tiles, split-K tile, row scales; the kernel's own LDS (tables, activation image) follows
//   image          M <= 4: the workgroup's K range of 4 activation rows as three bf16 planes in LDS, loaded before the weight
//                  stream starts and split and stored behind it
//   row scales     the 16 strip partials of a row requested at once before the stream, reduced into inv_s behind it
//   wave sum       the waves' partial tiles through LDS, summed in wave order, one tile element per thread
//   finish         cross-workgroup split-K hand-off (splitk_combine), then the element-per-thread epilogue (run_epilogue_rows)
//   strip loop     the persistent form's walk over strip pairs with two weight buffers
// and on the host the refusals, the split-K check and the sk / ktw / spw preamble common to the streams.
//
// Order every kernel keeps (the helpers hold no wait, barrier or scheduling barrier of their own; the kernels place them):
//   gf_image_load, gf_scales_load, the kernel's own small loads     L2-resident operands requested
//   __builtin_amdgcn_sched_barrier(0); load_strip; sched_barrier(0)  the HBM stream starts behind them and ahead of all else
//   gf_image_store, gf_scales_reduce, the kernel's own tables        their latency overlaps the stream's
//   lds_barrier()
#pragma once
#include "gemm_common.hpp"
#include <cstdio>

namespace {

constexpr int GF_MAXW = 8;                         // waves per workgroup

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// ---- LDS prefix: red [2][GF_MAXW][64] f32x4 (double-buffered wave tiles), tile [16][17] (split-K hand-off), inv_s [16]
struct GfLds {
  f32x4* red;
  float* tile;
  float* inv_s;
  unsigned char* rest;                             // first byte behind the prefix (16-byte aligned)
};
constexpr size_t gf_lds_bytes() { return sizeof(f32x4) * 2 * GF_MAXW * 64 + sizeof(float) * (16 * 17 + 16); }
// the image of `ktiles` dense k-tiles: [plane][k-tile][quarter][4 rows] bf16x8
constexpr size_t gf_image_bytes(int ktiles) { return (size_t)DIA_NPLANES * ktiles * 4 * 4 * 16; }

__device__ __forceinline__ GfLds gf_lds(unsigned char* smem) {
  GfLds L;
  L.red = reinterpret_cast<f32x4*>(smem);
  L.tile = reinterpret_cast<float*>(smem + sizeof(f32x4) * 2 * GF_MAXW * 64);
  L.inv_s = L.tile + 16 * 17;
  L.rest = smem + gf_lds_bytes();
  return L;
}

// ---- activation image (M <= 4).  KD = dense k-tiles per wave; a thread carries gf_image_ce(KD) entries of 8 fp32 values
constexpr int gf_image_ce(int kd) { return (kd * 4 * 4 + 63) / 64; }

// before the weight stream: request this thread's entries (rows >= M re-read the last valid row; they are never stored)
template <int KD>
__device__ __forceinline__ void gf_image_load(const GemmK& p, int tid, int NT, float4* ex, float4* ey) {
  const float* Af = reinterpret_cast<const float*>(p.A);
  const int ktw = (NT >> 6) * KD, nentries = ktw * 16;
  const long kta = (long)blockIdx.y * ktw;           // first dense activation k-tile of the workgroup's range
#pragma unroll
  for (int u = 0; u < gf_image_ce(KD); ++u) {
    const int c = min(tid + u * NT, nentries - 1);
    const int row = c % 4, kq = (c / 4) & 3, kt = c / 16;
    const float4* src = reinterpret_cast<const float4*>(Af + ((kta + kt) * 64 + min(row, p.M - 1) + 16 * kq) * 8);
    ex[u] = src[0]; ey[u] = src[1];
  }
}
// behind it: hi / mid / lo planes into As
template <int KD>
__device__ __forceinline__ void gf_image_store(bf16x8* As, int tid, int NT, const float4* ex, const float4* ey) {
  const int nentries = (NT >> 6) * KD * 16;
#pragma unroll
  for (int u = 0; u < gf_image_ce(KD); ++u)
    if (tid + u * NT < nentries) {
      const int c = tid + u * NT;
      bf16x8 h, mi, lo;
      split3x8(ex[u], ey[u], h, mi, lo);
      As[c] = h; As[nentries + c] = mi; As[2 * nentries + c] = lo;
    }
}

// ---- row scales: 8 threads per row, 16 strip partials each requested at once on clamped addresses (as k_gemv_small: a loop of
// dependent loads here delayed the weight stream by 4 us in the step); summed after the weight loads are in flight
__device__ __forceinline__ void gf_scales_load(const GemmK& p, int tid, float* sq) {
#pragma unroll
  for (int i = 0; i < 16; ++i) sq[i] = 0.f;
  if (tid < 128 && p.ssq_in != nullptr) {
    const float* sp = p.ssq_in + min(tid >> 3, p.M - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) sq[i] = sp[(long)min((tid & 7) + 8 * i, p.ssq_in_n - 1) * p.ssq_ld];
  }
}
__device__ __forceinline__ void gf_scales_reduce(const GemmK& p, int tid, int NT, const float* sq, float* inv_s) {
  const bool has_norm = p.ssq_in != nullptr;
  for (int t = tid; t < 128; t += NT) {              // (a one-wave workgroup also serves rows 8..15, loading them here)
    const int r = t >> 3, part = t & 7;
    float s0 = 0.f;
    if (t == tid) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s0 += (part + 8 * i < p.ssq_in_n && r < p.M) ? sq[i] : 0.f;
      if (has_norm && r < p.M)
        for (int i = part + 128; i < p.ssq_in_n; i += 8) s0 += p.ssq_in[(long)i * p.ssq_ld + r];   // D > 2048 only
    } else if (has_norm && r < p.M) {
      for (int i = part; i < p.ssq_in_n; i += 8) s0 += p.ssq_in[(long)i * p.ssq_ld + r];
    }
    s0 += __shfl_xor(s0, 1, 64);
    s0 += __shfl_xor(s0, 2, 64);
    s0 += __shfl_xor(s0, 4, 64);
    if (part == 0) inv_s[r] = has_norm ? rsqrtf(s0 * p.inv_d + p.eps) : 1.0f;
  }
}

// ---- wave sum.  RS = rows the tile carries (4 or 16).  WA = the weights are the A operand (k_gemv24), so the accumulator is
// transposed: element (row m, column c) sits in lane 16 (c >> 2) + m, register c & 3; otherwise in lane 16 (m >> 2) + c,
// register m & 3.  A thread finishes gf_ne(RS) elements e = tid + u NT = 16 m + c (at least one wave per workgroup).
constexpr int gf_ne(int rs) { return (16 * rs + 63) / 64; }

// the wave's tile into the current red buffer: the lanes that hold rows < RS
template <int RS, bool WA>
__device__ __forceinline__ void gf_tile_store(f32x4* rb, int w, int lane, f32x4 acc) {
  if (RS == 16 || (WA ? (lane & 15) < RS : lane < 16)) rb[w * 64 + lane] = acc;
}
// behind the barrier: this thread's elements, summed over the waves in wave order
template <int RS, bool WA>
__device__ __forceinline__ void gf_wave_sum(const f32x4* rb, int tid, int NT, float* vs) {
  const int NW = NT >> 6;
#pragma unroll
  for (int u = 0; u < gf_ne(RS); ++u) {
    const int e = tid + u * NT;
    vs[u] = 0.f;
    if (e < 16 * RS) {
      const int m = e >> 4, c = e & 15;
      const float* rf = reinterpret_cast<const float*>(rb) + (WA ? ((c >> 2) * 16 + m) * 4 + (c & 3) : ((m >> 2) * 16 + c) * 4 + (m & 3));
      float v = rf[0];
      for (int ww = 1; ww < NW; ++ww) v += rf[ww * 256];
      vs[u] = v;
    }
  }
}

// ---- finish: the last statement of a strip's body (a workgroup that is not the last arriver of a split-K strip ends here)
template <int RS, bool MULTI>
__device__ __forceinline__ void gf_finish(const GemmK& p, const GfLds& L, float* vs, int tid, int NT, int strip) {
  __shared__ int sk_flag;
  float* tile = L.tile;
  if (!MULTI && gridDim.y > 1) {   // cross-workgroup split-K (wo): the last arriver sums the slabs in split order and runs the epilogue
#pragma unroll
    for (int u = 0; u < gf_ne(RS); ++u)
      if (tid + u * NT < 16 * RS) tile[((tid + u * NT) >> 4) * 17 + ((tid + u * NT) & 15)] = vs[u];
    // (splitk_combine publishes all 16 rows of the tile: rows RS.. carry zeros, never read back)
    if constexpr (RS < 16)
      for (int e = 16 * RS + tid; e < 256; e += NT) tile[(e >> 4) * 17 + (e & 15)] = 0.f;
    lds_barrier();
    if (!splitk_combine(p, tile, strip, tid, &sk_flag)) return;
#pragma unroll
    for (int u = 0; u < gf_ne(RS); ++u)
      if (tid + u * NT < 16 * RS) vs[u] = tile[((tid + u * NT) >> 4) * 17 + ((tid + u * NT) & 15)];
  }
#pragma unroll
  for (int u = 0; u < gf_ne(RS); ++u) {
    const int e = tid + u * NT;
    if (e >= 16 * RS) break;
    float xpre1 = 0.f, gpre1 = 1.f;
    if (p.epi == DIA_EPI_RESID_EMIT) {
      const int m = e >> 4, n = strip * 16 + (e & 15);
      xpre1 = p.out[(long)min(m, p.M - 1) * p.ldo + n];
      gpre1 = p.gnext[n];
    }
    run_epilogue_rows<RS, true>(p, vs[u], L.inv_s, e, strip, xpre1, gpre1);
  }
}

// ---- strip loop.  MULTI: the workgroup walks strips blockIdx.x, + gridDim.x, ... as pairs, then at most one more (see
// k_gemv_small); `fwd` runs the body on the kernel's weight buffers 0 with the next strip prefetched into buffers 1, `back` the
// other way round.  Otherwise one strip, `fwd` alone.
template <bool MULTI, class Fwd, class Back>
__device__ __forceinline__ void gf_strips(int nstrips, Fwd&& fwd, Back&& back) {
  if constexpr (MULTI) {
    const int G = gridDim.x;
    int strip = blockIdx.x;
    for (; strip + G < nstrips; strip += 2 * G) {
      [[clang::always_inline]] fwd(strip);
      [[clang::always_inline]] back(strip + G);
    }
    if (strip < nstrips) [[clang::always_inline]] fwd(strip);
  } else {
    [[clang::always_inline]] fwd(blockIdx.x);
  }
}

// ---- host side
struct GfShape { int sk, ktw, spw; };              // split-K factor (>= 1), k-tiles per workgroup, strips per workgroup
inline GfShape gf_shape(const dia_gemm_args* a) {
  const int sk = a->sk > 1 ? a->sk : 1;
  return {sk, a->KT / sk, stream_spw(a->spw, a->nstrips)};   // (persistent form: next strip's weights in flight during this one's epilogue)
}

// "dia_gemm: the <name> stream <what>" (dia_fail copies its message)
inline int gf_refuse(const char* name, const char* what) {
  char msg[224];
  snprintf(msg, sizeof msg, "dia_gemm: the %s stream %s", name, what);
  return dia_fail(DIA_E_ARG, msg);
}

// what no stream serves.  The 2:4 stream words two of the refusals its own way: `one_plane`, `tiles`
inline int gf_check_common(const dia_gemm_args* a, const char* name, int max_rows,
                           const char* one_plane = "holds one weight encoding (w_planes must be 0 or 1)",
                           const char* tiles = "needs fp32 activation tiles in and out (act_f32 = 3), not planes") {
  if (a->w_planes > 1) return gf_refuse(name, one_plane);
  if (a->w_layout == 1) return gf_refuse(name, "has no diagonal layout (w_layout must be 0)");
  if (a->sp_blocks || a->sp_toff) return gf_refuse(name, "and the zero-skipping stream (sp_blocks) exclude each other");
  if (a->epi == DIA_EPI_CROSSKV) return gf_refuse(name, "has no CROSSKV epilogue (prefill only)");
  if (a->cmap || a->strip_map) return gf_refuse(name, "has no compaction maps (cmap / strip_map)");
  char rows[32];
  snprintf(rows, sizeof rows, "serves at most %d rows", max_rows);
  if (a->M > max_rows) return gf_refuse(name, rows);
  const bool emits = a->epi == DIA_EPI_RESID_EMIT || a->epi == DIA_EPI_SWIGLU_EMIT;
  if (!(a->act_f32 & 1) || (emits && !(a->act_f32 & 2))) return gf_refuse(name, tiles);
  if (a->epi == DIA_EPI_RESID_EMIT && !a->gnext) return gf_refuse(name, "needs gnext with RESID_EMIT");
  return DIA_OK;
}

inline int gf_check_splitk(const dia_gemm_args* a) {
  if (a->sk > 1 && (!a->sk_scratch || !a->sk_tickets || a->KT % a->sk != 0))
    return dia_fail(DIA_E_ARG, "dia_gemm: split-K needs sk_scratch, sk_tickets and KT % sk == 0");
  return DIA_OK;
}

}  // namespace
