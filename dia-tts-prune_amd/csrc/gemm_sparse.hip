// 2:4 sparse decode GEMV: out[M][N] = X[M][K] . W[K][N] for M <= 16 rows with W 2:4-pruned along K and streamed in the
// compressed form of dia_hip/layout.py tile_weight_24 (dia_gemm_args.w_format = DIA_W_SPARSE24).
//
// Mapping (CDNA4): v_smfmac_f32_16x16x64_bf16 takes a 2:4-compressed 16 x 64 A operand (8 bf16 + a 16-bit index word per lane)
// and a dense 64 x 16 B operand (16 bf16 per lane).  The WEIGHTS are the A operand — the reverse of the dense kernels, where they
// feed B — so the accumulator tile is transposed: its rows are the 16 output columns of the strip, its columns the activation
// rows (lane l, element i of the f32x4 = column 4 (l >> 4) + i of the strip, activation row l & 15).  The B operand of sparse
// k-tile t is the A fragment pair of dense k-tiles 2t and 2t + 1 of the fp32 activation tiles, split into hi / mid / lo bf16
// in registers: three smfmac per sparse k-tile, products exact w.r.t. the fp32 activations as in the dense kernels.
//
// One workgroup owns one 16-column strip (persistent form: several, the next one's weights streaming during this one's
// reduction and epilogue); its waves split K into ranges of KPW sparse k-tiles = KPW / 8 stream groups (metadata block +
// 8 value slots, 9 KiB); gridDim.y > 1 splits K across workgroups (wo) with the dense path's hand-off (splitk_combine).
// Every weight load of a wave is issued before its first smfmac.  Activations:
//   RS = 4   M <= 4: the workgroup's K range of the first 4 rows is staged once into LDS as bf16 planes (as k_gemv_small)
//   RS = 16  5..16 rows (and M <= 4 when that image would not fit): each wave loads its fragments from the fp32 tiles, ahead of
//            its weights; one strip per workgroup (the persistent form would hold the fragments and two weight buffers: spills)
// Partial tiles of the waves are summed through LDS in wave order; the element-per-thread epilogue (run_epilogue_rows) follows.
#include "gemm_common.hpp"

namespace {

constexpr int SP_GROUP = 8;                  // sparse k-tiles per stream group (layout.SP24_GROUP)
constexpr int SP_SLOTS = SP_GROUP + 1;       // metadata block + value slots, 1 KiB each
constexpr int SP_MAXW = 8;                   // waves per workgroup

typedef __attribute__((ext_vector_type(16))) __bf16 bf16x16;

__device__ __forceinline__ bf16x16 cat16(const bf16x8 lo, const bf16x8 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
}

constexpr size_t sp_smem_fixed() { return sizeof(f32x4) * 2 * SP_MAXW * 64 + sizeof(float) * (16 * 17 + 16); }
size_t sp_smem(int kt32w, int rs) { return sp_smem_fixed() + (rs == 4 ? (size_t)DIA_NPLANES * kt32w * 4 * rs * 16 : 0); }

template <int KPW, int RS, bool MULTI>
__global__ __launch_bounds__(SP_MAXW * 64) void k_gemv24(GemmK p) {
  static_assert(KPW % SP_GROUP == 0, "whole stream groups per wave");
  constexpr int NG = KPW / SP_GROUP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                                   // [2][SP_MAXW][64]
  float* tile = reinterpret_cast<float*>(smem_raw + sizeof(f32x4) * 2 * SP_MAXW * 64); // [16][17] (split-K hand-off)
  float* inv_s = tile + 16 * 17;                                                     // [16]
  bf16x8* As = reinterpret_cast<bf16x8*>(inv_s + 16);                               // RS = 4: [plane][kt32][kq][row]
  __shared__ int sk_flag;

  const int NT = blockDim.x, NW = NT >> 6;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ktw = NW * KPW;                          // sparse k-tiles of this workgroup's K range
  const int kt0 = blockIdx.y * ktw + w * KPW;        // first global sparse k-tile of this wave
  const int G = gridDim.x;
  const long strip_len = (long)(p.KT / SP_GROUP) * SP_SLOTS * 64;                   // bf16x8 per strip
  const bf16x8* Wl = reinterpret_cast<const bf16x8*>(p.W) + (long)(kt0 / SP_GROUP) * SP_SLOTS * 64 + lane;
  auto load_strip = [&](bf16x8* b, u32x4* mt, int strip) {
    const bf16x8* Wt = Wl + (long)strip * strip_len;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      mt[g] = __builtin_bit_cast(u32x4, DIA_WLOAD(Wt + (long)g * SP_SLOTS * 64));
#pragma unroll
      for (int i = 0; i < SP_GROUP; ++i) b[g * SP_GROUP + i] = DIA_WLOAD(Wt + (long)(g * SP_SLOTS + 1 + i) * 64);
    }
  };
  const float* Af = reinterpret_cast<const float*>(p.A);

  // ---- small, L2-resident operands first (see k_gemv_small): activation image / fragments, row scales
  constexpr int CE = (2 * KPW * 4 * RS + 63) / 64;    // RS = 4: image entries per thread (2 KPW dense k-tiles x 4 quarters x RS rows per wave)
  const int kt32w = 2 * ktw, nentries = kt32w * 4 * RS;
  float4 ex[RS == 4 ? CE : 1], ey[RS == 4 ? CE : 1];
  constexpr int AP = (RS == 16 && KPW <= 8) ? KPW : 1;   // RS = 16: fragments of the wave's k-tiles held from the start
  float4 af[AP][4];
  const int alane = (lane & 48) | min(lane & 15, p.M - 1);   // rows >= M re-read the last valid row (never stored)
  auto load_frag = [&](float4* f, int t) {               // the two dense k-tiles of global sparse k-tile t, this lane's 8 + 8 values
    const float4* s0 = reinterpret_cast<const float4*>(Af + ((long)(2 * t) * 64 + alane) * 8);
    const float4* s1 = reinterpret_cast<const float4*>(Af + ((long)(2 * t + 1) * 64 + alane) * 8);
    f[0] = s0[0]; f[1] = s0[1]; f[2] = s1[0]; f[3] = s1[1];
  };
  if constexpr (RS == 4) {
    const long kta = (long)blockIdx.y * kt32w;         // first dense activation k-tile of the range
#pragma unroll
    for (int u = 0; u < CE; ++u) {
      const int c = min(tid + u * NT, nentries - 1);
      const int row = c % RS, kq = (c / RS) & 3, kt = c / (4 * RS);
      const float4* src = reinterpret_cast<const float4*>(Af + ((kta + kt) * 64 + row + 16 * kq) * 8);
      ex[u] = src[0]; ey[u] = src[1];
    }
  } else if constexpr (AP == KPW) {
#pragma unroll
    for (int i = 0; i < KPW; ++i) load_frag(af[i], kt0 + i);
  }
  // row scales: 8 threads per row, 16 strip partials each requested at once on clamped addresses (as k_gemv_small: a loop of
  // dependent loads here delayed the weight stream by 4 us in the step); summed after the weight loads are in flight
  const bool has_norm = p.ssq_in != nullptr;
  const int s_row = tid >> 3, s_part = tid & 7;
  const bool s_thread = tid < 128 && has_norm;
  float sq[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) sq[i] = 0.f;
  if (s_thread) {
    const float* sp = p.ssq_in + min(s_row, p.M - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) sq[i] = sp[(long)min(s_part + 8 * i, p.ssq_in_n - 1) * p.ssq_ld];
  }
  __builtin_amdgcn_sched_barrier(0);
  bf16x8 b0[KPW], b1[MULTI ? KPW : 1];
  u32x4 m0[NG], m1[MULTI ? NG : 1];
  load_strip(b0, m0, blockIdx.x);                     // the HBM stream starts here
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (RS == 4) {
#pragma unroll
    for (int u = 0; u < CE; ++u)
      if (tid + u * NT < nentries) {
        const int c = tid + u * NT;
        bf16x8 h, mi, lo;
        split3x8(ex[u], ey[u], h, mi, lo);
        As[c] = h; As[nentries + c] = mi; As[2 * nentries + c] = lo;
      }
  }
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
  lds_barrier();                                      // image + row scales visible; the weight loads stay in flight

  const int arow = min(lane & 15, RS - 1), akq = lane >> 4;
  int sbuf = 0;
  auto body = [&](bf16x8* bc, u32x4* mc, bf16x8* bn, u32x4* mn, int strip) {
    const int next = strip + G;
    if constexpr (MULTI) load_strip(bn, mn, DIA_PREFETCH_CLAMP(next, p.nstrips));   // unconditional: see k_gemv_small
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
      bf16x8 h[2], mi[2], lo[2];
      if constexpr (RS == 4) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int kt = 2 * (w * KPW + i) + hf;        // dense k-tile inside the image
          h[hf] = As[(kt * 4 + akq) * RS + arow];
          mi[hf] = As[nentries + (kt * 4 + akq) * RS + arow];
          lo[hf] = As[2 * nentries + (kt * 4 + akq) * RS + arow];
        }
      } else {
        float4 f[4];
        if constexpr (AP == KPW) { f[0] = af[i < AP ? i : 0][0]; f[1] = af[i < AP ? i : 0][1]; f[2] = af[i < AP ? i : 0][2]; f[3] = af[i < AP ? i : 0][3]; }
        else load_frag(f, kt0 + i);
        split3x8(f[0], f[1], h[0], mi[0], lo[0]);
        split3x8(f[2], f[3], h[1], mi[1], lo[1]);
      }
      const unsigned word = mc[i / SP_GROUP][(i % SP_GROUP) >> 1];
      // index word of k-tile i: bits 0-15 (abid 0) for even, 16-31 (abid 1) for odd k-tiles of the group
      if ((i & 1) == 0) {
        acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(bc[i], cat16(h[0], h[1]), acc, (int)word, 0, 0);
        acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(bc[i], cat16(mi[0], mi[1]), acc, (int)word, 0, 0);
        acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(bc[i], cat16(lo[0], lo[1]), acc, (int)word, 0, 0);
      } else {
        acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(bc[i], cat16(h[0], h[1]), acc, (int)word, 0, 1);
        acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(bc[i], cat16(mi[0], mi[1]), acc, (int)word, 0, 1);
        acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(bc[i], cat16(lo[0], lo[1]), acc, (int)word, 0, 1);
      }
    }
    // cross-wave sum: element (row m, column c) of the output tile sits in lane 16 (c >> 2) + m, register c & 3 of every wave
    f32x4* rb = red + sbuf * (SP_MAXW * 64);
    sbuf ^= 1;
    if (RS == 16 || (lane & 15) < RS) rb[w * 64 + lane] = acc;
    lds_barrier();
    const bool split = !MULTI && gridDim.y > 1;
    constexpr int NE = (16 * RS + 63) / 64;          // epilogue elements per thread (at least one wave per workgroup)
    float vs[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + u * NT;
      vs[u] = 0.f;
      if (e < 16 * RS) {
        const int m = e >> 4, c = e & 15;
        const float* rf = reinterpret_cast<const float*>(rb) + ((c >> 2) * 16 + m) * 4 + (c & 3);
        float v = rf[0];
        for (int ww = 1; ww < NW; ++ww) v += rf[ww * 256];
        vs[u] = v;
        if (split) tile[m * 17 + c] = v;
      }
    }
    if (split) {            // cross-workgroup split-K (wo): the last arriver sums the slabs in split order and runs the epilogue
      // (splitk_combine publishes all 16 rows of the tile: rows RS.. carry zeros, never read back)
      if constexpr (RS < 16)
        for (int e = 16 * RS + tid; e < 256; e += NT) tile[(e >> 4) * 17 + (e & 15)] = 0.f;
      lds_barrier();
      if (!splitk_combine(p, tile, strip, tid, &sk_flag)) return;
#pragma unroll
      for (int u = 0; u < NE; ++u)
        if (tid + u * NT < 16 * RS) vs[u] = tile[((tid + u * NT) >> 4) * 17 + ((tid + u * NT) & 15)];
    }
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + u * NT;
      if (e >= 16 * RS) break;
      float xpre1 = 0.f, gpre1 = 1.f;
      if (p.epi == DIA_EPI_RESID_EMIT) {
        const int m = e >> 4, n = strip * 16 + (e & 15);
        xpre1 = p.out[(long)min(m, p.M - 1) * p.ldo + n];
        gpre1 = p.gnext[n];
      }
      run_epilogue_rows<RS, true>(p, vs[u], inv_s, e, strip, xpre1, gpre1);
    }
  };
  if constexpr (MULTI) {
    int strip = blockIdx.x;                            // strip pairs, then at most one more (see k_gemv_small)
    for (; strip + G < p.nstrips; strip += 2 * G) {
      body(b0, m0, b1, m1, strip);
      body(b1, m1, b0, m0, strip + G);
    }
    if (strip < p.nstrips) body(b0, m0, b1, m1, strip);
  } else {
    body(b0, m0, b1, m1, blockIdx.x);
  }
}

template <int KPW, int RS>
int launch24(const GemmK& k, int nw, int sk, int spw, hipStream_t st) {
  const size_t smem = sp_smem(2 * nw * KPW, RS);
  if (spw > 1 && sk == 1) {
    if constexpr (KPW == 8 && RS == 4) {     // (5..16 rows: the fragments held for every strip and two weight buffers spill — one strip per workgroup)
      launch_kernel<k_gemv24<KPW, RS, true>>(dim3((k.nstrips + spw - 1) / spw), dim3(nw * 64), smem, st, k);
      return dia_check_launch("k_gemv24");
    }
  }
  launch_kernel<k_gemv24<KPW, RS, false>>(dim3(k.nstrips, sk), dim3(nw * 64), smem, st, k);
  return dia_check_launch("k_gemv24");
}

}  // namespace

// dia_gemm with w_format == DIA_W_SPARSE24: what the sparse stream cannot serve (checked before dia_gemm's other weight forms)
int dia_gemm_sparse24_check(const dia_gemm_args* a) {
  if (a->w_planes > 1) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream holds one bf16 weight plane (w_planes must be 0 or 1)");
  if (a->w_layout == 1) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream has no diagonal layout (w_layout must be 0)");
  if (a->sp_blocks || a->sp_toff) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream and the zero-skipping stream (sp_blocks) exclude each other");
  if (a->epi == DIA_EPI_CROSSKV) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream has no CROSSKV epilogue (prefill only)");
  if (a->cmap || a->strip_map) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream has no compaction maps (cmap / strip_map)");
  if (a->M > 16) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream serves at most 16 rows");
  const bool emits = a->epi == DIA_EPI_RESID_EMIT || a->epi == DIA_EPI_SWIGLU_EMIT;
  if (!(a->act_f32 & 1) || (emits && !(a->act_f32 & 2)))
    return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream needs fp32 activation tiles in and out (act_f32 = 3)");
  if (!a->W) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream needs W");
  if (a->epi == DIA_EPI_RESID_EMIT && !a->gnext) return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream needs gnext with RESID_EMIT");
  if (2 * a->KT > a->a_ktiles) return dia_fail(DIA_E_ARG, "dia_gemm: weight K exceeds the activation tiles' K");
  return DIA_OK;
}

// the launch (dia_gemm has run dia_gemm_sparse24_check and its own argument checks)
int dia_gemm_sparse24(const dia_gemm_args* a, void* stream) {
  const int sk = a->sk > 1 ? a->sk : 1;
  if (sk > 1 && (!a->sk_scratch || !a->sk_tickets || a->KT % sk != 0)) return dia_fail(DIA_E_ARG, "dia_gemm: split-K needs sk_scratch, sk_tickets and KT % sk == 0");
  const int ktw = a->KT / sk;                          // sparse k-tiles per workgroup
  if (a->KT % SP_GROUP != 0 || ktw % SP_GROUP != 0)
    return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream needs K a multiple of 512 per workgroup (whole groups of 8 sparse k-tiles)");
  GemmK k;
  fill_gemmk(a, k);
  hipStream_t st = (hipStream_t)stream;
  int kpw = (ktw / 8 <= SP_MAXW) ? 8 : ((ktw % 16 == 0 && ktw / 16 <= SP_MAXW) ? 16 : 0);
  if (!kpw)
    return dia_fail(DIA_E_ARG, "dia_gemm: the 2:4 sparse stream needs the sparse k-tiles per workgroup (KT / sk) to be at most 64, "
                               "or a multiple of 16 up to 128 (K <= 8192 per workgroup; use split-K)");
  const int nw = ktw / kpw;
  const int spw = stream_spw(a->spw, a->nstrips);      // persistent form: next strip's weights in flight during this one's epilogue
  const bool image = a->M <= 4 && sp_smem(2 * ktw, 4) <= 150 * 1024;
  if (kpw == 8) return image ? launch24<8, 4>(k, nw, sk, spw, st) : launch24<8, 16>(k, nw, sk, spw, st);
  return launch24<16, 16>(k, nw, sk, 1, st);
}
