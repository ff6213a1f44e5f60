// 2:4 sparse decode GEMV: out[M][N] = X[M][K] . W[K][N] for M <= 16 rows with W 2:4-pruned along K and streamed in the
// compressed form of dia_hip/layout.py tile_weight_24 (dia_gemm_args.w_format = DIA_W_SPARSE24).  The frame around the inner
// loop (LDS prefix, activation image, row scales, wave sum, split-K hand-off, epilogue, strip loop) is gemv_frame.hpp's.
//
// Mapping (CDNA4): v_smfmac_f32_16x16x64_bf16 takes a 2:4-compressed 16 x 64 A operand (8 bf16 + a 16-bit index word per lane)
// and a dense 64 x 16 B operand (16 bf16 per lane).  The WEIGHTS are the A operand — the reverse of the dense kernels, where they
// feed B — so the accumulator tile is transposed: its rows are the 16 output columns of the strip, its columns the activation
// rows (lane l, element i of the f32x4 = column 4 (l >> 4) + i of the strip, activation row l & 15).  The B operand of sparse
// k-tile t is the A fragment pair of dense k-tiles 2t and 2t + 1 of the fp32 activation tiles, split into hi / mid / lo bf16
// in registers: three smfmac per sparse k-tile, products exact w.r.t. the fp32 activations as in the dense kernels.
//
// A wave's K range is KPW sparse k-tiles = KPW / 8 stream groups (metadata block + 8 value slots, 9 KiB) = 2 KPW dense k-tiles
// of the activations.  Every weight load of a wave is issued before its first smfmac.  Activations:
//   RS = 4   M <= 4: the frame's LDS image
//   RS = 16  5..16 rows (and M <= 4 when that image would not fit): each wave loads its fragments from the fp32 tiles, ahead of
//            its weights; one strip per workgroup (the persistent form would hold the fragments and two weight buffers: spills)
#include "gemv_frame.hpp"

namespace {

constexpr int SP_GROUP = 8;                  // sparse k-tiles per stream group (layout.SP24_GROUP)
constexpr int SP_SLOTS = SP_GROUP + 1;       // metadata block + value slots, 1 KiB each

typedef __attribute__((ext_vector_type(16))) __bf16 bf16x16;

__device__ __forceinline__ bf16x16 cat16(const bf16x8 lo, const bf16x8 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
}

size_t sp_smem(int kt32w, int rs) { return gf_lds_bytes() + (rs == 4 ? gf_image_bytes(kt32w) : 0); }

template <int KPW, int RS, bool MULTI>
__global__ __launch_bounds__(GF_MAXW * 64) void k_gemv24(GemmK p) {
  static_assert(KPW % SP_GROUP == 0, "whole stream groups per wave");
  constexpr int NG = KPW / SP_GROUP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const GfLds L = gf_lds(smem_raw);
  bf16x8* As = reinterpret_cast<bf16x8*>(L.rest);                                    // RS = 4: [plane][kt32][kq][row]

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
  constexpr int CE = gf_image_ce(2 * KPW);
  const int nentries = 2 * ktw * 4 * RS;
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
    gf_image_load<2 * KPW>(p, tid, NT, ex, ey);
  } else if constexpr (AP == KPW) {
#pragma unroll
    for (int i = 0; i < KPW; ++i) load_frag(af[i], kt0 + i);
  }
  float sq[16];
  gf_scales_load(p, tid, sq);
  __builtin_amdgcn_sched_barrier(0);
  bf16x8 b0[KPW], b1[MULTI ? KPW : 1];
  u32x4 m0[NG], m1[MULTI ? NG : 1];
  load_strip(b0, m0, blockIdx.x);                     // the HBM stream starts here
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (RS == 4) gf_image_store<2 * KPW>(As, tid, NT, ex, ey);
  gf_scales_reduce(p, tid, NT, sq, L.inv_s);
  lds_barrier();                                      // image + row scales visible; the weight loads stay in flight

  const int arow = min(lane & 15, RS - 1), akq = lane >> 4;
  int sbuf = 0;
  auto body = [&](bf16x8* bc, u32x4* mc, bf16x8* bn, u32x4* mn, int strip) __attribute__((always_inline)) {
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
    f32x4* rb = L.red + sbuf * (GF_MAXW * 64);
    sbuf ^= 1;
    gf_tile_store<RS, true>(rb, w, lane, acc);       // (the weights are the A operand: the transposed tile)
    lds_barrier();
    float vs[gf_ne(RS)];
    gf_wave_sum<RS, true>(rb, tid, NT, vs);
    gf_finish<RS, MULTI>(p, L, vs, tid, NT, strip);
  };
  gf_strips<MULTI>(p.nstrips, [&](int strip) { body(b0, m0, b1, m1, strip); }, [&](int strip) { body(b1, m1, b0, m0, strip); });
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
  const int rc = gf_check_common(a, "2:4 sparse", 16, "holds one bf16 weight plane (w_planes must be 0 or 1)",
                                 "needs fp32 activation tiles in and out (act_f32 = 3)");
  if (rc != DIA_OK) return rc;
  if (!a->W) return gf_refuse("2:4 sparse", "needs W");
  if (2 * a->KT > a->a_ktiles) return dia_fail(DIA_E_ARG, "dia_gemm: weight K exceeds the activation tiles' K");
  return DIA_OK;
}

// the launch (dia_gemm has run dia_gemm_sparse24_check and its own argument checks)
int dia_gemm_sparse24(const dia_gemm_args* a, void* stream) {
  const int rc = gf_check_splitk(a);
  if (rc != DIA_OK) return rc;
  const auto [sk, ktw, spw] = gf_shape(a);             // ktw: sparse k-tiles per workgroup
  if (a->KT % SP_GROUP != 0 || ktw % SP_GROUP != 0)
    return gf_refuse("2:4 sparse", "needs K a multiple of 512 per workgroup (whole groups of 8 sparse k-tiles)");
  GemmK k;
  fill_gemmk(a, k);
  hipStream_t st = (hipStream_t)stream;
  int kpw = (ktw / 8 <= GF_MAXW) ? 8 : ((ktw % 16 == 0 && ktw / 16 <= GF_MAXW) ? 16 : 0);
  if (!kpw)
    return gf_refuse("2:4 sparse", "needs the sparse k-tiles per workgroup (KT / sk) to be at most 64, "
                                   "or a multiple of 16 up to 128 (K <= 8192 per workgroup; use split-K)");
  const int nw = ktw / kpw;
  const bool image = a->M <= 4 && sp_smem(2 * ktw, 4) <= 150 * 1024;
  if (kpw == 8) return image ? launch24<8, 4>(k, nw, sk, spw, st) : launch24<8, 16>(k, nw, sk, spw, st);
  return launch24<16, 16>(k, nw, sk, 1, st);
}
