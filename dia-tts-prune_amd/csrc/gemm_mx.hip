// MX decode GEMMs: out[M][N] = X[M][K] . W[K][N] for M <= 16 rows with W stored as OCP MX blocks (one E8M0 power-of-two scale per
// 32 consecutive K of a column) in the streams of dia_hip/layout.py: e4m3 elements (tile_weight_fp8, dia_gemm_args.w_format =
// DIA_W_MXFP8) or e2m1 elements (tile_weight_fp4, DIA_W_MXFP4).  One kernel template, k_gemm_mx<Fmt, ...>, serves both: the
// formats differ in the traits Fp8 / Fp4 below (k-tiles per value slot, bytes per group, the converts of a B fragment) and in
// nothing else (DESIGN.md "MXFP4 weight stream" says why the kernel itself is the shared body).
//
// Mapping (CDNA4): the weights stay the B operand of the dense v_mfma_f32_16x16x32_bf16 (lane l: column l & 15 of the strip,
// K = 8 (l >> 4) + [0, 8) of the k-tile), so the accumulator keeps the dense kernels' orientation (lane l, element i = row
// 4 (l >> 4) + i, column l & 15).  A lane's 8 values of a k-tile belong to ONE MX block (the block is the 4 lanes x 8 values of
// a column inside a k-tile): v_cvt_scalef32_pk_bf16_fp8 / _fp4 turns two of them and the block's scale (E8M0 byte << 23 is the
// float it wants) into two bf16 — exactly, an e4m3 or e2m1 value times a power of two is a bf16 value — so a k-tile costs one
// scale extraction and four converts in front of the same three MFMAs (hi / mid / lo planes of the fp32 activations), with
// no LDS round trip on the weight side.
//
// Stream of a strip: groups of 16 k-tiles (512 K), each a 256-byte scale block [16 columns][16 k-tiles] (lane l reads the
// bytes of column l & 15) followed by value slots of 1 KiB, slot p = [64 lanes][16 bytes]:
//   MXFP8  a lane's 8 values of a k-tile are 8 bytes (two dwords); slot p holds its 8 of k-tile 2p and its 8 of k-tile 2p + 1:
//          8 slots, 8448 bytes per group, 0.515625 of the dense tiles'
//   MXFP4  a lane's 8 values of a k-tile are ONE dword (element j in byte j >> 1, the even element in the low nibble; the convert's
//          byte select b takes byte b); slot p holds its dwords of k-tiles 4p .. 4p + 3: 4 slots, 4352 bytes per group, 0.265625
//          of the dense tiles'.  One 16-byte load feeds four B fragments: a wave's 8 k-tiles are two loads per strip, its 16 four.
//
// The frame around the inner loop (LDS prefix, activation image, row scales, wave sum, split-K hand-off, epilogue, strip loop)
// is gemv_frame.hpp's.  A wave's K range is KPW k-tiles (8 = half a group, 16 = a whole one); every weight load of a wave is
// issued before its first MFMA.  Activations:
//   RS = 4   M <= 4: the frame's LDS image
//   RS = 16  5..16 rows: each wave holds the three bf16 planes of its K range's fragments in registers for every strip it walks
//            (as k_gemm16: 96 VGPRs at 8 k-tiles per wave); with 16 k-tiles per wave it reads them from L2 inside the loop
#include "gemv_frame.hpp"

namespace {

constexpr int MX_GROUP = 16;                       // k-tiles per stream group (layout.FP8_GROUP)
constexpr int MX_SCALE_BYTES = 256;                // scale block of a group
constexpr int MX_SLOT_BYTES = 1024;                // one value slot

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

__device__ __forceinline__ bf16x8 join4(bf16x2 r0, bf16x2 r1, bf16x2 r2, bf16x2 r3) {
  const bf16x4 lo = __builtin_shufflevector(r0, r1, 0, 1, 2, 3), hi = __builtin_shufflevector(r2, r3, 0, 1, 2, 3);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Per element format: k-tiles per value slot, bytes per group (layout.FP8_GROUP_BYTES / FP4_GROUP_BYTES), the name in messages
// and frag(): the B fragment of k-tile i of a wave's loaded slots bc, the 8 values of one MX block times its scale
struct Fp8 {
  static constexpr int SLOT_KT = 2;
  static constexpr int GROUP_BYTES = MX_SCALE_BYTES + (MX_GROUP / SLOT_KT) * MX_SLOT_BYTES;
  static constexpr const char* NAME = "MXFP8";
  static constexpr const char* KERNEL = "k_gemm_mx<Fp8>";
  static __device__ __forceinline__ bf16x8 frag(const u32x4* bc, int i, float scale) {      // 8 e4m3 bytes (two dwords)
    const unsigned d0 = bc[i >> 1][2 * (i & 1)], d1 = bc[i >> 1][2 * (i & 1) + 1];
    const bf16x2 r0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, scale, false);
    const bf16x2 r1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, scale, true);
    const bf16x2 r2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, scale, false);
    const bf16x2 r3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, scale, true);
    return join4(r0, r1, r2, r3);
  }
};
struct Fp4 {
  static constexpr int SLOT_KT = 4;
  static constexpr int GROUP_BYTES = MX_SCALE_BYTES + (MX_GROUP / SLOT_KT) * MX_SLOT_BYTES;
  static constexpr const char* NAME = "MXFP4";
  static constexpr const char* KERNEL = "k_gemm_mx<Fp4>";
  static __device__ __forceinline__ bf16x8 frag(const u32x4* bc, int i, float scale) {      // 8 e2m1 nibbles (one dword)
    const unsigned d = bc[i >> 2][i & 3];
    const bf16x2 r0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
    const bf16x2 r1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
    const bf16x2 r2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
    const bf16x2 r3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
    return join4(r0, r1, r2, r3);
  }
};
static_assert(Fp8::GROUP_BYTES == 8448 && Fp4::GROUP_BYTES == 4352, "the group sizes of dia_hip/layout.py");

size_t mx_smem(int ktw, int rs) { return gf_lds_bytes() + (rs == 4 ? gf_image_bytes(ktw) : 0); }

template <class Fmt, int KPW, int RS, bool MULTI>
__global__ __launch_bounds__(GF_MAXW * 64) void k_gemm_mx(GemmK p) {
  static_assert(KPW == 8 || KPW == 16, "half a stream group or a whole one per wave");
  constexpr int NS = KPW / Fmt::SLOT_KT;               // value slots per wave
  constexpr int NSC = KPW / 4;                         // dwords of scale bytes per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const GfLds L = gf_lds(smem_raw);
  bf16x8* As = reinterpret_cast<bf16x8*>(L.rest);                                    // RS = 4: [plane][kt][kq][row]

  const int NT = blockDim.x, NW = NT >> 6;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ktw = NW * KPW;                          // k-tiles of this workgroup's K range
  const int kt0 = blockIdx.y * ktw + w * KPW;        // first global k-tile of this wave (a multiple of KPW)
  const int G = gridDim.x;
  const long strip_bytes = (long)(p.KT / MX_GROUP) * Fmt::GROUP_BYTES;
  // this wave's part of a group: its scale bytes (column l & 15, k-tiles kt0 % 16 ..) and its value slots
  const unsigned char* Wg = reinterpret_cast<const unsigned char*>(p.W) + (long)(kt0 / MX_GROUP) * Fmt::GROUP_BYTES;
  const unsigned char* Wsc = Wg + (lane & 15) * 16 + (kt0 % MX_GROUP);
  const unsigned char* Wv = Wg + MX_SCALE_BYTES + (long)((kt0 % MX_GROUP) / Fmt::SLOT_KT) * MX_SLOT_BYTES + lane * 16;
  auto load_strip = [&](u32x4* b, unsigned* sc, int strip) {
    const long so = (long)strip * strip_bytes;
    if constexpr (KPW == 8) {
      const u32x2 s = DIA_WLOAD(reinterpret_cast<const u32x2*>(Wsc + so));
      sc[0] = s[0]; sc[1] = s[1];
    } else {
      const u32x4 s = DIA_WLOAD(reinterpret_cast<const u32x4*>(Wsc + so));
      sc[0] = s[0]; sc[1] = s[1]; sc[2] = s[2]; sc[3] = s[3];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) b[i] = DIA_WLOAD(reinterpret_cast<const u32x4*>(Wv + so + (long)i * MX_SLOT_BYTES));
  };
  const float* Af = reinterpret_cast<const float*>(p.A);

  // ---- small, L2-resident operands first (see k_gemv_small): activation image / fragments, row scales
  constexpr int CE = gf_image_ce(KPW);
  const int nentries = ktw * 4 * RS;
  float4 ex[RS == 4 ? CE : 1], ey[RS == 4 ? CE : 1];
  constexpr int AP = (RS == 16 && KPW == 8) ? KPW : 1;   // RS = 16: fragments of the wave's k-tiles held from the start
  float4 af[AP][2];
  const int alane = (lane & 48) | min(lane & 15, p.M - 1);   // rows >= M re-read the last valid row (never stored)
  auto load_frag = [&](float4* f, int t) {               // global k-tile t, this lane's 8 values
    const float4* s0 = reinterpret_cast<const float4*>(Af + ((long)t * 64 + alane) * 8);
    f[0] = s0[0]; f[1] = s0[1];
  };
  if constexpr (RS == 4) {
    gf_image_load<KPW>(p, tid, NT, ex, ey);
  } else if constexpr (AP == KPW) {
#pragma unroll
    for (int i = 0; i < KPW; ++i) load_frag(af[i], kt0 + i);
  }
  float sq[16];
  gf_scales_load(p, tid, sq);
  __builtin_amdgcn_sched_barrier(0);
  u32x4 b0[NS], b1[MULTI ? NS : 1];
  unsigned c0[NSC], c1[MULTI ? NSC : 1];
  load_strip(b0, c0, blockIdx.x);                     // the HBM stream starts here
  __builtin_amdgcn_sched_barrier(0);
  bf16x8 a3[AP][DIA_NPLANES];                         // RS = 16: the three planes of the held fragments (12 VGPRs per k-tile, as k_gemm16)
  if constexpr (AP == KPW) {
#pragma unroll
    for (int i = 0; i < KPW; ++i) split3x8(af[i][0], af[i][1], a3[i][0], a3[i][1], a3[i][2]);
  }
  if constexpr (RS == 4) gf_image_store<KPW>(As, tid, NT, ex, ey);
  gf_scales_reduce(p, tid, NT, sq, L.inv_s);
  lds_barrier();                                      // image + row scales visible; the weight loads stay in flight

  const int arow = min(lane & 15, RS - 1), akq = lane >> 4;
  int sbuf = 0;
  auto body = [&](u32x4* bc, unsigned* cc, u32x4* bn, unsigned* cn, int strip) __attribute__((always_inline)) {
    const int next = strip + G;
    if constexpr (MULTI) load_strip(bn, cn, DIA_PREFETCH_CLAMP(next, p.nstrips));   // unconditional: see k_gemv_small
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
      bf16x8 h, mi, lo;
      if constexpr (RS == 4) {
        const int kt = w * KPW + i;                     // k-tile inside the image
        h = As[(kt * 4 + akq) * RS + arow];
        mi = As[nentries + (kt * 4 + akq) * RS + arow];
        lo = As[2 * nentries + (kt * 4 + akq) * RS + arow];
      } else if constexpr (AP == KPW) {
        h = a3[i < AP ? i : 0][0]; mi = a3[i < AP ? i : 0][1]; lo = a3[i < AP ? i : 0][2];
      } else {
        float4 f[2];
        load_frag(f, kt0 + i);
        split3x8(f[0], f[1], h, mi, lo);
      }
      const float scale = __builtin_bit_cast(float, ((cc[i >> 2] >> (8 * (i & 3))) & 0xffu) << 23);
      const bf16x8 b = Fmt::frag(bc, i, scale);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h, b, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mi, b, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, b, acc, 0, 0, 0);
    }
    f32x4* rb = L.red + sbuf * (GF_MAXW * 64);
    sbuf ^= 1;
    gf_tile_store<RS, false>(rb, w, lane, acc);
    lds_barrier();
    float vs[gf_ne(RS)];
    gf_wave_sum<RS, false>(rb, tid, NT, vs);
    gf_finish<RS, MULTI>(p, L, vs, tid, NT, strip);
  };
  gf_strips<MULTI>(p.nstrips, [&](int strip) { body(b0, c0, b1, c1, strip); }, [&](int strip) { body(b1, c1, b0, c0, strip); });
}

template <class Fmt, int KPW, int RS>
int launch_mx(const GemmK& k, int nw, int sk, int spw, hipStream_t st) {
  const size_t smem = mx_smem(nw * KPW, RS);
  if (spw > 1 && sk == 1) {
    if constexpr (KPW == 8) {     // (16 k-tiles per wave: wo's split-K ranges only, one strip per workgroup)
      launch_kernel<k_gemm_mx<Fmt, KPW, RS, true>>(dim3((k.nstrips + spw - 1) / spw), dim3(nw * 64), smem, st, k);
      return dia_check_launch(Fmt::KERNEL);
    }
  }
  launch_kernel<k_gemm_mx<Fmt, KPW, RS, false>>(dim3(k.nstrips, sk), dim3(nw * 64), smem, st, k);
  return dia_check_launch(Fmt::KERNEL);
}

template <class Fmt>
int launch_mx_shape(const GemmK& k, int ktw, int sk, int spw, bool image, hipStream_t st) {
  const int kpw = ktw / 8 <= GF_MAXW ? 8 : 16;
  const int nw = ktw / kpw;
  if (kpw == 8) return image ? launch_mx<Fmt, 8, 4>(k, nw, sk, spw, st) : launch_mx<Fmt, 8, 16>(k, nw, sk, spw, st);
  return image ? launch_mx<Fmt, 16, 4>(k, nw, sk, 1, st) : launch_mx<Fmt, 16, 16>(k, nw, sk, 1, st);
}

}  // namespace

// dia_gemm with w_format == DIA_W_MXFP8 / DIA_W_MXFP4: what an MX stream cannot serve (checked before dia_gemm's other weight forms)
int dia_gemm_mx_check(const dia_gemm_args* a) {
  const char* name = a->w_format == DIA_W_MXFP4 ? Fp4::NAME : Fp8::NAME;
  const int rc = gf_check_common(a, name, 16);
  if (rc != DIA_OK) return rc;
  if (!a->W) return gf_refuse(name, "needs W");
  const int sk = gf_shape(a).sk;
  if (a->KT % MX_GROUP != 0 || a->KT % sk != 0 || (a->KT / sk) % MX_GROUP != 0)
    return gf_refuse(name, "needs K a multiple of 512 per workgroup (whole groups of 16 k-tiles)");
  if (a->KT / sk > 16 * GF_MAXW) return gf_refuse(name, "serves at most 128 k-tiles per workgroup (K <= 4096; use split-K)");
  return DIA_OK;
}

// the launch (dia_gemm has run dia_gemm_mx_check and its own argument checks)
int dia_gemm_mx(const dia_gemm_args* a, void* stream) {
  const int rc = gf_check_splitk(a);
  if (rc != DIA_OK) return rc;
  const auto [sk, ktw, spw] = gf_shape(a);
  GemmK k;
  fill_gemmk(a, k);
  hipStream_t st = (hipStream_t)stream;
  const bool image = a->M <= 4;                        // (128 k-tiles x 4 rows x 3 planes = 96 KiB at most)
  if (a->w_format == DIA_W_MXFP4) return launch_mx_shape<Fp4>(k, ktw, sk, spw, image, st);
  return launch_mx_shape<Fp8>(k, ktw, sk, spw, image, st);
}
