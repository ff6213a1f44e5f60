// Unstructured sparse decode GEMV: out[M][N] = X[M][K] . W[K][N] for M <= 4 rows with W an unstructured-pruned bf16 matrix stored
// as the lane-local fixed-rate stream of dia_hip/layout.py tile_weight_us (dia_gemm_args.w_format = DIA_W_USPARSE, W = a HOST
// dia_us_mat naming the stream and its rate).  Lossless: the stream holds exactly the numbers of the dense tiles.
//
// A kernel of its own beside k_gemm_mx, not a third trait of it: what the two share is the frame, and that is gemv_frame.hpp's
// functions, called here at RS = 4 only.  What differs sits inside the strip body in three places — the B fragment needs an LDS
// table where the MX formats need a scale, a second per-strip operand (the overflow run bounds and entries) travels with the
// weights, and a VALU pass adds into the tile between the wave sum and the finish — so a trait would have had to grow hooks at
// each of them, and the 5..16-row forms of k_gemm_mx (RS = 16) have no counterpart here (DESIGN.md "Unstructured sparse weight
// stream").
//
// Mapping (CDNA4): the weights stay the B operand of the dense v_mfma_f32_16x16x32_bf16 (lane l: column l & 15 of the strip,
// K = 8 (l >> 4) + [0, 8) of the k-tile).  Per lane and k-tile the stream holds an 8-bit mask (bit j = element j is non-zero) and
// a window of R bf16 slots (R = 4: 8 bytes, R = 2: 4 bytes) with the lane's first R non-zeros in element order.  The fragment is
// rebuilt in registers: the mask indexes a 256-entry LDS table of four v_perm_b32 selectors (bytes 2r, 2r + 1 of the window for
// the element of rank r < R, 0x0c = zero for the others), and four permutes produce the four dwords of the fragment: per k-tile
// one v_bfe_u32, one ds_read_b128 and four v_perm_b32 in front of the three MFMAs, no LDS traffic of weight VALUES.
//
// What does not fit a window (the non-zeros of rank >= R) is an overflow entry: per strip, stream group and column a run of
// (k within the group | bf16 bits << 16), bounded by two neighbouring entries of a run table.  Thread t of the workgroup owns
// column t & 15 of one group of the workgroup's K range and every SS-th entry of that run (SS = 64 / KPW), multiplies with the
// exact activation (hi + mid + lo of the LDS image) and leaves four row sums in LDS; the thread that finishes element (row,
// column) adds them in thread order behind the waves' partial tiles.  No atomics: the same bits eager and replayed.  The run
// bounds travel with the weight loads, the first PRE entries of every thread are requested before the MFMA loop.  A strip whose
// K range has no entry at all (the range's first and last bound are equal: one pair of table words, the same for every thread)
// skips the pass, its LDS exchange and its sum.
#include "gemv_frame.hpp"

namespace {

constexpr int US_GROUP = 16;                       // k-tiles per stream group (layout.US_GROUP)
constexpr int US_MASK_BYTES = 1024;                // mask block of a group: [64 lanes][16 k-tiles]
constexpr int US_SLOT_BYTES = 1024;                // one value slot: [64 lanes][16 bytes]
constexpr int US_PRE = 4;                          // overflow entries per thread requested before the MFMA loop
constexpr int US_OSLOTS = GF_MAXW * 4;             // threads per column in the overflow pass, at most

constexpr int us_group_bytes(int rate) { return US_MASK_BYTES + rate * 2 * US_SLOT_BYTES; }
static_assert(us_group_bytes(4) == 9216 && us_group_bytes(2) == 5120, "the group sizes of dia_hip/layout.py");

struct UsK {
  GemmK g;
  const unsigned* otab;      // run table [nstrips * KT / 16 * 16 + 1]
  const unsigned* oent;      // overflow entries
};

// LDS behind the frame's prefix: overflow sums [2][US_OSLOTS][4][16], selector table [256] u32x4, then the activation image
size_t us_smem(int ktw) { return gf_lds_bytes() + sizeof(float) * 2 * US_OSLOTS * 64 + sizeof(u32x4) * 256 + gf_image_bytes(ktw); }

template <int R, int KPW, bool MULTI>
__global__ __launch_bounds__(GF_MAXW * 64) void k_gemm_us(UsK q) {
  static_assert((R == 4 || R == 2) && (KPW == 8 || KPW == 16), "window slots; half a stream group or a whole one per wave");
  const GemmK& p = q.g;
  constexpr int RS = 4;
  constexpr int SLOT_KT = 8 / R;                       // k-tiles per value slot
  constexpr int NS = KPW / SLOT_KT;                    // value slots per wave
  constexpr int NM = KPW / 4;                          // dwords of mask bytes per wave
  constexpr int GB = us_group_bytes(R);
  constexpr int SS = 64 / KPW;                         // threads per overflow run
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const GfLds L = gf_lds(smem_raw);
  float* ored = reinterpret_cast<float*>(L.rest);                                    // [2][US_OSLOTS][4][16]
  u32x4* seltab = reinterpret_cast<u32x4*>(ored + 2 * US_OSLOTS * 64);               // [256]
  bf16x8* As = reinterpret_cast<bf16x8*>(seltab + 256);                              // [plane][kt][kq][row]

  const int NT = blockDim.x, NW = NT >> 6;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ktw = NW * KPW;                          // k-tiles of this workgroup's K range
  const int kt0 = blockIdx.y * ktw + w * KPW;        // first global k-tile of this wave (a multiple of KPW)
  const int G = gridDim.x;
  const int groups = p.KT / US_GROUP;                // stream groups of a strip
  const long strip_bytes = (long)groups * GB;
  const unsigned char* Wg = reinterpret_cast<const unsigned char*>(p.W) + (long)(kt0 / US_GROUP) * GB;
  const unsigned char* Wm = Wg + lane * 16 + (kt0 % US_GROUP);
  const unsigned char* Wv = Wg + US_MASK_BYTES + (long)((kt0 % US_GROUP) / SLOT_KT) * US_SLOT_BYTES + lane * 16;
  // overflow pass: this thread's column, its group inside the workgroup's range and its place in the run
  const int ng = ktw / US_GROUP;
  const int ocol = tid & 15, ogi = (tid >> 4) % ng, osub = (tid >> 4) / ng;
  const long orun = ((long)blockIdx.y * ng + ogi) * 16 + ocol;      // + strip * groups * 16
  auto load_strip = [&](u32x4* b, unsigned* mk, unsigned* ob, int strip) {
    const unsigned* t = q.otab + (long)strip * groups * 16 + orun;
    ob[0] = t[0]; ob[1] = t[1];                       // the run bounds first: they are needed before the weights
    // ... and the first and last bound of the workgroup's whole K range (the same two words for every thread): equal = no overflow
    // entry in this strip and range, and the pass below is skipped by the whole workgroup
    const unsigned* tw = q.otab + ((long)strip * groups + (long)blockIdx.y * ng) * 16;
    ob[2] = tw[0]; ob[3] = tw[ng * 16];
    const long so = (long)strip * strip_bytes;
    if constexpr (KPW == 8) {
      const u32x2 s = DIA_WLOAD(reinterpret_cast<const u32x2*>(Wm + so));
      mk[0] = s[0]; mk[1] = s[1];
    } else {
      const u32x4 s = DIA_WLOAD(reinterpret_cast<const u32x4*>(Wm + so));
      mk[0] = s[0]; mk[1] = s[1]; mk[2] = s[2]; mk[3] = s[3];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) b[i] = DIA_WLOAD(reinterpret_cast<const u32x4*>(Wv + so + (long)i * US_SLOT_BYTES));
  };

  // ---- small, L2-resident operands first (see k_gemv_small): activation image, row scales
  const int nentries = ktw * 4 * RS;
  float4 ex[gf_image_ce(KPW)], ey[gf_image_ce(KPW)];
  gf_image_load<KPW>(p, tid, NT, ex, ey);
  float sq[16];
  gf_scales_load(p, tid, sq);
  __builtin_amdgcn_sched_barrier(0);
  u32x4 b0[NS], b1[MULTI ? NS : 1];
  unsigned m0[NM], m1[MULTI ? NM : 1];
  unsigned o0[4], o1[4];
  load_strip(b0, m0, o0, blockIdx.x);                 // the HBM stream starts here
  __builtin_amdgcn_sched_barrier(0);
  // selector table: entry m, dword d = the v_perm_b32 selector of elements 2d (low half) and 2d + 1 of a lane whose mask is m
  for (int m = tid; m < 256; m += NT) {
    u32x4 sel;
    int rank = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      unsigned s = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * d + h;
        const bool take = ((m >> j) & 1) && rank < R;
        const unsigned two = take ? (unsigned)((2 * rank) | ((2 * rank + 1) << 8)) : 0x0c0cu;
        s |= two << (16 * h);
        rank += (m >> j) & 1;
      }
      sel[d] = s;
    }
    seltab[m] = sel;
  }
  gf_image_store<KPW>(As, tid, NT, ex, ey);
  gf_scales_reduce(p, tid, NT, sq, L.inv_s);
  lds_barrier();                                     // image, table and row scales visible; the weight loads stay in flight

  const int arow = min(lane & 15, RS - 1), akq = lane >> 4;
  const unsigned short* Ab = reinterpret_cast<const unsigned short*>(As);      // the image as bf16 bits
  const int plane_e = nentries * 8;                   // elements of one image plane
  int sbuf = 0;
  auto body = [&](u32x4* bc, unsigned* mc, unsigned* oc, u32x4* bn, unsigned* mn, unsigned* on, int strip) __attribute__((always_inline)) {
    const int next = strip + G;
    if constexpr (MULTI) load_strip(bn, mn, on, DIA_PREFETCH_CLAMP(next, p.nstrips));   // unconditional: see k_gemv_small
    // this thread's overflow entries oc[0] + osub, + SS, ... below oc[1]: the first US_PRE in flight during the MFMA loop
    const unsigned ob = oc[0] + osub, oe = oc[1];
    const bool spills = __builtin_amdgcn_readfirstlane(oc[2]) != __builtin_amdgcn_readfirstlane(oc[3]);      // workgroup-uniform
    unsigned en[US_PRE];
#pragma unroll
    for (int u = 0; u < US_PRE; ++u) en[u] = ob + u * SS < oe ? q.oent[ob + u * SS] : 0u;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
      const int kt = w * KPW + i;                     // k-tile inside the image
      const bf16x8 h = As[(kt * 4 + akq) * RS + arow];
      const bf16x8 mi = As[nentries + (kt * 4 + akq) * RS + arow];
      const bf16x8 lo = As[2 * nentries + (kt * 4 + akq) * RS + arow];
      const u32x4 sel = seltab[(mc[i >> 2] >> (8 * (i & 3))) & 0xffu];
      unsigned wl, wh;                                // the window: bytes 0-3 and 4-7 of the permute's source
      if constexpr (R == 4) { wl = bc[i >> 1][2 * (i & 1)]; wh = bc[i >> 1][2 * (i & 1) + 1]; }
      else { wl = bc[i >> 2][i & 3]; wh = 0u; }
      u32x4 bw;
#pragma unroll
      for (int d = 0; d < 4; ++d) bw[d] = __builtin_amdgcn_perm(wh, wl, sel[d]);
      const bf16x8 b = __builtin_bit_cast(bf16x8, bw);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h, b, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mi, b, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, b, acc, 0, 0, 0);
    }
    // overflow: acc[m][column] += x[m][k] * v with x = hi + mid + lo of the image (exact)
    float oa[RS] = {0.f, 0.f, 0.f, 0.f};
    auto add = [&](unsigned e) {                      // (an entry of zero adds x * 0)
      const float v = __builtin_bit_cast(float, e & 0xffff0000u);
      const int k = ogi * (US_GROUP * 32) + (int)(e & 0xffffu);
      const int base = (k >> 3) * (RS * 8) + (k & 7);
#pragma unroll
      for (int m = 0; m < RS; ++m) {
        const int o = base + m * 8;
        const float x = (__builtin_bit_cast(float, (unsigned)Ab[o] << 16) + __builtin_bit_cast(float, (unsigned)Ab[plane_e + o] << 16)) +
                        __builtin_bit_cast(float, (unsigned)Ab[2 * plane_e + o] << 16);
        oa[m] = fmaf(x, v, oa[m]);
      }
    };
    if (spills) {
#pragma unroll
      for (int u = 0; u < US_PRE; ++u) add(en[u]);
      for (unsigned i = ob + US_PRE * SS; i < oe; i += SS) add(q.oent[i]);
    }
    // the overflow sums of thread t go beside the wave's tile, at [t >> 4][row][column] ...
    f32x4* rb = L.red + sbuf * (GF_MAXW * 64);
    float* ob_s = ored + sbuf * (US_OSLOTS * 64);
    sbuf ^= 1;
    gf_tile_store<RS, false>(rb, w, lane, acc);
    if (spills) {
#pragma unroll
      for (int m = 0; m < RS; ++m) ob_s[((tid >> 4) * RS + m) * 16 + ocol] = oa[m];
    }
    lds_barrier();
    float vs[gf_ne(RS)];                              // (one: thread t < 64 finishes row t >> 4, column t & 15)
    gf_wave_sum<RS, false>(rb, tid, NT, vs);
    if (spills && tid < 16 * RS)                      // ... and are added in thread order behind the waves' partial tiles
      for (int r = 0; r < NW * 4; ++r) vs[0] += ob_s[(r * RS + (tid >> 4)) * 16 + (tid & 15)];
    gf_finish<RS, MULTI>(p, L, vs, tid, NT, strip);
  };
  gf_strips<MULTI>(p.nstrips, [&](int strip) { body(b0, m0, o0, b1, m1, o1, strip); }, [&](int strip) { body(b1, m1, o1, b0, m0, o0, strip); });
}

template <int R, int KPW>
int launch_us(const UsK& k, int nw, int sk, int spw, hipStream_t st) {
  const size_t smem = us_smem(nw * KPW);
  if (spw > 1 && sk == 1) {
    if constexpr (KPW == 8) {     // (16 k-tiles per wave: wo's split-K ranges only, one strip per workgroup)
      launch_kernel<k_gemm_us<R, KPW, true>>(dim3((k.g.nstrips + spw - 1) / spw), dim3(nw * 64), smem, st, k);
      return dia_check_launch("k_gemm_us");
    }
  }
  launch_kernel<k_gemm_us<R, KPW, false>>(dim3(k.g.nstrips, sk), dim3(nw * 64), smem, st, k);
  return dia_check_launch("k_gemm_us");
}

template <int R>
int launch_us_shape(const UsK& k, int ktw, int sk, int spw, hipStream_t st) {
  const int kpw = ktw / 8 <= GF_MAXW ? 8 : 16;
  const int nw = ktw / kpw;
  return kpw == 8 ? launch_us<R, 8>(k, nw, sk, spw, st) : launch_us<R, 16>(k, nw, sk, 1, st);
}

}  // namespace

// dia_gemm with w_format == DIA_W_USPARSE: what the stream cannot serve (checked before dia_gemm's other weight forms)
int dia_gemm_us_check(const dia_gemm_args* a) {
  const char* name = "unstructured sparse";
  const int rc = gf_check_common(a, name, 4);
  if (rc != DIA_OK) return rc;
  const dia_us_mat* m = static_cast<const dia_us_mat*>(a->W);
  if (!m || !m->stream) return gf_refuse(name, "needs W to point to a dia_us_mat that names the stream (w_format = DIA_W_USPARSE)");
  if (m->rate != 4 && m->rate != 2) return gf_refuse(name, "has windows of 4 or 2 values (dia_us_mat.rate)");
  const int sk = gf_shape(a).sk;
  if (a->KT % US_GROUP != 0 || a->KT % sk != 0 || (a->KT / sk) % US_GROUP != 0)
    return gf_refuse(name, "needs K a multiple of 512 per workgroup (whole groups of 16 k-tiles)");
  if (a->KT / sk > 16 * GF_MAXW) return gf_refuse(name, "serves at most 128 k-tiles per workgroup (K <= 4096; use split-K)");
  return DIA_OK;
}

// the launch (dia_gemm has run dia_gemm_us_check and its own argument checks)
int dia_gemm_us(const dia_gemm_args* a, void* stream) {
  const int rc = gf_check_splitk(a);
  if (rc != DIA_OK) return rc;
  const dia_us_mat* m = static_cast<const dia_us_mat*>(a->W);
  const auto [sk, ktw, spw] = gf_shape(a);
  UsK k;
  fill_gemmk(a, k.g);
  // the three parts of the stream (layout.tile_weight_us): fixed part, run table (padded to 16 bytes), overflow entries
  const unsigned char* base = static_cast<const unsigned char*>(m->stream);
  const long runs = (long)a->nstrips * (a->KT / US_GROUP) * 16;
  const long tab_off = (long)a->nstrips * (a->KT / US_GROUP) * us_group_bytes(m->rate);
  k.g.W = reinterpret_cast<const bf16_raw*>(base);
  k.otab = reinterpret_cast<const unsigned*>(base + tab_off);
  k.oent = reinterpret_cast<const unsigned*>(base + tab_off + (4 * (runs + 1) + 15) / 16 * 16);
  hipStream_t st = (hipStream_t)stream;
  return m->rate == 4 ? launch_us_shape<4>(k, ktw, sk, spw, st) : launch_us_shape<2>(k, ktw, sk, spw, st);
}
