// What the run-time row kernel (attn_fwd_row16.hip, and the units that compile it) and the inference unit (attn_fwd_row16_infer.hip)
// share: the workgroup shapes and the padded LDS slab images, the two step bodies of a wave -- 32 keys (two key rows) and 16 keys
// (an odd last row) -- and the 16-byte output epilogue.  The step is stated HERE, once; a kernel supplies as callables what is its
// own: when the running maximum moves (hot) and how (rescale), the logits probe, the 8-wide rim mask and which LDS-DMA requests go
// out at the issue points inside a 32-key step (at).  The algorithm and why the step looks as it does: attn_fwd_row16.hip.
#pragma once
#include "attn_common.h"

// Compile-time ablations for timing experiments (tools/variants builds; results are garbage): bit 0 no LDS fragment reads,
// bit 1 no softmax arithmetic, bit 2 no MFMAs, bit 3 no V staging, bit 4 no K staging, bit 5 no slab loop at all, bit 6 one key plane only,
// bit 7 odd waves stage but do not compute.  0 in the product.
#ifndef WMZ_ATTN_ABL
#define WMZ_ATTN_ABL 0
#endif

namespace {

template <typename A, typename B>
__device__ __forceinline__ void mma16_abl(f32x4& acc, const A& a, const B& b) {
  if constexpr (WMZ_ATTN_ABL & 4) { asm volatile("" :: "v"(a.v), "v"(b.v)); } else { mma16(acc, a, b); }
}

// Workgroup shapes.  A plane is cut into chunks of CH rows, a slab holds every RS-th row of a chunk (KC = CH / RS rows: plane
// row = base + RS * slab row), two slabs (K and V images each) in LDS, one in flight.
//   Big   (NW 16, CH 16, KC 8): a workgroup = 16 query rows = a whole 16x16 plane, two 74 KB slabs, one workgroup per CU;
//   Small (NW  4, CH  4, KC 2): a workgroup = 4 query rows, two 18 KB slabs, four workgroups per CU -- planes of up to 8 tile rows
//         (8-wide planes), where the big shape would run a quarter full and stage 8-row slabs holding 2 rows.
// (Round 2 / 3 measured and dropped, now removed: 4-row slabs in a ring of four with three in flight, two 8-wave half-plane
//  workgroups per CU, a two-query-rows-per-wave kernel on MFMA 32x32x16: all equal or slower.)
template <int NW_, int CH_, int KC_> struct Shape {
  static constexpr int NW = NW_, CH = CH_, KC = KC_, RS = CH_ / KC_, LOG_RS = RS == 2 ? 1 : (RS == 1 ? 0 : 2);
  static_assert(KC_ * RS == CH_ && (1 << LOG_RS) == RS, "a slab is one phase of a chunk");
};
using Big = Shape<16, 16, 8>;
using Small = Shape<4, 4, 2>;
constexpr int NBUF = 2;               // LDS slab pair
constexpr float DEFER = 8.f;          // log2 units

template <int DH, typename SH> struct Img {
#ifndef WMZ_ATTN_KPAD
#define WMZ_ATTN_KPAD 32
#endif
  static constexpr int NW = SH::NW, KC = SH::KC;
  static constexpr int KROW = DH * 2 + WMZ_ATTN_KPAD, VROW = DH * 2 + 32;
  static constexpr int KIMG = KC * 16 * KROW, VIMG = KC * 16 * VROW;
  static constexpr int BUF = KIMG + VIMG;
  static constexpr int PK = KIMG / 1024, PV = VIMG / 1024;            // 1 KB DMA pieces per image
  static constexpr int NPK = (PK + NW - 1) / NW, NPV = (PV + NW - 1) / NW;   // ... per wave
  static_assert(KIMG % 1024 == 0 && VIMG % 1024 == 0, "images must be whole 1 KB DMA pieces");
};

struct StepNop { template <typename... A> __device__ __forceinline__ void operator()(A&&...) const {} };   // a callable a kernel has no use for

// ---- two key rows: 32 keys.  Sb: the slab's K image (V image behind it); ko: byte offset of the lane's K fragment of the first row,
// KROW the K row pitch; va0 / va1: LDS addresses of the lane's V^T fragments of the two rows.  at(1..3): the kernel's LDS-DMA issue
// points behind the QK^T MFMAs, behind the softmax and behind the PV MFMAs.
template <int KROW, int KS, int MT, typename Hot, typename Rescale, typename Probe, typename Mask, typename At>
__device__ __forceinline__ void attn_step32(const char* Sb, int ko, unsigned va0, unsigned va1, const Frag8<bf16_t> (&qf)[KS],
                                            f32x4 (&o)[MT], const float (&bm)[4], float c2, float& l_run, Hot hot, const Rescale& rescale,
                                            Probe probe, Mask mask, At at) {
  // ---- S^T = K Q^T for the two key rows
  f32x4 sc0 = (f32x4)(0.f), sc1 = (f32x4)(0.f);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    Frag8<bf16_t> ka, kb;
    if constexpr (WMZ_ATTN_ABL & 1) { ka.v = qf[ks].v; kb.v = qf[ks].v; }
    else {
      ka.v = *reinterpret_cast<const s16x8*>(Sb + ko + ks * 64);
      kb.v = *reinterpret_cast<const s16x8*>(Sb + ko + 16 * KROW + ks * 64);
    }
    mma16_abl(sc0, ka, qf[ks]);
    mma16_abl(sc1, kb, qf[ks]);
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- V^T fragments requested now: their LDS latency runs under the softmax
  s16x4 x0[MT], x1[MT];
  if constexpr (WMZ_ATTN_ABL & 1) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { x0[mt] = (s16x4)((short)va0); x1[mt] = (s16x4)((short)va1); }
  } else {
    static_for<MT>([&](auto mt) {
      x0[mt] = ds_read_tr16_asm<mt * 32>(va0);
      x1[mt] = ds_read_tr16_asm<mt * 32>(va1);
    });
  }
  at(std::integral_constant<int, 1>{});
  probe(sc0, sc1);
  // ---- softmax: exponent of 2 by one fma per logit; deferred running max
  float t[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    t[r] = fmaf(sc0[r], c2, bm[r]);
    t[4 + r] = fmaf(sc1[r], c2, bm[r]);
  }
  mask(t);
  const float mx = fmaxf(__builtin_fmaxf(__builtin_fmaxf(t[0], t[1]), __builtin_fmaxf(t[2], t[3])),
                         __builtin_fmaxf(__builtin_fmaxf(t[4], t[5]), __builtin_fmaxf(t[6], t[7])));
  if (hot(mx)) rescale(mx, t);
  float p[8];
  Frag8<bf16_t> pf;
  if constexpr (WMZ_ATTN_ABL & 2) {
#pragma unroll
    for (int r = 0; r < 8; ++r) pf.v[r] = (short)__builtin_bit_cast(int, sc0[r & 3]);
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) p[r] = __builtin_amdgcn_exp2f(t[r]);
    l_run += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    frag_from_f32<bf16_t>(pf, p);
  }
  at(std::integral_constant<int, 2>{});
  // ---- O^T += V^T P^T
  ds_tr_wait();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    asm volatile("" : "+v"(x0[mt]), "+v"(x1[mt]));       // uses stay behind the wait
    Frag8<bf16_t> vf;
    vf.v = __builtin_shufflevector(x0[mt], x1[mt], 0, 1, 2, 3, 4, 5, 6, 7);
    mma16_abl(o[mt], vf, pf);
  }
  at(std::integral_constant<int, 3>{});
}

// ---- odd last key row of a slab: a 16-key step (4 MFMAs + MT MFMA 16x16x16 instead of a half-empty 32-key step)
template <int KS, int MT, typename Hot, typename Rescale, typename Probe, typename Mask>
__device__ __forceinline__ void attn_step16(const char* Sb, int ko, unsigned va0, const Frag8<bf16_t> (&qf)[KS], f32x4 (&o)[MT],
                                            const float (&bm)[4], float c2, float& l_run, Hot hot, const Rescale& rescale, Probe probe,
                                            Mask mask) {
  f32x4 sc0 = (f32x4)(0.f);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    Frag8<bf16_t> ka;
    ka.v = *reinterpret_cast<const s16x8*>(Sb + ko + ks * 64);
    mma16(sc0, ka, qf[ks]);
  }
  __builtin_amdgcn_sched_barrier(0);
  s16x4 x0[MT];
  static_for<MT>([&](auto mt) { x0[mt] = ds_read_tr16_asm<mt * 32>(va0); });
  probe(sc0);
  float t[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = fmaf(sc0[r], c2, bm[r]);
  mask(t);
  const float mx = __builtin_fmaxf(__builtin_fmaxf(t[0], t[1]), __builtin_fmaxf(t[2], t[3]));
  if (hot(mx)) rescale(mx, t);
  float p[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(t[r]);
  l_run += (p[0] + p[1]) + (p[2] + p[3]);
  s16x4 pf;
#pragma unroll
  for (int r = 0; r < 4; ++r) pf[r] = (short)f32_to_bf16_bits(p[r]);
  ds_tr_wait();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    asm volatile("" : "+v"(x0[mt]));
    o[mt] = op16_mfma_16x16x16(x0[mt], pf, o[mt]);
  }
}

}  // namespace

// ---- 16-byte output stores of a query row: o the wave's f32x4[MT] accumulators, inv = 1 / l, orow the row of the lane's query in O
// (bf16_t*, dh 0), g = lane >> 4.  Lane (g, li) holds dh 16 mt + 4g .. +3 of query li; lanes g and g ^ 1 swap halves of an (mt, mt + 1)
// pair, so that the even lane owns dh 16 mt + 4g .. +7 and the odd lane dh 16 (mt + 1) + 4 (g - 1) .. +7: one 16-byte store each.
// (A macro, not a function: behind a call, in every signature tried, the inference unit's listing came out with the operands of these
//  eight multiplications swapped, and that listing is kept to the instruction -- profiles/attn_shared_step/README.md.)
#define WMZ_ATTN_STORE_EPI16(o, inv, orow, g)                                                                                      \
  do {                                                                                                                             \
    _Pragma("unroll") for (int mt = 0; mt < (int)(sizeof(o) / sizeof((o)[0])); mt += 2) {                                          \
      unsigned a0 = (unsigned)f32_to_bf16_bits((o)[mt][0] * (inv)) | ((unsigned)f32_to_bf16_bits((o)[mt][1] * (inv)) << 16);         \
      unsigned a1 = (unsigned)f32_to_bf16_bits((o)[mt][2] * (inv)) | ((unsigned)f32_to_bf16_bits((o)[mt][3] * (inv)) << 16);         \
      unsigned b0 = (unsigned)f32_to_bf16_bits((o)[mt + 1][0] * (inv)) | ((unsigned)f32_to_bf16_bits((o)[mt + 1][1] * (inv)) << 16); \
      unsigned b1 = (unsigned)f32_to_bf16_bits((o)[mt + 1][2] * (inv)) | ((unsigned)f32_to_bf16_bits((o)[mt + 1][3] * (inv)) << 16); \
      const auto s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);     /* odd rows of a <-> even rows of b */            \
      const auto s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);                                                      \
      i32x4 pk;                                                                                                                    \
      pk[0] = (int)s0[0]; pk[1] = (int)s1[0]; pk[2] = (int)s0[1]; pk[3] = (int)s1[1];                                              \
      const int col = ((g) & 1) ? (mt + 1) * 16 + 4 * ((g) - 1) : mt * 16 + 4 * (g);                                               \
      *reinterpret_cast<i32x4*>((orow) + col) = pk;                                                                                \
    }                                                                                                                              \
  } while (0)
