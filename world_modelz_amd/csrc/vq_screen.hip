// VectorQuantizerEMA nearest code (vq-video-diffusion/vq.py:30-33, :77-87) by SCREENING + EXACT RE-CHECK, for the embedding
// widths of vq_screen_widths.h and any codebook size.
// Compiled with -ffp-contract=off like vq.hip.  Results are bit-identical to wmz_vq_argmin's (indices and minimum distances
// in the reference's fp32 summation order): the screening only decides WHICH code is evaluated exactly.
//
// Why: the pinned distance is three un-fused fp32 lane operations per (row, code, element) -- 12.9 G lane-ops at N = 65 536,
// C = 1 024, E = 64: 164 us at the vector ALU's peak however it is scheduled (vq.hip runs at 0.55-0.62 of it).  But the ARGMIN
// needs that arithmetic only where two codes are closer than what cheaper arithmetic can tell apart:
//   d(n, c) = |x_n|^2 + |e_c|^2 - 2 x_n.e_c   =>   argmin_c d = argmax_c a(n, c),   a = x_n.e_c - |e_c|^2 / 2.
// a~ is computed on the matrix cores with x and e split into bf16 head + tail (x.e ~= xh.eh + xh.el + xl.eh: three bf16 MFMAs
// per 16 elements, fp32 accumulate, -|e_c|^2 / 2 as the accumulator's initial value), i.e. 3/16 of the cost of an fp32 MFMA
// product.
//
// The error bound, as a function of the width E (u = 2^-8, the bf16 unit round-off as charged here; v = 2^-24, the fp32 one;
// |.| Euclidean norms; emax = max_c |e_c|; a_pinned = (|x_n|^2 - d_pinned) / 2 with d_pinned what dist_exact<E> returns):
//   |a~ - a_pinned| <= eps_n(E) = 8e-5 |x_n| emax + K2(E) (|x_n| + emax)^2,   K2(E) = 1e-5 (2 E + 8) / 136   (vq_eps_k2)
// First term, independent of E: the dropped tail product xl.el and the double-rounded tails are bounded element by element and
// summed by Cauchy-Schwarz, <= 3.1 u^2 |x||e| = 4.7e-5 |x||e| at every width.
// Second term, in units of v (|x_n| + emax)^2:
//   (3 E + 1) / 2   fp32 accumulation of the 3 E products and the start value: (3 E + 1) v times the sum of their magnitudes,
//                   |x||e| (1 + 2 u) + |e|^2 / 2 <= (|x| + |e|)^2 / 2.  This charges ONE fp32 rounding (v, relative to the
//                   running sum) per accumulated product, in whatever order -- i.e. it assumes the MFMA adds its 16 products
//                   per step no worse than 16 separately rounded fp32 additions would.  That per-step cost of the matrix
//                   core's internal accumulation has NOT been measured on this hardware; it is the assumption the E = 64
//                   kernel was built on, and the margin below is what stands between it and a wrong "sure" decision.
//   E / 2           |e|^2 in fp32 (E fused multiply-adds, lane tree or chain: <= E v |e|^2), halved exactly;
//   (E / 32 + 13) / 2   d_pinned against the real-number distance: one rounding for x - e, one for the square (3 v on the term),
//                   then a sum E / 32 + 10 additions deep (rounds of the four accumulators, their combination, the 8 lanes).
//   sum: (2 E + 7 + E / 64) v (|x| + emax)^2 = 2.3e-6 / 4.3e-6 / 8.1e-6 / 1.58e-5 / 3.12e-5 at E = 16 / 32 / 64 / 128 / 256;
//   K2(E) = 2.9e-6 / 5.3e-6 / 1e-5 / 1.94e-5 / 3.82e-5 keeps 22-26 % over it at every width (exactly 1e-5 at E = 64).
// Every lane keeps the largest and second-largest a~ of the codes it sees.  If the row's best beats its runner-up by more
// than 2 eps_n, NO other code can be the pinned argmin (strictly: ties are impossible then), and the row costs one exact
// evaluation (its minimum distance).  Otherwise (equal codes, near ties: 0.8-1.2 % of rows on Gaussian data at E = 64, C = 512-8 192) the row goes
// to a list, and a second kernel scans the whole codebook for it in the pinned arithmetic.
//
// Any codebook size: the workspace holds the operands of Cp = C rounded up to 64 codes.  The prep kernel writes the padding
// codes as zero heads and tails with a start value of -inf: a~ of a padding code is -inf for every finite row, so it never wins
// and never becomes a runner-up above a real code.  With a single code the runner-up stays -inf, the gap is +inf and the row is
// "sure" (unless eps itself overflowed, which sends it to the re-check: also right).
//
// Resources per width (vq_geo): rows per workgroup and the x fragments in registers are the same everywhere (8 E / 16 VGPRs:
// 128 at E = 256); what shrinks at the wide end is the LDS tile.  E <= 64: 64 codes, double-buffered.  E = 128: 32 codes,
// double-buffered.  E = 256: 32 codes in ONE buffer (two barriers per tile behind 48 MFMAs per wave) -- a second buffer at pitch
// 2 E + 16 would pass 64 KB.  The re-check keeps x in registers up to E = 64 and reads it through the scalar path beyond, fills
// its 64-code wave tiles sixteen 16-byte chunks per lane at a time, and runs two waves instead of four at E = 256 (two
// 64 x 257 images are 129 KB).
#include "vq_dist.h"
#include "vq_screen_widths.h"
#include <limits.h>

namespace {

constexpr int ROWS_W = 32;            // rows per wave (the MFMA's N)
constexpr int NWAVE = 4;
constexpr int ROWS_WG = ROWS_W * NWAVE;

template <int E>
struct vq_geo {
  static_assert(E % 16 == 0 && E >= 16, "whole MFMA k-steps");
  static constexpr int KS = E / 16;                       // k-steps
  static constexpr int CT = E <= 64 ? 64 : 32;            // codes per LDS tile (32-code MFMA groups)
  static constexpr int NBUF = E <= 128 ? 2 : 1;
  static constexpr int CROW = 2 * E + 16;                 // LDS pitch of a bf16 code row: an odd number of 16-byte slots -> the 32 codes on the lanes of ds_read_b128 are conflict-free
  static constexpr int TILE_B = 2 * CT * CROW + CT * 4;   // eh rows, el rows, -|e|^2/2
  static constexpr int CPR = E / 8;                       // 16-byte chunks of a bf16 row
  static constexpr int NCHUNK = CT * CPR;                 // ... of a tile's heads (as many for its tails)
  static constexpr int NST = (NCHUNK + 255) / 256;        // staging chunks per thread
  static constexpr int PREP_LPC = E / 16;                 // prep: lanes per code, 16 elements each
  static constexpr int PREP_NT = 64 * PREP_LPC;           // prep: threads of a 64-code block
  // re-check: RC_NW waves, each with a private image of 64 codes pitched E + 1 floats
  static constexpr int RC_NW = E <= 128 ? 4 : 2;
  static constexpr int RC_PITCH = E + 1;
  static constexpr int RC_TILE = 64 * RC_PITCH;           // floats of one wave's tile image
  static constexpr int RC_LDS = RC_NW * RC_TILE * 4 + 64; // bytes: the images + the waves' minima
  static constexpr int RC_NQ = E / 4;                     // 16-byte chunks of a tile per lane
  static constexpr int RC_PQ = RC_NQ < 16 ? RC_NQ : 16;   // ... in flight at a time
  static_assert(NBUF * TILE_B <= 64 * 1024, "static LDS");
  static_assert(RC_LDS <= 160 * 1024, "LDS per workgroup on gfx950");
};

// K2(E) of the bound above.  (2 * 64 + 8) / 136 is exactly 1: the E = 64 constant is the literal 1e-5f.
// Mirrored by tests/test_vq_screen_widths_cpu.py::eps_bound.
template <int E>
constexpr float vq_eps_k2() { return 1e-5f * ((float)(2 * E + 8) / 136.f); }
constexpr float VQ_EPS_K1 = 8e-5f;

// codebook -> bf16 head / tail rows, -|e|^2 / 2, and the largest |e|^2 of every block of 64 codes (the screening kernel takes
// the maximum of those: no same-address atomic chain); block 0 also puts the flagged-row count back to zero.
// A block takes 64 codes: lane = (code, 16-element piece of its row).  Codes past C (the last block of a ragged codebook) are
// written as padding: zero heads and tails, start value -inf, no share in the block's maximum.  A codebook of fewer than 64
// codes is also copied in fp32 to CB64, rows C .. 63 repeating its last code (vq_recheck_kernel reads whole 64-code tiles).
template <int E>
__global__ __launch_bounds__(vq_geo<E>::PREP_NT) void vq_prep_kernel(const float* __restrict__ CB, unsigned short* __restrict__ EH,
                                                                     unsigned short* __restrict__ EL, float* __restrict__ NH,
                                                                     float* __restrict__ CB64, float* __restrict__ emax2_blk,
                                                                     int* __restrict__ nflag, int C) {
  constexpr int LPC = vq_geo<E>::PREP_LPC, NW = vq_geo<E>::PREP_NT / 64;
  __shared__ float wmax[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x * 64 + tid / LPC, q = tid % LPC;
  const bool real = c < C;
  const float* row = CB + (long)(real ? c : C - 1) * E + q * 16;
  f32x4 v[4];                                                 // (all four loads in flight before anything waits for one)
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(row + 4 * i);
  if (C < 64) {                                               // (one block: the re-check's 64-row copy)
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(CB64 + (long)c * E + q * 16 + 4 * i) = v[i];
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!real) v[i] = (f32x4)(0.f);
    s16x4 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned short hb = f32_to_bf16_bits(v[i][j]);
      h[j] = (short)hb;
      l[j] = (short)f32_to_bf16_bits(v[i][j] - bf16_bits_to_f32(hb));
      s = fmaf(v[i][j], v[i][j], s);
    }
    *reinterpret_cast<s16x4*>(EH + (long)c * E + q * 16 + 4 * i) = h;
    *reinterpret_cast<s16x4*>(EL + (long)c * E + q * 16 + 4 * i) = l;
  }
#pragma unroll
  for (int d = 1; d < LPC; d <<= 1) s += __shfl_xor(s, d);    // the code's lanes are neighbours: lanes LPC k .. LPC k + LPC - 1
  if (q == 0) NH[c] = real ? -0.5f * s : -INFINITY;
  float m = s;
#pragma unroll
  for (int d = LPC; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
  if (lane == 0) wmax[wave] = m;
  __syncthreads();
  if (tid == 0) {
    float bm = wmax[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) bm = fmaxf(bm, wmax[w]);
    emax2_blk[blockIdx.x] = bm;
    if (blockIdx.x == 0) *nflag = 0;
  }
}

// Cp: the codebook size rounded up to 64 (what the prep kernel wrote).
template <int E>
__global__ __launch_bounds__(ROWS_WG * 2) void vq_screen_kernel(const float* __restrict__ X, long ldx, const float* __restrict__ CB,
                                                                const unsigned short* __restrict__ EH,
                                                                const unsigned short* __restrict__ EL, const float* __restrict__ NH,
                                                                const float* __restrict__ emax2_blk, int64_t* __restrict__ IDX,
                                                                float* __restrict__ DMIN, int* __restrict__ nflag,
                                                                int* __restrict__ flagged, int N, int C, int Cp) {
  using G = vq_geo<E>;
  constexpr int KS = G::KS, CT = G::CT, CROW = G::CROW, TILE_B = G::TILE_B, CPR = G::CPR, NST = G::NST;
  __shared__ __attribute__((aligned(16))) char sm[G::NBUF * TILE_B];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n32 = lane & 31, hi = lane >> 5;
  const long row = (long)blockIdx.x * ROWS_WG + wave * ROWS_W + n32;
  const bool rok = row < N;
  const float* xrow = X + (rok ? row : (long)N - 1) * ldx;

  // B operands: this lane's 8 k-elements of every 16-wide k-step, split into bf16 head and tail
  s16x8 xh[KS], xl[KS];
  float x2 = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = xrow[ks * 16 + 8 * hi + j];
      const unsigned short h = f32_to_bf16_bits(v);
      xh[ks][j] = (short)h;
      xl[ks][j] = (short)f32_to_bf16_bits(v - bf16_bits_to_f32(h));
      x2 = x2 + v * v;
    }
  }
  x2 = wave_halves_sum(x2);                                // |x_n|^2 (both lanes of the row)

  // staging: 256 threads move one tile = CT codes x (2 E B head + 2 E B tail) + CT floats; chunk q = tid + 256 i
  auto stage_load = [&](int c0, i32x4 (&rh)[NST], i32x4 (&rl)[NST], f32x4& rn) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int q = tid + 256 * i, code = q / CPR, ch = q % CPR;
      if (G::NCHUNK % 256 == 0 || q < G::NCHUNK) {
        rh[i] = *reinterpret_cast<const i32x4*>(EH + (long)(c0 + code) * E + ch * 8);
        rl[i] = *reinterpret_cast<const i32x4*>(EL + (long)(c0 + code) * E + ch * 8);
      }
    }
    if (tid < CT / 4) rn = *reinterpret_cast<const f32x4*>(NH + c0 + tid * 4);
  };
  auto stage_store = [&](char* buf, const i32x4 (&rh)[NST], const i32x4 (&rl)[NST], const f32x4& rn) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int q = tid + 256 * i, code = q / CPR, ch = q % CPR;
      if (G::NCHUNK % 256 == 0 || q < G::NCHUNK) {
        *reinterpret_cast<i32x4*>(buf + code * CROW + ch * 16) = rh[i];
        *reinterpret_cast<i32x4*>(buf + CT * CROW + code * CROW + ch * 16) = rl[i];
      }
    }
    if (tid < CT / 4) *reinterpret_cast<f32x4*>(buf + 2 * CT * CROW + tid * 16) = rn;
  };

  // best, runner-up, and WHERE the best was seen: accumulator register (rsel) and 32-code group (gsel) -- the code index is put
  // together once, at the end (a per-element index costs as much vector ALU time as the comparison itself)
  float M1 = -INFINITY, M2 = -INFINITY;
  int rsel = 0, gsel = -1;
  i32x4 rh[NST], rl[NST];
  f32x4 rn = (f32x4)(0.f);
#pragma unroll
  for (int i = 0; i < NST; ++i) { rh[i] = (i32x4)(0); rl[i] = (i32x4)(0); }
  stage_load(0, rh, rl, rn);
  stage_store(sm, rh, rl, rn);
  __syncthreads();
  const int ntile = Cp / CT;
  for (int t = 0; t < ntile; ++t) {
    const char* buf = sm + (G::NBUF == 2 ? (t & 1) * TILE_B : 0);
    if (t + 1 < ntile) stage_load((t + 1) * CT, rh, rl, rn);
#pragma unroll
    for (int g = 0; g < CT / 32; ++g) {
      // initial accumulator: -|e_c|^2 / 2 of the 16 codes this lane's registers stand for: c = 32 g + (r & 3) + 8 (r >> 2) + 4 hi
      f32x16 acc;
      const float* nh = reinterpret_cast<const float*>(buf + 2 * CT * CROW) + 32 * g + 4 * hi;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(nh + 8 * q4);
        acc[4 * q4] = v[0]; acc[4 * q4 + 1] = v[1]; acc[4 * q4 + 2] = v[2]; acc[4 * q4 + 3] = v[3];
      }
      const char* ah = buf + (32 * g + n32) * CROW + hi * 16;
      const char* al = ah + CT * CROW;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const s16x8 eh = *reinterpret_cast<const s16x8*>(ah + ks * 32);
        const s16x8 el = *reinterpret_cast<const s16x8*>(al + ks * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(eh, xh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(el, xh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(eh, xl[ks], acc, 0, 0, 0);
      }
      const float m_before = M1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        M2 = __builtin_amdgcn_fmed3f(M1, v, M2);           // the runner-up: M1 <= .. is kept, v in between replaces it
        rsel = v > M1 ? r : rsel;
        M1 = __builtin_amdgcn_fmed3f(M1, v, INFINITY);     // max(M1, v) as one instruction (fmaxf adds two canonicalising ops)
      }
      gsel = M1 != m_before ? (CT / 32) * t + g : gsel;
    }
    if (G::NBUF == 1) __syncthreads();                     // (one buffer: every wave has read the tile before the next one lands)
    if (t + 1 < ntile) stage_store(sm + (G::NBUF == 2 ? ((t + 1) & 1) * TILE_B : 0), rh, rl, rn);
    __syncthreads();
  }
  int c1 = gsel < 0 ? INT_MAX : 32 * gsel + 4 * hi + (rsel & 3) + 8 * (rsel >> 2);
  // the row's two lanes (hi = 0 / 1 saw disjoint codes) merge: best, runner-up, index (lower index on equal values)
  {
    const auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(M1), __float_as_uint(M1), false, false);
    const auto s2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(M2), __float_as_uint(M2), false, false);
    const auto s3 = __builtin_amdgcn_permlane32_swap((unsigned)c1, (unsigned)c1, false, false);
    const float o1 = __uint_as_float(hi ? s1[0] : s1[1]), o2 = __uint_as_float(hi ? s2[0] : s2[1]);
    const int oc = (int)(hi ? s3[0] : s3[1]);
    const float best = fmaxf(M1, o1);
    const float second = fmaxf(fminf(M1, o1), fmaxf(M2, o2));
    c1 = (M1 > o1 || (M1 == o1 && c1 < oc)) ? c1 : oc;
    M1 = best; M2 = second;
  }
  if (hi == 0 && rok) {
    float e2 = 0.f;
    for (int i = 0; i < Cp / 64; ++i) e2 = fmaxf(e2, emax2_blk[i]);  // (wave-uniform addresses: scalar loads)
    const float xn = sqrtf(x2) * 1.0001f, em = sqrtf(e2) * 1.0001f;
    const float eps = VQ_EPS_K1 * xn * em + vq_eps_k2<E>() * (xn + em) * (xn + em);
    // (false for NaN / inf anywhere; c1 < C: no row is ever decided for a padding code, whatever the data)
    const bool sure = (M1 - M2) > 2.f * eps && M1 < INFINITY && x2 < INFINITY && c1 < C;
    if (sure) {
      IDX[row] = c1;
      if (DMIN != nullptr) {
        const float* crow = CB + (long)c1 * E;
        DMIN[row] = dist_exact<E>([&](int e) { return xrow[e]; }, [&](int e) { return crow[e]; });
      }
    } else {
      flagged[atomicAdd(nflag, 1)] = (int)row;
    }
  }
}

// rows the screening could not decide: the whole codebook in the pinned arithmetic -- exactly what vq_argmin_kernel computes for
// the row.  A block takes ONE flagged row, its waves an interleaved share of the codebook's 64-code tiles each: a tile goes
// through a WAVE-PRIVATE LDS image (coalesced 16-byte loads, the next tile's first sixteen per lane in flight while this one is
// evaluated; rows pitched E + 1 floats: lane = code reads its row conflict-free; no block barrier per tile); lexicographic
// (distance, index) minimum over the wave, then over the waves.  C >= 64 here.  A ragged last tile starts at C - 64 instead: the
// codes it evaluates a second time leave the lexicographic minimum as it is.  A codebook of fewer than 64 codes comes as the prep
// kernel's 64-row copy, filled up with repeats of its last code: a repeat has that code's distance and a higher index, so it is
// never the minimum either.
template <int E>
__global__ __launch_bounds__(64 * vq_geo<E>::RC_NW) void vq_recheck_kernel(const float* __restrict__ X, long ldx,
                                                                           const float* __restrict__ CB, int64_t* __restrict__ IDX,
                                                                           float* __restrict__ DMIN, const int* __restrict__ nflag,
                                                                           const int* __restrict__ flagged, int C) {
  using G = vq_geo<E>;
  constexpr int NW = G::RC_NW, PITCH = G::RC_PITCH, NQ = G::RC_NQ, PQ = G::RC_PQ;
  extern __shared__ __attribute__((aligned(16))) float rc_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const tile = rc_lds + wave * G::RC_TILE;
  float* const sd = rc_lds + NW * G::RC_TILE;
  int* const sc = reinterpret_cast<int*>(sd + NW);
  const int n = *nflag;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {                       // block-uniform trip count: barriers inside are safe
    const int row = __builtin_amdgcn_readfirstlane(flagged[i]);
    const float* xrow = X + (long)row * ldx;                              // wave-uniform: scalar loads
    float xr[E <= 64 ? E : 1];                                            // (wider rows stay on the scalar path: read where used)
    if constexpr (E <= 64) {
#pragma unroll
      for (int e = 0; e < E; ++e) xr[e] = xrow[e];
    }
    auto xf = [&](int e) {
      if constexpr (E <= 64) return xr[e]; else return xrow[e];
    };
    float bd = INFINITY;
    int bc = INT_MAX;
    // a tile = 64 codes x NQ chunks of 16 bytes: chunk q = lane + 64 k belongs to code q / NQ, columns 4 (q % NQ) ..; piece p is
    // the chunks k = PQ p .. PQ p + PQ - 1
    f32x4 nxt[PQ];
    auto fetch = [&](int c0, int p) {
      const float* src = CB + (long)min(c0, C - 64) * E + lane * 4;       // (past the end: the last whole tile)
#pragma unroll
      for (int k = 0; k < PQ; ++k) nxt[k] = *reinterpret_cast<const f32x4*>(src + 256 * (PQ * p + k));
    };
    auto put = [&](int p) {
#pragma unroll
      for (int k = 0; k < PQ; ++k) {
        const int q = lane + 64 * (PQ * p + k);
        float* d = tile + (q / NQ) * PITCH + (q % NQ) * 4;
        d[0] = nxt[k][0]; d[1] = nxt[k][1]; d[2] = nxt[k][2]; d[3] = nxt[k][3];
      }
    };
    fetch(64 * wave, 0);
    for (int c0 = 64 * wave; c0 < C; c0 += 64 * NW) {
      put(0);
      for (int p = 1; p < NQ / PQ; ++p) { fetch(c0, p); put(p); }
      fetch(c0 + 64 * NW, 0);
      __builtin_amdgcn_sched_barrier(0);                                  // (the requests stay above the evaluation: hipcc would sink them to their use)
      __builtin_amdgcn_wave_barrier();
      const float* cr = tile + lane * PITCH;
      const float d = dist_exact<E>(xf, [&](int e) { return cr[e]; });
      if (d < bd) { bd = d; bc = min(c0, C - 64) + lane; }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float od = __shfl_xor(bd, m);
      const int oc = __shfl_xor(bc, m);
      if (od < bd || (od == bd && oc < bc)) { bd = od; bc = oc; }
    }
    if (lane == 0) { sd[wave] = bd; sc[wave] = bc; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float od = sd[w];
        const int oc = sc[w];
        if (od < bd || (od == bd && oc < bc)) { bd = od; bc = oc; }
      }
      IDX[row] = bc == INT_MAX ? 0 : bc;
      if (DMIN != nullptr) DMIN[row] = bd;
    }
    __syncthreads();
  }
}

constexpr long vq_cp(int C) { return ((long)C + 63) / 64 * 64; }

template <int E>
void vq_screened_launch(const float* x, long ldx, const float* codebook, int64_t* idx, float* dist_min, int N, int C, char* ws,
                        hipStream_t st) {
  using G = vq_geo<E>;
  const long Cp = vq_cp(C);
  int* nflag = (int*)(ws + 4);
  unsigned short* EH = (unsigned short*)(ws + 16);
  unsigned short* EL = EH + Cp * E;
  float* NH = (float*)(EL + Cp * E);
  float* CB64 = NH + Cp;
  float* emax2_blk = CB64 + 64 * E;
  int* flagged = (int*)(emax2_blk + Cp / 64);
  // (no hipMemsetAsync here: the call is captured into hipGraphs, where a memset node in front of kernels reading its target
  //  proved unreliable on replay -- the prep kernel zeroes the flag count)
  hipLaunchKernelGGL(vq_prep_kernel<E>, dim3((unsigned)(Cp / 64)), dim3(G::PREP_NT), 0, st, codebook, EH, EL, NH, CB64, emax2_blk, nflag, C);
  hipLaunchKernelGGL(vq_screen_kernel<E>, dim3(wmz_cdiv(N, ROWS_WG)), dim3(ROWS_WG * 2), 0, st, x, ldx, codebook, EH, EL, NH,
                     emax2_blk, idx, dist_min, nflag, flagged, N, C, (int)Cp);
  if constexpr (G::RC_LDS > 64 * 1024) {
    static std::atomic<uint64_t> attr_devs{0};                     // (> 64 KB of dynamic LDS has to be asked for once per device)
    if (wmz_first_use_on_device(attr_devs)) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vq_recheck_kernel<E>), hipFuncAttributeMaxDynamicSharedMemorySize, G::RC_LDS);
    }
  }
  // (the flagged-row count lives on the device: a grid that gives ~0.4 % of the rows a workgroup each, the rest leave at once)
  const int rgrid = N / 128 < 256 ? 256 : (N / 128 > 2048 ? 2048 : N / 128);
  hipLaunchKernelGGL(vq_recheck_kernel<E>, dim3(rgrid), dim3(64 * G::RC_NW), G::RC_LDS, st, x, ldx, C < 64 ? CB64 : codebook, idx, dist_min, nflag,
                     flagged, C < 64 ? 64 : C);
}

#define WMZ_VQ_STR_(x) #x
#define WMZ_VQ_NAME(E) " " WMZ_VQ_STR_(E)
constexpr const char* VQ_WIDTH_NAMES = WMZ_VQ_SCREEN_WIDTHS(WMZ_VQ_NAME);

constexpr bool vq_width_built(int E) {
#define WMZ_VQ_IS(W) if (E == W) return true;
  WMZ_VQ_SCREEN_WIDTHS(WMZ_VQ_IS)
#undef WMZ_VQ_IS
  return false;
}

}  // namespace

// Workspace layout (Cp = C rounded up to 64): [16 B: flag count at +4] [Cp x E bf16 heads] [Cp x E bf16 tails] [Cp floats -|e|^2/2]
// [64 x E floats: the re-check's copy of a codebook of fewer than 64 codes] [Cp/64 floats: block maxima of |e|^2] [N ints flagged rows]
extern "C" long wmz_vq_argmin_screened_workspace_bytes(int N, int C, int E) {
  if (!vq_width_built(E) || C < 1 || N <= 0) return 0;                 // 0: shape not built, use wmz_vq_argmin
  const long Cp = vq_cp(C);
  return 16 + Cp * E * 2 * 2 + Cp * 4 + 64L * E * 4 + (Cp / 64) * 4 + (long)N * 4;
}

extern "C" int wmz_vq_argmin_screened(const float* x, long ldx, const float* codebook, int64_t* idx, float* dist_min, int N, int C,
                                      int E, void* workspace, long workspace_bytes, void* stream) {
  WMZ_REQUIRE(x && codebook && idx && workspace, "wmz_vq_argmin_screened: null tensor");
  const long need = wmz_vq_argmin_screened_workspace_bytes(N, C, E);
  if (need == 0) {
    wmz_set_error("wmz_vq_argmin_screened: built for embedding_dim in {%s }, at least one code and one row (got E=%d C=%d N=%d)",
                  VQ_WIDTH_NAMES, E, C, N);
    return WMZ_ERR_UNSUPPORTED;
  }
  WMZ_REQUIRE(workspace_bytes >= need, "wmz_vq_argmin_screened: workspace %ld < %ld bytes", workspace_bytes, need);
  WMZ_REQUIRE(ldx % 4 == 0 && (reinterpret_cast<size_t>(x) & 15) == 0, "wmz_vq_argmin_screened: x rows must be 16-byte aligned");
  switch (E) {
#define WMZ_VQ_CASE(W) case W: vq_screened_launch<W>(x, ldx, codebook, idx, dist_min, N, C, (char*)workspace, (hipStream_t)stream); break;
    WMZ_VQ_SCREEN_WIDTHS(WMZ_VQ_CASE)
#undef WMZ_VQ_CASE
  }
  WMZ_LAUNCH_CHECK("wmz_vq_argmin_screened");
  return WMZ_OK;
}
