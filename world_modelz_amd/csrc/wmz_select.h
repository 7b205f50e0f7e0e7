// The exact selection of the lowest scores, shared by the kernels that re-mask by confidence: remask_lowest_kernel (loss.hip, the
// dense sampler: a plane's rows) and the scored form of sparse_context_kernel (sparse_context.hip: a context's slots).
// include/wmz.h states the law next to wmz_remask_lowest_dev.
#pragma once
#include <hip/hip_runtime.h>

// a product / a difference that the law rounds on its own: never one half of a contracted multiply-add
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// order-preserving keys: flip all bits of negatives, the sign bit of non-negatives
__device__ __forceinline__ unsigned sw_key(float l) {
  const unsigned b = __float_as_uint(l);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sw_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <int NW>
struct RmTotal {                      // the sum over NW waves of one count per wave (two alternating sets in LDS; NW == 1: the wave's own)
  unsigned* red;
  int turn;
  __device__ __forceinline__ unsigned operator()(unsigned wave_count) {
    if constexpr (NW == 1) {
      return wave_count;
    } else {
      unsigned* set = red + (turn & 1) * NW;
      turn ^= 1;
      if ((threadIdx.x & 63) == 0) set[threadIdx.x >> 6] = wave_count;
      __syncthreads();
      unsigned t = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += set[w];
      return t;
    }
  }
};

// NW waves hold the keys of up to MAXP * 64 * NW rows: thread t owns the rows j * 64 * NW + t, j < P <= MAXP -- key[j] (sw_key of the
// score; 0xFFFFFFFF where the row is no candidate or lies past the end, which no search step counts) and bit j of `cand`.
// -> bit j set: that row is among the mm (<= #candidates, uniform over the waves) candidates with the lowest keys.
//   * V = the mm-th smallest candidate key by the bitwise search: bit by bit from the top, V takes the bit while fewer than mm
//     candidate keys lie below V | bit (counts by wave ballots, the waves' counts through `total`);
//   * keys below V are taken; of the keys equal to V the first mm - #{key < V} in ROW order: row order is j-major, so the rank of
//     a tie is the ties of all earlier (j, wave) groups -- one count each in `ties` (LDS, MAXP * NW words; NW == 1: registers, no
//     LDS and no barrier at all) -- plus the ties of lower lanes in its own ballot.
template <int NW, int MAXP>
__device__ __forceinline__ unsigned wmz_select_lowest(const unsigned (&key)[MAXP], unsigned cand, int P, unsigned mm, unsigned* ties,
                                                      RmTotal<NW>& total) {
  if (mm == 0) return 0u;                                                    // (uniform over the waves: the barriers below are met by all)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;           // (wave: read where NW > 1 only)
  unsigned V = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cv = V | (1u << bit);
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < MAXP; ++j)                                            // (one wave: all of them, without a branch: a key past P counts nothing)
      if (NW == 1 || j < P) cnt += (unsigned)__popcll(__ballot(key[j] < cv));
    if (total(cnt) < mm) V = cv;
  }
  unsigned below = 0;
  unsigned own[MAXP];                                                        // this wave's ties of group j
#pragma unroll
  for (int j = 0; j < MAXP; ++j) {
    own[j] = 0;
    if (j < P) {
      below += (unsigned)__popcll(__ballot(key[j] < V));
      own[j] = (unsigned)__popcll(__ballot(((cand >> j) & 1u) != 0 && key[j] == V));
      if constexpr (NW > 1) {
        if (lane == 0) ties[j * NW + wave] = own[j];
      }
    }
  }
  const unsigned need = mm - total(below);                                   // (>= 1; its barrier also publishes `ties` where NW > 1)
  unsigned run = 0, taken = 0;                                               // ties of the groups in front of (j, wave)
#pragma unroll
  for (int j = 0; j < MAXP; ++j) {
    if (j < P) {
      const bool c = ((cand >> j) & 1u) != 0;
      const bool tie = c && key[j] == V;
      const unsigned long long tb = __ballot(tie);
      unsigned before = run;
      if constexpr (NW == 1) {
        run += own[j];
      } else {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const unsigned t = ties[j * NW + w];
          if (w < wave) before += t;
          run += t;
        }
      }
      const unsigned rank = before + (unsigned)__popcll(tb & ((1ull << lane) - 1ull));
      if (c && (key[j] < V || (tie && rank < need))) taken |= 1u << j;
    }
  }
  return taken;
}
