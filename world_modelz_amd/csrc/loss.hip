// The two steps either side of the denoiser in the training loop:
//   wmz_corrupt_tokens  main.py:246-259  mask + uniform token corruption of the last latent frame, without the [B,HW,C]
//                                        one-hot / lerp / multinomial temporaries (closed form, counter-based RNG in-kernel)
//   wmz_ce_fwd / _bwd   main.py:266-274  CrossEntropyLoss(reduction='none') over the last-frame logits and its gradient,
//                                        written directly in the GEMM operand dtype
#include "wmz_common.h"
#include "wmz_internal.h"
#include "wmz_philox.h"
#include "wmz_select.h"
#include <type_traits>

namespace {

// one thread per last-frame position.  a = 0.1 r: with probability a redraw uniformly over the C codes, else keep the
// token (== multinomial(lerp(one_hot, 1/C, a))); then positions with u < r become the mask token C.
__global__ __launch_bounds__(256) void corrupt_kernel(const int64_t* __restrict__ z_last, long clip_stride,
                                                      const float* __restrict__ r, int64_t* __restrict__ out,
                                                      long out_stride, int64_t* __restrict__ target, int B, int HW, int C,
                                                      unsigned long long seed, unsigned long long stream,
                                                      const unsigned long long* __restrict__ counter) {
  if (counter != nullptr) stream |= *counter & ((1ull << 40) - 1);      // per-call stream id kept in device memory (hipGraph replay)
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const int p = (int)(i - (long)b * HW);
    const int64_t tok = z_last[b * clip_stride + p];
    float u[4];
    philox4_unit((unsigned long long)i, stream, seed, u);
    const float rb = r[b];
    int64_t d = tok;
    if (u[0] < rb * 0.1f) { int k = (int)(u[1] * (float)C); d = k < C ? k : C - 1; }
    if (u[2] < rb) d = C;
    if (target) target[i] = tok;
    out[b * out_stride + p] = d;
  }
}

// One step of the sampler loop between two forward passes (main.py:76-104: top-k filter -> softmax -> multinomial -> re-mask):
// one wave per row of logits, everything in registers, both uniforms from one Philox call (wmz_philox.h).  Lane l holds the NV consecutive
// classes l * NV .. (classes past C are -inf).
//   * top-k: the k-th largest logit by a 32-step bitwise search on order-preserving integer keys (count of keys >= candidate
//     by wave ballots); logits below it are dropped, ties with it kept (the reference's `logits < v[:, -1]`);
//   * softmax weights w = exp(l - max), total by wave reduction;
//   * the draw: the number of classes whose cumulative weight is <= u * total (inverse CDF, the definition of
//     sample.categorical_from_uniform), clamped to C - 1;
//   * re-mask: with a second uniform u2 > alpha (and, with `last_mask`, only where the previous iteration masked:
//     consistent masking) the position gets the mask token instead of the draw.
// alpha = alphas[*counter % n_alpha] and the Philox stream id = *counter live in device memory: the launch sits in a hipGraph.
// What wmz_sample_tokens_filtered_dev adds (include/wmz.h states the law), each compiled in only where it acts:
//   * TEMP: l = logits * inv_temperature on the way into the registers;
//   * TOPP: the nucleus threshold by the same bitwise search on the bits of the weights (non-negative floats order like their
//     bits), accumulating the mass of the weights >= candidate instead of a count; weights below it are dropped;
//   * PROBES: the uniforms from `uniforms` and the smallest kept l to `kept_floor`, each where the pointer is given.
struct SampleExtras {
  float top_p, inv_temperature;
  const float* uniforms;
  float* kept_floor;
};

// The scored form (wmz_sample_tokens_scored_dev; include/wmz.h states the law): a ScoreOut behind the SampleExtras compiles in
//   * SCORED: the sum of exp(l - max) over ALL classes, taken before top-k overwrites the values where a filter acts (else it is the
//     draw's own total), the drawn class's scaled logit read back from the row, score = (l_d - max) - log(sum) (+ the Gumbel term
//     from u1 with noise > 0) to `scores`; the draw goes to out_tokens as it is: no re-mask (wmz_remask_lowest_dev does that).
struct ScoreOut {
  float* scores;
  float noise;
};

__device__ __forceinline__ SampleExtras sample_extras() { return SampleExtras{}; }
__device__ __forceinline__ SampleExtras sample_extras(const SampleExtras& x) { return x; }
__device__ __forceinline__ SampleExtras sample_extras(const SampleExtras& x, const ScoreOut&) { return x; }
__device__ __forceinline__ ScoreOut score_out() { return ScoreOut{}; }
__device__ __forceinline__ ScoreOut score_out(const SampleExtras&) { return ScoreOut{}; }
__device__ __forceinline__ ScoreOut score_out(const SampleExtras&, const ScoreOut& s) { return s; }

// The sparse form (wmz_categorical_scatter_filtered: config 5's sampler): a SparseOut behind the SampleExtras compiles in
//   * SPARSE: u0 = uniforms[row] (one a row) or the first word of philox4(row, the SparseOut's stream, seed) -- the position
//     categorical_scatter_kernel reads --; no alpha, no counter of the dense step, no re-mask; the draw is the first KEPT class past
//     u0 * total (the last kept one if rounding leaves none) and goes where wmz_sparse_write puts it.
typedef WmzSparseOut SparseOut;
__device__ __forceinline__ SampleExtras sample_extras(const SampleExtras& x, const SparseOut&) { return x; }
__device__ __forceinline__ ScoreOut score_out(const SampleExtras&, const SparseOut&) { return ScoreOut{}; }
__device__ __forceinline__ SparseOut sparse_out() { return SparseOut{}; }
template <typename A, typename... Rest>
__device__ __forceinline__ SparseOut sparse_out(const A& a, const Rest&... rest) {
  if constexpr (std::is_same<A, SparseOut>::value) return a; else return sparse_out(rest...);
}
template <typename T, typename... Ts>
constexpr bool pack_has = (std::is_same<T, Ts>::value || ...);
// The scored sparse form (wmz_categorical_scatter_scored): a SparseScore behind the SparseOut compiles in SPARSE and the sum over
// all classes of SCORED; the score -- sample_score without noise -- goes where wmz_sparse_write_scored puts the token.
typedef WmzSparseScore SparseScore;
__device__ __forceinline__ SampleExtras sample_extras(const SampleExtras& x, const SparseOut&, const SparseScore&) { return x; }
__device__ __forceinline__ ScoreOut score_out(const SampleExtras&, const SparseOut&, const SparseScore&) { return ScoreOut{}; }
__device__ __forceinline__ SparseScore sparse_score() { return SparseScore{}; }
template <typename A, typename... Rest>
__device__ __forceinline__ SparseScore sparse_score(const A& a, const Rest&... rest) {
  if constexpr (std::is_same<A, SparseScore>::value) return a; else return sparse_score(rest...);
}
// the dense step's counter and alpha: not read in the sparse form, whose launch passes NULL for both
template <bool SPARSE>
__device__ __forceinline__ long dense_counter(const long long* counter) {
  if constexpr (SPARSE) return 0; else return *counter;
}
template <bool SPARSE>
__device__ __forceinline__ float dense_alpha(const float* alphas, int n_alpha, long ctr) {
  if constexpr (SPARSE) return 0.f; else return alphas[(int)(ctr % n_alpha)];
}

// score of a drawn row: lp = (l_d - max) - log(sum over all classes); NaN -> -inf
__device__ __forceinline__ float sample_score(float l_d, float m, float sum_all, float noise, float alpha, float u1) {
  float s = sub_rn(l_d, m) - logf(sum_all);
  if (noise > 0.f) s += noise * (1.f - alpha) * -logf(-logf(u1));
  return s == s ? s : -INFINITY;
}

// (`extras`: nothing -- the kernel of wmz_sample_tokens_dev, its arguments as they always were --, one SampleExtras, or a
//  SampleExtras and a ScoreOut: the scored form, or a SampleExtras and a SparseOut: the sparse form, which leaves the dense
//  step's own arguments -- alphas .. counter -- unread; a SparseScore behind the SparseOut: the scored sparse form)
template <int NV, bool TEMP = false, bool TOPP = false, typename... Extras>
__global__ __launch_bounds__(256) void sample_tokens_kernel(const float* __restrict__ logits, long ld, int R, int C, int top_k,
                                                            const float* __restrict__ alphas, int n_alpha, int64_t mask_token,
                                                            int64_t* __restrict__ out_tokens, long rows_per_block,
                                                            long block_stride, int64_t* __restrict__ denoised,
                                                            unsigned char* __restrict__ last_mask, unsigned long long seed,
                                                            const long long* __restrict__ counter, Extras... extras) {
  static_assert(sizeof...(Extras) <= 3 && (sizeof...(Extras) >= 1 || !(TEMP || TOPP)), "the filters read their values from a SampleExtras");
  constexpr bool PROBES = sizeof...(Extras) >= 1;
  constexpr bool SPARSE_SCORED = pack_has<SparseScore, Extras...>;
  constexpr bool SCORED = pack_has<ScoreOut, Extras...> || SPARSE_SCORED;
  constexpr bool SPARSE = pack_has<SparseOut, Extras...>;
  static_assert(!SPARSE_SCORED || SPARSE, "a SparseScore follows a SparseOut");
  const SampleExtras x = sample_extras(extras...);
  const ScoreOut so = score_out(extras...);
  const SparseOut sp = sparse_out(extras...);
  const SparseScore ss = sparse_score(extras...);
  const int lane = threadIdx.x & 63;
  const long ctr = dense_counter<SPARSE>(counter);
  const float alpha = dense_alpha<SPARSE>(alphas, n_alpha, ctr);
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (long)gridDim.x * 4) {
    const float* x_lane = logits + row * ld + lane * NV;
    float v[NV];
#pragma unroll
    for (int e = 0; e < NV; e += 4) {
      if (lane * NV + e + 3 < C) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(x_lane + e);
        v[e] = q[0]; v[e + 1] = q[1]; v[e + 2] = q[2]; v[e + 3] = q[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[e + i] = lane * NV + e + i < C ? x_lane[e + i] : -INFINITY;
      }
    }
    if constexpr (TEMP) {
#pragma unroll
      for (int e = 0; e < NV; ++e) v[e] *= x.inv_temperature;            // (-inf stays -inf: inv_temperature > 0)
    }
    const bool all_kept = !TOPP && !(top_k > 0 && top_k < C);    // no filter acts: the draw's total is the sum over all classes
    float sum_all = 0.f;
    if constexpr (SCORED) {
      if (!all_kept) {
        float m0 = v[0];
#pragma unroll
        for (int e = 1; e < NV; ++e) m0 = fmaxf(m0, v[e]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m0 = fmaxf(m0, __shfl_xor(m0, o));
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) part += __expf(sub_rn(v[e], m0));           // (no contraction with the scaling: l is the rounded product)
        sum_all = wave_sum(part);
      }
    }
    if (top_k > 0 && top_k < C) {
      // order-preserving keys: flip all bits of negatives, the sign bit of non-negatives
      unsigned key[NV];
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        const unsigned b = __float_as_uint(v[e]);
        key[e] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
      }
      unsigned T = 0;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = T | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < NV; ++e) cnt += __popcll(__ballot(key[e] >= cand));
        if (cnt >= top_k) T = cand;
      }
#pragma unroll
      for (int e = 0; e < NV; ++e) if (key[e] < T) v[e] = -INFINITY;
    }
    float m = v[0];
#pragma unroll
    for (int e = 1; e < NV; ++e) m = fmaxf(m, v[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if constexpr (TOPP) {
      float wt[NV], part = 0.f;
#pragma unroll
      for (int e = 0; e < NV; ++e) { wt[e] = __expf(v[e] - m); part += wt[e]; }
      // (one lane's sums decide for the wave: the lanes must agree on T)
      const float need = x.top_p * __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_sum(part))));
      unsigned T = 0;                                          // (bit 31 is the sign: never set in a weight)
      for (int bit = 30; bit >= 0; --bit) {
        const unsigned cand = T | (1u << bit);
        float mass = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) mass += __float_as_uint(wt[e]) >= cand ? wt[e] : 0.f;
        if (__uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_sum(mass)))) >= need) T = cand;
      }
#pragma unroll
      for (int e = 0; e < NV; ++e) if (__float_as_uint(wt[e]) < T) v[e] = -INFINITY;
    }
    float w[NV], part = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) { w[e] = __expf(v[e] - m); part += w[e]; w[e] = part; }    // lane-local running sums
    float inc = part;                                          // inclusive scan of the lane totals, in lane order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    const float total = __shfl(inc, 63);
    const float base = inc - part;
    float u[4];
    bool given = false;
    if constexpr (PROBES) given = x.uniforms != nullptr;
    if constexpr (SPARSE) {
      if (given) u[0] = x.uniforms[row];
      else philox4_unit((unsigned long long)row, wmz_sparse_stream(sp), seed, u);
      u[1] = 0.f;
    } else if (given) {
      u[0] = x.uniforms[2 * row];
      u[1] = x.uniforms[2 * row + 1];
    } else {
      philox4_unit((unsigned long long)row, (unsigned long long)ctr, seed, u);
    }
    const float xq = u[0] * total;
    int draw;
    if constexpr (SPARSE) {
      int first = 0x7fffffff, last = -1;                       // kept classes of this lane: the first past xq, the last
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        if (v[e] > -INFINITY && (e == 0 ? w[0] : w[e] - w[e - 1]) > 0.f) {
          last = lane * NV + e;
          if (base + w[e] > xq) first = min(first, lane * NV + e);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        first = min(first, __shfl_xor(first, o));
        last = max(last, __shfl_xor(last, o));
      }
      draw = first != 0x7fffffff ? first : (last >= 0 ? last : C - 1);
    } else {
      int below = 0;
#pragma unroll
      for (int e = 0; e < NV; ++e) below += (lane * NV + e < C && base + w[e] <= xq) ? 1 : 0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o);
      draw = below < C ? below : C - 1;
    }
    if constexpr (PROBES) {
      if (x.kept_floor != nullptr) {
        float f = INFINITY;
#pragma unroll
        for (int e = 0; e < NV; ++e) f = v[e] > -INFINITY ? fminf(f, v[e]) : f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) f = fminf(f, __shfl_xor(f, o));
        if (lane == 0) x.kept_floor[row] = f;
      }
    }
    if constexpr (SPARSE_SCORED) {
      if (lane == 0) {
        const float l_d = TEMP ? mul_rn(logits[row * ld + draw], x.inv_temperature) : logits[row * ld + draw];
        wmz_sparse_write_scored(sp, ss, row, draw, sample_score(l_d, m, all_kept ? total : sum_all, 0.f, 0.f, 0.f));
      }
    } else if constexpr (SPARSE) {
      if (lane == 0) wmz_sparse_write(sp, row, draw);
    } else if constexpr (SCORED) {
      if (lane == 0) {
        const float l_d = TEMP ? mul_rn(logits[row * ld + draw], x.inv_temperature) : logits[row * ld + draw];
        so.scores[row] = sample_score(l_d, m, all_kept ? total : sum_all, so.noise, alpha, u[1]);
        denoised[row] = draw;
        const long blk = row / rows_per_block;
        out_tokens[blk * block_stride + (row - blk * rows_per_block)] = (int64_t)draw;
      }
    } else if (lane == 0) {
      bool mask = u[1] > alpha;
      if (last_mask != nullptr) { mask = mask && last_mask[row] != 0; last_mask[row] = mask ? 1 : 0; }
      denoised[row] = draw;
      const long blk = row / rows_per_block;
      out_tokens[blk * block_stride + (row - blk * rows_per_block)] = mask ? mask_token : (int64_t)draw;
    }
  }
}

// The same step for rows that do not fit a wave's registers (2048 < C <= SW_MAX_CLASSES): one workgroup of SW_NT threads per row.
// The row is read from global memory ONCE -- 16-byte loads, scaled, turned into the order-preserving keys above -- into LDS, and
// every later pass works from there.  Thread t owns the P consecutive classes t * P .. (P a multiple of 8, classes past C are
// -inf), kept at a pitch of P + 4 words: P / 4 + 1 is odd, so the 16-byte slots that consecutive lanes read in one ds_read_b128
// fall on different banks.  The passes, each a walk of the thread's own slots:
//   * the maximum (of the keys: same order);
//   * top-k: the bitwise search, counts by wave ballots, the four waves' counts through LDS (one barrier per step);
//   * keys -> weights w = exp(l - max) in place, 0 for what top-k dropped;
//   * nucleus: the bitwise search on the weights' bits accumulating mass; weights below the threshold become 0;
//   * the prefix in class order -- sequential in the thread, shuffle scan over the lanes, the waves' totals in wave order --
//     and the draw: the FIRST KEPT class whose cumulative weight exceeds u0 * total (the last kept one if rounding leaves none):
//     a class of weight 0 is never drawn, whatever the rounding of the partial sums.
// The kept_floor probe alone walks the global row a second time (the keys are gone by then): it is NULL in production.
// (`score`: nothing, or one ScoreOut -- the scored form: where a filter acts, one more walk of the thread's slots in front of top-k
//  sums exp(l - max) over all classes; else that sum is the draw's total --, or one SparseOut, or a SparseOut and a SparseScore.)
constexpr int SW_NT = 256;
constexpr int SW_MAX_CLASSES = 16384;
constexpr int SW_RED_WORDS = 16;          // two alternating sets of (SW_NT / 64 waves) x 2 words behind the row

// (sw_key / sw_unkey, the order-preserving keys of the searches below: wmz_select.h)
// The four waves' (a, b) pairs to every thread: each wave's lane 0 writes, one barrier, all read.  The sets alternate, so a wave
// that runs ahead into the next exchange writes the other set while a slower one still reads this one.
struct SwExchange {
  unsigned* red;
  int turn;
  __device__ __forceinline__ void operator()(unsigned a, unsigned b, unsigned (&oa)[4], unsigned (&ob)[4]) {
    unsigned* set = red + (turn & 1) * 8;
    turn ^= 1;
    if ((threadIdx.x & 63) == 0) { set[threadIdx.x >> 6] = a; set[4 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) { oa[w] = set[w]; ob[w] = set[4 + w]; }
  }
};

template <typename... Score>
__global__ __launch_bounds__(SW_NT) void sample_tokens_wide_kernel(const float* __restrict__ logits, long ld, int R, int C, int P, int top_k,
                                                                   float top_p, float inv_temperature,
                                                                   const float* __restrict__ alphas, int n_alpha, int64_t mask_token,
                                                                   int64_t* __restrict__ out_tokens, long rows_per_block,
                                                                   long block_stride, int64_t* __restrict__ denoised,
                                                                   unsigned char* __restrict__ last_mask,
                                                                   const float* __restrict__ uniforms, float* __restrict__ kept_floor,
                                                                   unsigned long long seed, const long long* __restrict__ counter,
                                                                   Score... score) {
  static_assert(sizeof...(Score) <= 2, "one ScoreOut, or one SparseOut and its SparseScore, at the most");
  constexpr bool SPARSE_SCORED = pack_has<SparseScore, Score...>;
  constexpr bool SCORED = pack_has<ScoreOut, Score...> || SPARSE_SCORED;
  constexpr bool SPARSE = pack_has<SparseOut, Score...>;
  static_assert(!SPARSE_SCORED || SPARSE, "a SparseScore follows a SparseOut");
  const ScoreOut so = score_out(SampleExtras{}, score...);
  const SparseOut sp = sparse_out(score...);
  const SparseScore ss = sparse_score(score...);
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  extern __shared__ __attribute__((aligned(16))) unsigned sw_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pitch = P + 4, nq = P >> 2;
  u32x4* mine = reinterpret_cast<u32x4*>(sw_lds + tid * pitch);
  SwExchange exchange{sw_lds + SW_NT * pitch, 0};
  unsigned ra[4], rb[4];
  const long ctr = dense_counter<SPARSE>(counter);
  const float alpha = dense_alpha<SPARSE>(alphas, n_alpha, ctr);
  for (long row = blockIdx.x; row < R; row += gridDim.x) {
    const float* x = logits + row * ld;
    for (int c = tid * 4; c < SW_NT * P; c += SW_NT * 4) {
      f32x4 q;
      if (c + 3 < C) {
        q = *reinterpret_cast<const f32x4*>(x + c) * inv_temperature;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = c + i < C ? x[c + i] * inv_temperature : -INFINITY;
      }
      const u32x4 k = {sw_key(q[0]), sw_key(q[1]), sw_key(q[2]), sw_key(q[3])};
      *reinterpret_cast<u32x4*>(sw_lds + c + 4 * (c / P)) = k;             // (P is a multiple of 4: the four share an owner)
    }
    __syncthreads();
    unsigned kmax = 0;
    for (int q = 0; q < nq; ++q) {
      const u32x4 k = mine[q];
      kmax = max(max(kmax, max(k[0], k[1])), max(k[2], k[3]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
    exchange(kmax, 0u, ra, rb);
    const float m = sw_unkey(max(max(ra[0], ra[1]), max(ra[2], ra[3])));
    const bool all_kept = !(top_p < 1.f) && !(top_k > 0 && top_k < C);
    float sum_all = 0.f;
    if constexpr (SCORED) {
      if (!all_kept) {
        float part = 0.f;
        for (int q = 0; q < nq; ++q) {
          const u32x4 k = mine[q];
#pragma unroll
          for (int i = 0; i < 4; ++i) part += __expf(sub_rn(sw_unkey(k[i]), m));
        }
        exchange(__float_as_uint(wave_sum(part)), 0u, ra, rb);
        sum_all = (__uint_as_float(ra[0]) + __uint_as_float(ra[1])) + (__uint_as_float(ra[2]) + __uint_as_float(ra[3]));
      }
    }
    unsigned Tk = 0;
    if (top_k > 0 && top_k < C) {
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = Tk | (1u << bit);
        int cnt = 0;
        for (int q = 0; q < nq; ++q) {
          const u32x4 k = mine[q];
#pragma unroll
          for (int i = 0; i < 4; ++i) cnt += __popcll(__ballot(k[i] >= cand));
        }
        exchange((unsigned)cnt, 0u, ra, rb);
        if ((int)(ra[0] + ra[1] + ra[2] + ra[3]) >= top_k) Tk = cand;
      }
    }
    float part = 0.f;                                          // the thread's kept weight, summed in class order
    for (int q = 0; q < nq; ++q) {
      const u32x4 k = mine[q];
      u32x4 wq;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float w = k[i] >= Tk ? __expf(sw_unkey(k[i]) - m) : 0.f;
        part += w;
        wq[i] = __float_as_uint(w);
      }
      mine[q] = wq;
    }
    unsigned Tw = 0;
    if (top_p < 1.f) {
      exchange(__float_as_uint(wave_sum(part)), 0u, ra, rb);
      const float need = top_p * ((__uint_as_float(ra[0]) + __uint_as_float(ra[1])) + (__uint_as_float(ra[2]) + __uint_as_float(ra[3])));
      for (int bit = 30; bit >= 0; --bit) {                    // (bit 31 is the sign: never set in a weight)
        const unsigned cand = Tw | (1u << bit);
        float mass = 0.f;
        for (int q = 0; q < nq; ++q) {
          const u32x4 wq = mine[q];
#pragma unroll
          for (int i = 0; i < 4; ++i) mass += wq[i] >= cand ? __uint_as_float(wq[i]) : 0.f;
        }
        exchange(__float_as_uint(wave_sum(mass)), 0u, ra, rb);
        if ((__uint_as_float(ra[0]) + __uint_as_float(ra[1])) + (__uint_as_float(ra[2]) + __uint_as_float(ra[3])) >= need) Tw = cand;
      }
      part = 0.f;
      for (int q = 0; q < nq; ++q) {
        u32x4 wq = mine[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (wq[i] < Tw) wq[i] = 0u;
          part += __uint_as_float(wq[i]);
        }
        mine[q] = wq;
      }
    }
    float inc = part;                                          // inclusive scan of the threads' totals: lanes, then waves, in order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    exchange(__float_as_uint(__shfl(inc, 63)), 0u, ra, rb);
    float before = 0.f, total = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) before = total;
      total += __uint_as_float(ra[w]);
    }
    const float base = before + (inc - part);
    float u[4];
    if constexpr (SPARSE) {
      if (uniforms != nullptr) u[0] = uniforms[row];
      else philox4_unit((unsigned long long)row, wmz_sparse_stream(sp), seed, u);
      u[1] = 0.f;
    } else if (uniforms != nullptr) {
      u[0] = uniforms[2 * row];
      u[1] = uniforms[2 * row + 1];
    } else {
      philox4_unit((unsigned long long)row, (unsigned long long)ctr, seed, u);
    }
    const float xq = u[0] * total;
    int first = 0x7fffffff, last = -1;                            // kept classes of this thread: the first past xq, the last
    float run = 0.f;
    for (int q = 0; q < nq; ++q) {
      const u32x4 wq = mine[q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = tid * P + q * 4 + i;
        run += __uint_as_float(wq[i]);
        if (wq[i] != 0u) {
          last = c;
          if (base + run > xq) first = min(first, c);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      first = min(first, __shfl_xor(first, o));
      last = max(last, __shfl_xor(last, o));
    }
    exchange((unsigned)first, (unsigned)last, ra, rb);
    first = min(min((int)ra[0], (int)ra[1]), min((int)ra[2], (int)ra[3]));
    last = max(max((int)rb[0], (int)rb[1]), max((int)rb[2], (int)rb[3]));
    const int draw = first != 0x7fffffff ? first : (last >= 0 ? last : C - 1);
    if (kept_floor != nullptr) {                               // probe: the keys are gone, so the same law over the global row again
      unsigned kmin = 0xFFFFFFFFu;
      for (int c = tid; c < C; c += SW_NT) {
        const unsigned k = sw_key(x[c] * inv_temperature);
        if (k >= Tk) {
          const unsigned wb = __float_as_uint(__expf(sw_unkey(k) - m));
          if (Tw == 0u || wb >= Tw) kmin = min(kmin, k);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
      exchange(kmin, 0u, ra, rb);
      if (tid == 0) kept_floor[row] = sw_unkey(min(min(ra[0], ra[1]), min(ra[2], ra[3])));
    }
    if constexpr (SPARSE_SCORED) {
      if (tid == 0)
        wmz_sparse_write_scored(sp, ss, row, draw,
                                sample_score(mul_rn(x[draw], inv_temperature), m, all_kept ? total : sum_all, 0.f, 0.f, 0.f));
    } else if constexpr (SPARSE) {
      if (tid == 0) wmz_sparse_write(sp, row, draw);
    } else if constexpr (SCORED) {
      if (tid == 0) {
        so.scores[row] = sample_score(mul_rn(x[draw], inv_temperature), m, all_kept ? total : sum_all, so.noise, alpha, u[1]);
        denoised[row] = draw;
        const long blk = row / rows_per_block;
        out_tokens[blk * block_stride + (row - blk * rows_per_block)] = (int64_t)draw;
      }
    } else if (tid == 0) {
      bool mask = u[1] > alpha;
      if (last_mask != nullptr) { mask = mask && last_mask[row] != 0; last_mask[row] = mask ? 1 : 0; }
      denoised[row] = draw;
      const long blk = row / rows_per_block;
      out_tokens[blk * block_stride + (row - blk * rows_per_block)] = mask ? mask_token : (int64_t)draw;
    }
    __syncthreads();                                           // (the next row is staged over slots other threads own)
  }
}

// The selection behind the scored draw (wmz_remask_lowest_dev; include/wmz.h states the law): one workgroup of NW waves per clip of
// n rows, NW = 1 up to 256 rows (no LDS, no barrier in the search: the config-4 planes), 4 up to RM_MAX_ROWS.  Thread t owns the rows
// j * NT + t, j < MAXP: their keys (sw_key of the score: ascending like the scores) are read ONCE, coalesced, into MAXP registers --
// a non-candidate or a row past the clip as 0xFFFFFFFF, which no search step counts -- and the candidate bits into one more; a
// search step is then MAXP compares and ballots without a memory access (a first form that kept the keys in LDS spent ~140 ns per
// key read and ballot, one wave per SIMD having nothing to hide the LDS latency behind: 18 us at 256 rows, 67 us at 4096).
// The search itself -- the mm-th smallest candidate key, mm = min(m, #candidates), ties ranked in row order -- is
// wmz_select_lowest (wmz_select.h), which config 5's scored context draw runs too.
constexpr int RM_MAX_ROWS = 4096;
constexpr int RM_ONE_WAVE_ROWS = 256;

template <int NW>
__global__ __launch_bounds__(64 * NW) void remask_lowest_kernel(const float* __restrict__ scores, long n,
                                                                const float* __restrict__ alphas, int n_alpha, int64_t mask_token,
                                                                int64_t* __restrict__ out_tokens, long block_stride,
                                                                unsigned char* __restrict__ last_mask,
                                                                const long long* __restrict__ counter) {
  constexpr int NT = 64 * NW;
  constexpr int MAXP = (NW == 1 ? RM_ONE_WAVE_ROWS : RM_MAX_ROWS) / NT;
  __shared__ unsigned ties[MAXP * NW];
  __shared__ unsigned red[2 * NW];
  const int tid = threadIdx.x;
  const int rows = (int)n, P = (rows + NT - 1) / NT;                         // (P <= MAXP: the launch's check)
  const long clip = blockIdx.x;
  const float alpha = alphas[(int)(*counter % n_alpha)];
  const int m = (int)floorf(mul_rn(sub_rn(1.0f, alpha), (float)rows));
  RmTotal<NW> total{red, 0};
  unsigned key[MAXP];                                                        // 0xFFFFFFFF where the row is no candidate
  unsigned cand = 0;                                                         // bit j: row j * NT + tid is a candidate
  unsigned ncand = 0;
#pragma unroll
  for (int j = 0; j < MAXP; ++j) {
    const int row = j * NT + tid;
    bool c = false;
    key[j] = 0xFFFFFFFFu;
    if (j < P && row < rows) {
      c = last_mask == nullptr || last_mask[clip * n + row] != 0;
      if (c) key[j] = sw_key(scores[clip * n + row]);
    }
    cand |= (c ? 1u : 0u) << j;
    if (j < P) ncand += (unsigned)__popcll(__ballot(c));
  }
  ncand = total(ncand);
  const unsigned mm = m <= 0 ? 0u : ((unsigned)m < ncand ? (unsigned)m : ncand);
  const unsigned taken = wmz_select_lowest<NW, MAXP>(key, cand, P, mm, ties, total);
#pragma unroll
  for (int j = 0; j < MAXP; ++j) {
    const int row = j * NT + tid;
    if (j < P && row < rows) {
      const bool masked = ((taken >> j) & 1u) != 0;
      if (masked) out_tokens[clip * block_stride + row] = mask_token;
      if (last_mask != nullptr) last_mask[clip * n + row] = masked ? 1 : 0;
    }
  }
}

// one wave per row; C <= 64 * 4 * KV handled by a strided loop
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, long ld, const int64_t* __restrict__ target,
                                                     float* __restrict__ loss, float* __restrict__ lse, long R, int C) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (long)gridDim.x * 4) {
    const float* x = logits + row * ld;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += __expf(x[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
      const float l = m + logf(s);
      long t = target[row];
      t = t < 0 ? 0 : (t >= C ? C - 1 : t);
      lse[row] = l;
      loss[row] = l - x[t];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, long ld, const int64_t* __restrict__ target,
                                                     const float* __restrict__ lse, const float* __restrict__ grow,
                                                     T* __restrict__ dlogits, long R, int C) {
  const long total = R * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / C;
    const int c = (int)(i - row * C);
    const float p = __expf(logits[row * ld + c] - lse[row]);
    const float v = (p - (target[row] == c ? 1.f : 0.f)) * grow[row];
    dlogits[i] = Elem<T>::from_f32(v);
  }
}

// Both of the above in ONE pass: a wave holds its row in registers (NCH float4 per lane, C <= 256 NCH), so the [R, C] logits
// are read once instead of three times (max / sum-exp / gradient) and every access is 16 bytes (8 for the 16-bit gradient).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void ce_fused_kernel(const float* __restrict__ logits, long ld, const int64_t* __restrict__ target,
                                                       float* __restrict__ loss, float* __restrict__ lse,
                                                       const float* __restrict__ grow, T* __restrict__ dlogits, long R, int C) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (long)gridDim.x * 4) {
    const float* x = logits + row * ld;
    f32x4 v[NCH];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const int c = q * 256 + lane * 4;
      if (c + 4 <= C) {
        v[q] = *reinterpret_cast<const f32x4*>(x + c);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][e] = c + e < C ? x[c + e] : -INFINITY;
      }
      m = fmaxf(fmaxf(m, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += __expf(v[q][e] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float l = m + logf(s);
    long t = target[row];
    const int tc = (int)(t < 0 ? 0 : (t >= C ? C - 1 : t));
    if (lane == 0) {
      lse[row] = l;
      loss[row] = l - x[tc];
    }
    const float g = grow[row];
    // (an out-of-range target matches no column, as in ce_bwd_kernel -- decided on the 64-bit value: truncated to int, a target of
    //  2^32 + k would put a one-hot at column k)
    const int tt = t >= 0 && t < C ? (int)t : -1;
    T* d = dlogits + row * (long)C;
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const int c = q * 256 + lane * 4;
      float o4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = (__expf(v[q][e] - l) - (c + e == tt ? 1.f : 0.f)) * g;
      if (c + 4 <= C && (C & 3) == 0) {
        Elem<T>::store4(d + c, o4);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e < C) d[c + e] = Elem<T>::from_f32(o4[e]);
      }
    }
  }
}

}  // namespace

extern "C" int wmz_corrupt_tokens(const int64_t* z_last, long clip_stride, const float* r, int64_t* out, long out_stride,
                                  int64_t* target, int B, int HW, int C, unsigned long long seed, unsigned long long stream_id,
                                  void* stream) {
  WMZ_REQUIRE(z_last && r && out && B > 0 && HW > 0 && C > 0, "wmz_corrupt_tokens: bad arguments");
  const long total = (long)B * HW;
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(corrupt_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, z_last, clip_stride, r, out, out_stride,
                     target, B, HW, C, seed, stream_id, (const unsigned long long*)nullptr);
  WMZ_LAUNCH_CHECK("wmz_corrupt_tokens");
  return WMZ_OK;
}

// The same with the low 40 bits of the Philox stream id read from device memory at run time (`counter`, which the caller
// advances between launches): the launch can sit in a hipGraph and still draw a fresh mask on every replay.
extern "C" int wmz_corrupt_tokens_dev(const int64_t* z_last, long clip_stride, const float* r, int64_t* out, long out_stride,
                                      int64_t* target, int B, int HW, int C, unsigned long long seed,
                                      unsigned long long stream_hi, const unsigned long long* counter, void* stream) {
  WMZ_REQUIRE(z_last && r && out && counter && B > 0 && HW > 0 && C > 0, "wmz_corrupt_tokens_dev: bad arguments");
  const long total = (long)B * HW;
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(corrupt_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, z_last, clip_stride, r, out, out_stride,
                     target, B, HW, C, seed, stream_hi & ~((1ull << 40) - 1), counter);
  WMZ_LAUNCH_CHECK("wmz_corrupt_tokens_dev");
  return WMZ_OK;
}

// The sampler step's launches: `filtered` = reached through wmz_sample_tokens_filtered_dev (the checks are the callers').
static int sample_tokens_launch(const char* name, const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                                const float* alphas, int n_alpha, int64_t mask_token, int64_t* out_tokens, long rows_per_block,
                                long block_stride, int64_t* denoised, unsigned char* last_mask, const float* uniforms,
                                float* kept_floor, unsigned long long seed, const long long* counter, void* stream,
                                const ScoreOut* score = nullptr) {
  hipStream_t st = (hipStream_t)stream;
  const bool temp = inv_temperature != 1.f, topp = top_p < 1.f;
  if (C > 2048) {
    const int P = (wmz_cdiv(C, SW_NT) + 7) / 8 * 8;
    const size_t smem = ((size_t)SW_NT * (P + 4) + SW_RED_WORDS) * 4;
    static std::atomic<uint64_t> attr_devs{0};                       // (> 64 KB of dynamic LDS has to be asked for once per device)
    if (wmz_first_use_on_device(attr_devs)) {
      const int most = (int)(((size_t)SW_NT * (SW_MAX_CLASSES / SW_NT + 4) + SW_RED_WORDS) * 4);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tokens_wide_kernel<>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tokens_wide_kernel<ScoreOut>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                most);
    }
    if (score == nullptr)
      hipLaunchKernelGGL(sample_tokens_wide_kernel<>, dim3(R < 4096 ? R : 4096), dim3(SW_NT), smem, st, logits, ld, R, C, P, top_k, top_p,
                         inv_temperature, alphas, n_alpha, mask_token, out_tokens, rows_per_block, block_stride, denoised, last_mask,
                         uniforms, kept_floor, seed, counter);
    else
      hipLaunchKernelGGL(sample_tokens_wide_kernel<ScoreOut>, dim3(R < 4096 ? R : 4096), dim3(SW_NT), smem, st, logits, ld, R, C, P, top_k,
                         top_p, inv_temperature, alphas, n_alpha, mask_token, out_tokens, rows_per_block, block_stride, denoised,
                         last_mask, uniforms, kept_floor, seed, counter, *score);
    WMZ_LAUNCH_CHECK(name);
    return WMZ_OK;
  }
  const int grid = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
  if (score != nullptr) {
    const SampleExtras x = {top_p, inv_temperature, uniforms, kept_floor};
#define WMZ_SMP(NV, TEMP, TOPP) hipLaunchKernelGGL((sample_tokens_kernel<NV, TEMP, TOPP, SampleExtras, ScoreOut>), dim3(grid), dim3(256), 0, st, logits, ld, \
                                                   R, C, top_k, alphas, n_alpha, mask_token, out_tokens, rows_per_block, block_stride,             \
                                                   denoised, last_mask, seed, counter, x, *score)
#define WMZ_SMP_NV(TEMP, TOPP) \
  do { if (C <= 256) WMZ_SMP(4, TEMP, TOPP); else if (C <= 512) WMZ_SMP(8, TEMP, TOPP); else if (C <= 1024) WMZ_SMP(16, TEMP, TOPP); else WMZ_SMP(32, TEMP, TOPP); } while (0)
    if (temp && topp) WMZ_SMP_NV(true, true); else if (temp) WMZ_SMP_NV(true, false); else if (topp) WMZ_SMP_NV(false, true); else WMZ_SMP_NV(false, false);
#undef WMZ_SMP_NV
#undef WMZ_SMP
  } else if (!temp && !topp && uniforms == nullptr && kept_floor == nullptr) {
#define WMZ_SMP(NV) hipLaunchKernelGGL(sample_tokens_kernel<NV>, dim3(grid), dim3(256), 0, st, logits, ld, R, C, top_k, alphas, n_alpha, \
                                       mask_token, out_tokens, rows_per_block, block_stride, denoised, last_mask, seed, counter)
    if (C <= 256) WMZ_SMP(4); else if (C <= 512) WMZ_SMP(8); else if (C <= 1024) WMZ_SMP(16); else WMZ_SMP(32);
#undef WMZ_SMP
  } else {
    const SampleExtras x = {top_p, inv_temperature, uniforms, kept_floor};
#define WMZ_SMP(NV, TEMP, TOPP) hipLaunchKernelGGL((sample_tokens_kernel<NV, TEMP, TOPP, SampleExtras>), dim3(grid), dim3(256), 0, st, logits, ld, R, C, \
                                                   top_k, alphas, n_alpha, mask_token, out_tokens, rows_per_block, block_stride,          \
                                                   denoised, last_mask, seed, counter, x)
#define WMZ_SMP_NV(TEMP, TOPP) \
  do { if (C <= 256) WMZ_SMP(4, TEMP, TOPP); else if (C <= 512) WMZ_SMP(8, TEMP, TOPP); else if (C <= 1024) WMZ_SMP(16, TEMP, TOPP); else WMZ_SMP(32, TEMP, TOPP); } while (0)
    if (temp && topp) WMZ_SMP_NV(true, true); else if (temp) WMZ_SMP_NV(true, false); else if (topp) WMZ_SMP_NV(false, true); else WMZ_SMP_NV(false, false);
#undef WMZ_SMP_NV
#undef WMZ_SMP
  }
  WMZ_LAUNCH_CHECK(name);
  return WMZ_OK;
}

// The sparse form's launches (wmz_internal.h): the same two kernels, a SparseOut behind their arguments -- and, with `score`, its
// SparseScore behind that --; the dense step's own arguments are not read there.  The wide instantiations ask for their LDS
// themselves: the attribute is per instantiation.
int wmz_sparse_sample_launch(const char* name, const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                             const float* uniforms, float* kept_floor, unsigned long long seed, const WmzSparseOut& out,
                             hipStream_t st, const WmzSparseScore* score) {
  const bool temp = inv_temperature != 1.f, topp = top_p < 1.f;
  if (C > 2048) {
    const int P = (wmz_cdiv(C, SW_NT) + 7) / 8 * 8;
    const size_t smem = ((size_t)SW_NT * (P + 4) + SW_RED_WORDS) * 4;
    static std::atomic<uint64_t> attr_devs{0};
    if (wmz_first_use_on_device(attr_devs)) {
      const int most = (int)(((size_t)SW_NT * (SW_MAX_CLASSES / SW_NT + 4) + SW_RED_WORDS) * 4);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tokens_wide_kernel<SparseOut>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                most);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tokens_wide_kernel<SparseOut, SparseScore>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, most);
    }
    if (score != nullptr)
      hipLaunchKernelGGL((sample_tokens_wide_kernel<SparseOut, SparseScore>), dim3(R < 4096 ? R : 4096), dim3(SW_NT), smem, st, logits, ld, R,
                         C, P, top_k, top_p, inv_temperature, (const float*)nullptr, 0, (int64_t)0, (int64_t*)nullptr, 0L, 0L,
                         (int64_t*)nullptr, (unsigned char*)nullptr, uniforms, kept_floor, seed, (const long long*)nullptr, out, *score);
    else
      hipLaunchKernelGGL(sample_tokens_wide_kernel<SparseOut>, dim3(R < 4096 ? R : 4096), dim3(SW_NT), smem, st, logits, ld, R, C, P, top_k,
                       top_p, inv_temperature, (const float*)nullptr, 0, (int64_t)0, (int64_t*)nullptr, 0L, 0L, (int64_t*)nullptr,
                       (unsigned char*)nullptr, uniforms, kept_floor, seed, (const long long*)nullptr, out);
    WMZ_LAUNCH_CHECK(name);
    return WMZ_OK;
  }
  const int grid = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
  const SampleExtras x = {top_p, inv_temperature, uniforms, kept_floor};
#define WMZ_SMP(NV, TEMP, TOPP) hipLaunchKernelGGL((sample_tokens_kernel<NV, TEMP, TOPP, SampleExtras, SparseOut>), dim3(grid), dim3(256), 0, st, logits, ld, \
                                                   R, C, top_k, (const float*)nullptr, 0, (int64_t)0, (int64_t*)nullptr, 0L, 0L,                    \
                                                   (int64_t*)nullptr, (unsigned char*)nullptr, seed, (const long long*)nullptr, x, out)
#define WMZ_SMP_NV(TEMP, TOPP) \
  do { if (C <= 256) WMZ_SMP(4, TEMP, TOPP); else if (C <= 512) WMZ_SMP(8, TEMP, TOPP); else if (C <= 1024) WMZ_SMP(16, TEMP, TOPP); else WMZ_SMP(32, TEMP, TOPP); } while (0)
#define WMZ_SMP_S(NV, TEMP, TOPP) hipLaunchKernelGGL((sample_tokens_kernel<NV, TEMP, TOPP, SampleExtras, SparseOut, SparseScore>), dim3(grid), dim3(256), 0, st, \
                                                     logits, ld, R, C, top_k, (const float*)nullptr, 0, (int64_t)0, (int64_t*)nullptr, 0L, 0L,          \
                                                     (int64_t*)nullptr, (unsigned char*)nullptr, seed, (const long long*)nullptr, x, out, *score)
#define WMZ_SMP_S_NV(TEMP, TOPP) \
  do { if (C <= 256) WMZ_SMP_S(4, TEMP, TOPP); else if (C <= 512) WMZ_SMP_S(8, TEMP, TOPP); else if (C <= 1024) WMZ_SMP_S(16, TEMP, TOPP); else WMZ_SMP_S(32, TEMP, TOPP); } while (0)
  if (score != nullptr) {
    if (temp && topp) WMZ_SMP_S_NV(true, true); else if (temp) WMZ_SMP_S_NV(true, false); else if (topp) WMZ_SMP_S_NV(false, true); else WMZ_SMP_S_NV(false, false);
  } else if (temp && topp) WMZ_SMP_NV(true, true); else if (temp) WMZ_SMP_NV(true, false); else if (topp) WMZ_SMP_NV(false, true); else WMZ_SMP_NV(false, false);
#undef WMZ_SMP_S_NV
#undef WMZ_SMP_S
#undef WMZ_SMP_NV
#undef WMZ_SMP
  WMZ_LAUNCH_CHECK(name);
  return WMZ_OK;
}

extern "C" int wmz_sample_tokens_dev(const float* logits, long ld, int R, int C, int top_k, const float* alphas, int n_alpha,
                                     int64_t mask_token, int64_t* out_tokens, long rows_per_block, long block_stride,
                                     int64_t* denoised, unsigned char* last_mask, unsigned long long seed,
                                     const long long* counter, void* stream) {
  WMZ_REQUIRE(logits && alphas && out_tokens && denoised && counter && R > 0 && C > 0 && n_alpha > 0 && rows_per_block > 0,
              "wmz_sample_tokens_dev: bad arguments");
  WMZ_REQUIRE(ld >= C && ld % 4 == 0 && (((uintptr_t)logits) & 15) == 0, "wmz_sample_tokens_dev: logits rows must be 16-byte aligned");
  if (C > 2048) {
    wmz_set_error("wmz_sample_tokens_dev: built for <= 2048 classes (got %d)", C);
    return WMZ_ERR_UNSUPPORTED;
  }
  return sample_tokens_launch("wmz_sample_tokens_dev", logits, ld, R, C, top_k, 1.f, 1.f, alphas, n_alpha, mask_token, out_tokens,
                              rows_per_block, block_stride, denoised, last_mask, nullptr, nullptr, seed, counter, stream);
}

extern "C" int wmz_sample_tokens_max_classes(void) { return SW_MAX_CLASSES; }

extern "C" int wmz_sample_tokens_filtered_dev(const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                                              const float* alphas, int n_alpha, int64_t mask_token, int64_t* out_tokens,
                                              long rows_per_block, long block_stride, int64_t* denoised, unsigned char* last_mask,
                                              const float* uniforms, float* kept_floor, unsigned long long seed,
                                              const long long* counter, void* stream) {
  WMZ_REQUIRE(logits && alphas && out_tokens && denoised && counter && R > 0 && C > 0 && n_alpha > 0 && rows_per_block > 0,
              "wmz_sample_tokens_filtered_dev: bad arguments");
  WMZ_REQUIRE(ld >= C && ld % 4 == 0 && (((uintptr_t)logits) & 15) == 0,
              "wmz_sample_tokens_filtered_dev: logits rows must be 16-byte aligned");
  WMZ_REQUIRE(inv_temperature > 0.f && inv_temperature < INFINITY,
              "wmz_sample_tokens_filtered_dev: inv_temperature must be positive and finite (got %g)", (double)inv_temperature);
  WMZ_REQUIRE(top_p > 0.f, "wmz_sample_tokens_filtered_dev: top_p must be positive (got %g)", (double)top_p);
  if (C > SW_MAX_CLASSES) {
    wmz_set_error("wmz_sample_tokens_filtered_dev: built for <= %d classes (got %d)", SW_MAX_CLASSES, C);
    return WMZ_ERR_UNSUPPORTED;
  }
  return sample_tokens_launch("wmz_sample_tokens_filtered_dev", logits, ld, R, C, top_k, top_p, inv_temperature, alphas, n_alpha,
                              mask_token, out_tokens, rows_per_block, block_stride, denoised, last_mask, uniforms, kept_floor, seed,
                              counter, stream);
}

extern "C" int wmz_sample_tokens_scored_dev(const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                                            const float* alphas, int n_alpha, int64_t* out_tokens, long rows_per_block,
                                            long block_stride, int64_t* denoised, float* scores, float noise, const float* uniforms,
                                            float* kept_floor, unsigned long long seed, const long long* counter, void* stream) {
  WMZ_REQUIRE(logits && alphas && out_tokens && denoised && scores && counter && R > 0 && C > 0 && n_alpha > 0 && rows_per_block > 0,
              "wmz_sample_tokens_scored_dev: bad arguments");
  WMZ_REQUIRE(ld >= C && ld % 4 == 0 && (((uintptr_t)logits) & 15) == 0,
              "wmz_sample_tokens_scored_dev: logits rows must be 16-byte aligned");
  WMZ_REQUIRE(inv_temperature > 0.f && inv_temperature < INFINITY,
              "wmz_sample_tokens_scored_dev: inv_temperature must be positive and finite (got %g)", (double)inv_temperature);
  WMZ_REQUIRE(top_p > 0.f, "wmz_sample_tokens_scored_dev: top_p must be positive (got %g)", (double)top_p);
  WMZ_REQUIRE(noise >= 0.f && noise < INFINITY, "wmz_sample_tokens_scored_dev: noise must be non-negative and finite (got %g)",
              (double)noise);
  if (C > SW_MAX_CLASSES) {
    wmz_set_error("wmz_sample_tokens_scored_dev: built for <= %d classes (got %d)", SW_MAX_CLASSES, C);
    return WMZ_ERR_UNSUPPORTED;
  }
  const ScoreOut score = {scores, noise};
  return sample_tokens_launch("wmz_sample_tokens_scored_dev", logits, ld, R, C, top_k, top_p, inv_temperature, alphas, n_alpha, 0,
                              out_tokens, rows_per_block, block_stride, denoised, nullptr, uniforms, kept_floor, seed, counter, stream,
                              &score);
}

extern "C" int wmz_remask_lowest_max_rows(void) { return RM_MAX_ROWS; }

extern "C" int wmz_remask_lowest_dev(const float* scores, int R, long rows_per_block, const float* alphas, int n_alpha,
                                     int64_t mask_token, int64_t* out_tokens, long block_stride, unsigned char* last_mask,
                                     const long long* counter, void* stream) {
  WMZ_REQUIRE(scores && alphas && out_tokens && counter && R > 0 && n_alpha > 0 && rows_per_block > 0 && R % rows_per_block == 0,
              "wmz_remask_lowest_dev: bad arguments");
  if (rows_per_block > RM_MAX_ROWS) {
    wmz_set_error("wmz_remask_lowest_dev: built for <= %d rows per clip (got %ld)", RM_MAX_ROWS, rows_per_block);
    return WMZ_ERR_UNSUPPORTED;
  }
  const int clips = (int)(R / rows_per_block);
  if (rows_per_block <= RM_ONE_WAVE_ROWS)
    hipLaunchKernelGGL(remask_lowest_kernel<1>, dim3(clips), dim3(64), 0, (hipStream_t)stream, scores, rows_per_block, alphas, n_alpha,
                       mask_token, out_tokens, block_stride, last_mask, counter);
  else
    hipLaunchKernelGGL(remask_lowest_kernel<4>, dim3(clips), dim3(256), 0, (hipStream_t)stream, scores, rows_per_block, alphas, n_alpha,
                       mask_token, out_tokens, block_stride, last_mask, counter);
  WMZ_LAUNCH_CHECK("wmz_remask_lowest_dev");
  return WMZ_OK;
}

extern "C" int wmz_ce_fwd(const float* logits, long ld, const int64_t* target, float* loss, float* lse, long R, int C,
                          void* stream) {
  WMZ_REQUIRE(logits && target && loss && lse && R > 0 && C > 0, "wmz_ce_fwd: bad arguments");
  const int grid = (int)((R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, target, loss, lse, R, C);
  WMZ_LAUNCH_CHECK("wmz_ce_fwd");
  return WMZ_OK;
}

extern "C" int wmz_ce_fwd_bwd(const float* logits, long ld, const int64_t* target, float* loss, float* lse, const float* grad_rows,
                              void* dlogits, long R, int C, int dtype, void* stream) {
  WMZ_REQUIRE(logits && target && loss && lse && grad_rows && dlogits && R > 0 && C > 0, "wmz_ce_fwd_bwd: bad arguments");
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_ce_fwd_bwd: bad dtype %d", dtype);
  // the one-pass kernel reads 16 bytes of a row at a time and stores four gradients at a time (16 bytes fp32, 8 bytes bf16): rows
  // that do not fit a wave's registers, a row stride or a base address that leaves a row off those boundaries: the two passes
  const uintptr_t dmask = dtype == WMZ_F32 ? 15 : 7;
  if (C > 8192 || (ld & 3) != 0 || ((uintptr_t)logits & 15) != 0 || ((uintptr_t)dlogits & dmask) != 0) {
    const int rc = wmz_ce_fwd(logits, ld, target, loss, lse, R, C, stream);
    return rc != WMZ_OK ? rc : wmz_ce_bwd(logits, ld, target, lse, grad_rows, dlogits, R, C, dtype, stream);
  }
  const int grid = (int)((R + 3) / 4 < 4096 ? (R + 3) / 4 : 4096);
  hipStream_t st = (hipStream_t)stream;
#define WMZ_CEF(NCH) hipLaunchKernelGGL((ce_fused_kernel<T, NCH>), dim3(grid), dim3(256), 0, st, logits, ld, target, loss, lse, \
                                        grad_rows, (T*)dlogits, R, C)
  wmz_by_dtype2(dtype, [&](auto e) { typedef decltype(e) T;
    if (C <= 1024) WMZ_CEF(4); else if (C <= 2048) WMZ_CEF(8); else if (C <= 4096) WMZ_CEF(16); else WMZ_CEF(32);
  });
#undef WMZ_CEF
  WMZ_LAUNCH_CHECK("wmz_ce_fwd_bwd");
  return WMZ_OK;
}

extern "C" int wmz_ce_bwd(const float* logits, long ld, const int64_t* target, const float* lse, const float* grad_rows,
                          void* dlogits, long R, int C, int dtype, void* stream) {
  WMZ_REQUIRE(logits && target && lse && grad_rows && dlogits && R > 0 && C > 0, "wmz_ce_bwd: bad arguments");
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_ce_bwd: bad dtype %d", dtype);
  const long total = R * C;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipStream_t st = (hipStream_t)stream;
  wmz_by_dtype2(dtype, [&](auto e) { typedef decltype(e) T;
    hipLaunchKernelGGL(ce_bwd_kernel<T>, dim3(grid), dim3(256), 0, st, logits, ld, target, lse, grad_rows, (T*)dlogits, R, C);
  });
  WMZ_LAUNCH_CHECK("wmz_ce_bwd");
  return WMZ_OK;
}
