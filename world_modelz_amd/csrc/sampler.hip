// The inference sampler's draw step (main.py:76-104; config 5: sparse_diffusion.py:190-198): filter a row of logits, draw a class,
// put it where the sampler wants it.  Two row bodies do the first two -- sample_tokens_kernel (a wave per row, the row in registers,
// up to 2 048 classes) and sample_tokens_wide_kernel (a workgroup per row, the row in LDS, up to SW_MAX_CLASSES) -- and a DESTINATION
// type, the kernels' last argument, does the third.  include/wmz.h states the law of every entry point.
//   StepDest          wmz_sample_tokens_dev, _filtered_dev   the draw, or the mask token by a coin against alpha (random re-mask)
//   ScoredDest        wmz_sample_tokens_scored_dev           the draw and its score; wmz_remask_lowest_dev re-masks by the scores
//   SparseDest        wmz_categorical_scatter(_filtered)     the draw scattered into the clip at the row's position
//   SparseScoredDest  wmz_categorical_scatter_scored         the same with the score beside the token
// A destination states
//   SCORED       whether the score's sum of exp(l - max) over ALL classes is needed;
//   FIRST_KEPT   the register kernel's draw rule: the first kept class past u * total, else the last kept one (the rule of the wide
//                kernel whatever the destination) -- or, where false, the count of classes whose cumulative weight is <= u * total;
//   once()       what a launch reads once, ahead of its rows: the step's counter and alpha;
//   uniforms()   where a row's uniforms come from: `given` (the probe of the law tests) or Philox;
//   write()      what ONE lane does with a row's draw.
// A new sampler form is a destination type: neither row body changes for it.
// Behind the draw: remask_lowest_kernel (the confidence rule's selection) and categorical_scatter_kernel (config 5's neutral draw:
// three passes over a global row of any width and alignment).
#include "wmz_common.h"
#include "wmz_philox.h"
#include "wmz_select.h"
#include <type_traits>

namespace {

// what every form reads.  top_p, inv_temperature, uniforms and kept_floor are the filtered entry points': the register kernel
// compiles each in only where it acts (TEMP, TOPP, PROBES)
struct SampleIn {
  const float* logits;
  long ld;
  int R, C, top_k;
  float top_p, inv_temperature;
  const float* uniforms;      // optional probe: the row's uniforms instead of Philox
  float* kept_floor;          // optional probe [R]: the smallest kept scaled logit
  unsigned long long seed;
};

// what the score of a drawn row needs besides the draw: the drawn class's scaled logit, the row maximum, the sum over all classes
struct Drawn {
  int cls;
  float u1, l_d, m, sum_all;
};

// score of a drawn row: lp = (l_d - max) - log(sum over all classes); NaN -> -inf
__device__ __forceinline__ float sample_score(float l_d, float m, float sum_all, float noise, float alpha, float u1) {
  float s = sub_rn(l_d, m) - logf(sum_all);
  if (noise > 0.f) s += noise * (1.f - alpha) * -logf(-logf(u1));
  return s == s ? s : -INFINITY;
}

// The dense step (one launch of the sampler loop between two forward passes): alpha = alphas[*counter % n_alpha] and the Philox stream
// id = *counter live in device memory -- the launch sits in a hipGraph --; row `row` of block blk = row / rows_per_block goes to
// out_tokens[blk * block_stride + row - blk * rows_per_block] and to denoised[row].
struct DenseDest {
  static constexpr bool FIRST_KEPT = false;
  const float* alphas;
  int n_alpha;
  int64_t* out_tokens;
  long rows_per_block, block_stride;
  int64_t* denoised;
  const long long* counter;   // (last: between alphas and out_tokens it cost the wide kernel 1.7 % -- profiles/sampler_forms/README.md)
  struct Once { long ctr; float alpha; };
  __device__ __forceinline__ Once once() const {
    const long ctr = *counter;
    return Once{ctr, alphas[(int)(ctr % n_alpha)]};
  }
  __device__ __forceinline__ void uniforms(const Once& o, const float* given, unsigned long long seed, long row, float (&u)[4]) const {
    if (given != nullptr) {
      u[0] = given[2 * row];
      u[1] = given[2 * row + 1];
    } else {
      philox4_unit((unsigned long long)row, (unsigned long long)o.ctr, seed, u);
    }
  }
  __device__ __forceinline__ void put(long row, int draw, int64_t token) const {
    denoised[row] = draw;
    const long blk = row / rows_per_block;
    out_tokens[blk * block_stride + (row - blk * rows_per_block)] = token;
  }
};

// re-mask: with the second uniform u1 > alpha (and, with `last_mask`, only where the previous iteration masked: consistent masking)
// the position gets the mask token instead of the draw
struct StepDest : DenseDest {
  static constexpr bool SCORED = false;
  int64_t mask_token;
  unsigned char* last_mask;
  __device__ __forceinline__ void write(const Once& o, long row, const Drawn& d) const {
    bool mask = d.u1 > o.alpha;
    if (last_mask != nullptr) { mask = mask && last_mask[row] != 0; last_mask[row] = mask ? 1 : 0; }
    put(row, d.cls, mask ? mask_token : (int64_t)d.cls);
  }
};

// score = (l_d - max) - log(sum) (+ the Gumbel term from u1 with noise > 0) to `scores`; the draw goes out as it is: no re-mask
struct ScoredDest : DenseDest {
  static constexpr bool SCORED = true;
  float* scores;
  float noise;
  __device__ __forceinline__ void write(const Once& o, long row, const Drawn& d) const {
    scores[row] = sample_score(d.l_d, d.m, d.sum_all, noise, o.alpha, d.u1);
    put(row, d.cls, (int64_t)d.cls);
  }
};

// Config 5's sampler: samples[row] always; z[clip][indices[row]], clip = row / rows_per_clip, unless that position's `known` byte
// is set.  One uniform a row: given[row], or the first word of philox4(row, stream id, seed) -- `stream` with the counter's bits.
struct SparseDest {
  static constexpr bool SCORED = false, FIRST_KEPT = true;
  const int64_t* indices;
  int64_t* z;
  long clip_stride, rows_per_clip;
  int64_t* samples;
  const unsigned char* known;
  long known_stride;
  unsigned long long stream;
  const unsigned long long* counter;
  struct Once {};                                 // (nothing ahead of the rows: the stream id is formed where a row draws from it)
  __device__ __forceinline__ Once once() const { return Once{}; }
  __device__ __forceinline__ void uniforms(const Once&, const float* given, unsigned long long seed, long row, float (&u)[4]) const {
    if (given != nullptr) u[0] = given[row];
    else philox4_unit((unsigned long long)row, philox_stream(stream, counter), seed, u);
    u[1] = 0.f;
  }
  // true where the token went into z: at z's (clip, pos)
  __device__ __forceinline__ bool place(long row, int draw, long& clip, int64_t& pos) const {
    if (samples != nullptr) samples[row] = draw;
    if (z == nullptr) return false;
    clip = row / rows_per_clip;
    pos = indices[row];
    if (known != nullptr && known[clip * known_stride + pos] != 0) return false;
    z[clip * clip_stride + pos] = draw;
    return true;
  }
  __device__ __forceinline__ void write(const Once&, long row, const Drawn& d) const {
    long clip;
    int64_t pos;
    place(row, d.cls, clip, pos);
  }
};

// scores [clips, stride] fp32, addressed like z: the score of a draw -- sample_score without noise -- is written exactly where its
// token is written, and nowhere else
struct SparseScoredDest : SparseDest {
  static constexpr bool SCORED = true;
  float* scores;
  long stride;
  __device__ __forceinline__ void write(const Once&, long row, const Drawn& d) const {
    long clip;
    int64_t pos;
    if (place(row, d.cls, clip, pos)) scores[clip * stride + pos] = sample_score(d.l_d, d.m, d.sum_all, 0.f, 0.f, 0.f);
  }
};

// One wave per row of logits, everything in registers.  Lane l holds the NV consecutive classes l * NV .. (classes past C are -inf).
//   * TEMP: l = logits * inv_temperature on the way into the registers;
//   * SCORED: the sum of exp(l - max) over ALL classes, taken before top-k overwrites the values where a filter acts (else it is the
//     draw's own total);
//   * top-k: the k-th largest logit by a 32-step bitwise search on order-preserving integer keys (count of keys >= candidate
//     by wave ballots); logits below it are dropped, ties with it kept (the reference's `logits < v[:, -1]`);
//   * softmax weights w = exp(l - max), total by wave reduction;
//   * TOPP: the nucleus threshold by the same bitwise search on the bits of the weights (non-negative floats order like their
//     bits), accumulating the mass of the weights >= candidate instead of a count; weights below it are dropped;
//   * the draw by the destination's rule (inverse CDF, the definition of sample.categorical_from_uniform, clamped to C - 1);
//   * PROBES: the uniforms from `uniforms` and the smallest kept l to `kept_floor`, each where the pointer is given.  The probe keeps
//     the row's values alive to the end, so the form that production runs at its defaults -- the StepDest without filters -- is
//     compiled without it: an occupancy step at every NV.
template <int NV, bool TEMP, bool TOPP, bool PROBES, typename Dest>
__global__ __launch_bounds__(256) void sample_tokens_kernel(SampleIn in, Dest dest) {
  static_assert(PROBES || (!TEMP && !TOPP && std::is_same<Dest, StepDest>::value), "the probe-free form is the plain step's alone");
  const float* __restrict__ logits = in.logits;
  const long ld = in.ld;
  const int R = in.R, C = in.C, top_k = in.top_k;
  const int lane = threadIdx.x & 63;
  const typename Dest::Once once = dest.once();
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
      for (int e = 0; e < NV; ++e) v[e] *= in.inv_temperature;           // (-inf stays -inf: inv_temperature > 0)
    }
    const bool all_kept = !TOPP && !(top_k > 0 && top_k < C);    // no filter acts: the draw's total is the sum over all classes
    float sum_all = 0.f;
    if constexpr (Dest::SCORED) {
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
      const float need = in.top_p * __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_sum(part))));
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
    const float* given = nullptr;
    if constexpr (PROBES) given = in.uniforms;
    dest.uniforms(once, given, in.seed, row, u);
    const float xq = u[0] * total;
    int draw;
    if constexpr (Dest::FIRST_KEPT) {
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
      if (in.kept_floor != nullptr) {
        float f = INFINITY;
#pragma unroll
        for (int e = 0; e < NV; ++e) f = v[e] > -INFINITY ? fminf(f, v[e]) : f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) f = fminf(f, __shfl_xor(f, o));
        if (lane == 0) in.kept_floor[row] = f;
      }
    }
    if (lane == 0) {
      float l_d = 0.f;                                         // the drawn class's scaled logit, read back from the row
      if constexpr (Dest::SCORED) l_d = TEMP ? mul_rn(logits[row * ld + draw], in.inv_temperature) : logits[row * ld + draw];
      dest.write(once, row, Drawn{draw, u[1], l_d, m, all_kept ? total : sum_all});
    }
  }
}

// The same step for rows that do not fit a wave's registers (2048 < C <= SW_MAX_CLASSES): one workgroup of SW_NT threads per row.
// The row is read from global memory ONCE -- 16-byte loads, scaled, turned into the order-preserving keys above -- into LDS, and
// every later pass works from there.  Thread t owns the P consecutive classes t * P .. (P a multiple of 8, classes past C are
// -inf), kept at a pitch of P + 4 words: P / 4 + 1 is odd, so the 16-byte slots that consecutive lanes read in one ds_read_b128
// fall on different banks.  The passes, each a walk of the thread's own slots:
//   * the maximum (of the keys: same order);
//   * SCORED, where a filter acts: the sum of exp(l - max) over all classes (else that sum is the draw's total);
//   * top-k: the bitwise search, counts by wave ballots, the four waves' counts through LDS (one barrier per step);
//   * keys -> weights w = exp(l - max) in place, 0 for what top-k dropped;
//   * nucleus: the bitwise search on the weights' bits accumulating mass; weights below the threshold become 0;
//   * the prefix in class order -- sequential in the thread, shuffle scan over the lanes, the waves' totals in wave order --
//     and the draw: the FIRST KEPT class whose cumulative weight exceeds u0 * total (the last kept one if rounding leaves none):
//     a class of weight 0 is never drawn, whatever the rounding of the partial sums.
// The kept_floor probe alone walks the global row a second time (the keys are gone by then): it is NULL in production.
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

template <typename Dest>
__global__ __launch_bounds__(SW_NT) void sample_tokens_wide_kernel(SampleIn in, int P, Dest dest) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  extern __shared__ __attribute__((aligned(16))) unsigned sw_lds[];
  const float* __restrict__ logits = in.logits;
  const int R = in.R, C = in.C, top_k = in.top_k;
  const float top_p = in.top_p, inv_temperature = in.inv_temperature;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pitch = P + 4, nq = P >> 2;
  u32x4* mine = reinterpret_cast<u32x4*>(sw_lds + tid * pitch);
  SwExchange exchange{sw_lds + SW_NT * pitch, 0};
  unsigned ra[4], rb[4];
  const typename Dest::Once once = dest.once();
  for (long row = blockIdx.x; row < R; row += gridDim.x) {
    const float* x = logits + row * in.ld;
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
    if constexpr (Dest::SCORED) {
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
    dest.uniforms(once, in.uniforms, in.seed, row, u);
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
    if (in.kept_floor != nullptr) {                            // probe: the keys are gone, so the same law over the global row again
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
      if (tid == 0) in.kept_floor[row] = sw_unkey(min(min(ra[0], ra[1]), min(ra[2], ra[3])));
    }
    if (tid == 0) {
      float l_d = 0.f;
      if constexpr (Dest::SCORED) l_d = mul_rn(x[draw], inv_temperature);
      dest.write(once, row, Drawn{draw, u[1], l_d, m, all_kept ? total : sum_all});
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

// Config 5's neutral draw (sparse_diffusion.py:190-198): p = softmax(logits), one multinomial draw per row, scattered back into the
// clip at the row's position.  One wave per row of C fp32 logits (C = 8192 at config 5: too wide for registers, so three passes over
// the row, which sits in L2): the maximum, the sum of exp(l - max), then the inverse CDF in class order -- the first class whose
// cumulative weight exceeds u * total (lane l owns the contiguous classes [l C / 64, (l + 1) C / 64): lane sums -> a wave prefix ->
// the owning lane walks its classes).
__global__ __launch_bounds__(256) void categorical_scatter_kernel(const float* __restrict__ logits, long ld, long R, int C,
                                                                  SparseDest out, unsigned long long seed) {
  const unsigned long long stream = philox_stream(out.stream, out.counter);
  const int lane = threadIdx.x & 63;
  const int per = (C + 63) / 64, c0 = lane * per, c1 = min(c0 + per, C);
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (long)gridDim.x * 4) {
    const float* x = logits + row * ld;
    float m = -INFINITY;
    for (int c = c0; c < c1; ++c) m = fmaxf(m, x[c]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += __expf(x[c] - m);
    float incl = s;                                             // inclusive prefix of the lane sums
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    const float total = __shfl(incl, 63);
    unsigned cc[4];
    philox4((unsigned long long)row, stream, seed, cc);
    const float want = philox_unit(cc[0]) * total;
    // the owning lane: the first whose inclusive prefix exceeds `want` (the last lane if rounding leaves none)
    const unsigned long long owners = __ballot(incl > want);
    const int owner = owners ? (int)__builtin_ctzll(owners) : 63;
    int pick = C - 1;
    if (lane == owner) {
      float acc = incl - s;
      pick = c1 - 1 < 0 ? 0 : c1 - 1;
      for (int c = c0; c < c1; ++c) {
        acc += __expf(x[c] - m);
        if (acc > want) { pick = c; break; }
      }
    }
    pick = __shfl(pick, owner);
    if (lane == 0) out.write(SparseDest::Once{}, row, Drawn{pick, 0.f, 0.f, 0.f, 0.f});
  }
}

// ---------------------------------------------------------------- launches (the checks are the entry points')

template <bool TEMP, bool TOPP, bool PROBES, typename Dest>
void sample_launch_nv(const SampleIn& in, const Dest& dest, hipStream_t st) {
  const int grid = (in.R + 3) / 4 < 2048 ? (in.R + 3) / 4 : 2048;
#define WMZ_SMP(NV) hipLaunchKernelGGL((sample_tokens_kernel<NV, TEMP, TOPP, PROBES, Dest>), dim3(grid), dim3(256), 0, st, in, dest)
  if (in.C <= 256) WMZ_SMP(4); else if (in.C <= 512) WMZ_SMP(8); else if (in.C <= 1024) WMZ_SMP(16); else WMZ_SMP(32);
#undef WMZ_SMP
}

// the row body by width, the register kernel's filters by value; a StepDest without filter or probe runs the probe-free form
template <typename Dest>
int sample_launch(const char* name, const SampleIn& in, const Dest& dest, hipStream_t st) {
  const bool temp = in.inv_temperature != 1.f, topp = in.top_p < 1.f;
  if (in.C > 2048) {
    const int P = (wmz_cdiv(in.C, SW_NT) + 7) / 8 * 8;
    const size_t smem = ((size_t)SW_NT * (P + 4) + SW_RED_WORDS) * 4;
    static std::atomic<uint64_t> attr_devs{0};          // (> 64 KB of dynamic LDS has to be asked for once per device and instantiation)
    if (wmz_first_use_on_device(attr_devs)) {
      const int most = (int)(((size_t)SW_NT * (SW_MAX_CLASSES / SW_NT + 4) + SW_RED_WORDS) * 4);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tokens_wide_kernel<Dest>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
    }
    hipLaunchKernelGGL(sample_tokens_wide_kernel<Dest>, dim3(in.R < 4096 ? in.R : 4096), dim3(SW_NT), smem, st, in, P, dest);
  } else if (std::is_same<Dest, StepDest>::value && !temp && !topp && in.uniforms == nullptr && in.kept_floor == nullptr) {
    if constexpr (std::is_same<Dest, StepDest>::value) sample_launch_nv<false, false, false>(in, dest, st);
  } else if (temp && topp) sample_launch_nv<true, true, true>(in, dest, st);
  else if (temp) sample_launch_nv<true, false, true>(in, dest, st);
  else if (topp) sample_launch_nv<false, true, true>(in, dest, st);
  else sample_launch_nv<false, false, true>(in, dest, st);
  WMZ_LAUNCH_CHECK(name);
  return WMZ_OK;
}

// what the three dense entry points require (`pointers`: the entry point's own; a form without a noise passes 0)
int sample_check(const char* name, bool pointers, const float* logits, long ld, int R, int C, float top_p, float inv_temperature,
                 int n_alpha, long rows_per_block, float noise, int max_classes) {
  WMZ_REQUIRE(pointers && R > 0 && C > 0 && n_alpha > 0 && rows_per_block > 0, "%s: bad arguments", name);
  WMZ_REQUIRE(ld >= C && ld % 4 == 0 && (((uintptr_t)logits) & 15) == 0, "%s: logits rows must be 16-byte aligned", name);
  WMZ_REQUIRE(inv_temperature > 0.f && inv_temperature < INFINITY, "%s: inv_temperature must be positive and finite (got %g)", name,
              (double)inv_temperature);
  WMZ_REQUIRE(top_p > 0.f, "%s: top_p must be positive (got %g)", name, (double)top_p);
  WMZ_REQUIRE(noise >= 0.f && noise < INFINITY, "%s: noise must be non-negative and finite (got %g)", name, (double)noise);
  if (C > max_classes) {
    wmz_set_error("%s: built for <= %d classes (got %d)", name, max_classes, C);
    return WMZ_ERR_UNSUPPORTED;
  }
  return WMZ_OK;
}

// The scatter's three entry points: checks, the destination, and the kernel.  Neutral filters and no probe: categorical_scatter_kernel,
// at any C and any alignment.  Else the two row bodies above with a sparse destination.
int categorical_scatter_launch(const float* logits, long ld, long R, int C, int top_k, float top_p, float inv_temperature,
                               const int64_t* indices, int64_t* z, long clip_stride, long rows_per_clip, int64_t* samples,
                               const unsigned char* known, long known_stride, const float* uniforms, float* kept_floor,
                               unsigned long long seed, unsigned long long stream_id, const unsigned long long* counter, void* stream,
                               float* scores, long scores_stride) {
  WMZ_REQUIRE(logits && R > 0 && C > 0 && ld >= C, "wmz_categorical_scatter: bad arguments");
  WMZ_REQUIRE(z == nullptr || (indices != nullptr && rows_per_clip > 0), "wmz_categorical_scatter: the scatter needs indices and rows_per_clip");
  WMZ_REQUIRE(z != nullptr || samples != nullptr, "wmz_categorical_scatter: nothing to write");
  WMZ_REQUIRE(inv_temperature > 0.f && inv_temperature < INFINITY,
              "wmz_categorical_scatter_filtered: inv_temperature must be positive and finite (got %g)", (double)inv_temperature);
  WMZ_REQUIRE(top_p > 0.f, "wmz_categorical_scatter_filtered: top_p must be positive (got %g)", (double)top_p);
  const SparseDest out = {indices, z, clip_stride, rows_per_clip, samples, z != nullptr ? known : nullptr, known_stride,
                          philox_stream_base(stream_id, counter != nullptr) | (PHILOX_KEY_DOMAIN | PHILOX_WIN_DOMAIN), counter};
  const bool neutral = !(top_k > 0 && top_k < C) && !(top_p < 1.f) && inv_temperature == 1.f && uniforms == nullptr && kept_floor == nullptr &&
                       scores == nullptr;
  if (neutral) {
    const int grid = (int)((R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048);
    hipLaunchKernelGGL(categorical_scatter_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, R, C, out, seed);
    WMZ_LAUNCH_CHECK("wmz_categorical_scatter");
    return WMZ_OK;
  }
  if (C > SW_MAX_CLASSES) {
    wmz_set_error("wmz_categorical_scatter_filtered: filters are built for <= %d classes (got %d)", SW_MAX_CLASSES, C);
    return WMZ_ERR_UNSUPPORTED;
  }
  WMZ_REQUIRE(ld % 4 == 0 && (((uintptr_t)logits) & 15) == 0, "wmz_categorical_scatter_filtered: logits rows must be 16-byte aligned");
  WMZ_REQUIRE(R <= 0x7fffffffL, "wmz_categorical_scatter_filtered: more than 2^31 - 1 rows");
  const SampleIn in = {logits, ld, (int)R, C, top_k, top_p, inv_temperature, uniforms, kept_floor, seed};
  if (scores != nullptr)
    return sample_launch("wmz_categorical_scatter_filtered", in, SparseScoredDest{out, scores, scores_stride}, (hipStream_t)stream);
  return sample_launch("wmz_categorical_scatter_filtered", in, out, (hipStream_t)stream);
}

}  // namespace

extern "C" int wmz_sample_tokens_dev(const float* logits, long ld, int R, int C, int top_k, const float* alphas, int n_alpha,
                                     int64_t mask_token, int64_t* out_tokens, long rows_per_block, long block_stride,
                                     int64_t* denoised, unsigned char* last_mask, unsigned long long seed,
                                     const long long* counter, void* stream) {
  const char* name = "wmz_sample_tokens_dev";
  const int rc = sample_check(name, logits && alphas && out_tokens && denoised && counter, logits, ld, R, C, 1.f, 1.f, n_alpha,
                              rows_per_block, 0.f, 2048);
  if (rc != WMZ_OK) return rc;
  const SampleIn in = {logits, ld, R, C, top_k, 1.f, 1.f, nullptr, nullptr, seed};
  const StepDest dest = {{alphas, n_alpha, out_tokens, rows_per_block, block_stride, denoised, counter}, mask_token, last_mask};
  return sample_launch(name, in, dest, (hipStream_t)stream);
}

extern "C" int wmz_sample_tokens_max_classes(void) { return SW_MAX_CLASSES; }

extern "C" int wmz_sample_tokens_filtered_dev(const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                                              const float* alphas, int n_alpha, int64_t mask_token, int64_t* out_tokens,
                                              long rows_per_block, long block_stride, int64_t* denoised, unsigned char* last_mask,
                                              const float* uniforms, float* kept_floor, unsigned long long seed,
                                              const long long* counter, void* stream) {
  const char* name = "wmz_sample_tokens_filtered_dev";
  const int rc = sample_check(name, logits && alphas && out_tokens && denoised && counter, logits, ld, R, C, top_p, inv_temperature,
                              n_alpha, rows_per_block, 0.f, SW_MAX_CLASSES);
  if (rc != WMZ_OK) return rc;
  const SampleIn in = {logits, ld, R, C, top_k, top_p, inv_temperature, uniforms, kept_floor, seed};
  const StepDest dest = {{alphas, n_alpha, out_tokens, rows_per_block, block_stride, denoised, counter}, mask_token, last_mask};
  return sample_launch(name, in, dest, (hipStream_t)stream);
}

extern "C" int wmz_sample_tokens_scored_dev(const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                                            const float* alphas, int n_alpha, int64_t* out_tokens, long rows_per_block,
                                            long block_stride, int64_t* denoised, float* scores, float noise, const float* uniforms,
                                            float* kept_floor, unsigned long long seed, const long long* counter, void* stream) {
  const char* name = "wmz_sample_tokens_scored_dev";
  const int rc = sample_check(name, logits && alphas && out_tokens && denoised && scores && counter, logits, ld, R, C, top_p,
                              inv_temperature, n_alpha, rows_per_block, noise, SW_MAX_CLASSES);
  if (rc != WMZ_OK) return rc;
  const SampleIn in = {logits, ld, R, C, top_k, top_p, inv_temperature, uniforms, kept_floor, seed};
  const ScoredDest dest = {{alphas, n_alpha, out_tokens, rows_per_block, block_stride, denoised, counter}, scores, noise};
  return sample_launch(name, in, dest, (hipStream_t)stream);
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

// One multinomial draw per row of fp32 logits [R, C] (row stride ld) from softmax(logits) -- sparse_diffusion.py:190-194 -- and,
// with z != NULL, its scatter into the clips (:197): z[row / rows_per_clip][indices[row]] = the drawn class.  samples (optional):
// the draws [R].  Philox keyed as wmz_sparse_draw_context.
extern "C" int wmz_categorical_scatter(const float* logits, long ld, long R, int C, const int64_t* indices, int64_t* z,
                                       long clip_stride, long rows_per_clip, int64_t* samples, unsigned long long seed,
                                       unsigned long long stream_id, const unsigned long long* counter, void* stream) {
  return categorical_scatter_launch(logits, ld, R, C, -1, 1.f, 1.f, indices, z, clip_stride, rows_per_clip, samples, nullptr, 0, nullptr,
                                    nullptr, seed, stream_id, counter, stream, nullptr, 0);
}

// The same with a temperature, top-k, a nucleus and given positions (include/wmz.h states the law).
extern "C" int wmz_categorical_scatter_filtered(const float* logits, long ld, long R, int C, int top_k, float top_p, float inv_temperature,
                                                const int64_t* indices, int64_t* z, long clip_stride, long rows_per_clip,
                                                int64_t* samples, const unsigned char* known, long known_stride,
                                                const float* uniforms, float* kept_floor, unsigned long long seed,
                                                unsigned long long stream_id, const unsigned long long* counter, void* stream) {
  return categorical_scatter_launch(logits, ld, R, C, top_k, top_p, inv_temperature, indices, z, clip_stride, rows_per_clip, samples, known,
                                    known_stride, uniforms, kept_floor, seed, stream_id, counter, stream, nullptr, 0);
}

// The same draw with the score of every draw written beside its token (include/wmz.h states the law): `scores` counts as a probe,
// so the row-read-once kernels run whatever the filters are.  Without `scores` it is the entry point above.
extern "C" int wmz_categorical_scatter_scored(const float* logits, long ld, long R, int C, int top_k, float top_p, float inv_temperature,
                                              const int64_t* indices, int64_t* z, long clip_stride, long rows_per_clip,
                                              int64_t* samples, const unsigned char* known, long known_stride,
                                              const float* uniforms, float* kept_floor, unsigned long long seed,
                                              unsigned long long stream_id, const unsigned long long* counter, void* stream,
                                              float* scores, long scores_stride) {
  WMZ_REQUIRE(scores == nullptr || z != nullptr, "wmz_categorical_scatter_scored: a score is written where a token is: z expected");
  return categorical_scatter_launch(logits, ld, R, C, top_k, top_p, inv_temperature, indices, z, clip_stride, rows_per_clip, samples, known,
                                    known_stride, uniforms, kept_floor, seed, stream_id, counter, stream, scores, scores_stride);
}
