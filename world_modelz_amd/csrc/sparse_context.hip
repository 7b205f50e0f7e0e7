// The host-side prologue of config 5's training step as ONE launch (minecraft/sparse_diffusion.py:train, :398-449):
//   sample_time_dependent (:44-72)   per clip, a frame window whose width grows with the noise level t, placed uniformly, and
//                                    context_length distinct positions uniform inside it (`randperm(window)[:n] + offset`);
//   gather (:437)                    the clip's tokens at those positions (the targets);
//   perturbation & masking (:440-449) the corruption law of wmz_corrupt_tokens on the gathered tokens.
// On the op-by-op route this is ~45 device ops on 6-element tensors (window arithmetic), one top-k over [B, S H W] keys, a sort,
// a gather and the corruption launch: in the captured step every one of them is a graph node the host enqueues in ~10 us -- 0.45 ms
// of a 3.0 ms step in which the GPU mostly waits for the next 3-us kernel.
//
// One workgroup of 1 024 threads per clip:
//   * the window from r[b] and a uniform o (given, or Philox) exactly as the reference computes it (fp32 floor / clamp);
//   * a 32-bit Philox key per position of the window; the n smallest keys are n distinct positions, uniform without replacement,
//     and their key order is a uniform random order (ties -- probability 2^-32 a pair -- fall to the lower position:
//     deterministic).  Selection instead of a full sort (a bitonic sort of 16 384 packed keys in LDS measured 145 us): a histogram
//     of the keys' top 11 bits (LDS atomics) and a scan find the bin that holds the n-th smallest key; every key up to that bin
//     (n plus a bin's worth: <= 1 024) is a candidate, regenerated and compacted into LDS, and only the candidates are sorted
//     (bitonic, <= 1 024 packed (key, position) pairs);
//   * indices, gathered tokens (targets) and their corrupted copies are written from the sorted prefix.
// Deterministic in (seed, stream id, device counter): a hipGraph replay with the counter advanced draws a fresh context.
//
// The scored form (wmz_sparse_draw_context_scored; include/wmz.h states the law), a compile-time variant -- SCORED, which reads the
// ScScore at the end of the ScParams --: the sampler's masking ordered by confidence instead of a coin per slot.  Everything up to
// the sorted prefix is the same code reading the same Philox words; the last phase differs.  Slot i = thread i (n <= 512) gathers its position's score
// (+ the annealed Gumbel term from the very uniform the coin rule compares with r) and leaves its key and candidate flag in LDS --
// in the words of `hist`, which is dead behind the scan: the variant adds no LDS --; wave 0 then holds all <= 512 keys in 8
// registers a lane and runs wmz_select_lowest (wmz_select.h: 32 search steps of 8 ballots, no barrier, no memory access -- the
// one-wave form of remask_lowest_kernel); two barriers around it, and every slot writes its token.
#include "wmz_common.h"
#include "wmz_philox.h"
#include "wmz_select.h"

namespace {

constexpr int SC_THREADS = 1024;

struct ScScore {
  const float* scores; long stride;                 // [B, S * HW] fp32, addressed like z: the score of the token drawn there
  float noise;
  float* slot_scores;                               // optional probe [B, n]: the score each slot was ranked by
};

struct ScParams {
  const int64_t* z; long clip_stride;
  const float* r; const float* o;
  int64_t* indices; int64_t* tokens; int64_t* target;
  int B, S, HW, n, C, NP;
  float p_uniform;   // redraw probability per unit of r (training: 0.1, sparse_diffusion.py:447 p_max_uniform; the sampler: 0)
  unsigned long long seed, stream;
  const unsigned long long* counter;
  const unsigned char* known; long known_stride;   // optional bytes [B, S * HW]: a non-zero position is given -- gathered as it is
  ScScore score;                                   // the scored form's: not read when !SCORED
};

constexpr int SC_BINS = 2048, SC_CAND = 1024;
constexpr int SC_SLOTS = 512;                       // context positions at the most (wmz_sparse_draw_context_supported)

template <bool SCORED>
__global__ __launch_bounds__(SC_THREADS) void sparse_context_kernel(ScParams P) {
  __shared__ unsigned hist[SC_BINS];
  __shared__ unsigned long long cand[SC_CAND];                 // packed (key << 32 | position inside the window)
  __shared__ unsigned wave_tot[SC_THREADS / 64];
  __shared__ int win[2];
  __shared__ unsigned sel[2];                                  // the bin of the n-th smallest key; candidates taken so far
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long stream = philox_stream(P.stream, P.counter);
  if (tid == 0) {
    // the window (sparse_diffusion.py:53-64), in the reference's fp32 arithmetic
    const float t = fminf(fmaxf(P.r[b], 0.f), 1.f);
    const int need = (P.n + P.HW - 1) / P.HW;
    float frames = floorf((float)need + t * (float)(P.S - need + 1));
    frames = fminf(frames, (float)(P.S - need));
    float o;
    if (P.o != nullptr) o = fminf(fmaxf(P.o[b], 0.f), 1.f - 1e-5f);
    else {
      unsigned c[4];
      philox4((unsigned long long)b, stream | PHILOX_WIN_DOMAIN, P.seed, c);
      o = philox_unit(c[0]);
    }
    const float first = floorf(o * ((float)P.S - frames + 1.f));
    win[0] = (int)first;
    win[1] = (int)frames;
    sel[0] = SC_BINS - 1;                                      // (overwritten by the scan: the window holds >= n positions)
    sel[1] = 0;
  }
  for (int i = tid; i < SC_BINS; i += SC_THREADS) hist[i] = 0;
  cand[tid] = ~0ull;                                           // (SC_CAND == SC_THREADS: the sort's padding)
  __syncthreads();
  const int first = win[0], Wn = win[1] * P.HW;
  const int nq = (Wn + 3) / 4;                                 // Philox calls: four positions each
  const unsigned long long kbase = (unsigned long long)b * (unsigned long long)(P.NP / 4);
  // ---- pass 1: histogram of the keys' top 11 bits
  for (int q = tid; q < nq; q += SC_THREADS) {
    unsigned c[4];
    philox4(kbase + q, stream | PHILOX_KEY_DOMAIN, P.seed, c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < Wn) atomicAdd(&hist[c[e] >> 21], 1u);
  }
  __syncthreads();
  // ---- the bin of the n-th smallest key: exclusive prefix sums over the bins (two bins a thread)
  {
    const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
    unsigned incl = h0 + h1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned before = incl - (h0 + h1);
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    const unsigned want = (unsigned)P.n - 1;                   // rank of the n-th smallest key
    if (before <= want && want < before + h0) sel[0] = 2 * tid;
    else if (before + h0 <= want && want < before + h0 + h1) sel[0] = 2 * tid + 1;
  }
  __syncthreads();
  const unsigned bstar = sel[0];
  // ---- pass 2: the candidates (every key up to that bin: >= n of them, <= n + one bin's worth), regenerated and compacted
  for (int q = tid; q < nq; q += SC_THREADS) {
    unsigned c[4];
    philox4(kbase + q, stream | PHILOX_KEY_DOMAIN, P.seed, c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * q + e;
      if (i < Wn && (c[e] >> 21) <= bstar) {
        const unsigned slot = atomicAdd(&sel[1], 1u);
        if (slot < SC_CAND) cand[slot] = ((unsigned long long)c[e] << 32) | (unsigned)i;
      }
    }
  }
  __syncthreads();
  // ---- bitonic sort of the candidates, ascending (the order of the LDS atomics above does not matter: the sort decides)
  for (int k = 2; k <= SC_CAND; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < SC_CAND / 2) {
        const int lo = 2 * tid - (tid & (j - 1));              // the element of the pair with bit j clear
        const int hi = lo | j;
        const unsigned long long a = cand[lo], c = cand[hi];
        const bool up = (lo & k) == 0;
        if ((a > c) == up) { cand[lo] = c; cand[hi] = a; }
      }
      __syncthreads();
    }
  }
  // ---- the n smallest: positions, targets, corrupted tokens (the law and the stream layout of corrupt_kernel, loss.hip)
  const float rb = P.r[b];
  if constexpr (SCORED) {
    const ScScore& X = P.score;
    static_assert(2 * SC_SLOTS <= SC_BINS && SC_SLOTS % 64 == 0 && SC_SLOTS <= SC_THREADS, "keys and flags of every slot fit the histogram's words");
    unsigned* skey = hist;                                     // [SC_SLOTS] the slot's key; 0xFFFFFFFF: no candidate / past n
    unsigned* sflag = hist + SC_SLOTS;                         // [SC_SLOTS] in: candidate; out: masked
    const float rc = fminf(fmaxf(rb, 0.f), 1.f);
    const int i = tid;
    const long at = (long)b * P.n + i;
    int64_t tok = 0;
    if (i < SC_SLOTS) { skey[i] = 0xFFFFFFFFu; sflag[i] = 0u; }
    if (i < P.n) {
      unsigned wpos = (unsigned)cand[i];
      if (wpos >= (unsigned)Wn) wpos = 0;                      // (never: a padding entry would mean fewer than n candidates)
      const long pos = (long)wpos + (long)first * P.HW;
      tok = P.z[b * P.clip_stride + pos];
      float sc = X.scores[b * X.stride + pos];
      if (X.noise > 0.f) {
        unsigned c[4];
        philox4((unsigned long long)b * P.n + i, stream, P.seed, c);        // c[2]: the word the coin rule compares with r
        sc += X.noise * rc * -logf(-logf(philox_unit(c[2])));
      }
      sc = sc == sc ? sc : -INFINITY;
      const bool candidate = P.known == nullptr || P.known[b * P.known_stride + pos] == 0;
      if (candidate) { skey[i] = sw_key(sc); sflag[i] = 1u; }
      if (X.slot_scores != nullptr) X.slot_scores[at] = sc;
      P.indices[at] = pos;
      P.target[at] = tok;
    }
    __syncthreads();
    if (wave == 0) {
      constexpr int MAXP = SC_SLOTS / 64;
      unsigned key[MAXP], cbits = 0, ncand = 0;
#pragma unroll
      for (int j = 0; j < MAXP; ++j) {
        key[j] = skey[j * 64 + lane];
        const bool c = sflag[j * 64 + lane] != 0u;
        cbits |= (c ? 1u : 0u) << j;
        ncand += (unsigned)__popcll(__ballot(c));
      }
      const int m = (int)floorf(mul_rn(rc, (float)P.n));
      const unsigned mm = m <= 0 ? 0u : ((unsigned)m < ncand ? (unsigned)m : ncand);
      RmTotal<1> total{nullptr, 0};
      const unsigned taken = wmz_select_lowest<1, MAXP>(key, cbits, MAXP, mm, nullptr, total);
#pragma unroll
      for (int j = 0; j < MAXP; ++j) sflag[j * 64 + lane] = (taken >> j) & 1u;
    }
    __syncthreads();
    if (i < P.n) P.tokens[at] = sflag[i] != 0u ? (int64_t)P.C : tok;
    return;
  }
  for (int i = tid; i < P.n; i += SC_THREADS) {
    unsigned wpos = (unsigned)cand[i];
    if (wpos >= (unsigned)Wn) wpos = 0;                        // (never: a sort padding entry would mean fewer than n candidates)
    const long pos = (long)wpos + (long)first * P.HW;
    const int64_t tok = P.z[b * P.clip_stride + pos];
    unsigned c[4];
    philox4((unsigned long long)b * P.n + i, stream, P.seed, c);
    int64_t d = tok;
    if (philox_unit(c[0]) < rb * P.p_uniform) { const int kk = (int)(philox_unit(c[1]) * (float)P.C); d = kk < P.C ? kk : P.C - 1; }
    if (philox_unit(c[2]) < rb) d = P.C;
    if (P.known != nullptr && P.known[b * P.known_stride + pos] != 0) d = tok;       // (the uniforms above are drawn all the same)
    const long at = (long)b * P.n + i;
    P.indices[at] = pos;
    P.target[at] = tok;
    P.tokens[at] = d;
  }
}

}  // namespace

// 1 when wmz_sparse_draw_context holds the shape: n <= 512 context positions of a grid of <= 65 536 (the candidates -- n plus one
// histogram bin's worth of keys, S HW / 2048 expected -- must fit the 1 024-entry sort), and the reference's own precondition
extern "C" int wmz_sparse_draw_context_supported(int S, int HW, int n) {
  if (S <= 0 || HW <= 0 || n <= 0) return 0;
  const long G = (long)S * HW;
  const int need = (n + HW - 1) / HW;
  // (2 need <= S: the narrowest window, clamped to S - need frames, still holds n positions -- below that the reference's
  //  randperm(window)[:n] comes back short and its assignment raises)
  return G <= 65536 && n <= 512 && need < S && 2 * need <= S;
}

extern "C" int wmz_sparse_draw_context(const int64_t* z, long clip_stride, const float* r, const float* o, int64_t* indices,
                                       int64_t* tokens, int64_t* target, int B, int S, int HW, int n, int C, float p_uniform,
                                       unsigned long long seed, unsigned long long stream_id, const unsigned long long* counter,
                                       void* stream) {
  return wmz_sparse_draw_context_known(z, clip_stride, r, o, indices, tokens, target, B, S, HW, n, C, p_uniform, seed, stream_id, counter,
                                       stream, nullptr, 0);
}

// The same draw for a clip of which some positions are given (include/wmz.h states the law): `known` changes the corrupted copy
// of a given slot and nothing else.
static int sparse_context_launch(const int64_t* z, long clip_stride, const float* r, const float* o, int64_t* indices,
                                 int64_t* tokens, int64_t* target, int B, int S, int HW, int n, int C, float p_uniform,
                                 unsigned long long seed, unsigned long long stream_id, const unsigned long long* counter,
                                 void* stream, const unsigned char* known, long known_stride, const ScScore* score) {
  WMZ_REQUIRE(z && r && indices && tokens && target && B > 0 && C > 0, "wmz_sparse_draw_context: bad arguments");
  WMZ_REQUIRE(p_uniform >= 0.f && p_uniform <= 1.f, "wmz_sparse_draw_context: p_uniform in [0, 1] expected");
  WMZ_REQUIRE(known == nullptr || known_stride >= (long)S * HW, "wmz_sparse_draw_context_known: known_stride below S * HW");
  if (!wmz_sparse_draw_context_supported(S, HW, n)) {
    wmz_set_error("wmz_sparse_draw_context: grid %d x %d with %d context positions not built (<= 65536 positions, <= 512 of "
                  "them drawn, 2 ceil(n / HW) <= S)", S, HW, n);
    return WMZ_ERR_UNSUPPORTED;
  }
  ScParams P;
  P.z = z; P.clip_stride = clip_stride; P.r = r; P.o = o; P.indices = indices; P.tokens = tokens; P.target = target;
  P.B = B; P.S = S; P.HW = HW; P.n = n; P.C = C; P.p_uniform = p_uniform;
  int np = 4;
  while (np < S * HW) np <<= 1;
  P.NP = np;
  P.seed = seed;
  P.stream = philox_stream_base(stream_id, counter != nullptr) & ~(PHILOX_KEY_DOMAIN | PHILOX_WIN_DOMAIN);
  P.counter = counter;
  P.known = known; P.known_stride = known_stride;
  P.score = score != nullptr ? *score : ScScore{};
  if (score == nullptr)
    hipLaunchKernelGGL(sparse_context_kernel<false>, dim3(B), dim3(SC_THREADS), 0, (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL(sparse_context_kernel<true>, dim3(B), dim3(SC_THREADS), 0, (hipStream_t)stream, P);
  WMZ_LAUNCH_CHECK("wmz_sparse_draw_context");
  return WMZ_OK;
}

extern "C" int wmz_sparse_draw_context_known(const int64_t* z, long clip_stride, const float* r, const float* o, int64_t* indices,
                                             int64_t* tokens, int64_t* target, int B, int S, int HW, int n, int C, float p_uniform,
                                             unsigned long long seed, unsigned long long stream_id,
                                             const unsigned long long* counter, void* stream, const unsigned char* known,
                                             long known_stride) {
  return sparse_context_launch(z, clip_stride, r, o, indices, tokens, target, B, S, HW, n, C, p_uniform, seed, stream_id, counter, stream,
                               known, known_stride, nullptr);
}

// The sampler's masking ordered by confidence (include/wmz.h states the law): the scored variant of the kernel, same launch shape.
extern "C" int wmz_sparse_draw_context_scored(const int64_t* z, long clip_stride, const float* r, const float* o, int64_t* indices,
                                              int64_t* tokens, int64_t* target, int B, int S, int HW, int n, int C, float p_uniform,
                                              unsigned long long seed, unsigned long long stream_id,
                                              const unsigned long long* counter, void* stream, const unsigned char* known,
                                              long known_stride, const float* scores, long scores_stride, float noise,
                                              float* slot_scores) {
  WMZ_REQUIRE(scores != nullptr, "wmz_sparse_draw_context_scored: scores expected");
  WMZ_REQUIRE(p_uniform == 0.f, "wmz_sparse_draw_context_scored: the ordered rule masks only: p_uniform must be 0 (got %g)", (double)p_uniform);
  WMZ_REQUIRE(noise >= 0.f && noise < INFINITY, "wmz_sparse_draw_context_scored: noise must be non-negative and finite (got %g)",
              (double)noise);
  WMZ_REQUIRE(scores_stride >= (long)S * HW, "wmz_sparse_draw_context_scored: scores_stride below S * HW");
  const ScScore score = {scores, scores_stride, noise, slot_scores};
  return sparse_context_launch(z, clip_stride, r, o, indices, tokens, target, B, S, HW, n, C, p_uniform, seed, stream_id, counter, stream,
                               known, known_stride, &score);
}
