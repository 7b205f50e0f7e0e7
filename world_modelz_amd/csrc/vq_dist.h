// The pinned squared distance of VectorQuantizerEMA (vq-video-diffusion/vq.py:30), shared by the full scan (vq.hip) and by
// the screened search's two exact evaluations (vq_screen.hip).  Units that include this are compiled with -ffp-contract=off
// (build.py PER_FILE): the arithmetic must round exactly like the reference's separate sub / mul / add tensor ops.
#pragma once
#include "wmz_common.h"

namespace {

// sum_e (x[e]-c[e])^2 in the order ATen's CPU `vectorized_inner_sum` uses for the reference expression
// (vq.py:30): 8 SIMD lanes x 4 interleaved accumulators, leftover vectors added to a0, combined ((a0+a1)+a2)+a3, then
// the scalar tail first and the 8 lanes in order.  Pinned by oracle.vq.distances_avx_order / tests.
template <int E, typename XF, typename CF>
__device__ __forceinline__ float dist_exact(XF xf, CF cf) {
  constexpr int NV = E / 8, NI = NV / 4;
  float t[8];
  if constexpr (NI > 0) {
    float acc[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = xf(8 * k + j) - cf(8 * k + j); acc[k][j] = d * d; }
#pragma unroll
    for (int i = 1; i < NI; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int e = 8 * (4 * i + k) + j;
          const float d = xf(e) - cf(e);
          acc[k][j] = acc[k][j] + d * d;
        }
    // leftover vectors join accumulator 0 BEFORE the accumulators are combined (ATen row_sum)
#pragma unroll
    for (int v = NI * 4; v < NV; ++v)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = xf(8 * v + j) - cf(8 * v + j); acc[0][j] = acc[0][j] + d * d; }
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = ((acc[0][j] + acc[1][j]) + acc[2][j]) + acc[3][j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = xf(8 * v + j) - cf(8 * v + j); t[j] = t[j] + d * d; }
  }
  float fin = 0.f;
#pragma unroll
  for (int e = NV * 8; e < E; ++e) { const float d = xf(e) - cf(e); fin = fin + d * d; }
#pragma unroll
  for (int j = 0; j < 8; ++j) fin = fin + t[j];
  return fin;
}

}  // namespace
