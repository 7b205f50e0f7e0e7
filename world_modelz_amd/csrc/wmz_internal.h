// Library-internal entry points shared between translation units (not part of include/wmz.h).
#pragma once
#include <hip/hip_runtime.h>

// linear_bwd.hip: the second stage of the deterministic weight-gradient reduction -- sums `nsplit` partial results laid out as
// workspace[block of 256 floats of the flat [N, K] result][split][256] (+ [split][N] bias partials behind them) into dW / dbias;
// taps > 0: dW is nn.Conv2d's own [co, ci, taps] layout (k = tap * cin_p + c), channel padding cropped.
int wmz_wgrad_reduce_launch(const float* workspace, float* dW, float* dbias, long NK, int nsplit, int N, int overwrite, int taps,
                            int cin_p, int co, int ci, hipStream_t stream);
// Where config 5's sampler puts a drawn class and where its uniform comes from (sparse_context.hip; the filtered row bodies of
// loss.hip take one behind their SampleExtras): samples[row] always; z[clip][indices[row]], clip = row / rows_per_clip, unless that
// position's `known` byte is set.  The Philox stream is `stream` with the low 40 bits of *counter or'ed in when counter != NULL.
struct WmzSparseOut {
  const int64_t* indices;
  int64_t* z;
  long clip_stride, rows_per_clip;
  int64_t* samples;
  const unsigned char* known;
  long known_stride;
  unsigned long long stream;
  const unsigned long long* counter;
};
__device__ __forceinline__ unsigned long long wmz_sparse_stream(const WmzSparseOut& o) {
  return o.counter != nullptr ? (o.stream | (*o.counter & ((1ull << 40) - 1))) : o.stream;
}
__device__ __forceinline__ void wmz_sparse_write(const WmzSparseOut& o, long row, int draw) {
  if (o.samples != nullptr) o.samples[row] = draw;
  if (o.z != nullptr) {
    const long clip = row / o.rows_per_clip;
    const int64_t pos = o.indices[row];
    if (o.known == nullptr || o.known[clip * o.known_stride + pos] == 0) o.z[clip * o.clip_stride + pos] = draw;
  }
}
// The scored form's second destination (wmz_categorical_scatter_scored): scores [clips, stride] fp32, addressed like z -- the score of
// a draw is written exactly where its token is written, and nowhere else.
struct WmzSparseScore {
  float* scores;
  long stride;
};
__device__ __forceinline__ void wmz_sparse_write_scored(const WmzSparseOut& o, const WmzSparseScore& s, long row, int draw, float score) {
  if (o.samples != nullptr) o.samples[row] = draw;
  if (o.z != nullptr) {
    const long clip = row / o.rows_per_clip;
    const int64_t pos = o.indices[row];
    if (o.known == nullptr || o.known[clip * o.known_stride + pos] == 0) {
      o.z[clip * o.clip_stride + pos] = draw;
      s.scores[clip * s.stride + pos] = score;
    }
  }
}
// loss.hip: the filtered draw (the row bodies of wmz_sample_tokens_filtered_dev) with a WmzSparseOut as destination -- and, with
// `score`, the score of each draw beside it --; the checks are the caller's (wmz_categorical_scatter_filtered / _scored)
int wmz_sparse_sample_launch(const char* name, const float* logits, long ld, int R, int C, int top_k, float top_p, float inv_temperature,
                             const float* uniforms, float* kept_floor, unsigned long long seed, const WmzSparseOut& out,
                             hipStream_t stream, const WmzSparseScore* score = nullptr);
// conv_wgrad.hip: direct 3x3 weight gradient (bf16, stride 1, pad 1, Cout = 128, Cin in {64, 128}, H % 8 == 0, W % 16 == 0)
int wmz_convw_supported(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dtype);
long wmz_convw_workspace_floats(int B, int H, int W, int Cin, int Cout);
int wmz_convw_launch(const void* x, const void* dy, float* dW, float* dbias, int B, int H, int W, int Cin, int Cout, int overwrite,
                     int conv_layout_co, int conv_layout_ci, float* workspace, long workspace_floats, hipStream_t stream);
