// The two steps either side of the denoiser in the training loop:
//   wmz_corrupt_tokens  main.py:246-259  mask + uniform token corruption of the last latent frame, without the [B,HW,C]
//                                        one-hot / lerp / multinomial temporaries (closed form, counter-based RNG in-kernel)
//   wmz_ce_fwd / _bwd   main.py:266-274  CrossEntropyLoss(reduction='none') over the last-frame logits and its gradient,
//                                        written directly in the GEMM operand dtype
#include "wmz_common.h"
#include "wmz_philox.h"

namespace {

// one thread per last-frame position.  a = 0.1 r: with probability a redraw uniformly over the C codes, else keep the
// token (== multinomial(lerp(one_hot, 1/C, a))); then positions with u < r become the mask token C.
__global__ __launch_bounds__(256) void corrupt_kernel(const int64_t* __restrict__ z_last, long clip_stride,
                                                      const float* __restrict__ r, int64_t* __restrict__ out,
                                                      long out_stride, int64_t* __restrict__ target, int B, int HW, int C,
                                                      unsigned long long seed, unsigned long long stream,
                                                      const unsigned long long* __restrict__ counter) {
  stream = philox_stream(stream, counter);                      // per-call stream id kept in device memory (hipGraph replay)
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
                     target, B, HW, C, seed, philox_stream_base(stream_hi, true), counter);
  WMZ_LAUNCH_CHECK("wmz_corrupt_tokens_dev");
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
