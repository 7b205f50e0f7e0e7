// Byte frames in and out of the VQ auto-encoder: the two edges of the pipeline where pixels cross (frame_bytes.h holds the laws).
//   wmz_frames_u8_to_nhwc8   uint8 frames, [H, W, C] or [C, H, W] each -> the encoder's operand: NHWC, channels zero-padded to a
//                            multiple of 8, value byte / 255 rounded into the operand dtype.  Replaces the host side of
//                            minecraft/main2.py:51-56 and minecraft/sparse_diffusion.py:23-28 (permute, fp32 copy, divide: four
//                            times the bytes over the host link) AND the layout flip wmz_nchw_to_nhwc8 runs on what they upload.
//   wmz_nhwc8_to_frames_u8   the decoder's raw NHWC output -> uint8 frames by save_image's law (main.py:121-132): the download is
//                            the finished bytes.
// Both have the shape of conv_point.hip's nchw_to_nhwc8_kernel: a thread owns one pixel and one group of 8 channels.
#include "wmz_common.h"
#include "frame_bytes.h"

namespace {

// Consecutive threads own consecutive pixels (channel groups outermost), so the byte loads of a wave are contiguous ([C, H, W]:
// 64 bytes of a plane per channel; [H, W, C]: the 64 C bytes of its pixels, once per channel of the group) and its stores are
// consecutive 16-byte chunks (32-byte for fp32) per group.  x has no alignment: byte loads only.
// The law's table is staged in LDS once per workgroup (its 256 lanes read it in one coalesced load): a lookup is an LDS read, not
// a second trip through the vector cache behind every byte load (measured: profiles/frame_bytes/README.md).
// CN: the channel count when it is known at compile time (3, 1: the frames there are) -- CN loads, no branch; 0: any C, every
// lane loads 8 bytes, a padding channel's from channel C - 1 (valid memory; the value is dropped).  Branch-free either way: a
// load inside a branch is waited for where the branch ends, one memory latency per channel; here all of a thread's byte loads
// are in flight together.
template <typename TO, int CN>
__global__ __launch_bounds__(256) void frames_u8_to_nhwc8_kernel(const unsigned char* __restrict__ x, TO* __restrict__ y, int C, int C8,
                                                                 long HW, long npix, long frame_stride, int channels_last) {
  __shared__ float unit[256];
  unit[threadIdx.x] = frame_byte_to_unit(threadIdx.x);
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int ngrp = CN > 0 ? 1 : C8 >> 3;
  if (i >= npix * ngrp) return;
  const int grp = CN > 0 ? 0 : (int)(i / npix);
  const long pix = i - grp * npix;
  const long n = pix / HW, p = pix - n * HW;
  const int Cr = CN > 0 ? CN : C;
  const unsigned char* const src = x + n * frame_stride + (channels_last ? p * Cr : p);
  const long cstep = channels_last ? 1 : HW;
  constexpr int NL = CN > 0 ? CN : 8;
  unsigned b[NL];
#pragma unroll
  for (int e = 0; e < NL; ++e) {
    const int c = grp * 8 + e;
    b[e] = src[(c < Cr ? c : Cr - 1) * cstep];
  }
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = 0.f;
#pragma unroll
  for (int e = 0; e < NL; ++e) {
    const float u = unit[b[e]];
    f[e] = grp * 8 + e < Cr ? u : 0.f;
  }
  TO* const dst = y + pix * C8 + grp * 8;
  if constexpr (Elem<TO>::kPerChunk == 8) {
    *reinterpret_cast<i32x4*>(dst) = Elem<TO>::pack(f);
  } else {
    *reinterpret_cast<i32x4*>(dst) = Elem<TO>::pack(f);
    *reinterpret_cast<i32x4*>(dst + 4) = Elem<TO>::pack(f + 4);
  }
}

// The same ownership the other way: one 16-byte read per pixel and group (two for fp32), then the group's real channels as bytes.
// The padding channels are loaded with their chunk and never converted.  [C, H, W]: a wave's byte stores are 64 consecutive bytes
// of a plane per channel; [H, W, C]: the C bytes of a pixel from one lane, the wave's pixels back to back.
template <typename TI>
__global__ __launch_bounds__(256) void nhwc8_to_frames_u8_kernel(const TI* __restrict__ y, unsigned char* __restrict__ out, int C, int C8,
                                                                 long HW, long npix, int channels_last) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int ngrp = C8 >> 3;
  if (i >= npix * ngrp) return;
  const int grp = (int)(i / npix);
  const long pix = i - grp * npix;
  const long n = pix / HW, p = pix - n * HW;
  const TI* const src = y + pix * C8 + grp * 8;
  float f[8];
  Elem<TI>::unpack(*reinterpret_cast<const i32x4*>(src), f);
  if constexpr (Elem<TI>::kPerChunk == 4) Elem<TI>::unpack(*reinterpret_cast<const i32x4*>(src + 4), f + 4);
  unsigned char* const dst = out + (channels_last ? pix * C : n * C * HW + p);
  const long cstep = channels_last ? 1 : HW;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = grp * 8 + e;
    if (c < C) dst[c * cstep] = frame_unit_to_byte(f[e]);
  }
}

bool dtype3(int dt) { return dt == WMZ_F32 || dt == WMZ_BF16 || dt == WMZ_F16; }

}  // namespace

extern "C" int wmz_frames_u8_to_nhwc8(const void* x, void* y, long N, int C, int H, int W, long frame_stride, int channels_last,
                                      int out_dtype, void* stream) {
  WMZ_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "wmz_frames_u8_to_nhwc8: bad arguments");
  WMZ_REQUIRE(dtype3(out_dtype), "wmz_frames_u8_to_nhwc8: bad dtype");
  const long HW = (long)H * W;
  WMZ_REQUIRE(frame_stride >= HW * C, "wmz_frames_u8_to_nhwc8: frame_stride %ld is less than a frame's %ld bytes", frame_stride, HW * C);
  WMZ_REQUIRE(((size_t)y & 15) == 0, "wmz_frames_u8_to_nhwc8: y must be 16-byte aligned");
  const int C8 = (C + 7) & ~7;
  const long npix = N * HW, blocks = (npix * (C8 >> 3) + 255) / 256;
  WMZ_REQUIRE(blocks <= 0x7fffffffL, "wmz_frames_u8_to_nhwc8: too many pixels for one launch");
  wmz_by_dtype3(out_dtype, [&](auto e) {
    typedef decltype(e) TO;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)x, (TO*)y, C, C8, HW,
                         npix, frame_stride, channels_last != 0);
    };
    if (C == 3) launch(frames_u8_to_nhwc8_kernel<TO, 3>);
    else if (C == 1) launch(frames_u8_to_nhwc8_kernel<TO, 1>);
    else launch(frames_u8_to_nhwc8_kernel<TO, 0>);
  });
  WMZ_LAUNCH_CHECK("wmz_frames_u8_to_nhwc8");
  return WMZ_OK;
}

extern "C" int wmz_nhwc8_to_frames_u8(const void* y, void* out, long N, int C, int H, int W, int channels_last, int in_dtype,
                                      void* stream) {
  WMZ_REQUIRE(y && out && N > 0 && C > 0 && H > 0 && W > 0, "wmz_nhwc8_to_frames_u8: bad arguments");
  WMZ_REQUIRE(dtype3(in_dtype), "wmz_nhwc8_to_frames_u8: bad dtype");
  WMZ_REQUIRE(((size_t)y & 15) == 0, "wmz_nhwc8_to_frames_u8: y must be 16-byte aligned");
  const int C8 = (C + 7) & ~7;
  const long HW = (long)H * W, npix = N * HW, blocks = (npix * (C8 >> 3) + 255) / 256;
  WMZ_REQUIRE(blocks <= 0x7fffffffL, "wmz_nhwc8_to_frames_u8: too many pixels for one launch");
  wmz_by_dtype3(in_dtype, [&](auto e) {
    typedef decltype(e) TI;
    hipLaunchKernelGGL((nhwc8_to_frames_u8_kernel<TI>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const TI*)y,
                       (unsigned char*)out, C, C8, HW, npix, channels_last != 0);
  });
  WMZ_LAUNCH_CHECK("wmz_nhwc8_to_frames_u8");
  return WMZ_OK;
}
