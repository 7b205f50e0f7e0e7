// The two laws by which frames cross between bytes and the unit interval, stated once.  Plain fp32 code without HIP and without
// pointers: the kernels of frame_bytes.hip apply these functions, tests/frame_bytes_host.cpp runs them on the host and
// tests/test_frame_bytes_cpu.py says what they promise.
//   in   vq-video-diffusion minecraft/main2.py:51-56 (transform_batch) and minecraft/sparse_diffusion.py:23-28:
//        uint8 -> fp32 -> / 255, computed on the CPU;
//   out  torchvision.utils.save_image behind main.py:121-132: mul(255).add_(0.5).clamp_(0, 255).to(uint8).
// The 16-bit operand formats are not this header's business: a kernel takes them to fp32 exactly first, and rounds a unit value
// into them afterwards, with the conversions of wmz_common.h.
#pragma once
#ifndef WMZ_HD
#ifdef __HIPCC__
#define WMZ_HD __host__ __device__ __forceinline__
#else
#define WMZ_HD inline
#endif
#endif

// fl(float(b) / 255.0f), the correctly rounded IEEE quotient -- what x.to(torch.float32).div(255) gives on the CPU.  (The product with
// fl(1 / 255) is another number at 126 of the 256 bytes.)  A table the COMPILER fills, by constant evaluation of the division: no
// division instruction is left whose rounding a fast-math or reciprocal-division flag of the unit could change.
struct FrameUnitTable { float v[256]; };
constexpr FrameUnitTable frame_unit_table() {
  FrameUnitTable t{};
  for (int b = 0; b < 256; ++b) t.v[b] = (float)b / 255.0f;
  return t;
}
WMZ_HD float frame_byte_to_unit(unsigned b) {
  constexpr FrameUnitTable t = frame_unit_table();
  return t.v[b & 255u];
}

// save_image's law in fp32, operation by operation: t = fl(f * 255), t = fl(t + 0.5) -- two roundings, never one fused
// multiply-add --, clamp to [0, 255], truncate.  +-inf end at 255 / 0 through the clamp.  NaN gives 0: torch's clamp hands the NaN
// on and leaves its cast to uint8 undefined, so it is DEFINED here (the first comparison is false for a NaN).  -0.0 gives 0.
// (Compilers without the pragma -- a host build of the test driver -- get -ffp-contract=off on their command line.)
WMZ_HD unsigned char frame_unit_to_byte(float f) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  float t = f * 255.0f;
  t = t + 0.5f;
  t = t > 0.0f ? t : 0.0f;
  t = t < 255.0f ? t : 255.0f;
  return (unsigned char)(int)t;
}
