// Shared device/host helpers for libwmz_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <utility>
#include <atomic>

#include "../../include/wmz.h"

// ---------------------------------------------------------------- error plumbing (host)
void wmz_set_error(const char* fmt, ...);

#define WMZ_REQUIRE(cond, ...)                       \
  do {                                               \
    if (!(cond)) {                                   \
      wmz_set_error(__VA_ARGS__);                    \
      return WMZ_ERR_ARG;                            \
    }                                                \
  } while (0)

// Function attributes (the > 64 KB dynamic-LDS opt-in) are per DEVICE: a process that drives several GPUs has to set them on each.
// True the first time the calling thread's current device is seen through `mask` (thread-safe; setting an attribute twice is harmless).
static inline bool wmz_first_use_on_device(std::atomic<uint64_t>& mask) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  return (mask.fetch_or(bit, std::memory_order_relaxed) & bit) == 0;
}

#define WMZ_LAUNCH_CHECK(name)                                               \
  do {                                                                       \
    hipError_t e__ = hipGetLastError();                                      \
    if (e__ != hipSuccess) {                                                 \
      wmz_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));  \
      return WMZ_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)

static inline int wmz_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---------------------------------------------------------------- element types
typedef __hip_bfloat16 bf16_t;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short s16x8;   // 8 bf16 = one 16x16x32 / 32x32x16 operand
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// ---- the 16-bit MFMA operand format of a translation unit.  The kernels move 16-bit elements as raw bits (s16x8 fragments, the
// `bf16_t` storage tag) and touch their VALUE only through the few primitives below, so the number format is decided here, once
// per translation unit: bfloat16 (the speed mode BASELINE.json names) by default; IEEE half when the unit is compiled with
// WMZ_OP16_F16 -- the "precise" fused mode (same MFMA rate, 11 significand bits instead of 8: end-to-end logits 8x closer to the
// reference's fp32, range +-65504).  A precise unit is a second compilation of the same source (csrc/*_f16.hip) whose entry
// points carry the suffix _f16 (WMZ_FN below).
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
#ifdef WMZ_OP16_F16
#define WMZ_FN(name) name##_f16
constexpr int kOp16Dtype = WMZ_F16;
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
// round-to-nearest-even (v_cvt_f16_f32); beyond +-65504 the result is an infinity, like the hardware conversion
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
__device__ __forceinline__ s16x4 cvt_pk4_bf16(float a, float b, float c, float d) {
  const f16x2_t lo = __builtin_convertvector((f32x2){a, b}, f16x2_t), hi = __builtin_convertvector((f32x2){c, d}, f16x2_t);
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  const u32x2 w = {__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
  return __builtin_bit_cast(s16x4, w);
}
// acc + value(bits): as ONE v_fma_mix_f32 (the half operand converted inside the instruction, hi / lo half selected by op_sel) --
// no conversion temporaries where a whole operand row is added to the fp32 stream (fused_common.h add_bop)
__device__ __forceinline__ float op16_add_to(float acc, unsigned short b) { return __builtin_fmaf((float)__builtin_bit_cast(_Float16, b), 1.0f, acc); }
__device__ __forceinline__ f32x4 op16_mfma_16x16x32(const s16x8& a, const s16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 op16_mfma_32x32x16(const s16x8& a, const s16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 op16_mfma_16x16x16(const s16x4& a, const s16x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4_t, a), __builtin_bit_cast(f16x4_t, b), c, 0, 0, 0);
}
// two floats -> the two 16-bit values of one dword (a in the low half), round-to-nearest-even: one v_cvt_pk_f16_f32
__device__ __forceinline__ unsigned op16_pack2(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, f16x2_t));
}
// the two 16-bit values of a dword -> floats (low half first): two v_cvt_f32_f16 (the high half by op_sel)
__device__ __forceinline__ f32x2 op16_unpack2(unsigned w) { return __builtin_convertvector(__builtin_bit_cast(f16x2_t, w), f32x2); }
// one of them: the low / the high half (a caller that consumes the two at different places keeps its own instruction order)
__device__ __forceinline__ float op16_lo_f32(unsigned w) { return (float)__builtin_bit_cast(f16x2_t, w)[0]; }
__device__ __forceinline__ float op16_hi_f32(unsigned w) { return (float)__builtin_bit_cast(f16x2_t, w)[1]; }
#else
#define WMZ_FN(name) name
constexpr int kOp16Dtype = WMZ_BF16;
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __uint_as_float(((unsigned)b) << 16);
}
// round-to-nearest-even; the plain cast keeps NaN a NaN (v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  bf16_t h = __float2bfloat16(f);
  return *reinterpret_cast<unsigned short*>(&h);
}

// four floats -> four bf16 (round-to-nearest-even) in two registers: two v_cvt_pk_bf16_f32, nothing else
__device__ __forceinline__ s16x4 cvt_pk4_bf16(float a, float b, float c, float d) {
  const bf16x2_t lo = __builtin_convertvector((f32x2){a, b}, bf16x2_t), hi = __builtin_convertvector((f32x2){c, d}, bf16x2_t);
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  const u32x2 w = {__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
  return __builtin_bit_cast(s16x4, w);
}
__device__ __forceinline__ float op16_add_to(float acc, unsigned short b) { return acc + bf16_bits_to_f32(b); }
__device__ __forceinline__ f32x4 op16_mfma_16x16x32(const s16x8& a, const s16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 op16_mfma_32x32x16(const s16x8& a, const s16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 op16_mfma_16x16x16(const s16x4& a, const s16x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
// two floats -> the two 16-bit values of one dword (a in the low half), round-to-nearest-even: one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned op16_pack2(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2_t));
}
// the two 16-bit values of a dword -> floats (low half first): a shift and a mask
__device__ __forceinline__ f32x2 op16_unpack2(unsigned w) { return (f32x2){__uint_as_float(w << 16), __uint_as_float(w & 0xFFFF0000u)}; }
// one of them: the low / the high half (a caller that consumes the two at different places keeps its own instruction order)
__device__ __forceinline__ float op16_lo_f32(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float op16_hi_f32(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }
#endif

// ---- the half guard (DESIGN 4.7 "Range"; include/wmz.h wmz_half_guard_bind).  IEEE half holds +-65504: an fp32 value beyond that
// rounds to an infinity.  A kernel of a half unit passes the packed dwords it is about to STORE through HalfGuard::see (one
// v_pk_fma_f16 per dword: value * 0 + acc is +-0 while every value seen is finite and a NaN from the first infinity or NaN on), folds
// the lanes' accumulators into a wave-uniform mask of WMZ_HG_* kinds with one ballot, and at its very end -- behind its last
// counted vmcnt wait -- issues at most ONE vector atomic OR per wave, and only when that mask is non-zero: a clean run adds no
// memory traffic.  The values a kernel rounds only to feed an MFMA (LayerNorm output, GELU hidden) need no test of their own: a
// non-finite operand element makes every output feature of that token's product non-finite (inf * w is an infinity or a NaN for
// every w), so the next rows the kernel stores for that token carry it.  The word's address is per-unit __constant__ state set by
// wmz_half_guard_bind (each guarded unit registers its setter with capi_core.hip when the library loads): NULL -- the default --
// skips the tests behind one wave-uniform branch per store site.  Units without WMZ_HALF_GUARD get the empty form below: no code.
// INVARIANT the operand argument rests on: every product of an operand rounded without a test ends, in the SAME kernel, in a row
// that is stored through a tested site.  A kernel that writes such a product to an untested buffer needs a test of its own.
// (WMZ_HALF_GUARD is defined by the units that carry the guard -- layer_fused_f16, layer_chain*_f16, conv_direct_f16,
// conv_point_f16, conv2d -- in front of this header: only they own a copy of the word's address and register its setter.)
#ifdef WMZ_HALF_GUARD
typedef int (*wmz_hg_setter)(unsigned*);
void wmz_half_guard_register_unit(wmz_hg_setter set);          // capi_core.hip
namespace {
__constant__ unsigned* wmz_hg_word = nullptr;
int wmz_hg_set(unsigned* word) { return hipMemcpyToSymbol(HIP_SYMBOL(wmz_hg_word), &word, sizeof(word)) == hipSuccess ? 0 : 1; }
struct WmzHgUnit { WmzHgUnit() { wmz_half_guard_register_unit(wmz_hg_set); } } wmz_hg_unit;
}
struct HalfGuard {
  unsigned* word;      // wave-uniform: NULL = no guard
  unsigned acc;        // per lane: a half pair, +-0 or NaN
  unsigned kinds;      // wave-uniform: WMZ_HG_* of what overflowed so far
  unsigned long long bad;   // wave-uniform: lanes whose see_f32 saw a value that rounds out of range
  __device__ __forceinline__ HalfGuard() : word(wmz_hg_word), acc(0u), kinds(0u), bad(0ull) {}
  __device__ __forceinline__ bool on() const { return word != nullptr; }
  __device__ __forceinline__ void see(unsigned w) { asm("v_pk_fma_f16 %0, %1, 0, %0" : "+v"(acc) : "v"(w)); }
  __device__ __forceinline__ void see(const s16x4& v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const u32x2 w = __builtin_bit_cast(u32x2, v);
    see(w[0]); see(w[1]);
  }
  __device__ __forceinline__ void see(const s16x8& v) {
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const u32x4 w = __builtin_bit_cast(u32x4, v);
    see(w[0]); see(w[1]); see(w[2]); see(w[3]);
  }
  // the fp32 value in front of its conversion, for kernels with no register to spare: one compare into a scalar mask, no VGPR
  // (round-to-nearest-even takes |x| >= 65520 -- halfway between 65504 and 2^16 -- to an infinity; a NaN fails the < too)
  __device__ __forceinline__ void see_f32(float x) { bad |= __builtin_amdgcn_ballot_w64(!(__builtin_fabsf(x) < 65520.0f)); }
  // ... only where `use` holds (a lane whose value is never stored: a padded channel), and the plain non-finite test for an fp32
  // sum of stored values (the conv epilogues' BatchNorm sums of squares: finite unless a stored value was not)
  __device__ __forceinline__ void see_f32_if(bool use, float x) { bad |= __builtin_amdgcn_ballot_w64(use && !(__builtin_fabsf(x) < 65520.0f)); }
  __device__ __forceinline__ void see_nonfinite_if(bool use, float x) {
    bad |= __builtin_amdgcn_ballot_w64(use && !(__builtin_fabsf(x) < __builtin_inff()));
  }
  __device__ __forceinline__ void see(const i32x4& v) { see(__builtin_bit_cast(s16x8, v)); }
  __device__ __forceinline__ void see(_Float16 v) { see((unsigned)__builtin_bit_cast(unsigned short, v)); }
  // the lanes' accumulators -> the wave's mask; the accumulator register is free again
  __device__ __forceinline__ void fold(unsigned kind) {
    if ((bad | __builtin_amdgcn_ballot_w64((acc & 0x7C007C00u) != 0u)) != 0ull) kinds |= kind;
    acc = 0u;
    bad = 0ull;
  }
  // once per wave, at the kernel's end (behind every counted vmcnt wait: the atomic is a VMEM operation)
  __device__ __forceinline__ void commit() {
    // (the lane test is computed HERE: a lane id carried from the kernel's prologue would stay live across its GEMMs)
    if (word != nullptr && kinds != 0u) {
      if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        __hip_atomic_fetch_or(word, kinds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};
typedef HalfGuard HalfGuardOn;
#endif
struct HalfGuardNone {
  __device__ __forceinline__ bool on() const { return false; }
  template <typename V> __device__ __forceinline__ void see(const V&) {}
  __device__ __forceinline__ void see_f32(float) {}
  __device__ __forceinline__ void see_f32_if(bool, float) {}
  __device__ __forceinline__ void see_nonfinite_if(bool, float) {}
  __device__ __forceinline__ void fold(unsigned) {}
  __device__ __forceinline__ void commit() {}
};
#ifndef WMZ_HALF_GUARD
typedef HalfGuardNone HalfGuard;
#endif

// ---- element types and their conversions to and from fp32, defined here ONCE for every unit: one element (to_f32 / from_f32),
// four (load4 / store4: one 16- or 8-byte access) and a 16-byte chunk held in registers (unpack / pack: kPerChunk elements).
// The two 16-bit tags mean different things:
//   bf16_t    the UNIT's 16-bit operand format -- bfloat16, or IEEE half in a unit compiled with WMZ_OP16_F16 -- always through
//             bf16_bits_to_f32 / f32_to_bf16_bits above (in a bfloat16 unit those ARE the shift and the rounding cast);
//   _Float16  IEEE half BY NAME, whatever the unit's format: the element-wise kernels that take a WMZ_F16 dtype argument next to
//             WMZ_BF16 in one (bfloat16) unit -- conv2d.hip's channel_stats / affine_act / bilinear2x, wmz_nchw_to_nhwc8's output.
template <typename T> struct Elem;
template <> struct Elem<float> {
  static constexpr int kDtype = WMZ_F32;
  static constexpr int kPerChunk = 4;                  // elements per 16-byte chunk
  __device__ static __forceinline__ float to_f32(float v) { return v; }
  __device__ static __forceinline__ float from_f32(float v) { return v; }
  __device__ static __forceinline__ void load4(const float* p, float (&f)[4]) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = v[e];
  }
  __device__ static __forceinline__ void store4(float* p, const float (&f)[4]) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = f[e];
    *reinterpret_cast<f32x4*>(p) = v;
  }
  __device__ static __forceinline__ void unpack(const i32x4& c, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __int_as_float(c[i]);
  }
  __device__ static __forceinline__ i32x4 pack(const float* f) {
    i32x4 c;
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = __float_as_int(f[i]);
    return c;
  }
};
template <> struct Elem<bf16_t> {
  static constexpr int kDtype = WMZ_BF16;
  static constexpr int kPerChunk = 8;
  __device__ static __forceinline__ float to_f32(bf16_t v) { return bf16_bits_to_f32(__builtin_bit_cast(unsigned short, v)); }
  __device__ static __forceinline__ bf16_t from_f32(float v) { return __builtin_bit_cast(bf16_t, f32_to_bf16_bits(v)); }
  __device__ static __forceinline__ void load4(const bf16_t* p, float (&f)[4]) {
    const s16x4 v = *reinterpret_cast<const s16x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = bf16_bits_to_f32((unsigned short)v[e]);
  }
  __device__ static __forceinline__ void store4(bf16_t* p, const float (&f)[4]) {
    s16x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (short)f32_to_bf16_bits(f[e]);
    *reinterpret_cast<s16x4*>(p) = v;
  }
  __device__ static __forceinline__ void unpack(const i32x4& c, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = bf16_bits_to_f32((unsigned short)((unsigned)c[i] & 0xFFFFu));
      f[2 * i + 1] = bf16_bits_to_f32((unsigned short)((unsigned)c[i] >> 16));
    }
  }
  __device__ static __forceinline__ i32x4 pack(const float* f) {
    i32x4 c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      c[i] = (int)((unsigned)f32_to_bf16_bits(f[2 * i]) | ((unsigned)f32_to_bf16_bits(f[2 * i + 1]) << 16));
    return c;
  }
};
template <> struct Elem<_Float16> {
  static constexpr int kDtype = WMZ_F16;
  static constexpr int kPerChunk = 8;
  __device__ static __forceinline__ float to_f32(_Float16 v) { return (float)v; }
  __device__ static __forceinline__ _Float16 from_f32(float v) { return (_Float16)v; }
  __device__ static __forceinline__ void load4(const _Float16* p, float (&f)[4]) {
    const f32x4 v = __builtin_convertvector(*reinterpret_cast<const f16x4_t*>(p), f32x4);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = v[e];
  }
  __device__ static __forceinline__ void store4(_Float16* p, const float (&f)[4]) {
    *reinterpret_cast<f16x4_t*>(p) = __builtin_convertvector((f32x4){f[0], f[1], f[2], f[3]}, f16x4_t);
  }
  __device__ static __forceinline__ void unpack(const i32x4& c, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (through a scalar copy: a bit_cast straight from the vector element c[i] read element 0 for every i)
      const unsigned w = (unsigned)c[i];
      const f32x2 v = __builtin_convertvector(__builtin_bit_cast(f16x2_t, w), f32x2);
      f[2 * i] = v[0];
      f[2 * i + 1] = v[1];
    }
  }
  __device__ static __forceinline__ i32x4 pack(const float* f) {
    i32x4 c;
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = (int)__builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){f[2 * i], f[2 * i + 1]}, f16x2_t));
    return c;
  }
};

// ---- host: a runtime dtype argument -> the element type.  f is a generic lambda taking a value of the type (`[&](auto e) {
// typedef decltype(e) T; ... kernel<T> ... }`), so a kernel's launch is written once.  Two widths, because a lambda is instantiated
// for every type its dispatcher names: wmz_by_dtype2 for entry points built for fp32 and the unit's 16-bit format, wmz_by_dtype3
// for those that also take IEEE half by name.  The caller has checked dtype (WMZ_REQUIRE) before.
template <typename F> static inline void wmz_by_dtype2(int dtype, F&& f) {
  if (dtype == WMZ_BF16) f(bf16_t()); else f(float());
}
template <typename F> static inline void wmz_by_dtype3(int dtype, F&& f) {
  if (dtype == WMZ_F16) f(_Float16()); else wmz_by_dtype2(dtype, f);
}

// byte offset XOR of row r in a 128-byte-row LDS image (rows swizzled in pairs): conflict-free ds_read_b128 fragment reads
__device__ __forceinline__ int swz128(int r) { return ((r >> 1) << 4) & 112; }

// An MFMA operand fragment of 8 consecutive k-elements (lane-local).
template <typename T> struct Frag8;
template <> struct Frag8<float> { float v[8]; };
template <> struct Frag8<bf16_t> { s16x8 v; };

__device__ __forceinline__ void frag_zero(Frag8<float>& f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f.v[i] = 0.f;
}
__device__ __forceinline__ void frag_zero(Frag8<bf16_t>& f) { f.v = (s16x8)(0); }

// 16-byte chunk loads into a fragment half/whole.  bf16: one chunk = whole fragment; f32: two chunks.
__device__ __forceinline__ void frag_load(Frag8<bf16_t>& f, const bf16_t* p) {
  f.v = *reinterpret_cast<const s16x8*>(p);
}
__device__ __forceinline__ void frag_load(Frag8<float>& f, const float* p) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { f.v[i] = a[i]; f.v[4 + i] = b[i]; }
}

// D(16x16) += A(16x32) * B(32x16).  Lane l holds A[row l&15][k = 8*(l>>4)+j], B[k = 8*(l>>4)+j][col l&15],
// j = 0..7; D: col = l&15, row = 4*(l>>4)+reg.   f32: eight exact-f32 16x16x4 MFMAs (k = 8g+j summed over g).
__device__ __forceinline__ void mma16(f32x4& acc, const Frag8<bf16_t>& a, const Frag8<bf16_t>& b) {
  acc = op16_mfma_16x16x32(a.v, b.v, acc);
}
__device__ __forceinline__ void mma16(f32x4& acc, const Frag8<float>& a, const Frag8<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// D(32x32) += A(32x16) * B(16x32).  Lane l holds A[row l&31][k = 8*(l>>5)+j], B[k = 8*(l>>5)+j][col l&31];
// D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
__device__ __forceinline__ void mma32(f32x16& acc, const Frag8<bf16_t>& a, const Frag8<bf16_t>& b) {
  acc = op16_mfma_32x32x16(a.v, b.v, acc);
}
__device__ __forceinline__ void mma32(f32x16& acc, const Frag8<float>& a, const Frag8<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// exact-erf GELU (nn.GELU default) with erf from Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7 (fp32 round-off level,
// 4 orders below bf16 resolution) at about a third of libm erff's instruction count.  Shared by every kernel that
// applies GELU or its derivative.
__device__ __forceinline__ float wmz_erf(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  return copysignf(1.f - p * t * __expf(-ax * ax), x);
}
__device__ __forceinline__ float wmz_gelu(float v) { return 0.5f * v * (1.f + wmz_erf(v * 0.70710678118654752440f)); }
// d/dv GELU(v) = Phi(v) + v * phi(v)
__device__ __forceinline__ float wmz_dgelu(float v) {
  return 0.5f * (1.f + wmz_erf(v * 0.70710678118654752440f)) + v * 0.3989422804014327f * __expf(-0.5f * v * v);
}

// GELU for kernels whose output is rounded to bf16 anyway: v * sigmoid(v * (c1 + c3 v^2 + c5 v^4)), coefficients fitted
// (minimax over [-9, 9], tools in DESIGN.md) to the exact-erf GELU: max |error| 2.6e-5 absolute, two orders below the
// bf16 resolution of the result, at 9 instructions (the erf form above costs ~20).  v^2 is clamped at 50: beyond |v| = 7
// the sigmoid argument stays at 3.5 |v| (the polynomial would turn over at |v| = 11).
__device__ __forceinline__ float wmz_gelu_fast(float v) {
  const float w = fminf(v * v, 50.f);
  float p = fmaf(-1.0148166e-3f, w, 0.10677913f);          // -(c5, c3, c1) * log2(e): exp2 of the negated argument
  p = fmaf(p, w, 2.3011176f);
  const float e = __builtin_amdgcn_exp2f(-p * v);
  return v * __builtin_amdgcn_rcpf(1.f + e);
}

// wmz_gelu_fast(v) and its derivative in one go (the backward of the fused feed-forward): with s = sigmoid(u(v)),
// u = v (c1 + c3 v^2 + c5 v^4):  d/dv [v s] = s (1 + v (1 - s) u'(v)).  Max |error| against the exact-erf derivative
// Phi(v) + v phi(v): 1.1e-4 (checked over [-12, 12]); beyond the clamp u' is the clamped polynomial itself.
__device__ __forceinline__ void wmz_gelu_fast_both(float v, float& g, float& d) {
  constexpr float LN2 = 0.6931471805599453f;
  const float vv = v * v;
  const float w = fminf(vv, 50.f);
  float p = fmaf(-1.0148166e-3f, w, 0.10677913f);
  p = fmaf(p, w, 2.3011176f);
  const float e = __builtin_amdgcn_exp2f(-p * v);
  const float s = __builtin_amdgcn_rcpf(1.f + e);
  g = v * s;
  float q = fmaf(-5.f * 1.0148166e-3f * LN2, w, 3.f * 0.10677913f * LN2);
  q = fmaf(q, w, 2.3011176f * LN2);
  q = vv < 50.f ? q : p * LN2;
  d = s * fmaf(v * (1.f - s), q, 1.f);
}

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(<N-1>) -- for bodies that need the index as a constant
// expression (instruction immediates in inline asm)
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// LDS byte address of a pointer into __shared__ memory
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
// ds_read_b64_tr_b16 as inline asm.  The builtin form is an "unknown memory access" to hipcc: with an LDS-DMA
// (global_load_lds) in flight it puts s_waitcnt vmcnt(0) in front of every such read, i.e. it drains the slab being
// prefetched before the current one may be used (measured: the prefetch then overlaps nothing).  The asm form is invisible
// to that bookkeeping -- and to lgkmcnt tracking as well: the caller waits with ds_tr_wait() before using the results.
template <int OFF>
__device__ __forceinline__ s16x4 ds_read_tr16_asm(unsigned addr) {
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
__device__ __forceinline__ void ds_tr_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// ds_read_b128 as inline asm + a counted wait that names the value it releases (the consumer cannot be scheduled above it): a
// hand-ordered queue of LDS reads, retired one by one while the younger ones are still in flight.
template <int OFF>
__device__ __forceinline__ s16x8 ds_read_b128_asm(unsigned addr) {
  s16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <int N>
__device__ __forceinline__ void lgkm_wait_for(s16x8& v) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N) : "memory"); }
// the same queue discipline for the other shapes a hand-ordered LDS queue carries: four floats (an accumulator's initial
// value), one dword, and a wait that releases two / four values at once
template <int OFF>
__device__ __forceinline__ f32x4 ds_read_f32x4_asm(unsigned addr) {
  f32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <int OFF>
__device__ __forceinline__ unsigned ds_read_u32_asm(unsigned addr) {
  unsigned r;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <int N, typename A, typename B>
__device__ __forceinline__ void lgkm_wait_for2(A& a, B& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory"); }
template <int N, typename A>
__device__ __forceinline__ void lgkm_wait_for4(A& a, A& b, A& c, A& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
// lane id (0..63) that the optimiser can neither hoist out of a loop nor keep alive across it
__device__ __forceinline__ unsigned lane_id_volatile() {
  unsigned r;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(r));
  return r;
}

// Reductions over the four 16-lane groups of a wave (lanes l, l^16, l^32, l^48 -> the same result in all four) with the
// gfx950 row / half swaps: two VALU instructions per level, no LDS round trip (__shfl_xor is a ds_bpermute: ~100+ cycles
// of latency each, and with an LDS-DMA in flight hipcc drains vmcnt in front of it).
//   v_permlane16_swap d, s: rows 1, 3 of d <-> rows 0, 2 of s;   v_permlane32_swap d, s: upper half of d <-> lower half of s
__device__ __forceinline__ float wave_groups_max(float v) {
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const unsigned m = __float_as_uint(fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])));
  const auto b = __builtin_amdgcn_permlane32_swap(m, m, false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float wave_groups_sum(float v) {
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const unsigned m = __float_as_uint(__uint_as_float(a[0]) + __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(m, m, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float wave_halves_sum(float v) {          // lanes l, l^32
  const unsigned u = __float_as_uint(v);
  const auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Sum over all 64 lanes, result in every lane: four DPP row rotations (within the 16-lane rows) and the two swaps above
// (across the rows) -- VALU only.  The __shfl_xor butterfly is six ds_bpermute round trips per reduction.
template <int N> __device__ __forceinline__ float dpp_row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 | N, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_row_ror<8>(v);
  v += dpp_row_ror<4>(v);
  v += dpp_row_ror<2>(v);
  v += dpp_row_ror<1>(v);
  return wave_groups_sum(v);
}

// wave64 butterfly helpers
__device__ __forceinline__ float wave_xor_max(float v, int mask) { return fmaxf(v, __shfl_xor(v, mask)); }
__device__ __forceinline__ float wave_xor_add(float v, int mask) { return v + __shfl_xor(v, mask); }

// XCD-aware block remap: consecutive logical ids land on one XCD (blocks b, b+8, .. share an XCD's L2).
// Bijective for any grid size (cdna guide T1).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}
