// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011), stated once: the generator of the
// token corruption (loss.hip), the sampler step and config 5's categorical sampler (sampler.hip) and the sparse context draw
// (sparse_context.hip).  The
// trainers and sample.py build their stream ids on the three drawing from ONE generator.  Plain integer code without HIP types:
// tests/philox_host.cpp runs it on the host and tests/test_philox_cpu.py checks its words against the published algorithm.
#pragma once
#ifndef WMZ_HD
#ifdef __HIPCC__
#define WMZ_HD __host__ __device__ __forceinline__
#else
#define WMZ_HD inline
#endif
#endif

WMZ_HD void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
  const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
  const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
// ten rounds (the key bumped by the Weyl constants between them) on the project's keying: counter = (index, stream), key = seed,
// low word first
WMZ_HD void philox4(unsigned long long idx, unsigned long long stream, unsigned long long seed, unsigned (&c)[4]) {
  c[0] = (unsigned)idx; c[1] = (unsigned)(idx >> 32); c[2] = (unsigned)stream; c[3] = (unsigned)(stream >> 32);
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// a word -> [0, 1): its top 24 bits, exact in fp32
WMZ_HD float philox_unit(unsigned w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
// the four words of a block as [0, 1) values
WMZ_HD void philox4_unit(unsigned long long idx, unsigned long long stream, unsigned long long seed, float (&u)[4]) {
  unsigned c[4];
  philox4(idx, stream, seed, c);
  for (int i = 0; i < 4; ++i) u[i] = philox_unit(c[i]);
}

// The layout of a stream id: the rank from bit 40 up, the per-call counter in bits 0..39, and in bits 62 and 63 the domain that
// separates config 5's uses of the generator (none: a context slot's corruption words; KEY: the position keys; WIN: the window
// offset; both: the categorical sampler's rows).
constexpr unsigned long long PHILOX_KEY_DOMAIN = 1ull << 63, PHILOX_WIN_DOMAIN = 1ull << 62;
constexpr unsigned long long PHILOX_COUNTER_BITS = (1ull << 40) - 1;
// the id a launch hands its kernel: with a device counter, its bits cleared for ...
WMZ_HD unsigned long long philox_stream_base(unsigned long long stream_id, bool has_counter) {
  return has_counter ? stream_id & ~PHILOX_COUNTER_BITS : stream_id;
}
// ... the kernel to or the low 40 bits of *counter in (counter != NULL: the per-call id lives in device memory, hipGraph replay)
WMZ_HD unsigned long long philox_stream(unsigned long long stream, const unsigned long long* counter) {
  return counter != nullptr ? stream | (*counter & PHILOX_COUNTER_BITS) : stream;
}
