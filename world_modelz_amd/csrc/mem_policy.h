// Cache policy of the global stores that hand an activation tensor to the NEXT launch, as a compile-time parameter of the row-store
// helpers of fused_common.h.  The same bytes, addresses and order either way: only the policy bits of the instruction differ.
//   Plain   what every run-time kernel uses: the line stays in the XCD's L2, dirty, until it is evicted or the kernel boundary
//           writes it back
//   SC1     `sc1`: written through as it is stored and dropped from this XCD's L2 -- the reader is another launch, almost always on
//           another XCD, so nothing is gained by keeping the line, and the write-back runs under the kernel's own store phases
//           instead of at its end (measurements, and `nt` / `sc0 sc1`, which both cost time: profiles/handoff_policy/README.md)
// No form the compiler tracks yields a 16-byte `sc1` store on gfx950: __builtin_nontemporal_store sets `nt`, a volatile access
// `sc0 sc1`, an agent-scope atomic store is 8 bytes at most, and the buffer builtins' aux operand needs a buffer instruction with a
// descriptor of its own.  So the store is inline assembly, in the scalar-base form the compiler itself emits for the whole-workgroup
// row stores, followed by the two wait states a 16-byte store needs before its data registers may be overwritten (the compiler does
// not look inside the string); it counts in vmcnt like the store it replaces, which is all the weight ring's tallies need.
// tools/check_untracked.py checks every one of them in the listing.
#pragma once

enum class MemPolicy { Plain, SC1 };

// 16 bytes to a wave-uniform base + 32-bit per-lane byte offset + an immediate that folds to a literal (0 .. 4095)
template <MemPolicy P, typename T>
__device__ __forceinline__ void gstore_at(char* base, unsigned voff, int imm, const T& v) {
  static_assert(sizeof(T) == 16, "one dwordx4");
  if constexpr (P == MemPolicy::SC1)
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc1\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(base), "i"(imm) : "memory");
  else *reinterpret_cast<T*>(base + (voff + (unsigned)imm)) = v;
}
