// Host driver of csrc/fused_pack_rows.h (no HIP): prints the block rows of fused weight streams built on fake addresses, for
// tests/test_fused_pack_rows_cpu.py to check against its own statement of the layout.
//   fused_pack_rows_host START8 STREAM...      STREAM = ht | h | t (forward boundary with head and / or tail) | q | f (backward qkv / ff)
// Parameter slot k of a stream (wmz_layer_fused_pack's fourteen / wmz_layer_fused_bwd_pack's eight, an absent head's or tail's
// NULL) sits at address (k + 1) << 32, stream i is written at (100 + i) << 32; the streams follow each other in the launch's
// numbering of 8-element groups from START8 on.  Per block:
//   row <stream> <w> <rs> <ks> <N> <K> <gn> <gk> <gamma> <rgamma> <dst> <start8>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../world_modelz_amd/csrc/fused_pack_rows.h"

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s START8 ht|h|t|q|f ...\n", argv[0]); return 2; }
  long start8 = std::atol(argv[1]);
  for (int i = 2; i < argc; ++i) {
    const char* k = argv[i];
    const bool fwd = !std::strcmp(k, "ht") || !std::strcmp(k, "h") || !std::strcmp(k, "t");
    if (!fwd && std::strcmp(k, "q") && std::strcmp(k, "f")) return 2;
    const float* p[14];
    for (long s = 0; s < 14; ++s) {
      const bool absent = fwd && (s < 8 ? std::strchr(k, 'h') == nullptr : std::strchr(k, 't') == nullptr);
      p[s] = absent ? nullptr : reinterpret_cast<const float*>((s + 1) << 32);
    }
    FusedPackRow rows[24];
    unsigned short* dst = reinterpret_cast<unsigned short*>((100L + (i - 2)) << 32);
    const int n = fwd ? fused_fwd_rows(rows, p, dst, start8) : k[0] == 'q' ? fused_bwd_qkv_rows(rows, p, dst, start8)
                                                                           : fused_bwd_ff_rows(rows, p, dst, start8);
    for (int j = 0; j < n; ++j) {
      const FusedPackRow& r = rows[j];
      std::printf("row %d %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", i - 2, (long)r.w, r.rs, r.ks, r.N, r.K, r.gn, r.gk, (long)r.gamma,
                  (long)r.rgamma, (long)r.dst, r.start8);
    }
    start8 += fused_rows_groups(rows, n);
  }
  return 0;
}
