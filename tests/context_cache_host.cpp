// Host enumeration of csrc/fused_row_maps.h -- the source and destination row maps of a per-token launch, the very lines the
// kernel's option policies call -- for tests/test_context_cache_cpu.py.  One line per case:
//   dst B HW planes_out dst_planes dst_plane0 total : row of t = 0, 1, ..      (fused_dst_row; total = fused_dst_total)
//   src B HW planes_out planes_in : row of t = 0, 1, ..                       (fused_src_row, the trailing planes)
//   idn n : row of t = 0 .. n-1 under rows_out == 0, both maps                (the launch that never asked for a map)
//   ok planes_out dst_planes dst_plane0 flag                                  (fused_slots_ok: what the _slots entry points accept)
#include <cstdio>

#include "../world_modelz_amd/csrc/fused_row_maps.h"

int main() {
  const int Bs[] = {1, 2}, HWs[] = {16, 80, 256}, POs[] = {1, 3};
  for (int B : Bs)
    for (int HW : HWs)
      for (int po : POs) {
        const int DPs[] = {po, po + 1, 5};
        for (int dp : DPs) {
          for (int d0 = -1; d0 <= dp; ++d0) {
            const bool ok = fused_slots_ok(po, dp, d0);
            if (B == 1 && HW == 16) std::printf("ok %d %d %d %d\n", po, dp, d0, ok ? 1 : 0);
            if (!ok) continue;
            std::printf("dst %d %d %d %d %d %ld :", B, HW, po, dp, d0, fused_dst_total(B, dp * HW));
            for (long t = 0; t < (long)B * po * HW; ++t) std::printf(" %ld", fused_dst_row(po * HW, dp * HW, d0 * HW, t));
            std::printf("\n");
          }
        }
        const int PIs[] = {po, po + 2};
        for (int pi : PIs) {
          std::printf("src %d %d %d %d :", B, HW, po, pi);
          for (long t = 0; t < (long)B * po * HW; ++t) std::printf(" %ld", fused_src_row(po * HW, pi * HW, (pi - po) * HW, t));
          std::printf("\n");
        }
      }
  std::printf("idn 700 :");
  for (long t = 0; t < 700; ++t) std::printf(" %ld %ld", fused_src_row(0, 5, 7, t), fused_dst_row(0, 5, 7, t));
  std::printf("\n");
  return 0;
}
