// Prints the row map and the issue plan of the 16-wave whole-plane attention forward from csrc/attn_slab_walk.h itself, for
// tests/test_attn_issue_plan_cpu.py to check against the rules restated there.  Lines:
//   row  <wave> <query row>
//   plan <query row> <class or -1> <issues during parity 0> <issues during parity 1> <key rows of parity 0> <key rows of parity 1>
//   voff <piece> <lane> <byte offset>          (the headline layout: dim_head 128, padded rows of 288 bytes, row stride 2, ld 256)
//   step <bytes between the pieces of a class>
#include <cstdio>

#include "../world_modelz_amd/csrc/attn_slab_walk.h"

int main() {
  constexpr int DH = 128, ROWP = DH * 2 + 32, RS = 2;
  static_assert(slab_wave_row(5) == 4 && slab_issue_class(3) == -1, "the plan is usable in constant expressions");
  for (int w = 0; w < 16; ++w) std::printf("row %d %d\n", w, slab_wave_row(w));
  for (int r = 0; r < 16; ++r)
    std::printf("plan %d %d %d %d %d %d\n", r, slab_issue_class(r), (int)slab_issues(r, 0), (int)slab_issues(r, 1),
                slab_rows_of_parity(r, 3, 0), slab_rows_of_parity(r, 3, 1));
  for (int p = 0; p < 36; ++p)
    for (int lane = 0; lane < 64; ++lane) std::printf("voff %d %d %u\n", p, lane, piece_voff<DH, ROWP, RS>(p, lane, 256u, 16 - RS));
  std::printf("step %u\n", SLAB_CLASS_STEP);
  return 0;
}
