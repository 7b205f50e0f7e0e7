// Host driver of the 32-wide window law of csrc/attn_slab_walk.h (w32_*; no HIP), for tests/test_attn_32_wide_cpu.py.
//   attn_32_wide_host law H eH eW
//     every (query, key) pair of a [H, 32] plane that the law admits -- the key's tile row inside the owner's visited rows (clipped to
//     the plane's 2H tile rows) and the column rule true --, one line each:   <query token> <key token> <dh> <dw>
//     (token = 32 h + w = 16 R + c, the same number in both views; dh, dw: the window slot computed from TILE coordinates)
//   attn_32_wide_host walk H eH big|small
//     per workgroup of the [2H, 16] view:   wg <og>
//     the valid rows its slab walk stages with the 32-wide staging extent, and with the 16-wide walk's extent 2 eH + 1:
//                                           stage32 <row> ...      stage16 <row> ...
//     and per owner row of the workgroup its visited rows, clipped:       owner <R> <lo> <hi>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../world_modelz_amd/csrc/attn_slab_walk.h"

static int law(int H, int eH, int eW) {
  const int Ht = 2 * H;
  for (int R = 0; R < Ht; ++R)
    for (int c = 0; c < 16; ++c) {
      const int lo = slab_max(w32_row_lo(R, eH), 0), hi = slab_min(w32_row_hi(R, eH), Ht - 1);
      for (int Rk = lo; Rk <= hi; ++Rk)
        for (int ck = 0; ck < 16; ++ck)
          if (w32_col_ok(R, c, Rk, ck, eW)) std::printf("%d %d %d %d\n", 16 * R + c, 16 * Rk + ck, w32_dh(R, Rk), w32_dw(R, c, Rk, ck));
    }
  return 0;
}

template <int CH, int KC>
static std::set<int> staged(int Ht, int eHv, int h0, int NW) {
  constexpr int RS = CH / KC;
  const SlabGeom g = slab_geom<CH, KC>(Ht, 1, 0, eHv, h0, NW, 0);
  SlabWalk<CH, KC> w(g, slab_first_plane(g, 0, 0));
  std::set<int> rows;
  for (int j = 0; j < g.nslab; ++j) {
    w.next_state(g);
    for (int r = 0; r < KC; ++r)
      if (w.base + RS * r < Ht) rows.insert(w.base + RS * r);
    w.advance(g, [](long) {});
  }
  return rows;
}

template <int CH, int KC, int NW>
static int walk(int H, int eH) {
  const int Ht = 2 * H;
  for (int og = 0; og < (Ht + NW - 1) / NW; ++og) {
    std::printf("wg %d\n", og);
    std::printf("stage32");
    for (int r : staged<CH, KC>(Ht, w32_stage_extent(eH), og * NW, NW)) std::printf(" %d", r);
    std::printf("\nstage16");
    for (int r : staged<CH, KC>(Ht, 2 * eH + 1, og * NW, NW)) std::printf(" %d", r);
    std::printf("\n");
    for (int R = og * NW; R < slab_min(og * NW + NW, Ht); ++R)
      std::printf("owner %d %d %d\n", R, slab_max(w32_row_lo(R, eH), 0), slab_min(w32_row_hi(R, eH), Ht - 1));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "law")) return law(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  if (argc == 5 && !std::strcmp(argv[1], "walk")) {
    const int H = std::atoi(argv[2]), eH = std::atoi(argv[3]);
    if (!std::strcmp(argv[4], "big")) return walk<16, 8, 16>(H, eH);
    if (!std::strcmp(argv[4], "small")) return walk<4, 2, 4>(H, eH);
  }
  std::fprintf(stderr, "usage: %s law H eH eW | walk H eH big|small\n", argv[0]);
  return 2;
}
