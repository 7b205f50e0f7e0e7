// Host driver of the asymmetric slab walk of csrc/attn_slab_walk.h (no HIP), for tests/test_causal_window_cpu.py.  For every clip
// length S <= 6, every time window (b, f) with b, f <= 4, every query plane s and every workgroup og of a plane of H tile rows it
// prints the walk of the overloads that take (eSb, eSf):
//   wg <form> <H> <S> <b> <f> <s> <og> <sk_lo> <sk_hi> <nch> <nslab> <p_first> <same>
//   slab <plane> <first row>                (one per slab, in walking order)
// <same>: for b == f, whether the overloads that take one eS give the same SlabGeom, field for field, and the same first plane
// (1 / 0); -1 where b != f.  Forms as in attn_slab_walk_host.cpp: `clamp` the forward and dq kernels, `whole` the dk | dv plane kernel.
//   causal_window_host H eHv big|small
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../world_modelz_amd/csrc/attn_slab_walk.h"

static bool same_geom(const SlabGeom& a, const SlabGeom& b) {
  return a.H == b.H && a.s_last == b.s_last && a.t_lo == b.t_lo && a.t_hi == b.t_hi && a.sk_lo == b.sk_lo && a.sk_hi == b.sk_hi &&
         a.c_first == b.c_first && a.nch == b.nch && a.nslab == b.nslab;
}

template <int CH, int KC, int NW, bool CLAMP>
static void run(const char* form, int H, int eHv) {
  for (int S = 1; S <= 6; ++S)
    for (int b = 0; b <= 4; ++b)
      for (int f = 0; f <= 4; ++f)
        for (int s = 0; s < S; ++s)
          for (int og = 0; og < (H + NW - 1) / NW; ++og) {
            const SlabGeom g = slab_geom<CH, KC, CLAMP>(H, S, b, f, eHv, og * NW, NW, s);
            const int p_first = slab_first_plane(g, b, f, s);
            int same = -1;
            if (b == f) {
              const SlabGeom g1 = slab_geom<CH, KC, CLAMP>(H, S, b, eHv, og * NW, NW, s);
              same = same_geom(g, g1) && slab_first_plane(g1, b, s) == p_first;
            }
            std::printf("wg %s %d %d %d %d %d %d %d %d %d %d %d %d\n", form, H, S, b, f, s, og, g.sk_lo, g.sk_hi, g.nch, g.nslab, p_first, same);
            SlabWalk<CH, KC, CLAMP> w(g, p_first);
            long plane = p_first;
            for (int j = 0; j < g.nslab; ++j) {
              w.next_state(g);
              std::printf("slab %ld %d\n", plane, w.base);
              w.advance(g, [&](long d) { plane += d; });
            }
          }
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s H eHv big|small\n", argv[0]); return 2; }
  const int H = std::atoi(argv[1]), eHv = std::atoi(argv[2]);
  if (H < 1 || eHv < 0) return 2;
  if (!std::strcmp(argv[3], "big")) {
    run<16, 8, 16, true>("clamp", H, eHv);
    if (H % 16 == 0) run<16, 8, 16, false>("whole", H, eHv);
    return 0;
  }
  if (!std::strcmp(argv[3], "small")) { run<4, 2, 4, true>("clamp", H, eHv); return 0; }
  return 2;
}
