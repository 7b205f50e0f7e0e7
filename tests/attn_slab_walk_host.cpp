// Host driver of csrc/attn_slab_walk.h (no HIP): prints what the attention row kernels' slab walk does for one geometry, for
// tests/test_attn_slab_walk_cpu.py to check against its own restatement of the rules.
//   attn_slab_walk_host S H eS eHv big|big8|small dh ld heads      (H, eHv in tile rows; ld in elements of 2 bytes)
// Per (form, query plane s, workgroup og):   wg <form> <s> <og> <t_lo> <t_hi> <sk_lo> <sk_hi> <c_first> <nch> <nslab> <p_first>
// and per slab in walking order:             slab <plane> <first row> <min byte> <max byte> <min column byte> <max column byte>
// The bytes are those any lane of any DMA piece of any head fetches, relative to the start of a [S, H, 16, ld] tensor.  Form `clamp` is
// the forward and dq kernels (per-slab row limit unless H is whole chunks), form `whole` the dk | dv plane kernel (H % 16 == 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../world_modelz_amd/csrc/attn_slab_walk.h"

template <int CH, int KC, int NW, int DH, bool CLAMP>
static void run(const char* form, int S, int H, int eS, int eHv, long ld, int heads) {
  constexpr int RS = CH / KC, ROWP = DH * 2 + 32, PIECES = KC * 16 * ROWP / 1024;
  const unsigned ld_b = (unsigned)ld * 2u;
  const bool aligned = H % CH == 0;                      // the kernels' ALIGNED: offsets computed once with the limit CH - RS
  for (int s = 0; s < S; ++s)
    for (int og = 0; og < (H + NW - 1) / NW; ++og) {
      const SlabGeom g = slab_geom<CH, KC, CLAMP>(H, S, eS, eHv, og * NW, NW, s);
      const int p_first = slab_first_plane(g, eS, s);
      std::printf("wg %s %d %d %d %d %d %d %d %d %d %d\n", form, s, og, g.t_lo, g.t_hi, g.sk_lo, g.sk_hi, g.c_first, g.nch, g.nslab, p_first);
      SlabWalk<CH, KC, CLAMP> w(g, p_first);
      long plane = p_first;                               // the caller's "pointer": moved by the walker's deltas only
      for (int j = 0; j < g.nslab; ++j) {
        w.next_state(g);
        const int lim = (CLAMP && !aligned) ? w.dlim : CH - RS;
        const long row0 = (plane * H + w.bsafe) * 16;
        long lo = -1, hi = -1, clo = -1, chi = -1;
        for (int head = 0; head < heads; ++head)
          for (int piece = 0; piece < PIECES; ++piece)
            for (int lane = 0; lane < 64; ++lane) {
              const long off = row0 * ld_b + (long)head * DH * 2 + piece_voff<DH, ROWP, RS>(piece, lane, ld_b, lim);
              const long col = off % ld_b;
              if (lo < 0 || off < lo) lo = off;
              if (off + 15 > hi) hi = off + 15;
              if (clo < 0 || col < clo) clo = col;
              if (col + 15 > chi) chi = col + 15;
            }
        std::printf("slab %ld %d %ld %ld %ld %ld\n", plane, w.base, lo, hi, clo, chi);
        w.advance(g, [&](long d) { plane += d; });
      }
    }
}

template <int CH, int KC, int NW>
static int by_dh(int S, int H, int eS, int eHv, int dh, long ld, int heads) {
  const bool whole = CH == 16 && NW == 16 && H % 16 == 0;
  if (dh == 32) { run<CH, KC, NW, 32, true>("clamp", S, H, eS, eHv, ld, heads); if (whole) run<CH, KC, NW, 32, false>("whole", S, H, eS, eHv, ld, heads); }
  else if (dh == 64) { run<CH, KC, NW, 64, true>("clamp", S, H, eS, eHv, ld, heads); if (whole) run<CH, KC, NW, 64, false>("whole", S, H, eS, eHv, ld, heads); }
  else if (dh == 128) { run<CH, KC, NW, 128, true>("clamp", S, H, eS, eHv, ld, heads); if (whole) run<CH, KC, NW, 128, false>("whole", S, H, eS, eHv, ld, heads); }
  else return 2;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 9) { std::fprintf(stderr, "usage: %s S H eS eHv big|big8|small dh ld heads\n", argv[0]); return 2; }
  const int S = std::atoi(argv[1]), H = std::atoi(argv[2]), eS = std::atoi(argv[3]), eHv = std::atoi(argv[4]);
  const int dh = std::atoi(argv[6]), heads = std::atoi(argv[8]);
  const long ld = std::atol(argv[7]);
  if (S < 1 || H < 1 || eS < 0 || eHv < 0 || heads < 1 || ld < (long)heads * dh) return 2;
  if (!std::strcmp(argv[5], "big")) return by_dh<16, 8, 16>(S, H, eS, eHv, dh, ld, heads);
  if (!std::strcmp(argv[5], "big8")) return by_dh<16, 8, 8>(S, H, eS, eHv, dh, ld, heads);      // backward: 8 waves on 16-row chunks
  if (!std::strcmp(argv[5], "small")) return by_dh<4, 2, 4>(S, H, eS, eHv, dh, ld, heads);
  return 2;
}
