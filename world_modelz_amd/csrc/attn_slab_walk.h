// The slab walk of the attention row kernels (attn_fwd_row16.hip and both kernels of attn_bwd_row16.hip), stated once: which key /
// visitor rows a workgroup stages, in which order, and which bytes a lane's LDS-DMA pieces fetch.  Plain integer code without HIP
// and without pointers (a caller keeps its own and moves them by the walker's plane deltas): tests/attn_slab_walk_host.cpp runs it on
// the host and tests/test_attn_slab_walk_cpu.py says what it promises.  The kernels take piece_voff from here; the geometry and the
// walker they still write out by hand, expression for expression as below (with the walker in their place every row kernel compiled
// to other scalar code: profiles/attn_slab_walk/README.md) -- a change to the walk is made here first, under the test, then there.
#pragma once
#ifdef __HIPCC__
#define WMZ_HD __host__ __device__ __forceinline__
#else
#define WMZ_HD inline
#endif

WMZ_HD int slab_min(int a, int b) { return a < b ? a : b; }
WMZ_HD int slab_max(int a, int b) { return a > b ? a : b; }
constexpr int slab_log2(int n) { return n <= 1 ? 0 : 1 + slab_log2(n >> 1); }

// What a workgroup (NW owner rows from h0, query / owner plane s) stages: rows [t_lo, t_hi] of the planes [sk_lo, sk_hi], i.e.
// nch slabs per plane from chunk c_first on, nslab in all.
struct SlabGeom { int H, s_last, t_lo, t_hi, sk_lo, sk_hi, c_first, nch, nslab; };      // (s_last = S - 1)

// Key planes are walked in a ROTATED order: at its t-th plane every workgroup reads the plane p = t (mod 2 eS + 1) of its
// window, so the 2 eS + 1 workgroups that need plane p (query planes p - eS .. p + eS, one per CU of the same XCD, started
// together and in step) stage it at the same time: one of them misses in L2, the others hit.  Walking s - eS .. s + eS in
// order instead, a plane is read at 2 eS + 1 different times and has left the 4 MiB L2 (the clip's K / V alone fill it) in
// between.  The softmax is order-independent (online), the logits probe records the plane it actually visits.
// (The phase counts planes from the END of the clip: the trailing-planes entry point hands over only the last planes of a
// clip, and its visiting order -- hence every rounding -- must be the full grid's.)
// The time window is a pair: the owner plane s sees the planes s - eSb .. s + eSf (symmetric: eSb == eSf == eS; causal: eSf == 0;
// the dk | dv role, whose owners are keys, takes the swapped pair).  Its eSb + eSf + 1 planes rotate as above, by that length.
WMZ_HD int slab_first_plane(const SlabGeom& g, int eSb, int eSf, int s) {
  const int nwin = eSb + eSf + 1;
  int p_first = s - eSb;
  { const int a = (((g.s_last - p_first) % nwin) + nwin) % nwin; p_first += a; }         // first plane of the window with S-1-p = 0 (mod nwin)
  if (p_first > g.sk_hi || p_first < g.sk_lo) p_first = g.sk_lo;
  return p_first;
}
WMZ_HD int slab_first_plane(const SlabGeom& g, int eS, int s) { return slab_first_plane(g, eS, eS, s); }

// A plane is cut into chunks of CH rows, a slab holds every RS-th row of a chunk (KC = CH / RS rows: plane row = base + RS * slab
// row).  eHv: the window's row extent in tile rows.  CLAMP = false is the whole-plane form (H % CH == 0 and NW == CH: no owner row
// and no slab row lies past the plane), which carries none of the clamps.  (The inner min of t_hi changes no value -- both forms
// give min(h0 + NW - 1 + eHv, H - 1) -- and dlim stays CH - RS without CLAMP: they are the kernels' own expressions, kept so that
// this code and theirs can be held side by side.)
template <int CH, int KC, bool CLAMP = true>
WMZ_HD SlabGeom slab_geom(int H, int S, int eSb, int eSf, int eHv, int h0, int NW, int s) {
  constexpr int RS = CH / KC, LOG_CH = slab_log2(CH);
  static_assert(KC * RS == CH && (1 << LOG_CH) == CH && (1 << slab_log2(RS)) == RS, "a slab is one phase of a chunk of 2^n rows");
  SlabGeom g;
  g.H = H;
  g.t_lo = slab_max(h0 - eHv, 0);
  g.t_hi = slab_min((CLAMP ? slab_min(h0 + NW - 1, H - 1) : h0 + NW - 1) + eHv, H - 1);
  g.sk_lo = slab_max(0, s - eSb); g.s_last = S - 1; g.sk_hi = slab_min(g.s_last, s + eSf);
  g.c_first = g.t_lo >> LOG_CH;
  g.nch = ((g.t_hi >> LOG_CH) - g.c_first + 1) * RS;        // slabs per plane: (chunk) x (row phase)
  g.nslab = (g.sk_hi - g.sk_lo + 1) * g.nch;
  return g;
}
template <int CH, int KC, bool CLAMP = true>
WMZ_HD SlabGeom slab_geom(int H, int S, int eS, int eHv, int h0, int NW, int s) { return slab_geom<CH, KC, CLAMP>(H, S, eS, eS, eHv, h0, NW, s); }

// The slab being prefetched: plane (from sk_lo), slab in the plane, first row, index; and where its DMA may read: bsafe, the
// row the fetch starts from, and dlim, the last row offset piece_voff may add to it.
template <int CH, int KC, bool CLAMP = true> struct SlabWalk {
  static constexpr int RS = CH / KC, LOG_RS = slab_log2(RS), LOG_CH = slab_log2(CH);
  int pl, rem = 0, base = 0, j = 0, bsafe = 0, dlim = CH - RS;
  WMZ_HD SlabWalk(const SlabGeom& g, int p_first) : pl(p_first - g.sk_lo) {}
  WMZ_HD void next_state(const SlabGeom& g) {                                // descriptors of slab (pl, rem)
    base = ((g.c_first + (rem >> LOG_RS)) << LOG_CH) + (rem & (RS - 1));
    // (a one-row plane has no row of phase 1: that slab -- which no wave reads -- is fetched from the last row instead of from
    //  behind the plane; found by tools/guard_overread.py: a read past the end of the K / V tensor for H = 1)
    bsafe = CLAMP ? slab_min(base, g.H - 1) : base;
    if (CLAMP) dlim = slab_max(g.H - 1 - base, 0);
  }
  // step (pl, rem) to the following slab; move_planes(d) moves the caller's plane pointers by d planes: +1, or back to the
  // window's first plane behind its last
  template <typename Move> WMZ_HD void advance(const SlabGeom& g, Move move_planes) {
    ++j;
    if (++rem == g.nch) {
      rem = 0;
      if (g.sk_lo + pl == g.sk_hi) { move_planes(-(long)pl); pl = 0; }
      else { ++pl; move_planes(1); }
    }
  }
};

// ---- Planes 32 wide.  A plane [H, 32] IS a plane [2H, 16] in memory, and is handed to the row kernels as 2H tile rows of 16: token
// (h, w) sits in tile row R = 2h + (w >> 4), tile column c = w & 15, and a = R & 1 says which column half the tile row is.  Staging,
// fragments, clamps and piece_voff are those of the 16-wide plane of 2H rows; only the window is stated in tile coordinates:
//   rows     an owner of tile row R visits the tile rows [R - a - 2 eH, R - a + 2 eH + 1] (both halves of the plane rows h - eH ..
//            h + eH), clipped to the plane by the caller;
//   columns  (R, c) sees (R', c') iff |16 ((R' & 1) - a) + c' - c| <= eW: the 16-wide mask against a row of the owner's half, the
//            seam mask against a row of the other half.  A slab holds ONE row parity (RS = 2), so which of the two applies is
//            uniform per wave and slab;
//   slot     the pair sits at dh = (R' - R + a - a') / 2 (the numerator is even), dw = 16 (a' - a) + c' - c of the window.
// tests/test_attn_32_wide_cpu.py checks all three against the plain rule |h' - h| <= eH and |w' - w| <= eW.
WMZ_HD int w32_row_lo(int R, int eH) { return R - (R & 1) - 2 * eH; }
WMZ_HD int w32_row_hi(int R, int eH) { return R - (R & 1) + 2 * eH + 1; }
WMZ_HD int w32_dw(int R, int c, int Rk, int ck) { return 16 * ((Rk & 1) - (R & 1)) + ck - c; }
WMZ_HD int w32_dh(int R, int Rk) { return (Rk - R + (R & 1) - (Rk & 1)) / 2; }
WMZ_HD bool w32_col_ok(int R, int c, int Rk, int ck, int eW) { const int d = w32_dw(R, c, Rk, ck); return d <= eW && -d <= eW; }
// What slab_geom takes as eHv in this mode.  A workgroup starts on an even tile row and owns an even number of them (NW is 4 or 16,
// and the plane has 2H tile rows), so its first owner is a left half (reaching down to h0 - 2 eH) and its last one a right half
// (reaching up to itself + 2 eH): the symmetric extent 2 eH covers every owner's rows; 2 eH + 1 would only stage one row more.
WMZ_HD int w32_stage_extent(int eH) { return 2 * eH; }

// ---- The whole-plane forward with one wave per query row (16 waves, H = 16, row extent 3, two parity slabs of 8 rows a plane:
// attn_fwd_row16_infer.hip).  Which wave owns which query row, and which wave requests which DMA pieces of the next slab, enter no
// result; they decide who waits for whom at the slab's barrier.  tests/attn_issue_plan_host.cpp checks what is promised here.
//
// Row map.  Waves w, w + 4, w + 8, w + 12 share a SIMD.  A query row's window holds 2, 3 or 4 key rows of a parity slab; with row =
// wave the four SIMDs carry 11, 14, 11, 14 key rows of the even slab (14, 11, 14, 11 of the odd one).  Swapping the two waves of a
// pair in every second group of four gives 12, 13, 12, 13 in both slabs -- in steps (two rows a step, an odd row half a step) 6,
// 6.5, 6, 6.5 of 25, and since the sums are multiples of a half no map does better than 6.5.
constexpr int slab_wave_row(int wave) { return wave ^ ((wave >> 2) & 1); }
// key rows of parity `par` in the window [row - eH, row + eH] of a plane of H rows
constexpr int slab_rows_of_parity(int row, int eH, int par, int H = 16) {
  const int lo = row - eH > 0 ? row - eH : 0, hi = row + eH < H - 1 ? row + eH : H - 1;
  return (hi - par + 2) / 2 - (lo - par + 1) / 2;
}
// Issue plan.  The 36 one-KB pieces of a slab image fall into 9 classes mod 9; nine pieces are 32 padded rows = two slab rows, so
// the pieces c, c + 9, c + 18, c + 27 of a class are fetched from one per-lane offset plus 0, 1, 2, 3 times SLAB_CLASS_STEP (see
// piece_voff) and land 9 KB apart.  While the slab of parity P is computed, class c of the K and of the V image of the NEXT slab is
// requested by the one wave whose row has slab_issue_class(row) == c and fewer than four key rows in P: rows 0 .. 2 and 13 .. 15
// (never four rows) serve both parities, rows 4, 6, 8 (three even rows) and 11, 9, 7 (three odd rows) one each, rows 3, 5, 10, 12
// none.  A row keeps ONE class, hence one offset register, whichever parity it serves.
constexpr unsigned SLAB_CLASS_STEP = 16384u;
constexpr int slab_issue_class(int row) {
  return row <= 2 ? row : row >= 13 ? row - 10 : (row == 4 || row == 11) ? 6 : (row == 6 || row == 9) ? 7 : (row == 7 || row == 8) ? 8 : -1;
}
constexpr bool slab_issues(int row, int par) { return slab_issue_class(row) >= 0 && slab_rows_of_parity(row, 3, par) < 4; }

// Byte offset (inside a plane, relative to plane row `base`) of the 16 bytes this lane fetches for DMA piece `piece` of a padded
// image (rows of ROWP bytes): the lane landing on (slab row, 16-byte chunk) fetches that chunk of plane row base + RS * (slab row
// / 16), column slab row % 16; pad chunks fetch chunk 0 (never read).  `row_lim`: rows past the plane are redirected to the last
// valid one (never read either).
template <int DH, int ROWP, int RS>
WMZ_HD unsigned piece_voff(int piece, int lane, unsigned ld_bytes, int row_lim) {
  const int off = piece * 1024 + lane * 16;
  const int r = off / ROWP;
  int c = (off - r * ROWP) >> 4;
  c = c < DH / 8 ? c : 0;
  const int prow = slab_min(RS * (r >> 4), row_lim);
  return (unsigned)((prow << 4) + (r & 15)) * ld_bytes + (unsigned)c * 16u;
}
