// The weight streams of the default-width per-token kernels (layer_fused.hip, layer_fused_bwd.hip), stated once: which blocks a
// stream holds, in which order, with which strides and ownership groups.  The kernels consume 1 KB pieces in exactly this order;
// nothing else in the repository writes it down.  Plain C++ without HIP (tests/fused_pack_rows_host.cpp runs it on the host,
// tests/test_fused_pack_rows_cpu.py holds it against a second statement): wmz_layer_fused_pack / wmz_layer_fused_bwd_pack hand the
// rows to their kernel by value, wmz_fused_pack_rows hands them to fused.PackSet for wmz_fused_pack_table's device table.
#pragma once

// One block of a stream, eleven 64-bit fields (wmz_fused_pack_table's row format, part of the C ABI): element (f, k) of the block
// = w[f * rs + k * ks] (* gamma[k]) (* rgamma[f]); N output features, K contraction length.  gn / gk: ownership groups -- within
// every group of gn output features (gk contraction indices) lane half 0 owns the first half and lane half 1 the second (forward:
// gn = N, gk = K: a lane owns one contiguous half row; the backward kernels use groups of 128, the width of an LDS-staged row tile,
// and of 32 for the hidden axis walked in chunks).  dst: its first 16-bit stream element; start8: its first 8-element group.
struct FusedPackRow { const float* w; long rs, ks, N, K, gn, gk; const float* gamma; const float* rgamma; unsigned short* dst; long start8; };
static_assert(sizeof(FusedPackRow) == 88, "the row format is part of the C ABI");

constexpr int kFusedD = 256, kFusedI = 128, kFusedM = 256, kFusedMC = 32;      // the widths the kernels are built for; MC: hidden chunk
enum { FUSED_STREAM_FWD = 0, FUSED_STREAM_BWD_QKV = 1, FUSED_STREAM_BWD_FF = 2 };   // wmz_fused_pack_rows' kinds: <= 20, 3, 10 rows

struct FusedRowWriter {     // appends blocks to rows[], each behind the one before in the stream and in the launch's group numbering
  FusedPackRow* rows; int n; unsigned short* dst; long start8;
  void add(const float* w, long rs, long ks, long N, long K, long gn, long gk, const float* gamma, const float* rgamma) {
    rows[n++] = FusedPackRow{w, rs, ks, N, K, gn, gk, gamma, rgamma, dst, start8};
    dst += N * K;
    start8 += N * K / 8;
  }
  // [N, K] block of a row-major matrix with leading dimension ld, a lane owning a contiguous half row; gamma scales the columns ...
  void fwd(const float* w, long ld, long N, long K, const float* gamma) { add(w, ld, 1, N, K, N, K, gamma, nullptr); }
  // ... and of the TRANSPOSE of such a matrix: element (f, k) = w[f + k * ld]; rgamma scales the rows
  void bwd(const float* w, long ld, long N, long K, long gn, long gk, const float* rgamma) { add(w, 1, ld, N, K, gn, gk, nullptr, rgamma); }
};

// One function per stream kind: writes the rows of a stream at dst, whose first group is start8 of the launch, and returns their number.
// A forward boundary (layer_fused_kernel).  p: wmz_layer_fused_pack's fourteen parameters -- wout, bout, g2, be2, w1, b1, w2, b2 (the
// head; p[0] == NULL: none), g1, be1, wq, wk, wv, bv (the tail; p[10] == NULL: none).  Head: Wout, then the feed-forward MC hidden
// units at a time with the W1' rows one chunk AHEAD of the W2 columns -- W1[0], W1[1], W2[0], W1[2], W2[1], .., W1[7], W2[6], W2[7]:
// GELU(c) rides under the two stages between W1[c] and W2[c]; tail: Wq, Wk', Wv'.  ' = a LayerNorm weight folded in: g2 (the
// feed-forward's norm) into W1, g1 (the NEXT layer's attention norm) into Wk / Wv.
inline int fused_fwd_rows(FusedPackRow* rows, const float* const* p, unsigned short* dst, long start8) {
  constexpr int D = kFusedD, I = kFusedI, M = kFusedM, MC = kFusedMC;
  const float *wout = p[0], *g2 = p[2], *w1 = p[4], *w2 = p[6], *g1 = p[8], *wq = p[10], *wk = p[11], *wv = p[12];
  FusedRowWriter s{rows, 0, dst, start8};
  if (wout != nullptr) {
    s.fwd(wout, I, D, I, nullptr);
    s.fwd(w1, D, MC, D, g2);                                             // W1[0]
    for (int c = 1; c < M / MC; ++c) {
      s.fwd(w1 + (long)c * MC * D, D, MC, D, g2);                        // W1[c]
      s.fwd(w2 + (c - 1) * MC, M, D, MC, nullptr);                       // W2[:, c-1]
    }
    s.fwd(w2 + (M / MC - 1) * MC, M, D, MC, nullptr);
  }
  if (wq != nullptr) {
    s.fwd(wq, D, I, D, nullptr);
    s.fwd(wk, D, I, D, g1);
    s.fwd(wv, D, I, D, g1);
  }
  return s.n;
}
// A layer's backward streams (layer_fused_bwd.hip), TRANSPOSED blocks in consumption order.  p: wmz_layer_fused_bwd_pack's eight
// parameters -- wq, wk, wv, g1, wout, w1, g2, w2.
//   qkv:  Wk'^T | Wv'^T | Wq^T          ([D x I] each; ' = the attention LayerNorm's gamma folded in: rows scaled)
inline int fused_bwd_qkv_rows(FusedPackRow* rows, const float* const* p, unsigned short* dst, long start8) {
  constexpr int D = kFusedD, I = kFusedI;
  FusedRowWriter s{rows, 0, dst, start8};
  s.bwd(p[1], D, D, I, 128, 128, p[3]);
  s.bwd(p[2], D, D, I, 128, 128, p[3]);
  s.bwd(p[0], D, D, I, 128, 128, nullptr);
  return s.n;
}
//   ff:   W2^T[c] (c = 0 .. M/32-1: [32 x D]) | W1'^T [D x M] | Wout^T [I x D]
inline int fused_bwd_ff_rows(FusedPackRow* rows, const float* const* p, unsigned short* dst, long start8) {
  constexpr int D = kFusedD, I = kFusedI, M = kFusedM;
  const float *wout = p[4], *w1 = p[5], *g2 = p[6], *w2 = p[7];
  FusedRowWriter s{rows, 0, dst, start8};
  for (int c = 0; c < M / 32; ++c) s.bwd(w2 + c * 32, M, 32, D, 32, 128, nullptr);      // dg_c = W2[:, c]^T dy
  s.bwd(w1, D, D, M, 128, 32, g2);                                                      // dxhat = W1'^T dz
  s.bwd(wout, I, I, D, 128, 128, nullptr);                                              // do = Wout^T dx1
  return s.n;
}
// groups of 8 elements in n rows written from start8 on (the stream's length / 8; start8 + this = the next stream's start8)
inline long fused_rows_groups(const FusedPackRow* rows, int n) {
  return n == 0 ? 0 : rows[n - 1].start8 + rows[n - 1].N * rows[n - 1].K / 8 - rows[0].start8;
}
