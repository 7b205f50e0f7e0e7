// Embedding widths the screened nearest-code search (vq_screen.hip) is instantiated for; any codebook size C >= 1.
// The templates need E % 16 == 0 (whole 16-wide MFMA k-steps and whole 8-lane vectors of the pinned order); a width costs three
// kernels.  The table is the reference's default (train_vqae.py --embedding_dim 64), its power-of-two neighbours, and the 16-wide
// slices of a num_latents > 1 quantiser.  Every other width takes the full scan (wmz_vq_argmin).
#pragma once

#define WMZ_VQ_SCREEN_WIDTHS(X) X(16) X(32) X(64) X(128) X(256)
