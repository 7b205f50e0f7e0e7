// Development probes of libwmz_hip.so: process-wide switches for kernel timing experiments (tools/), NOT part of the product
// interface (include/wmz.h) -- production callers never touch them, and with all of them at their defaults (NULL / 0) the library
// has no global state.
#pragma once
#ifdef __cplusplus
extern "C" {
#endif

/* Kernel-development probe: workgroup 0 of the fused layer kernel writes the shader clock at its stage boundaries into
 * buf (device, 8 waves x 64 int64); NULL (default) switches the probe off. */
int wmz_debug_fused_timestamps(void* buf);
/* Ablation switches of the fused per-token kernel (timing experiments only, results are garbage): 1 = skip the MFMA loops,
 * 2 = skip the weight DMA and its waits, 4 = skip the per-slab workgroup barrier (bits combine); 8 = keep the run-time kernel where
 * the inference unit (layer_fused_infer_kernel) would run -- same results, A/B timing and tests; 0 = product behaviour. */
int wmz_debug_fused_knobs(int dbg);
/* Waves per workgroup of the context cache's per-token launches (wmz_layer_fused_fwd_slots, wmz_embed_qkv_fused_fwd_slots and
 * their half forms): 4 = the small-workgroup build (csrc/layer_fused_slots_w4.hip: 128 tokens per workgroup), 8 = the 256-token
 * build, whatever the launch's size; 0 = the product rule (4 waves up to 8192 tokens per launch, else 8).  Same results bit for
 * bit; A/B timing and tests. */
int wmz_debug_fused_slots_waves(int waves);
/* Same for the 16-wide-plane attention forward kernel (16 waves x 64 int64). */
int wmz_debug_attn_timestamps(void* buf);
/* development knobs of the attention forward: dbg = ablation switches (1 skip the per-tile compute, 2 skip the K/V
 * staging: timing experiments only, results are garbage), variant = reserved (the library carries one instantiation per
 * shape class; other schedules are separate builds, tools/build_variant.py); (0, 0) is the product behaviour. */
int wmz_debug_attn_knobs(int dbg, int variant);

/* development knobs of the direct convolution (csrc/conv_direct.hip): skew = start delay (units of s_sleep 127) of the second
 * workgroup per CU; dbg = ablation switches (1 skip the epilogue, 2 one weight slab only: timing experiments, results are garbage). */
int wmz_debug_conv_knobs(int skew, int dbg);

/* development knob of the nn.Linear kernel (csrc/linear_fwd.hip): dma = 0 runs the small-M GEMMs on the register-staged K loop
 * instead of the LDS-DMA ring (A/B timing; same results). */
int wmz_debug_linear_knobs(int dma);
/* Which instantiation of the nn.Linear kernel a problem takes (kernel-level tests name the tile they cover through this): the
 * host-side decision of the launch itself, asked without launching anything or touching a device -- A and Wt are looked at as
 * addresses only (their alignment decides the K loop).  prologue: 0 none, 1 LayerNorm, 2 GELU-in; block_stride: 0, or the block
 * stride of wmz_linear_fwd_blocked; dtype: WMZ_F32 / WMZ_BF16 / WMZ_F16.  Returns the row-tile height (64 or 128), plus 256 when
 * the K loop is the LDS-DMA ring; the wmz_debug_linear_knobs setting counts for bf16. */
int wmz_debug_linear_route(const void* A, long lda, const void* Wt, long block_stride, int M, int N, int K, int prologue,
                           int out_f32, int dtype);

/* Timeline probe for captured steps: one thread writes the device's constant-rate wall clock (wall_clock64: 100 MHz) into
 * buf[slot] (device int64) when the launch executes on `stream` -- a marker between the phases of a hipGraph replay, where a
 * profiler's own per-node cost (rocprofv3 --kernel-trace: ~9 us a node) would distort the very overlap under study. */
int wmz_debug_stamp(void* buf, int slot, void* stream);

/* In-kernel stage stamps of the direct convolution (csrc/conv_direct.hip, built with -DWMZ_CONV_STAMPS) and of the 256-wide
 * weight-gradient kernel (csrc/linear_bwd.hip, -DWMZ_W3_STAMPS): copies the n 64-bit words the last launch left into the HOST
 * array out.  Exported by such builds only (tools/build_variant.py, tools/conv_stamps.py). */
int wmz_debug_conv_stamps(unsigned long long* out, int n);
int wmz_debug_w3_stamps(unsigned long long* out, int n);
/* Likewise the per-wave slab stamps of the attention forward's inference unit (csrc/attn_fwd_row16_infer.hip, built with
 * -DWMZ_ATTN_INFER_TS; 16 waves x 64 words in the slot layout of wmz_debug_attn_timestamps; tools/ts_attn.py). */
int wmz_debug_attn_infer_stamps(unsigned long long* out, int n);

#ifdef __cplusplus
}
#endif
