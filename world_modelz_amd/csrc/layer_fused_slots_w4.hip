// The small-workgroup form of layer_fused_slots.hip: 4 waves = 128 tokens per workgroup (twice the workgroups of a decode launch),
// 16 KB weight slabs in a ring of two (4 LDS-DMA pieces per wave and slab, the count the kernel's literal waits are written for).
// A unit of its own.  Measured against the 8-wave form per launch (tools/time_context_cache.py, profiles/context_cache/README.md:
// 23.7 against 34.1 us at 8 clips) and bit-identical to it (tests/test_context_cache_gpu.py): the _slots entry points take it for
// launches of up to 32 eight-wave workgroups, i.e. for every decode step; wmz_debug_fused_slots_waves forces either form.
#define WMZ_FUSED_FW 4
#define WMZ_FUSED_HPS 1
#define WMZ_FUSED_RING 2
#define WMZ_FUSED_SLOTS_UNIT 1
#include "layer_fused.hip"
