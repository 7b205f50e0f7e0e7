// The context cache's forms of the fused per-token launches (include/wmz.h: wmz_layer_fused_fwd_slots,
// wmz_embed_qkv_fused_fwd_slots): the kernel body of layer_fused.hip under the option policy OptSlots -- q and k | v leave through
// the destination row map of fused_row_maps.h, into plane slots of buffers that hold more planes than the launch computes.  Same
// source as layer_fused.hip, compiled for these entry points alone: a unit of its own, so that the code objects of layer_fused.hip
// and layer_fused_f16.hip hold the kernels they held, unchanged.
#define WMZ_FUSED_SLOTS_UNIT 1
#include "layer_fused.hip"
