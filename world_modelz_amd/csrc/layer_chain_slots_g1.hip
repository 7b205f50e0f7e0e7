// Group 1 of the chain kernels' width triples (chain_widths.h): the context cache's form of the inference launch (include/wmz.h:
// wmz_layer_chain_fwd_slots), bfloat16 unit.  Same source as layer_chain.hip with the destination row map of fused_row_maps.h on the
// q and k | v stores, compiled for the launches that place something (a tail) alone: a unit of its own, so that the code objects of
// layer_chain*.hip hold the kernels they held, unchanged.
#define WMZ_CHAIN_SLOTS_UNIT 1
#define WMZ_CHAIN_GROUP 1
#include "layer_chain.hip"
