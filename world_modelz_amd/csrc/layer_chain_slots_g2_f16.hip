// Group 2 of the chain kernels' width triples (chain_widths.h): the context cache's form of the inference launch with IEEE-half
// operands (include/wmz.h: wmz_layer_chain_fwd_f16_slots; precise mode).  layer_chain_slots_g2.hip with the unit's 16-bit format switched.
#define WMZ_OP16_F16 1
#define WMZ_HALF_GUARD 1      // this unit carries the half guard (wmz_common.h HalfGuard)
#define WMZ_CHAIN_SLOTS_UNIT 1
#define WMZ_CHAIN_GROUP 2
#include "layer_chain.hip"
