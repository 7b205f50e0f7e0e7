// layer_fused_slots_w4.hip with IEEE-half operands (the precise mode); carries the half guard like layer_fused_f16.hip.
#define WMZ_OP16_F16 1
#define WMZ_HALF_GUARD 1
#define WMZ_FUSED_FW 4
#define WMZ_FUSED_HPS 1
#define WMZ_FUSED_RING 2
#define WMZ_FUSED_SLOTS_UNIT 1
#include "layer_fused.hip"
