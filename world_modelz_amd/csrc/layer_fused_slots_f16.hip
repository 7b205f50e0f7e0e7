// layer_fused_slots.hip with IEEE-half MFMA operands and a half residual stream: the precise mode's context cache
// (wmz_layer_fused_fwd_f16_slots, wmz_embed_qkv_fused_fwd_f16_slots).  Carries the half guard like layer_fused_f16.hip.
#define WMZ_OP16_F16 1
#define WMZ_HALF_GUARD 1
#define WMZ_FUSED_SLOTS_UNIT 1
#include "layer_fused.hip"
