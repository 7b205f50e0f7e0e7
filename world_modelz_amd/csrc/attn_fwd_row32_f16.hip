// The attention row kernel for planes 32 wide with IEEE-half MFMA operands (the precise fused inference mode on 32-wide planes);
// the dispatcher of this unit is wmz_attn_fwd_row32_dispatch_f16.
#define WMZ_OP16_F16 1
#define WMZ_ATTN_ROW32 1
#include "attn_fwd_row16.hip"
