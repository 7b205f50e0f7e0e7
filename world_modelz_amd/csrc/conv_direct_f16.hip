// The direct 3x3 convolution forward (stride 1 and 2) of the conv encoder / decoder with IEEE-half MFMA operands and a half output:
// the precise mode's conv route (include/wmz.h: wmz_conv3x3_direct_fwd_strided_f16).  Same source as conv_direct.hip with the
// translation unit's 16-bit operand format switched (wmz_common.h); the weight pack and the support queries are the bfloat16 unit's.
#define WMZ_OP16_F16 1
#define WMZ_HALF_GUARD 1      // this unit carries the half guard (wmz_common.h HalfGuard)
#include "conv_direct.hip"
