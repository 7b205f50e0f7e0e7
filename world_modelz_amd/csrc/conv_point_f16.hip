// The small-K convolutions (1x1 with and without the BatchNorm prologue, 2x2 / stride 2, the 3-channel conv_1) of the conv encoder /
// decoder with IEEE-half MFMA operands and a half output: the precise mode's conv route (include/wmz.h: wmz_conv_point_fwd_bn_f16).
// Same source as conv_point.hip with the translation unit's 16-bit operand format switched (wmz_common.h); the weight pack, the
// support query and wmz_nchw_to_nhwc8 are the bfloat16 unit's.
#define WMZ_OP16_F16 1
#define WMZ_HALF_GUARD 1      // this unit carries the half guard (wmz_common.h HalfGuard)
#include "conv_point.hip"
