// The attention row kernel for planes 32 wide (the W32 mode of attn_fwd_row16.hip), bfloat16 operands: a unit of its own, so that
// attn_fwd_row16.hip keeps exactly its kernels; the dispatcher of this unit is wmz_attn_fwd_row32_dispatch.
#define WMZ_ATTN_ROW32 1
#include "attn_fwd_row16.hip"
