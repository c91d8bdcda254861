// decode_splitkv_kernel's PACK = 4 instantiations - multi-token decode steps on four column groups: 64 / G query tokens of a
// sequence in a wave's 64 matrix columns - as a translation unit of their own (see launch_decode_pack4 in decode_splitkv.hip).
#define DECODE_TU 2
#include "decode_splitkv.hip"
