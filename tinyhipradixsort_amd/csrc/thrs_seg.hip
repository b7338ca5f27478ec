// thrs_seg.hip -- one key type's segmented-sort kernels and launch sequence
// (thrs_segmented.hpp run_segments), compiled once per key type:
// -DTHRS_SEG_KT=0..3 (U32, U64, F32, F64).
#include "thrs_segmented.hpp"

namespace thrs_host {
template int run_segments<THRS_SEG_KT>(int, void*, void*, uint32_t, const uint32_t*, uint32_t, void*, int, int, bool,
                                       hipStream_t);
}  // namespace thrs_host
