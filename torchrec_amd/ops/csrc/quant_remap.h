// Per-id decision of the serving path's bounds check / pruning remap
// (quant_tbe.hip: quant_tbe_remap_indices). Plain C++: no HIP or torch
// header, so a host program can include this file alone and run the very
// code the kernel runs.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TREC_HOST_DEVICE __host__ __device__
#else
#define TREC_HOST_DEVICE
#endif

namespace trec_amd {

// The physical row of logical id `idx` in a table of `logical_rows` ids, or
// -1 where the id is dropped. `remap` is the table's own int32
// [logical_rows] segment (entries in [-1, physical rows)), or nullptr for a
// table that is not pruned. *out_of_range is set for an id outside
// [0, logical_rows) and cleared otherwise; a pruned id (remap entry -1) is
// in range.
//
// The range test is one unsigned compare: a negative idx becomes a value
// >= 2^63, which no row count reaches. There is no subtraction and nothing
// that can overflow for any int64, and remap is read only at an index that
// passed the test.
TREC_HOST_DEVICE inline int64_t quant_remap_id(int64_t idx, int64_t logical_rows,
                                               const int32_t* remap, bool* out_of_range) {
  bool ok = static_cast<uint64_t>(idx) < static_cast<uint64_t>(logical_rows);
  *out_of_range = !ok;
  if (!ok) return -1;
  return remap ? static_cast<int64_t>(remap[idx]) : idx;
}

}  // namespace trec_amd
