// ldb_strset.h — the string-set scan (ldb_strset.hip) and its seam with the scan operator (ldb_scan.hip).  Host only.
#pragma once
#include "ldb_internal.h"
#include <functional>

// constants whose keys and lengths a workgroup stages in LDS; a longer list is searched in global memory (derivation: ldb_strset.hip)
#define LDB_STRSET_LDS_MAX 5376

// is this conjunct evaluated by the string-set kernel?  A utf8 column without a dictionary and an IN list of more than LDB_MAX_IN constants,
// of at least `scan_strset_min_in` constants (option, default LDB_MAX_IN + 1) or of more bytes than DPred::in_blob holds — or a comparison with
// a constant longer than LDB_STR_INLINE.  Everything else keeps the inline descriptor (ldb_make_dpred).
bool ldb_strset_wanted(const ldb_rel* r, const ldb_filter_desc* p);
bool ldb_strset_any(const ldb_rel* r, const ldb_filter_desc* preds, int32_t n_preds);
// one such conjunct over the logical rows of `in` (not lazy) → ascending row numbers (device, owned by the caller)
int32_t ldb_strset_run(ldb_ctx* ctx, ldb_rel* in, const ldb_filter_desc* p, uint32_t** sel_out, uint64_t* total_out);
// scan_run_with for a kernel of another unit: launch(bitmap, block_counts, n_blocks, parts) writes the ballot words and the per-part counts
using ldb_scan_launch = std::function<int32_t(uint64_t*, uint32_t*, unsigned, unsigned)>;
int32_t ldb_scan_run_launch(ldb_ctx* ctx, int64_t n, const ldb_scan_launch& launch, uint32_t** sel_out, uint64_t* total_out);
