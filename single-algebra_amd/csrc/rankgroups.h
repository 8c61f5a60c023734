// The length classes of the rank pass (rankgroups.hip; sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_*).
// A column of A -- a row of A^T -- is classed by its STORED length, before excluded rows and stored zeros are dropped:
//   length <= kRankWaveMax               one wave sorts it in its own LDS, four columns per workgroup;
//   kRankWaveMax < length <= kRankLdsMax  one 256-thread workgroup sorts it in LDS (bitonic);
//   longer                               its keys are sorted in global scratch (rocPRIM's segmented radix sort over the long
//                                        columns only), then one workgroup per column walks the sorted segment
//                                        kRankWalkChunk positions at a time.
// The LDS of a workgroup at 1,024 groups (8 + 4 bytes of counters per group and column in flight, 8 bytes per thread for the
// tie sums, keys of 4 / 8 bytes and 2-byte labels): wave class 4 x (12,288 + 512 + 16 + 256 x 6 / 10) = 57,408 / 61,504 bytes,
// workgroup class 12,288 + 2,048 + 16 + 4,096 x 6 / 10 = 38,928 / 55,312 bytes: below 64 KiB, two workgroups per CU.
#pragma once
#include <cstdint>

namespace sapca {
namespace k {

constexpr int kRankWaveMax = 256;
constexpr int kRankLdsMax = 4096;
constexpr int kRankWalkChunk = 256;
// most entries one segmented sort takes: the long columns go through the scratch in batches of whole columns (a column
// longer than this is a batch of its own; a column has fewer than 2^31 entries)
constexpr int64_t kRankLongBatch = (int64_t)1 << 26;

}  // namespace k
}  // namespace sapca
