// The tile-major "quad" operator format: what its builders (tiled_build.hip) and its sweeps (spmm_tiled.hip, spmm_dq.hip)
// share.  Internal to those three files; spmm_tiled.hip's header describes the format, DESIGN.md §5 has the measurements.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sapca {
namespace k {

// Steps of a quad in a tile = its longest row segment: a quad may end on any step (round 4; the generated main loop counts
// per step, tools/gen_spmm_dq2.py DQ2_ODD=1).  -DSAPCA_EVEN_STEPS brings back the format of rounds 2-3, which rounded a quad's
// steps up to an even count (3.8 % more executed slots at C2, 10 % more at C5's 3.2 entries per row and tile) for a counter
// per two-step group; the main loop must then be generated with DQ2_ODD=0.  Measured same-box (profiles/r04_ab_odd_*.txt):
// C2 sweep -1.4 %, C5 sweep -3.4 % and preparation -5 %, C4 -0.1 %.
#ifdef SAPCA_EVEN_STEPS
constexpr bool kOddSteps = false;
#else
constexpr bool kOddSteps = true;
#endif

// (an unnamed namespace in a header: every including file gets its own copy, and the kernels that take an Ent keep the
// file-local names they had when these definitions stood in spmm_tiled.hip)
namespace {

constexpr int WAVE = 64;
constexpr int LDS_TOTAL = 160 * 1024;

struct Ent { uint32_t off; float val; };
struct EntD { uint32_t off; uint32_t pad; double val; };   // the same entry for f64 values (16 bytes)
template <typename VT> struct EntOf { typedef Ent type; };
template <> struct EntOf<double> { typedef EntD type; };

inline int grid_for(int64_t work_items, int block, int cap = 8192) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

#ifndef SAPCA_QWAVES
#define SAPCA_QWAVES 16   // waves per workgroup of the quad sweep: 16 x 8 quads, or 8 x 16 quads with 8-step batches
#endif
constexpr int QGROUPS = 4, QLANES = WAVE / QGROUPS, QWAVES = SAPCA_QWAVES, QTHREADS = QWAVES * WAVE;
constexpr int Q_TILE_BYTES = 80 * 1024;          // default split of the 160 KiB: 80 KiB panel tile + 79 KiB entry staging
constexpr int Q_MAX_TILES_RUNS = 16384;          // tile-major builder (bounded by the tile arithmetic's float reciprocal and the index tables' size)
constexpr int q_stage_bytes(int tile_bytes) { return LDS_TOTAL - tile_bytes - 1024; }
// most entries of one (row block, tile) the staged-entry sweep can stage beside a panel tile of `tile_bytes`
constexpr int q_stage_cap(int tile_bytes, int entry_bytes) { return q_stage_bytes(tile_bytes) / entry_bytes - WAVE; }
// panel rows of one column tile, for panel rows of `ldp` floats (an f64 panel of 64 columns: 128)
constexpr int q_tile_rows(int ldp) { return Q_TILE_BYTES / (ldp * 4); }
constexpr int QBLOCK_ROWS = 1024;                // most rows of a quad-format block (the DPP-fed sweep with 16 row slots per lane group)
constexpr int Q_BLOCK_QUADS = QBLOCK_ROWS / 4;   // stride of the per-chunk quad step table
constexpr int ENT_SLACK = 4 * WAVE;             // zero entries behind the last chunk: the sweeps read whole 16-step chunks (and three ahead)
constexpr int q_rows_per_group(int ldp) { return (ldp == 64 ? 128 : 64) / QWAVES; }
// steps of a quad in a tile: its longest row segment, rounded up to an even count (the DPP-fed sweep of spmm_dq.hip
// switches row slots every two steps)
__host__ __device__ inline int q_steps(int longest) { return kOddSteps ? longest : (longest + 1) & ~1; }
// quads (4 consecutive rows) of a block are dealt to its 16 waves in contiguous, balanced ranges
__host__ __device__ inline int q_first(int wave, int nquads) { return wave * nquads / QWAVES; }

}  // namespace

}  // namespace k
}  // namespace sapca
