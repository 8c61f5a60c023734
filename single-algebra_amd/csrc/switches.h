// Experiment / route switches (SAPCA_* environment variables).
//
// A RELEASE build of libsapca reads none of them: dbg_env() is a constant null there and every switch below is compiled
// out, so a stray variable in a caller's process cannot change a route or a data layout.  The variant built with
// -DSAPCA_DEBUG_SWITCHES (lib/libsapca_dbg.so, `make debug`) reads them; the route tests (tests/, fixture `debug_switches`)
// and the A/B scripts under tools/ load that variant through SAPCA_LIB_PATH.
//
// What a release build does read, as plain getenv calls at their two sites:
//   SAPCA_AT_OVERLAP=0|1    engine.cpp   0: the A^T sweep of a multi-rank fit in one piece (no collective on a side stream);
//                                        1: in two pieces under RCCL too (opt-in there until it has run on more than one GPU)
//   SAPCA_MULTI_INPROCESS=1 multi.cpp    sapca_multi_* members talk through page-locked host memory instead of RCCL
//
// The switches of the debug variant (name: effect), by file:
//   engine.cpp   SAPCA_TILED_MIN_ENTRIES (floor of the staged sweep), SAPCA_AT_NATURAL, SAPCA_AT_UNPACK, SAPCA_AT_SORT,
//                SAPCA_LANCZOS_TRANSPOSE, SAPCA_MASK_STATS_INLINE, SAPCA_Q3_ROWKERNEL
//   tiled_build.hip (BuildSwitches, read once per build)  SAPCA_DQ_BLOCK_ROWS, SAPCA_SPLIT_WGS, SAPCA_QF_CAP_FIXED, SAPCA_NO_ROWSORT,
//                SAPCA_ROWSORT_ALWAYS, SAPCA_FILL_DIRECT, SAPCA_AT_BUCKETS, SAPCA_AT_SORT, SAPCA_RUNS_SEG_LDS_MAX, SAPCA_NO_DQ, SAPCA_DEBUG
//   spmm_tiled.hip  SAPCA_SWEEP_STAGED
//   spmm_dq.hip  SAPCA_NO_DQ, SAPCA_NO_DQ_F64      prep.hip  SAPCA_TRANSPOSE_GATHER
//   chol.hip     SAPCA_CHOL_GENERAL              sym_eig.hip  SAPCA_EIG_DEVICE
//   lanczos.hip  SAPCA_SPMV_NO_LDS, SAPCA_SPMV_NO_SLICE_GRID, SAPCA_SPMV_IDX32 (SpmvSwitches: read once per fit, so one process can
//                walk the routes), SAPCA_LANCZOS_CHECK
//   tsne.hip     SAPCA_TSNE_SPLIT (0 | 1: the repulsion's j chunks walked by one workgroup per i block | one workgroup each)
//   spectral.cpp SAPCA_SPECTRAL_GROUP (8 | 16 | 32 | 64: the lanes a row gets in the scale and the short-row product, whatever the
//                mean row length; read on every call), SAPCA_SPECTRAL_SPMV_ROW (the stage call's product through the wave-per-row
//                k::spmv: the yardstick of tools/time_spectral.py), SAPCA_SPECTRAL_STEP_SHORT (the solve's step through the short-row
//                kernel instead of k::spmv), SAPCA_SPECTRAL_APPLY_REPS (the stage call runs its product that often)
//   api.cpp      SAPCA_UPLOAD_STATS_OFF, SAPCA_UP_CHUNK (entries per chunk of the host upload, >= 1; read on every upload)
//   comm.cpp     SAPCA_COMM_FORCE_RCCL (a one-rank RCCL communicator: how a one-GPU box tests the binding), SAPCA_COMM_NO_SPLIT,
//                SAPCA_RCCL_LIBRARY (path of the tests' stand-in for librccl: tests/fake_rccl)
#pragma once
#include <cstdlib>

namespace sapca {

#ifdef SAPCA_DEBUG_SWITCHES
inline const char* dbg_env(const char* name) { return std::getenv(name); }
constexpr bool kDebugSwitches = true;
#else
inline const char* dbg_env(const char*) { return nullptr; }
constexpr bool kDebugSwitches = false;
#endif
inline bool dbg_on(const char* name) { return dbg_env(name) != nullptr; }

}  // namespace sapca
