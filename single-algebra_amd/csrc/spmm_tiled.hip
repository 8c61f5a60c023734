// LDS-staged sparse x dense-panel sweep (f32 and f64) and the tile-major "quad" operator format it reads.
//
// Why: per stored entry the sweep reads 8 B of A but a whole panel row (256 B at l = 60).  Served
// from L2 that gather caps the sweep far below the HBM roofline (measured 5.8 % with
// the row kernel of spmm.hip).  Here the panel rows of one column tile are staged in LDS once per
// workgroup and every gather is an LDS read, while A streams from HBM exactly once, contiguously.
//
// The format (DESIGN.md §5 has the measurements that led to it): rows in blocks of <= 512 (one workgroup
// of 16 waves), columns in `nct` INTERLEAVED tiles (tile t = columns == t mod nct, 80 KiB of LDS).  A wave
// is four groups of 16 lanes and every group walks its own row with ds_read_b128; four consecutive rows (a
// quad) advance in lockstep, so the format stores a quad's segment step by step, 4 entries per step,
// padded with {0, 0.0f} to its longest row.  8 quads per wave, accumulators in VGPRs across all tiles,
// no cross-lane reduction.  The builders are tiled_build.hip's; the constants and entry types that builders
// and sweeps share stand in quad_format.h.  The production sweep over this format is spmm_dq.hip's; the
// staged-entry sweep here takes the operators it refuses.
//
// Panels wider than 64 columns take two column passes over the same format (spmm_tiled); f64 values and
// panels use the same format with 16-byte entries and 512-byte panel rows (spmm_quad_f64_kernel).
//
// An entry is {u32 byte offset of its panel row inside the LDS tile, f32 value}; per column tile the
// workgroup does  barrier; panel tile + the block's entry chunk -> LDS (both prefetched into registers
// during the previous tile's compute); barrier; compute.  Tile ranges can be split over workgroups
// (A^T has few rows): partial sums go to a slab that a second kernel adds in fixed order.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kernels.h"
#include "quad_format.h"
#include "spmm_dq.h"

namespace sapca {
namespace k {

namespace {

// ---------------------------------------------------------------------------------- sweep
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));   // output rows are only element-aligned (ldo = k)

// loads are unconditional (addresses clamped into the valid range) so the arrays stay in VGPRs
template <int N, int THREADS>
__device__ __forceinline__ void load_regs(v4f (&r)[N], const char* src, int bytes) {
#pragma unroll
  for (int i = 0; i < N; ++i)
    r[i] = *reinterpret_cast<const v4f*>(src + min((i * THREADS + (int)threadIdx.x) * 16, bytes - 16));
}
template <int N, int THREADS>
__device__ __forceinline__ void store_regs(const v4f (&r)[N], char* dst, int capacity) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int b = (i * THREADS + (int)threadIdx.x) * 16;
    if ((i + 1) * THREADS * 16 <= capacity || b + 16 <= capacity) *reinterpret_cast<v4f*>(dst + b) = r[i];
  }
}

// out[r][j] = sum_sp part[sp][r][j] - cvec[j]   (fixed order)
template <typename VT>
__global__ void split_reduce_kernel(const VT* __restrict__ part, int nsplit, int64_t rows, int ldo, int ncols,
                                    const VT* __restrict__ cvec, VT* __restrict__ out, int ldy) {
  const int64_t total = rows * ldo;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int j = (int)(i % ldo);
    if (j >= ncols) continue;
    VT s = 0;
    for (int sp = 0; sp < nsplit; ++sp) s += part[(int64_t)sp * total + i];
    out[(i / ldo) * ldy + j] = s - (cvec ? cvec[j] : (VT)0);
  }
}

// the same for a run of rows: slab sp starts `slab_stride` elements behind slab sp - 1
__global__ void split_reduce_rows_kernel(const float* __restrict__ part, int nsplit, int64_t slab_stride, int64_t rows, int ldo, int ncols,
                                         float* __restrict__ out, int ldy) {
  const int64_t total = rows * ldo;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int j = (int)(i % ldo);
    if (j >= ncols) continue;
    float s = 0;
    for (int sp = 0; sp < nsplit; ++sp) s += part[(int64_t)sp * slab_stride + i];
    out[(i / ldo) * ldy + j] = s;
  }
}

// ------------------------------------------------------------------------ "quad" format and sweep
// Measured on round 1's first formulation, two half-waves per row (profiles/): a
// SIMD retires about one instruction per 4-6 cycles whatever its kind, so the sweep time follows
// the number of instructions per stored entry.  Here a wave is four groups of 16 lanes and every
// group walks its OWN row (ds_read_b128: a lane holds 4 of the 64 panel columns, 8 of 128), so
// one instruction stream advances four entries, there is no duplicate accumulator to reduce at
// the end, and the accumulators of a 512-row block take 32 VGPRs instead of 64.  The four rows of
// a quad advance in lockstep: the format pads every quad's segment in a tile to its longest row
// (zero entries: offset 0, value 0).

// U consecutive steps of one quad: four rows advance together, one per lane group
template <int NV, int U>
__device__ __forceinline__ void quad_batch(v4f (&acc)[NV], const char* stage_lane, const char* tile_lane) {
  typedef unsigned int u2 __attribute__((ext_vector_type(2)));
  u2 e[U];
#pragma unroll
  for (int u = 0; u < U; ++u) e[u] = *reinterpret_cast<const u2*>(stage_lane + u * (QGROUPS * 8));
  v4f w[U][NV];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < NV; ++v) w[u][v] = *reinterpret_cast<const v4f*>(tile_lane + e[u].x + v * 256);
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] += __uint_as_float(e[u].y) * w[u][v];
}

// panel rows t, t + nct, t + 2 nct, ... (clamped: slots past the last row are never referenced)
template <int N, int LDP>
__device__ __forceinline__ void load_tile_interleaved(v4f (&r)[N], const float* __restrict__ X, int ldx, int t, int nct,
                                                      int64_t panel_rows) {
  constexpr int CPR = LDP / 4;   // 16-byte chunks per panel row (LDP of the panel's ldx columns)
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int j = i * QTHREADS + (int)threadIdx.x;
    const int64_t grow = min((int64_t)(j / CPR) * nct + t, panel_rows - 1);
    r[i] = *reinterpret_cast<const v4f*>(X + grow * ldx + (j % CPR) * 4);
  }
}

#define SAPCA_QPREFETCH(CT)                                                                         \
  {                                                                                                 \
    const int64_t cidx_ = (int64_t)rb * nct + (CT);                                                 \
    const int64_t c_lo_ = chunk_off[cidx_];                                                         \
    load_tile_interleaved<NP_TILE, LDP>(pt, X, ldx, (CT), nct, panel_rows);                              \
    load_regs<NP_STAGE, QTHREADS>(ps, reinterpret_cast<const char*>(ent + c_lo_),                   \
                                  max(16, (int)(chunk_off[cidx_ + 1] - c_lo_) * 8));                \
  }
#define SAPCA_QBOOKKEEPING(CT)                                                                      \
  {                                                                                                 \
    const int64_t cidx_ = (int64_t)rb * nct + (CT);                                                 \
    cnt_next = lane < my_quads ? (int)steps[cidx_ * Q_BLOCK_QUADS + quad0 + lane] : 0;             \
    woff_next = wave_off[cidx_ * QWAVES + wave];                                                    \
  }

template <int LDP, bool PREFETCH, int TILE_B>
__global__ void __launch_bounds__(QTHREADS)
spmm_quad_kernel(const int32_t* __restrict__ blk_row0, const uint32_t* __restrict__ perm, int nct, int tc,
                 const int64_t* __restrict__ chunk_off,
                 const uint32_t* __restrict__ wave_off, const uint16_t* __restrict__ steps, const Ent* __restrict__ ent,
                 int64_t panel_rows, const float* __restrict__ X, int ldx, int nsplit, int tiles_per_split,
                 float* __restrict__ out, int64_t out_rows_total, int ldo, int ncols, const float* __restrict__ cvec) {
  constexpr int NV = LDP / 64;            // b128 reads per panel row per lane
  constexpr int RG = q_rows_per_group(LDP);
  constexpr int STAGE_B = q_stage_bytes(TILE_B);
  constexpr int NP_TILE = TILE_B / (QTHREADS * 16), NP_STAGE = (STAGE_B + QTHREADS * 16 - 1) / (QTHREADS * 16);
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* tile = lds;
  char* stage = lds + TILE_B;
  const int rb = blockIdx.x / nsplit, sp = blockIdx.x % nsplit;
  const int ct0 = sp * tiles_per_split, ct1 = min(nct, ct0 + tiles_per_split);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int g = lane / QLANES, q = lane % QLANES;
  const int row0 = blk_row0[rb], nrows = blk_row0[rb + 1] - row0;
  const int nquads = (nrows + 3) / 4;
  const int quad0 = q_first(wave, nquads), my_quads = q_first(wave + 1, nquads) - quad0;   // <= RG
  const int my_rows = min(nrows, 4 * (quad0 + my_quads)) - 4 * quad0;
  const char* tl = tile + q * 16;

  v4f acc[RG][NV];
#pragma unroll
  for (int i = 0; i < RG; ++i)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[i][v] = v4f(0.f);

  v4f pt[NP_TILE], ps[NP_STAGE];
  int cnt_next = 0;
  unsigned woff_next = 0;
  if (ct0 < ct1) SAPCA_QBOOKKEEPING(ct0)
  if (PREFETCH && ct0 < ct1) SAPCA_QPREFETCH(ct0)
  for (int ct = ct0; ct < ct1; ++ct) {
    __syncthreads();  // the previous tile's readers are done
    if (!PREFETCH) SAPCA_QPREFETCH(ct)
    store_regs<NP_TILE, QTHREADS>(pt, tile, TILE_B);
    store_regs<NP_STAGE, QTHREADS>(ps, stage, STAGE_B);
    __syncthreads();
    const int cnt_v = cnt_next;
    const unsigned woff = woff_next;
    if (ct + 1 < ct1) SAPCA_QBOOKKEEPING(ct + 1)
    if (PREFETCH && ct + 1 < ct1) SAPCA_QPREFETCH(ct + 1)
    if (my_quads > 0) {
      const char* sl = stage + (size_t)woff * 8 + g * 8;
#pragma unroll
      for (int j = 0; j < RG; ++j) {
        int n = __builtin_amdgcn_readlane(cnt_v, j);
        if constexpr (QWAVES == 8 && NV == 1) {   // 256 VGPRs per lane: 8 steps in flight per wave
          while (n >= 8) {
            quad_batch<NV, 8>(acc[j], sl, tl);
            sl += 8 * QGROUPS * 8;
            n -= 8;
          }
        }
        while (n >= 4) {
          quad_batch<NV, 4>(acc[j], sl, tl);
          sl += 4 * QGROUPS * 8;
          n -= 4;
        }
        if (n >= 2) {
          quad_batch<NV, 2>(acc[j], sl, tl);
          sl += 2 * QGROUPS * 8;
          n -= 2;
        }
        if (n) {
          quad_batch<NV, 1>(acc[j], sl, tl);
          sl += QGROUPS * 8;
        }
      }
    }
  }

  // lane (g, q) holds columns 4q..4q+3 (and 64+4q.. for 128-wide panels) of row 4j+g of its wave
  float* dst_base = out + (nsplit > 1 ? (int64_t)sp * out_rows_total * ldo : 0);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int col = v * 64 + q * 4;
    float cv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[i] = (cvec && nsplit == 1 && col + i < ncols) ? cvec[col + i] : 0.f;
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int r = 4 * j + g;
      if (r < my_rows) {
        const int64_t sp = (int64_t)row0 + 4 * quad0 + r;   // slot position -> output row
        float* y = dst_base + (perm ? (int64_t)perm[sp] : sp) * ldo + col;
        if (col + 3 < ncols) {
          v4f o = acc[j][v];
          o.x -= cv[0]; o.y -= cv[1]; o.z -= cv[2]; o.w -= cv[3];
          *reinterpret_cast<v4f_a4*>(y) = o;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (col + i < ncols) y[i] = acc[j][v][i] - cv[i];
        }
      }
    }
  }
}
#undef SAPCA_QPREFETCH
#undef SAPCA_QBOOKKEEPING

template <int LDP, bool PREFETCH, int TILE_B>
void launch_quad(const TiledOp& op, const float* X, int ldx, float* out, int ldo, int ncols, const float* cvec, hipStream_t s) {
  static LdsAttrState attr;
  ensure_dynamic_lds(reinterpret_cast<const void*>(&spmm_quad_kernel<LDP, PREFETCH, TILE_B>), LDS_TOTAL, attr);
  hipLaunchKernelGGL((spmm_quad_kernel<LDP, PREFETCH, TILE_B>), dim3((unsigned)(op.nrb * op.nsplit)), dim3(QTHREADS), LDS_TOTAL, s,
                     op.blk_row0, op.row_perm, op.nct, op.tc, op.chunk_off, op.wave_off, reinterpret_cast<const uint16_t*>(op.steps),
                     reinterpret_cast<const Ent*>(op.ent), op.cols, X, ldx, op.nsplit, op.tiles_per_split, out, op.rows, ldo,
                     ncols, cvec);
}

// ---- the same sweep for f64 panels and values ------------------------------------------------------
// A 64-column f64 panel row is 512 bytes: the tile geometry of the 128-float panels (160 rows per
// 80 KiB tile, 4 rows per lane group, 256 rows per workgroup).  A lane holds the doubles 2q, 2q+1 and
// 32+2q, 32+2q+1 of its row (two ds_read_b128); entries are 16 bytes {offset, pad, f64 value}.
typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v2d_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef unsigned int u4v __attribute__((ext_vector_type(4)));

template <int U>
__device__ __forceinline__ void quad_batch_f64(v2d (&acc)[2], const char* stage_lane, const char* tile_lane) {
  u4v e[U];
#pragma unroll
  for (int u = 0; u < U; ++u) e[u] = *reinterpret_cast<const u4v*>(stage_lane + u * (QGROUPS * 16));
  v2d w[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) w[u][v] = *reinterpret_cast<const v2d*>(tile_lane + e[u].x + v * 256);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double val = __hiloint2double((int)e[u].w, (int)e[u].z);
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[v] += val * w[u][v];
  }
}

template <int TILE_B>
__global__ void __launch_bounds__(QTHREADS)
spmm_quad_f64_kernel(const int32_t* __restrict__ blk_row0, const uint32_t* __restrict__ perm, int nct,
                     const int64_t* __restrict__ chunk_off, const uint32_t* __restrict__ wave_off,
                     const uint16_t* __restrict__ steps, const EntD* __restrict__ ent, int64_t panel_rows,
                     const double* __restrict__ X, int ldx, int nsplit, int tiles_per_split, double* __restrict__ out,
                     int64_t out_rows_total, int ldo, int ncols, const double* __restrict__ cvec) {
  constexpr int RG = q_rows_per_group(128);
  constexpr int STAGE_B = q_stage_bytes(TILE_B);
  constexpr int NP_TILE = TILE_B / (QTHREADS * 16), NP_STAGE = (STAGE_B + QTHREADS * 16 - 1) / (QTHREADS * 16);
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* tile = lds;
  char* stage = lds + TILE_B;
  const int rb = blockIdx.x / nsplit, sp = blockIdx.x % nsplit;
  const int ct0 = sp * tiles_per_split, ct1 = min(nct, ct0 + tiles_per_split);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int g = lane / QLANES, q = lane % QLANES;
  const int row0 = blk_row0[rb], nrows = blk_row0[rb + 1] - row0;
  const int nquads = (nrows + 3) / 4;
  const int quad0 = q_first(wave, nquads), my_quads = q_first(wave + 1, nquads) - quad0;   // <= RG
  const int my_rows = min(nrows, 4 * (quad0 + my_quads)) - 4 * quad0;
  const char* tl = tile + q * 16;

  v2d acc[RG][2];
#pragma unroll
  for (int i = 0; i < RG; ++i)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[i][v] = v2d(0.0);

  for (int ct = ct0; ct < ct1; ++ct) {
    const int64_t cidx = (int64_t)rb * nct + ct;
    const int64_t c_lo = chunk_off[cidx];
    const int cnt_v = lane < my_quads ? (int)steps[cidx * Q_BLOCK_QUADS + quad0 + lane] : 0;
    const unsigned woff = wave_off[cidx * QWAVES + wave];
    {
      v4f pt[NP_TILE], ps[NP_STAGE];
      // the panel as 128 floats per row: the same interleaved 16-byte chunks
      load_tile_interleaved<NP_TILE, 128>(pt, reinterpret_cast<const float*>(X), 2 * ldx, ct, nct, panel_rows);
      load_regs<NP_STAGE, QTHREADS>(ps, reinterpret_cast<const char*>(ent + c_lo), max(16, (int)(chunk_off[cidx + 1] - c_lo) * 16));
      __syncthreads();  // the previous tile's readers are done
      store_regs<NP_TILE, QTHREADS>(pt, tile, TILE_B);
      store_regs<NP_STAGE, QTHREADS>(ps, stage, STAGE_B);
      __syncthreads();
    }
    if (my_quads > 0) {
      const char* sl = stage + (size_t)woff * 16 + g * 16;
#pragma unroll
      for (int j = 0; j < RG; ++j) {
        int n = __builtin_amdgcn_readlane(cnt_v, j);
        while (n >= 4) {
          quad_batch_f64<4>(acc[j], sl, tl);
          sl += 4 * QGROUPS * 16;
          n -= 4;
        }
        if (n >= 2) {
          quad_batch_f64<2>(acc[j], sl, tl);
          sl += 2 * QGROUPS * 16;
          n -= 2;
        }
        if (n) {
          quad_batch_f64<1>(acc[j], sl, tl);
          sl += QGROUPS * 16;
        }
      }
    }
  }

  // lane (g, q) holds columns 2q, 2q+1 and 32+2q, 32+2q+1 of row 4j+g of its wave
  double* dst_base = out + (nsplit > 1 ? (int64_t)sp * out_rows_total * ldo : 0);
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int col = v * 32 + q * 2;
    double cv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) cv[i] = (cvec && nsplit == 1 && col + i < ncols) ? cvec[col + i] : 0.0;
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int r = 4 * j + g;
      if (r < my_rows) {
        const int64_t spos = (int64_t)row0 + 4 * quad0 + r;   // slot position -> output row
        double* y = dst_base + (perm ? (int64_t)perm[spos] : spos) * ldo + col;
        if (col + 1 < ncols) {
          v2d o = acc[j][v];
          o.x -= cv[0]; o.y -= cv[1];
          *reinterpret_cast<v2d_a8*>(y) = o;
        } else if (col < ncols) {
          y[0] = acc[j][v].x - cv[0];
        }
      }
    }
  }
}

template <int TILE_B>
void launch_quad_f64(const TiledOp& op, const double* X, int ldx, double* out, int ldo, int ncols, const double* cvec,
                     hipStream_t s) {
  static LdsAttrState attr;
  ensure_dynamic_lds(reinterpret_cast<const void*>(&spmm_quad_f64_kernel<TILE_B>), LDS_TOTAL, attr);
  hipLaunchKernelGGL((spmm_quad_f64_kernel<TILE_B>), dim3((unsigned)(op.nrb * op.nsplit)), dim3(QTHREADS), LDS_TOTAL, s,
                     op.blk_row0, op.row_perm, op.nct, op.chunk_off, op.wave_off, reinterpret_cast<const uint16_t*>(op.steps),
                     reinterpret_cast<const EntD*>(op.ent), op.cols, X, ldx, op.nsplit, op.tiles_per_split, out, op.rows, ldo,
                     ncols, cvec);
}

}  // namespace

// ---------------------------------------------------------------------------------- host side
void spmm_tiled(const TiledOp& op, const float* X, int ldx, float* Y, int ldy, int ncols, const float* cvec, DevBuf& scratch,
                hipStream_t s, PanelSource<float>* keep) {
  SAPCA_CHECK(op.valid && op.elem == 4, SAPCA_ERR_ARG, "tiled sweep: operator not built");
  SAPCA_CHECK(ldx == op.ldp || (op.ldp == 64 && ldx % 64 == 0), SAPCA_ERR_ARG,
              "tiled sweep: panel leading dimension does not match the operator's tile geometry");
  // A 128-wide panel over the 64-wide tile geometry goes through in two column passes: twice the entry
  // traffic, but a tile holds twice the panel rows of the 128-wide geometry (half the tiles, less quad
  // padding, chunks that amortise their refill) -- what keeps wide panels on sparse operators (C5) staged.
  const int passes = ldx / op.ldp;
  float* part = op.nsplit > 1 ? scratch.as<float>((size_t)op.nsplit * op.rows * op.ldp) : nullptr;
  for (int pass = 0; pass < passes; ++pass) {
    const int c0 = pass * op.ldp;
    if (c0 >= ncols && pass > 0) break;
    const float* Xp = X + c0;
    const float* cv = cvec ? cvec + c0 : nullptr;
    const int ncp = std::min(ncols - c0, op.ldp);
    float* out = Y + c0;
    int ldo = ldy, nc = ncp;
    if (op.nsplit > 1) {
      out = part;
      ldo = op.ldp;
      nc = op.ldp;
    }
    static const bool force_staged = dbg_env("SAPCA_SWEEP_STAGED") != nullptr;   // A/B: the staged-entry quad sweep
    // (blocks of more than 512 rows exist only for the DPP-fed sweep: the switches below do not apply to them)
    const bool staged_ok = op.block_rows <= 512 && op.max_chunk <= (int64_t)q_stage_cap(op.tile_bytes, (int)sizeof(Ent));
    SAPCA_CHECK(staged_ok || dq_usable(op, ldx), SAPCA_ERR_ARG, "tiled sweep: this operator needs the DPP-fed sweep");
    if (dq_usable(op, ldx) && (!staged_ok || !force_staged)) {
      launch_dq(op, Xp, ldx, out, ldo, nc, cv, s);
    } else {
      launch_quad<64, true, Q_TILE_BYTES>(op, Xp, ldx, out, ldo, nc, cv, s);
    }
    if (op.nsplit > 1) {
      const int64_t total = op.rows * (int64_t)op.ldp;
      if (keep && passes == 1 && !cv && ldy == op.ldp && ncp == op.ldp) {   // the caller's next pass over Y sums the slabs
        keep->parts = part;
        keep->nsplit = op.nsplit;
        keep->slab_stride = total;
        break;
      }
      hipLaunchKernelGGL(split_reduce_kernel<float>, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, part, op.nsplit, op.rows,
                         op.ldp, ncp, cv, Y + c0, ldy);
    }
  }
  SAPCA_HIP(hipGetLastError());
}

// Output rows [first, first + count) of the DPP-fed sweep, for callers that sweep an operator in pieces (the row-sharded
// A^T sweep of a multi-rank fit: a piece's all-reduce runs while the next piece is swept).  `piece` of `npieces`: the row
// blocks are cut into npieces runs; every piece cuts its tile range finely enough to occupy `wgs` workgroups, its partial
// slabs are summed in fixed order.  Requires natural row order (no row_perm: a block's rows are then a contiguous range of
// the output) and a 64-column panel.  Returns false when the operator cannot be swept this way (nothing is launched).
bool spmm_tiled_pieces_ok(const TiledOp& op, int npieces, int ldx) {
  return op.valid && op.elem == 4 && dq_usable(op, ldx) && ldx == op.ldp && op.row_perm == nullptr && npieces >= 1 && op.nrb >= npieces;
}

// bounds[p] = first output row of piece p (bounds[npieces] = rows): one small copy from the device, synchronous
void spmm_tiled_piece_bounds(const TiledOp& op, int npieces, std::vector<int64_t>& bounds, hipStream_t s) {
  if (npieces == 2 && op.mid_row0 >= 0) {   // (the builder kept the one boundary on the host: no copy, no wait)
    bounds = {0, op.mid_row0, op.rows};
    return;
  }
  std::vector<int32_t> b((size_t)npieces + 1);
  for (int p = 0; p <= npieces; ++p)
    SAPCA_HIP(hipMemcpyAsync(&b[(size_t)p], op.blk_row0 + (int64_t)op.nrb * p / npieces, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  bounds.assign(b.begin(), b.end());
}

void spmm_tiled_piece(const TiledOp& op, int piece, int npieces, int wgs, int64_t first_row, int64_t row_count, const float* X, int ldx, float* Y,
                      int ldy, int ncols, DevBuf& scratch, hipStream_t s) {
  SAPCA_CHECK(spmm_tiled_pieces_ok(op, npieces, ldx), SAPCA_ERR_ARG, "tiled sweep: operator cannot be swept in pieces");
  const int rb0 = (int)((int64_t)op.nrb * piece / npieces), rb1 = (int)((int64_t)op.nrb * (piece + 1) / npieces);
  int nsplit = std::max(1, std::min(op.nct, wgs / std::max(1, rb1 - rb0)));
  const int tps = (op.nct + nsplit - 1) / nsplit;
  nsplit = (op.nct + tps - 1) / tps;
  const int64_t* first = &first_row;
  const int64_t* count = &row_count;
  float* part = nsplit > 1 ? scratch.as<float>((size_t)nsplit * op.rows * op.ldp) : nullptr;
  if (nsplit > 1) {
    launch_dq_blocks(op, rb0, rb1, nsplit, tps, X, ldx, part, op.ldp, op.ldp, nullptr, s);
    const int64_t total = *count * (int64_t)op.ldp;
    // (slabs keep absolute row positions: the piece's rows start at first * ldp in every slab, slabs are op.rows * ldp apart)
    hipLaunchKernelGGL(split_reduce_rows_kernel, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, part + *first * op.ldp, nsplit,
                       op.rows * (int64_t)op.ldp, *count, op.ldp, ncols, Y + *first * ldy, ldy);
  } else {
    launch_dq_blocks(op, rb0, rb1, 1, op.nct, X, ldx, Y, ldy, ncols, nullptr, s);
  }
  SAPCA_HIP(hipGetLastError());
}

void spmm_tiled(const TiledOp& op, const double* X, int ldx, double* Y, int ldy, int ncols, const double* cvec, DevBuf& scratch,
                hipStream_t s, PanelSource<double>* keep) {
  SAPCA_CHECK(op.valid && op.elem == 8, SAPCA_ERR_ARG, "tiled sweep: no f64 operator built");
  SAPCA_CHECK(ldx >= op.ldp && ldx % op.ldp == 0, SAPCA_ERR_ARG,
              "tiled sweep: panel leading dimension does not match the operator's tile geometry");
  double* part = op.nsplit > 1 ? scratch.as<double>((size_t)op.nsplit * op.rows * op.ldp) : nullptr;
  const int passes = ldx / op.ldp;   // 128-column f64 panels: two column passes, as for f32
  for (int pass = 0; pass < passes; ++pass) {
    const int c0 = pass * op.ldp;
    if (c0 >= ncols && pass > 0) break;
    const double* Xp = X + c0;
    const double* cv = cvec ? cvec + c0 : nullptr;
    const int ncp = std::min(ncols - c0, op.ldp);
    double* out = Y + c0;
    int ldo = ldy, nc = ncp;
    if (op.nsplit > 1) {
      out = part;
      ldo = op.ldp;
      nc = op.ldp;
    }
    if (op.dq) launch_dq_f64(op, Xp, ldx, out, ldo, nc, cv, s);   // the DPP-fed sweep (spmm_dq.hip)
    else launch_quad_f64<Q_TILE_BYTES>(op, Xp, ldx, out, ldo, nc, cv, s);
    if (op.nsplit > 1) {
      const int64_t total = op.rows * (int64_t)op.ldp;
      if (keep && passes == 1 && !cv && ldy == op.ldp && ncp == op.ldp) {   // the caller's next pass over Y sums the slabs
        keep->parts = part;
        keep->nsplit = op.nsplit;
        keep->slab_stride = total;
        break;
      }
      hipLaunchKernelGGL(split_reduce_kernel<double>, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, part, op.nsplit, op.rows,
                         op.ldp, ncp, cv, Y + c0, ldy);
    }
  }
  SAPCA_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace sapca
