// Builders of the tile-major "quad" operator format (spmm_tiled.hip's header describes it; quad_format.h holds what
// builders and sweeps share).
//
// From a CSR: a per-row tile index (histogram, or a search / the statistics pass for rows already grouped by tile), a
// count of every quad's steps per (row block, tile) chunk, one scan, one fill -- LDS-staged for A, streaming for the
// tile-major rows of A^T, direct scatter as the fallback.  Or A^T straight from A through per-chunk buckets (atd_*,
// round 2: the default for unmasked f32 fits; no transposed CSR, no sort).  The kernels come first, the host side --
// geometry, eligibility, named stages -- after them.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "kernels.h"
#include "quad_format.h"
#include "spmm_dq.h"

namespace sapca {
namespace k {

namespace {

// Column tiles of this format are INTERLEAVED: tile t holds the panel rows {c : c mod nct == t}, at
// position c / nct.  Contiguous column ranges with their own density (gene modules, a dense band of
// a cluster) are thereby spread over all tiles, every (row, tile) segment has about the same length,
// the waves of a workgroup reach the per-tile barrier together and quads pad little.
__device__ __forceinline__ void divmod_small(int c, int d, float inv, int& q, int& r) {   // c < 2^24
  q = (int)((float)c * inv);
  r = c - q * d;
  if (r < 0) { r += d; --q; }
  if (r >= d) { r -= d; ++q; }
}

// seg[r][t] = number of entries of row r in tiles < t (t = 0..nct): LDS histogram per row, one wave per row
__global__ void __launch_bounds__(256)
tile_hist_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t rows, int nct, float inv_nct,
                 int32_t* __restrict__ seg) {
  extern __shared__ uint32_t hist_all[];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  uint32_t* hist = hist_all + (size_t)wave * nct;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    for (int t = lane; t < nct; t += WAVE) hist[t] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    for (int64_t eb = e0 + lane; eb < e1; eb += 8 * WAVE) {   // eight loads in flight per lane
      int c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = eb + u * WAVE < e1 ? idx[eb + u * WAVE] : -1;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c[u] >= 0) {
          int q, t;
          divmod_small(c[u], nct, inv_nct, q, t);
          atomicAdd(&hist[t], 1u);
        }
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t carry = 0;
    int32_t* out = seg + r * (nct + 1);
    for (int t0 = 0; t0 < nct; t0 += WAVE) {
      const int t = t0 + lane;
      const uint32_t v = t < nct ? hist[t] : 0u;
      uint32_t x = v;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
      }
      if (t < nct) out[t] = (int32_t)(carry + x - v);
      carry += __shfl(x, WAVE - 1);
    }
    if (lane == 0) out[nct] = (int32_t)carry;
    __builtin_amdgcn_wave_barrier();
  }
}

// one block per (row block, group of QC_TILES column tiles), one thread per quad: steps of every quad (= its longest row
// segment), entry offset of every wave, chunk size
constexpr int QC_TILES = 8;   // tiles per workgroup of quad_count_kernel: a thread reads its rows' 9 consecutive segment bounds (one or two lines)
                              // instead of one line per (row, tile) -- a table with a 4 KiB row pitch (A^T of C2 in f64) went at 1.6 ms
__global__ void __launch_bounds__(Q_BLOCK_QUADS)
quad_count_kernel(const int32_t* __restrict__ seg, const int32_t* __restrict__ blk_row0, const uint32_t* __restrict__ perm,
                  int nct, uint16_t* __restrict__ steps, uint32_t* __restrict__ quad_off, uint32_t* __restrict__ wave_off,
                  int64_t* __restrict__ chunk_size, const uint16_t* __restrict__ cnt16 = nullptr, int64_t cnt_stride = 0,
                  int64_t* __restrict__ raw_size = nullptr) {
  __shared__ uint32_t scan[Q_BLOCK_QUADS];
  __shared__ uint32_t wave_total[Q_BLOCK_QUADS / WAVE], raw_part[Q_BLOCK_QUADS / WAVE];
  const int groups = (nct + QC_TILES - 1) / QC_TILES;
  const int rb = blockIdx.x / groups, ct0 = (blockIdx.x % groups) * QC_TILES;
  const int row0 = blk_row0[rb], nrows = blk_row0[rb + 1] - row0;
  const int nquads = (nrows + 3) / 4;
  const int q = threadIdx.x, lane = q & (WAVE - 1);
  int len[4][QC_TILES];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int lr = 4 * q + g;
    const bool have = lr < nrows;
    const int64_t r = have ? (perm ? (int64_t)perm[row0 + lr] : (int64_t)row0 + lr) : 0;   // slot -> row (rows sorted by length)
    if (cnt16) {
      // (the bucket builder of A^T counts entries per (tile, row) instead of indexing a transposed CSR)
#pragma unroll
      for (int j = 0; j < QC_TILES; ++j) len[g][j] = (have && ct0 + j < nct) ? (int)cnt16[(int64_t)(ct0 + j) * cnt_stride + r] : 0;
    } else {
      int bound[QC_TILES + 1];
#pragma unroll
      for (int j = 0; j <= QC_TILES; ++j) bound[j] = (have && ct0 + j <= nct) ? seg[r * (nct + 1) + ct0 + j] : 0;
#pragma unroll
      for (int j = 0; j < QC_TILES; ++j) len[g][j] = (have && ct0 + j < nct) ? bound[j + 1] - bound[j] : 0;
    }
  }
#pragma unroll
  for (int j = 0; j < QC_TILES; ++j) {
    const int ct = ct0 + j;
    if (ct >= nct) break;
    const int64_t chunk = (int64_t)rb * nct + ct;
    const int longest = max(max(len[0][j], len[1][j]), max(len[2][j], len[3][j]));
    int raw = len[0][j] + len[1][j] + len[2][j] + len[3][j];
    const int qmax = q_steps(longest);
    const uint32_t padded = (uint32_t)qmax * 4u;
    steps[chunk * Q_BLOCK_QUADS + q] = (uint16_t)qmax;
    // inclusive scan of the padded quad sizes over the block: inside each wave by shuffles, the wave totals through LDS
    uint32_t inc = padded;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const uint32_t y = __shfl_up(inc, off);
      if (lane >= off) inc += y;
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) raw += __shfl_xor(raw, off);
    __syncthreads();   // (the previous tile's readers are done)
    if (lane == WAVE - 1) wave_total[q / WAVE] = inc;
    if (lane == 0) raw_part[q / WAVE] = (uint32_t)raw;
    __syncthreads();
    for (int w = 0; w < q / WAVE; ++w) inc += wave_total[w];
    scan[q] = inc;
    __syncthreads();
    // [row block][quad][tile]: the builder reads one quad's offsets in all tiles contiguously
    if (quad_off && q < nquads) quad_off[((int64_t)rb * Q_BLOCK_QUADS + q) * nct + ct] = inc - padded;   // (the bucket route rebuilds them from `steps`)
    if (q < QWAVES) {
      const int first_quad = q_first(q, nquads);
      wave_off[chunk * QWAVES + q] = first_quad > 0 ? scan[first_quad - 1] : 0u;
    }
    if (q == Q_BLOCK_QUADS - 1) {
      chunk_size[chunk] = inc;
      if (raw_size) {
        uint32_t total = 0;
        for (int w = 0; w < Q_BLOCK_QUADS / WAVE; ++w) total += raw_part[w];
        raw_size[chunk] = total;
      }
    }
  }
}

// one wave per row: the k-th entry (in column order) that the row has in tile t goes to slot
// (k*4 + g) of its quad's segment in that tile's chunk (g = row mod 4 within the block)
template <typename VT>
__global__ void __launch_bounds__(256)
quad_fill_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const VT* __restrict__ val,
                 int64_t rows, const int32_t* __restrict__ blk_row0, const uint32_t* __restrict__ perm, int nrb, int nct,
                 float inv_nct, int ldp_bytes, const int64_t* __restrict__ chunk_off, const uint32_t* __restrict__ quad_off,
                 typename EntOf<VT>::type* __restrict__ ent) {
  typedef typename EntOf<VT>::type E;
  extern __shared__ uint32_t cnt_all[];   // per wave and tile: slot of the row's next entry (relative to the block's first chunk)
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  uint32_t* cnt = cnt_all + (size_t)wave * nct;
  const int64_t sp = (int64_t)blockIdx.x * 4 + wave;   // slot position; its row is perm[sp]
  if (sp >= rows) return;
  const int64_t r = perm ? (int64_t)perm[sp] : sp;
  int lo = 0, hi = nrb;   // row block: the last b with blk_row0[b] <= sp
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)blk_row0[mid] <= sp) lo = mid; else hi = mid;
  }
  const int rb = lo;
  const int lr = (int)(sp - blk_row0[rb]);
  const int qd = lr >> 2;
  const uint32_t g = (uint32_t)(lr & 3);
  const int64_t* __restrict__ coff = chunk_off + (int64_t)rb * nct;
  const uint32_t* __restrict__ qoff = quad_off + ((int64_t)rb * Q_BLOCK_QUADS + qd) * nct;
  const int64_t block_base = coff[0];
  for (int t = lane; t < nct; t += WAVE) cnt[t] = (uint32_t)(coff[t] - block_base) + qoff[t] + g;
  __builtin_amdgcn_wave_barrier();
  const int64_t e0 = ptr[r], e1 = ptr[r + 1];
  E* __restrict__ out = ent + block_base;
  // batches of 64 entries in column order; within a batch the LDS atomic hands out the ranks of
  // equal tiles (a fixed function of the input: the format is reproducible run to run)
  for (int64_t eb = e0; eb < e1; eb += 8 * WAVE) {   // 8 batches loaded ahead: one round trip per 512 entries
    int c[8];
    VT v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t e = eb + u * WAVE + lane;
      c[u] = e < e1 ? idx[e] : -1;
      v[u] = e < e1 ? val[e] : (VT)0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (c[u] >= 0) {
        int i, t;
        divmod_small(c[u], nct, inv_nct, i, t);
        E x = E();
        x.off = (uint32_t)i * (uint32_t)ldp_bytes;
        x.val = v[u];
        out[atomicAdd(&cnt[t], 4u)] = x;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// The same fill with the quad assembled in LDS first: a workgroup owns one quad (a wave per row),
// scatters the entries into an LDS image of the quad's segments (padding pre-zeroed) and then writes
// every tile's segment out as one contiguous run -- the direct version above issues one isolated
// 8-byte store per entry, which is what it spends its time on.  Quads larger than the LDS image
// (very long rows) take the direct route and zero their padding themselves, so the entry buffer
// needs no memset on this path.
constexpr int QF_CAP_MIN = 4096, QF_CAP_MAX = 6144;   // entries of one quad staged in LDS: 32 KiB (more workgroups per CU) .. 48 KiB
// (quad `qi` of the operator: rb = qi / Q_BLOCK_QUADS, qd = qi % Q_BLOCK_QUADS; all 256 threads of the workgroup)
template <typename VT>
__device__ __forceinline__ void quad_fill_staged_one(int qi, uint32_t* qf_lds, const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                     const VT* __restrict__ val, const int32_t* __restrict__ seg,
                                                     const int32_t* __restrict__ blk_row0, const uint32_t* __restrict__ perm, int nct, int cap,
                                                     float inv_nct, int ldp_bytes, const int64_t* __restrict__ chunk_off,
                                                     const uint32_t* __restrict__ quad_off, typename EntOf<VT>::type* __restrict__ ent) {
  typedef typename EntOf<VT>::type E;
  constexpr int EW = (int)sizeof(E) / 4;   // entry size in LDS words
  E* stage = reinterpret_cast<E*>(qf_lds);         // [cap]
  int64_t* gofs = reinterpret_cast<int64_t*>(qf_lds + EW * cap);   // [nct] where the quad's segment of tile t goes
  uint32_t* lofs = qf_lds + EW * cap + 2 * nct;     // [nct + 1] start of every tile's segment in the image
  uint32_t* cnt_all = lofs + nct + 1;              // [4][nct] entries of row g seen so far in tile t
  const int rb = qi / Q_BLOCK_QUADS, qd = qi % Q_BLOCK_QUADS;
  const int row0 = blk_row0[rb], nrows = blk_row0[rb + 1] - row0;
  if (4 * qd >= nrows) return;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int qrows = min(4, nrows - 4 * qd);
  const int64_t s0 = (int64_t)row0 + 4 * qd;   // first slot position of the quad
  int64_t rowof[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) rowof[g] = g < qrows ? (perm ? (int64_t)perm[s0 + g] : s0 + g) : 0;
  const int64_t* __restrict__ coff = chunk_off + (int64_t)rb * nct;
  const uint32_t* __restrict__ qoff = quad_off + ((int64_t)rb * Q_BLOCK_QUADS + qd) * nct;
  // segment sizes (4 x the longest of the quad's rows in the tile), then their exclusive scan
  for (int t = threadIdx.x; t < nct; t += 256) {
    int mx = 0;
    for (int g = 0; g < qrows; ++g) {
      const int32_t* sg = seg + rowof[g] * (nct + 1);
      mx = max(mx, sg[t + 1] - sg[t]);
    }
    lofs[t + 1] = (uint32_t)q_steps(mx) * 4u;
    gofs[t] = coff[t] + (int64_t)qoff[t];   // (fetched here, beside the segment bounds: the write-out below waits on LDS only)
    for (int g = 0; g < 4; ++g) cnt_all[g * nct + t] = 0;
  }
  if (threadIdx.x == 0) lofs[0] = 0;
  __syncthreads();
  if (wave == 0) {
    uint32_t carry = 0;
    for (int t0 = 0; t0 < nct; t0 += WAVE) {
      const int t = t0 + lane;
      const uint32_t v = t < nct ? lofs[t + 1] : 0u;
      uint32_t x = v;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
      }
      if (t < nct) lofs[t + 1] = carry + x;
      carry += __shfl(x, WAVE - 1);
    }
  }
  __syncthreads();
  const uint32_t total = lofs[nct];
  const bool staged = total <= (uint32_t)cap;
  if (staged) {
    uint64_t* z = reinterpret_cast<uint64_t*>(stage);
    for (uint32_t i = threadIdx.x; i < total * (EW / 2); i += 256) z[i] = 0;
  } else {
    // direct route: zero the padding slots of this wave's row in global memory
    if (wave < qrows) {
      const int32_t* sg = seg + rowof[wave] * (nct + 1);
      for (int t = lane; t < nct; t += WAVE) {
        const uint32_t steps = (lofs[t + 1] - lofs[t]) / 4u;
        E* dst = ent + gofs[t];
        for (uint32_t k = (uint32_t)(sg[t + 1] - sg[t]); k < steps; ++k) dst[k * 4u + wave] = E();
      }
    } else {
      for (int t = lane; t < nct; t += WAVE) {   // rows past the end of the block: all padding
        const uint32_t steps = (lofs[t + 1] - lofs[t]) / 4u;
        E* dst = ent + gofs[t];
        for (uint32_t k = 0; k < steps; ++k) dst[k * 4u + wave] = E();
      }
    }
  }
  __syncthreads();
  if (wave < qrows) {
    const int64_t r = rowof[wave];
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    uint32_t* cnt = cnt_all + (size_t)wave * nct;
    // batches of 64 entries in column order; within a batch the LDS atomic hands out the ranks of
    // equal tiles (a fixed function of the input: the format is reproducible run to run)
    // 8 batches are loaded ahead so that one memory round trip serves 512 entries
    for (int64_t eb = e0; eb < e1; eb += 8 * WAVE) {
      int c[8];
      VT v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t e = eb + u * WAVE + lane;
        c[u] = e < e1 ? idx[e] : -1;
        v[u] = e < e1 ? val[e] : (VT)0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (c[u] >= 0) {
          int i, t;
          divmod_small(c[u], nct, inv_nct, i, t);
          E x = E();
          x.off = (uint32_t)i * (uint32_t)ldp_bytes;
          x.val = v[u];
          const uint32_t k = atomicAdd(&cnt[t], 1u);
          if (staged) stage[lofs[t] + k * 4u + (uint32_t)wave] = x;
          else ent[gofs[t] + k * 4u + (uint32_t)wave] = x;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (!staged) return;
  __syncthreads();
  for (int t = wave; t < nct; t += 4) {
    const uint32_t lo = lofs[t], n = lofs[t + 1] - lo;
    E* dst = ent + gofs[t];
    for (uint32_t j = lane; j < n; j += WAVE) dst[j] = stage[lo + j];
  }
}

// A workgroup walks quads qi = blockIdx.x, blockIdx.x + gridDim.x, ... (the default grid is one workgroup per quad: qf_grid).
template <typename VT>
__global__ void __launch_bounds__(256)
quad_fill_staged_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const VT* __restrict__ val,
                        const int32_t* __restrict__ seg, const int32_t* __restrict__ blk_row0,
                        const uint32_t* __restrict__ perm, int nct, int cap, float inv_nct,
                        int ldp_bytes, const int64_t* __restrict__ chunk_off, const uint32_t* __restrict__ quad_off,
                        typename EntOf<VT>::type* __restrict__ ent, int nquads_all) {
  extern __shared__ __attribute__((aligned(16))) uint32_t qf_lds[];
  for (int qi = blockIdx.x; qi < nquads_all; qi += gridDim.x) {
    quad_fill_staged_one<VT>(qi, qf_lds, ptr, idx, val, seg, blk_row0, perm, nct, cap, inv_nct, ldp_bytes, chunk_off, quad_off, ent);
    __syncthreads();   // (the image and its tables are reused by the next quad)
  }
}

// ---- rows whose entries are already grouped by tile (transpose_csr(..., tile_major_nct)) ----------
// seg[r][t] = number of entries of row r in tiles < t: the tile of an entry (idx mod nct) is
// non-decreasing along the row, so a binary search per boundary does it
__global__ void tile_index_mod_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                      const uint64_t* __restrict__ packed, int64_t rows, int nct, float inv_nct,
                                      int32_t* __restrict__ seg) {
  const int64_t total = rows * (int64_t)(nct + 1);
  int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; o < total; o += stride) {
    const int64_t r = o / (nct + 1);
    const int t = (int)(o - r * (nct + 1));
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    int64_t lo = e0, hi = e1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      int q, tm;
      divmod_small(packed ? (int)(packed[mid] >> 32) : idx[mid], nct, inv_nct, q, tm);
      if (tm < t) lo = mid + 1; else hi = mid;
    }
    seg[o] = (int32_t)(lo - e0);
  }
}

// One pass over the packed tile-major rows: the column statistics of A (row sums of A^T, accumulated in
// exactly the order of prep.hip's row_sums kernels) and seg[r][t] from the places where the tile changes.
__global__ void at_stats_index_kernel(const int64_t* __restrict__ ptr, const uint64_t* __restrict__ packed, int64_t rows,
                                      int nct, float inv_nct, double* __restrict__ sum, double* __restrict__ sumsq,
                                      int32_t* __restrict__ seg) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t r = wave; r < rows; r += nwaves) {
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    int32_t* sg = seg + r * (nct + 1);
    double a = 0, b = 0;
    int carry = -1;   // tile of the entry before this batch
    for (int64_t eb = e0; eb < e1; eb += WAVE) {
      const int64_t e = eb + lane;
      const bool valid = e < e1;
      int t = nct;   // past the end: closes every remaining boundary
      if (valid) {
        const uint64_t pv = packed[e];
        const double v = (double)__uint_as_float((uint32_t)pv);
        a += v;
        b += v * v;
        int q;
        divmod_small((int)(pv >> 32), nct, inv_nct, q, t);
      }
      int tprev = __shfl_up(t, 1);
      if (lane == 0) tprev = carry;
      // entry e is the first one of tiles (tprev, t]; lanes past the end write the closing boundaries once
      if (valid || e == e1)
        for (int tt = tprev + 1; tt <= t; ++tt) sg[tt] = (int32_t)(e - e0);
      carry = __shfl(t, WAVE - 1);
    }
    // rows whose length is a multiple of 64 (or zero) have not closed their boundaries yet
    if (((e1 - e0) & (WAVE - 1)) == 0)
      for (int tt = carry + 1 + lane; tt <= nct; tt += WAVE) sg[tt] = (int32_t)(e1 - e0);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      a += __shfl_xor(a, off);
      b += __shfl_xor(b, off);
    }
    if (lane == 0) {
      sum[r] = a;
      if (sumsq) sumsq[r] = b;
    }
  }
}

// rows sorted by length: keys for the descending sort and the identity payload
__global__ void row_len_iota_kernel(const int64_t* __restrict__ ptr, int64_t rows, uint32_t* __restrict__ len,
                                    uint32_t* __restrict__ iota) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) {
    len[r] = (uint32_t)(ptr[r + 1] - ptr[r]);
    iota[r] = (uint32_t)r;
  }
}

// sum over consecutive groups of four rows of 4 * (longest of the four): what the quads would hold if the
// rows kept their natural order (the quad padding estimate that decides whether sorting is worth its cost)
__global__ void __launch_bounds__(256)
natural_quad_slots_kernel(const int64_t* __restrict__ ptr, int64_t rows, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[4];
  unsigned long long acc = 0;
  const int64_t nq = (rows + 3) / 4;
  for (int64_t qd = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; qd < nq; qd += (int64_t)gridDim.x * blockDim.x) {
    int64_t mx = 0;
    for (int g = 0; g < 4 && 4 * qd + g < rows; ++g) mx = max(mx, ptr[4 * qd + g + 1] - ptr[4 * qd + g]);
    acc += (unsigned long long)(4 * mx);
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// Streaming fill: a workgroup owns a quad; every (quad, tile) segment is four contiguous source runs
// interleaved step by step ([k][g]) and padded with zero entries, written as one contiguous piece.
// SEG_LDS: the quad's four rows of seg are staged in LDS (few tiles: the table is small and the
// workgroups stay many per CU); otherwise every lane reads its row's bounds from global memory one
// tile step ahead (many tiles: a [4][tiles + 1] table would leave one or two workgroups per CU).
template <bool SEG_LDS, typename VT = float>
__global__ void __launch_bounds__(256)
quad_fill_runs_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const VT* __restrict__ val,
                      const uint64_t* __restrict__ packed, const int32_t* __restrict__ seg, const int32_t* __restrict__ blk_row0,
                      const uint32_t* __restrict__ perm, int nct, float inv_nct, int ldp_bytes,
                      const int64_t* __restrict__ chunk_off, const uint32_t* __restrict__ quad_off,
                      typename EntOf<VT>::type* __restrict__ ent) {
  typedef typename EntOf<VT>::type Ent;   // (f64: 16-byte entries; the packed rows are an f32 route)
  extern __shared__ int32_t sg_lds[];   // [4][nct + 1] the quad's rows of seg
  const int rb = blockIdx.x / Q_BLOCK_QUADS, qd = blockIdx.x % Q_BLOCK_QUADS;
  const int row0 = blk_row0[rb], nrows = blk_row0[rb + 1] - row0;
  if (4 * qd >= nrows) return;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int qrows = min(4, nrows - 4 * qd);
  const int64_t s0q = (int64_t)row0 + 4 * qd;   // first slot position of the quad; slot -> row through perm
  if (SEG_LDS) {
    for (int i = threadIdx.x; i < 4 * (nct + 1); i += 256) {
      const int g = i / (nct + 1);
      const int64_t rg = g < qrows ? (perm ? (int64_t)perm[s0q + g] : s0q + g) : 0;
      sg_lds[i] = g < qrows ? seg[rg * (nct + 1) + (i - g * (nct + 1))] : 0;
    }
    __syncthreads();
  }
  const int g = lane & 3, k0 = lane >> 2;   // lane -> (step k0 + 16*pass, row g)
  const int64_t myrow = g < qrows ? (perm ? (int64_t)perm[s0q + g] : s0q + g) : -1;
  const int64_t base = myrow >= 0 ? ptr[myrow] : 0;
  const int32_t* mysg = SEG_LDS ? sg_lds + g * (nct + 1) : seg + (myrow >= 0 ? myrow : 0) * (nct + 1);
  const int64_t* __restrict__ coff = chunk_off + (int64_t)rb * nct;
  const uint32_t* __restrict__ qoff = quad_off + ((int64_t)rb * Q_BLOCK_QUADS + qd) * nct;
  int s_nx = 0, e_nx = 0;
  int64_t d_nx = 0;
  if (!SEG_LDS && wave < nct) {
    s_nx = myrow >= 0 ? mysg[wave] : 0;
    e_nx = myrow >= 0 ? mysg[wave + 1] : 0;
    d_nx = coff[wave] + qoff[wave];
  }
  for (int t = wave; t < nct; t += 4) {
    int s0, len;
    Ent* dst;
    if (SEG_LDS) {
      s0 = mysg[t];
      len = mysg[t + 1] - s0;
      dst = ent + coff[t] + qoff[t];
    } else {
      s0 = s_nx;
      len = e_nx - s_nx;
      dst = ent + d_nx;
      if (t + 4 < nct) {
        s_nx = myrow >= 0 ? mysg[t + 4] : 0;
        e_nx = myrow >= 0 ? mysg[t + 5] : 0;
        d_nx = coff[t + 4] + qoff[t + 4];
      }
    }
    int qmax = max(len, __shfl_xor(len, 1));
    qmax = q_steps(max(qmax, __shfl_xor(qmax, 2)));
    for (int k = k0; k < qmax; k += 16) {
      Ent x{};
      if (k < len) {
        const int64_t e = base + s0 + k;
        int c;
        if constexpr (sizeof(VT) == 4) {
          if (packed) {
            const uint64_t pv = packed[e];
            c = (int)(pv >> 32);
            x.val = __uint_as_float((uint32_t)pv);
          } else {
            c = idx[e];
            x.val = val[e];
          }
        } else {
          c = idx[e];
          x.val = val[e];
        }
        int i, tm;
        divmod_small(c, nct, inv_nct, i, tm);
        x.off = (uint32_t)i * (uint32_t)ldp_bytes;
      }
      dst[k * 4 + g] = x;
    }
  }
}

// Exclusive scans of one or two int64 arrays of count + 1 elements (the last input element is ignored; the last output is
// the total) by ONE workgroup, plus the maximum of the first array: the tables here have 1e4 .. 1e6 elements, and one
// launch replaces six of the library's (histogram / lookback / scan kernels for each of reduce and scan).
// Rounds of 1024 x PER elements: a thread loads its PER consecutive elements of the round together and keeps them in
// registers -- one round trip to memory per round instead of one per element, which is what the kernel's time is at
// these sizes; the running totals carry from round to round.
template <int PER, bool HAS_B>
__global__ void __launch_bounds__(1024)
small_scan_kernel(int64_t* __restrict__ a, int64_t* __restrict__ b, int64_t count, int64_t* __restrict__ out_max_total) {
  __shared__ int64_t wsum[2][16], wmax[16];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  int64_t carry_a = 0, carry_b = 0, m = 0;
  for (int64_t base = 0; base < count; base += 1024 * PER) {
    const int64_t lo = min(count, base + (int64_t)tid * PER), hi = min(count, lo + PER);
    int64_t sa = 0, sb = 0, mx = 0;
    int64_t ra_[PER], rb_[HAS_B ? PER : 1];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      ra_[u] = lo + u < hi ? a[lo + u] : 0;
      if constexpr (HAS_B) rb_[u] = lo + u < hi ? b[lo + u] : 0;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      sa += ra_[u];
      mx = max(mx, ra_[u]);
      if constexpr (HAS_B) sb += rb_[u];
    }
    // exclusive scan of the 1024 per-thread sums: inside a wave by shuffles, across the 16 waves through LDS
    int64_t ia = sa, ib = sb;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const int64_t ya = __shfl_up(ia, off), yb = __shfl_up(ib, off);
      if (lane >= off) { ia += ya; ib += yb; }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
    __syncthreads();   // (the previous round's readers of wsum are done)
    if (lane == WAVE - 1) { wsum[0][wave] = ia; wsum[1][wave] = ib; }
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    int64_t ra = carry_a + ia - sa, rb = carry_b + ib - sb, ta = 0, tb = 0;
#pragma unroll 2
    for (int w = 0; w < 16; ++w) {
      if (w < wave) { ra += wsum[0][w]; rb += wsum[1][w]; }
      ta += wsum[0][w];
      tb += wsum[1][w];
      m = max(m, wmax[w]);
    }
    carry_a += ta;
    carry_b += tb;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (lo + u < hi) {
        a[lo + u] = ra;
        if constexpr (HAS_B) b[lo + u] = rb;
      }
      ra += ra_[u];
      if constexpr (HAS_B) rb += rb_[u];
    }
  }
  if (tid == 0) {
    a[count] = carry_a;
    if (HAS_B && b) b[count] = carry_b;
    if (out_max_total) { out_max_total[0] = m; out_max_total[1] = carry_a; }
  }
}

void launch_small_scan(int64_t* a, int64_t* b, int64_t count, int64_t* out_max_total, hipStream_t s) {
  const int64_t per = (count + 1023) / 1024;
  if (b && per <= 8) hipLaunchKernelGGL((small_scan_kernel<8, true>), dim3(1), dim3(1024), 0, s, a, b, count, out_max_total);
  else if (b) hipLaunchKernelGGL((small_scan_kernel<16, true>), dim3(1), dim3(1024), 0, s, a, b, count, out_max_total);
  else hipLaunchKernelGGL((small_scan_kernel<24, false>), dim3(1), dim3(1024), 0, s, a, b, count, out_max_total);
}

// ---- A^T's format straight from A through per-chunk buckets (no transposed CSR, no sort) -----------------------
// The transposition route moves every entry five times (pack, two radix passes, statistics, fill).  Here a histogram
// pass counts the entries of every (tile of A rows, column), which is all the quad counting needs; a scatter pass drops
// every entry of A into the bucket of its chunk (block of A^T rows, tile) as {slot in the block, row in the tile, value};
// one workgroup per chunk then ranks the entries of every A^T row by their row in the tile with per-slot bit masks (the
// ranks of the column-sorted transposed row) and writes the chunk's region of the format, padding included.  The bytes
// are those of the other routes.  The column statistics come from the finished chunks: every (tile, A^T row) segment is
// summed in its stored order, the per-tile partial sums are added in tile order (a fixed order: reproducible).
constexpr int ATD_MAX_COLS = 65536;       // the histogram keeps two 16-bit counters per LDS word
constexpr int ATD_THREADS = 1024;
constexpr int ATD_MASK_WORDS = 10;        // 320 rows of a tile

constexpr int ATD_HIST_THREADS = 512;   // (a tile per workgroup; eight waves: three or four tiles per CU at once, no second round at C2)
constexpr int ATD_HIST_THREADS_WIDE = 1024;   // histograms above 64 KiB leave one workgroup per CU: sixteen waves then (C5: 100 KB)

// With `bnd` (the gather fill below, natural row order of A^T): A^T's row blocks are contiguous column ranges -- block b
// holds the columns c with (int)((float)c * blk_scale) == b -- and bnd[t * tc + i][b] becomes the position in A's arrays of the first entry of row
// t + i * nct whose column lies in block b or behind (b = 0..nrb; the row's end for the blocks it does not reach), counted
// from the row's first entry (uint32: half the table of round 4's absolute int64 positions, and no memset of it).  A row is
// sorted by column, so these are the places where the block of the column changes: found in the registers that hold the
// row's indices for the histogram anyway.
__global__ void __launch_bounds__(ATD_HIST_THREADS_WIDE)
atd_hist_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t m, int nct, int tc, int64_t n2,
                uint16_t* __restrict__ cnt16, float blk_scale, int nrb, uint32_t* __restrict__ bnd, int64_t* __restrict__ disorder,
                unsigned long long* __restrict__ slots_to_clear) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && slots_to_clear) *slots_to_clear = 0ull;   // (atd_rowlen_kernel, next on this stream, adds to it)
  // disorder: set when a row's entries leave the order the run ends rely on (a block after a later block: the caller handed
  // over rows whose columns do not ascend) -- the host then takes the bucket route, which maps every column through a table
  extern __shared__ uint32_t atd_h32[];   // n2 / 2 words: counters of columns 2w, 2w + 1
  const int t = blockIdx.x;
  const int nw = (int)(n2 / 2);
  const int nthreads = (int)blockDim.x, nwaves = nthreads / WAVE;
  for (int i = threadIdx.x; i < nw; i += nthreads) atd_h32[i] = 0u;
  __syncthreads();
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  // (the next row's offsets are fetched while this row's indices are in flight: a row is one batch at C5's 500 entries)
  int64_t r = (int64_t)t + (int64_t)wave * nct;
  int64_t e0 = (wave < tc && r < m) ? ptr[r] : 0, e1 = (wave < tc && r < m) ? ptr[r + 1] : 0;
  for (int i = wave; i < tc; i += nwaves) {
    if (r >= m) {   // tile rows past the last row of A: empty runs (the table is not cleared beforehand)
      if (bnd)
        for (int j = lane; j <= nrb; j += WAVE) bnd[((int64_t)t * tc + i) * (nrb + 1) + j] = 0u;
      continue;     // (r only grows: every later row of this wave is past the end too)
    }
    const int64_t rn = r + (int64_t)nwaves * nct;
    const bool more = i + nwaves < tc && rn < m;
    const int64_t n0 = more ? ptr[rn] : 0, n1 = more ? ptr[rn + 1] : 0;
    int lastb = -1;   // block of the last entry seen in this row (wave-uniform)
    // a row's run ends side by side, as offsets from the row's first entry (32 bits: a row of A holds fewer than 2^32 entries)
    uint32_t* __restrict__ bnd_row = bnd ? bnd + ((int64_t)t * tc + i) * (nrb + 1) : nullptr;
    const int64_t row_e0 = e0;
    for (int64_t base = e0; base < e1; base += 8 * WAVE) {   // eight loads in flight per lane (a wave-uniform trip count: the
      const int64_t eb = base + lane;                         //  boundary search below talks across lanes)
      int c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = eb + u * WAVE < e1 ? idx[eb + u * WAVE] : -1;
      if (bnd) {   // (ahead of the LDS atomics: nothing here waits on the LDS queue)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool valid = c[u] >= 0;   // (valid lanes are a prefix of the wave)
          const unsigned long long valids = __ballot(valid);
          if (valids == 0ull) break;
          // block of column c: (int)((float)c * scale) -- the partition is DEFINED by this expression (the host derives the
          // block table from the same single-precision product: build_tiled_at_direct), so three instructions decide it
          const int b = (int)((float)max(c[u], 0) * blk_scale);
          const int up = __builtin_amdgcn_update_dpp(0, b, 0x138, 0xf, 0xf, false);   // wave_shr:1 -- lane l reads lane l - 1
          const int prev = lane == 0 ? lastb : up;
          if (valid && b != prev)
            for (int j = prev + 1; j <= b; ++j) bnd_row[j] = (uint32_t)(eb + u * WAVE - row_e0);
          if (valid && b < prev) *disorder = 1;   // (rare, benign race: every writer stores the same value)
          lastb = __builtin_amdgcn_readlane(b, __builtin_popcountll(valids) - 1);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c[u] >= 0) atomicAdd(&atd_h32[c[u] >> 1], 1u << (16 * (c[u] & 1)));   // (at most 320 rows per tile: no carry into the neighbour)
    }
    if (bnd)
      for (int j = lastb + 1 + lane; j <= nrb; j += WAVE) bnd_row[j] = (uint32_t)(e1 - row_e0);
    r = rn;
    e0 = n0;
    e1 = n1;
  }
  __syncthreads();
  uint32_t* out = reinterpret_cast<uint32_t*>(cnt16 + (int64_t)t * n2);
  for (int i = threadIdx.x; i < nw; i += nthreads) out[i] = atd_h32[i];
}

// len[c] = entries of column c (summed over the tiles); the caller scans it into A^T's row offsets.
// A workgroup takes 64 columns, its 16 waves a sixteenth of the tiles each.
__global__ void __launch_bounds__(1024)
atd_rowlen_kernel(const uint16_t* __restrict__ cnt16, int64_t n, int64_t n2, int nct, int64_t* __restrict__ len,
                  unsigned long long* __restrict__ natural_slots) {
  __shared__ uint32_t part[16][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const int per = (nct + 15) / 16;
  uint32_t a = 0;
  if (c < n) {
    // (eight independent loads in flight: one dependent round trip per tile made this small kernel 66 us at C2's 625 tiles)
    const int t1 = min(nct, (grp + 1) * per);
    int t = grp * per;
    for (; t + 8 <= t1; t += 8) {
      uint32_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = cnt16[(int64_t)(t + u) * n2 + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; t < t1; ++t) a += cnt16[(int64_t)t * n2 + c];
  }
  part[grp][lane] = a;
  __syncthreads();
  if (grp == 0) {
    int64_t total = 0;
    if (c < n)
      for (int g = 0; g < 16; ++g) total += part[g][lane];
    if (c <= n) len[c] = total;   // (len[n] = 0: the scan turns it into the total)
    // what the quads would hold if A^T's rows kept their natural order: 4 x the longest of every four consecutive rows
    // (natural_quad_slots_kernel's sum, gathered here: the builder then needs neither that kernel nor the memset in front of it)
    if (natural_slots) {
      int64_t mx = max(total, __shfl_xor(total, 1));
      mx = max(mx, __shfl_xor(mx, 2));
      unsigned long long acc = (lane & 3) == 0 ? (unsigned long long)(4 * mx) : 0ull;
#pragma unroll
      for (int off = WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
      if (lane == 0 && acc) atomicAdd(natural_slots, acc);
    }
  }
}

// colmap[row of A^T] = block << 10 | slot inside the block
__global__ void atd_colmap_kernel(const int32_t* __restrict__ blk, int nrb, const uint32_t* __restrict__ perm, int64_t rows,
                                  uint32_t* __restrict__ colmap) {
  const int64_t sp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sp >= rows) return;
  int lo = 0, hi = nrb;   // last block with blk[b] <= sp
  while (lo + 1 < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)blk[mid] <= sp) lo = mid; else hi = mid;
  }
  const int64_t row = perm ? (int64_t)perm[sp] : sp;
  colmap[row] = ((uint32_t)lo << 10) | (uint32_t)(sp - blk[lo]);
}

// one wave per row of A: its entries go to the buckets (block of their column, tile of the row).  Every contiguous run of
// lanes bound for the same bucket reserves its places with one atomic on the bucket's cursor; the atomics of a whole row
// (ten batches of 64 entries) are in flight together.  The order inside a bucket is whatever the atomics make it: the
// fill ranks entries by their row in the tile, not by their place in the bucket.
__global__ void __launch_bounds__(256)
atd_scatter_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const float* __restrict__ val, int64_t m, int nct,
                   int tc, const uint32_t* __restrict__ colmap, const int64_t* __restrict__ bucket_off, uint32_t* __restrict__ cursor,
                   uint2* __restrict__ bucket) {
  const int lane = threadIdx.x & (WAVE - 1);
  // workgroups are dealt to the eight XCDs round-robin: XCD x takes the tiles t = x (mod 8), so the partial lines of a bucket
  // (all its writers handle rows of one tile) meet in one L2 instead of being written back piecemeal from several
  const int xcd = blockIdx.x & 7;
  const int64_t wave = (int64_t)(blockIdx.x >> 3) * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  const int64_t nwaves = (int64_t)(gridDim.x >> 3) * (blockDim.x / WAVE);
  const int tiles_x = (nct - xcd + 7) / 8;                 // tiles of this XCD
  const int64_t items = (int64_t)tiles_x * tc;             // (tile, row in the tile)
  constexpr int UB = 10;
  for (int64_t item = wave; item < items; item += nwaves) {
    const int i = (int)(item / tiles_x), t = xcd + 8 * (int)(item - (int64_t)i * tiles_x);
    const int64_t r = (int64_t)t + (int64_t)i * nct;
    if (r >= m) continue;
    const int64_t e1 = ptr[r + 1];
    for (int64_t eb = ptr[r]; eb < e1; eb += UB * WAVE) {
      int cc[UB];
      uint32_t cmv[UB];
      float vv[UB];
      int64_t base[UB];
      int mine[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int64_t e = eb + u * WAVE + lane;
        cc[u] = e < e1 ? idx[e] : -1;
        vv[u] = e < e1 ? val[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) cmv[u] = cc[u] >= 0 ? colmap[cc[u]] : 0xffffffffu;
      // run leaders reserve: nothing below waits for an atomic before all of them are issued
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const uint32_t rb = cmv[u] >> 10;
        const uint32_t prev = __shfl_up(rb, 1);
        const bool valid = cc[u] >= 0;
        const bool leader = valid && (lane == 0 || rb != prev);
        const unsigned long long leaders = __ballot(leader), valids = __ballot(valid);
        const unsigned long long upto = leaders & ((2ull << lane) - 1ull);   // leaders at or before this lane
        mine[u] = upto ? 63 - __builtin_clzll(upto) : 0;
        base[u] = 0;
        if (leader) {
          const unsigned long long above = leaders & ~((2ull << lane) - 1ull);   // leaders past this lane
          const int next = above ? __builtin_ctzll(above) : __builtin_popcountll(valids);   // (valid lanes are a prefix)
          const int64_t b = (int64_t)rb * nct + t;
          base[u] = bucket_off[b] + (int64_t)atomicAdd(&cursor[b], (uint32_t)(next - lane));
        }
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int64_t b0 = __shfl(base[u], mine[u]);
        if (cc[u] >= 0)
          bucket[b0 + (lane - mine[u])] = make_uint2(((cmv[u] & 1023u) << 9) | (uint32_t)i, __float_as_uint(vv[u]));
      }
    }
  }
}

// one workgroup per chunk: ranks from per-slot bit masks over the tile's rows, the chunk's region of the format
// assembled in LDS a few dozen quads at a time (written out in whole lines, padding included), the partial column sums
// of this tile from the assembled segments
constexpr int ATD_STAGE_ENT = 4096;   // entries of the LDS image (a quad holds at most 4 x 320)

// GATHER (natural row order of A^T: a block is a contiguous column range): the chunk's entries come straight from A -- in
// every row of the tile the columns of the block are one contiguous run, whose ends atd_hist_kernel left in `bnd` -- and
// there are no buckets and no scatter pass.  A thread takes every 1024th entry of the concatenated runs.
template <bool GATHER>
__global__ void __launch_bounds__(ATD_THREADS, 8)   // 64 VGPRs: two workgroups per CU
atd_fill_kernel(const uint2* __restrict__ bucket, const int64_t* __restrict__ bucket_off, const int32_t* __restrict__ blk_row0,
                const uint32_t* __restrict__ perm, int nct, int ldp_bytes, const int64_t* __restrict__ chunk_off,
                const uint32_t* __restrict__ quad_off, const uint16_t* __restrict__ steps, Ent* __restrict__ ent,
                double* __restrict__ psum, double* __restrict__ psq, int64_t n,
                const int32_t* __restrict__ a_idx, const float* __restrict__ a_val, const uint32_t* __restrict__ bnd,
                const int64_t* __restrict__ a_ptr, int64_t a_rows, int tc, int nrb_all) {
  // one pool: the rows' bit masks (40 KiB) and the image the chunk is assembled in (32 KiB); once the ranks are known the
  // masks are dead and the image takes the whole pool (chunks whose entries the threads hold in registers)
  constexpr int MASK_WORDS_ALL = QBLOCK_ROWS * ATD_MASK_WORDS;
  __shared__ __attribute__((aligned(16))) uint32_t pool[MASK_WORDS_ALL + 2 * ATD_STAGE_ENT];
  uint32_t* mask = pool;
  Ent* stage = reinterpret_cast<Ent*>(pool + MASK_WORDS_ALL);
  __shared__ uint32_t qoff_s[Q_BLOCK_QUADS + 1];
  __shared__ uint32_t wtot[Q_BLOCK_QUADS / WAVE];
  __shared__ uint16_t len_s[QBLOCK_ROWS];
  __shared__ int64_t run_lo[GATHER ? 32 * ATD_MASK_WORDS : 1];        // first entry of every tile row's run
  __shared__ uint32_t run_pre[GATHER ? 32 * ATD_MASK_WORDS + 1 : 1];  // entries of the runs before it
  __shared__ uint32_t rtot[GATHER ? 32 * ATD_MASK_WORDS / WAVE : 1];
  // GATHER: the chunks of one tile read neighbouring runs of the same rows of A -- they run back to back on one XCD (workgroups
  // are dealt to the eight XCDs round-robin), so a row's lines and pages are fetched once while its blocks pass
  int rb, t;
  if constexpr (GATHER) {   // grid: 8 x ceil(nct / 8) x nrb workgroups; XCD x takes the tiles t = x (mod 8), block after block
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    t = xcd + 8 * (j / nrb_all);
    rb = j % nrb_all;
    if (t >= nct) return;
  } else {
    rb = (int)(blockIdx.x / nct);
    t = (int)(blockIdx.x % nct);
  }
  const int64_t chunk = (int64_t)rb * nct + t;
  const int row0 = blk_row0[rb], nrows = blk_row0[rb + 1] - row0;
  const int nquads = (nrows + 3) / 4;
  for (int i = threadIdx.x; i < QBLOCK_ROWS * ATD_MASK_WORDS; i += ATD_THREADS) mask[i] = 0u;
  // entry offsets of the quads inside the chunk: the scan of their step counts (4 entries per step)
  if (threadIdx.x < Q_BLOCK_QUADS) {
    const int q = threadIdx.x, lane = q & (WAVE - 1);
    const uint32_t sz = q < nquads ? 4u * (uint32_t)steps[chunk * Q_BLOCK_QUADS + q] : 0u;
    uint32_t inc = sz;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const uint32_t y = __shfl_up(inc, off);
      if (lane >= off) inc += y;
    }
    qoff_s[q + 1] = inc;                       // inclusive, within the wave
    if (lane == WAVE - 1) wtot[q / WAVE] = inc;
  }
  if constexpr (GATHER) {
    if (threadIdx.x < 32 * ATD_MASK_WORDS) {   // (the same first waves; tc <= 320)
      const int i = threadIdx.x, lane = i & (WAVE - 1);
      // (bnd[row][block]: the chunks of one tile, run back to back on this XCD, read neighbouring words of the same lines)
      const uint32_t* br = bnd + ((int64_t)t * tc + i) * (nrb_all + 1) + rb;
      const int64_t arow = (int64_t)t + (int64_t)i * nct;                 // the row of A behind tile row i
      const int64_t e0 = (i < tc && arow < a_rows) ? a_ptr[arow] : 0;
      const int64_t lo = i < tc ? e0 + br[0] : 0;
      const int64_t hi = i < tc ? e0 + br[1] : 0;
      run_lo[i] = lo;
      uint32_t inc = hi > lo ? (uint32_t)(hi - lo) : 0u;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
      }
      run_pre[i + 1] = inc;
      if (lane == WAVE - 1) rtot[i / WAVE] = inc;
    }
  }
  __syncthreads();
  if (threadIdx.x < Q_BLOCK_QUADS) {
    uint32_t add = 0;
    for (int w = 0; w < (int)threadIdx.x / WAVE; ++w) add += wtot[w];
    qoff_s[threadIdx.x + 1] += add;
    if (threadIdx.x == 0) qoff_s[0] = 0u;
  }
  if constexpr (GATHER) {
    if (threadIdx.x < 32 * ATD_MASK_WORDS) {
      uint32_t add = 0;
      for (int w = 0; w < (int)threadIdx.x / WAVE; ++w) add += rtot[w];
      run_pre[threadIdx.x + 1] += add;
      if (threadIdx.x == 0) run_pre[0] = 0u;
    }
  }
  __syncthreads();
  const int64_t b0 = GATHER ? 0 : bucket_off[chunk];
  const int64_t b1 = GATHER ? (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)run_pre[32 * ATD_MASK_WORDS]) : bucket_off[chunk + 1];
  constexpr int HOLD = 10;   // entries a thread keeps in registers (chunks of up to 10240 entries: one read of the bucket)
  // GATHER: the tile row of each of the first 10240 concatenated entries, written run by run into the (still unused) LDS
  // image -- a thread then finds its entries with one LDS read each instead of a search over the runs
  uint16_t* row_of = reinterpret_cast<uint16_t*>(stage);
  if constexpr (GATHER) {
    if (threadIdx.x < 3 * 32 * ATD_MASK_WORDS) {   // three threads per run
      const uint32_t i = threadIdx.x / 3u;
      const uint32_t k1 = min(run_pre[i + 1], (uint32_t)(HOLD * ATD_THREADS));
      for (uint32_t k = run_pre[i] + threadIdx.x % 3u; k < k1; k += 3u) row_of[k] = (uint16_t)i;
    }
    __syncthreads();
  }
  // entry f of the chunk as {slot in the block << 9 | row in the tile, value}
  auto fetch = [&](int64_t f, bool tabled) -> uint2 {
    if constexpr (GATHER) {
      int lo = 0;
      if (tabled) {
        lo = row_of[f];
      } else {
        int hi = 32 * ATD_MASK_WORDS - 1;   // the last row with run_pre[row] <= f
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if ((int64_t)run_pre[mid] <= f) lo = mid; else hi = mid - 1;
        }
      }
      const int64_t e = run_lo[lo] + (f - (int64_t)run_pre[lo]);
      return make_uint2(((uint32_t)(a_idx[e] - row0) << 9) | (uint32_t)lo, __float_as_uint(a_val[e]));
    } else {
      return bucket[f];
    }
  };
  Ent* dst = ent + chunk_off[chunk];
  uint2 kv[HOLD];
#pragma unroll
  for (int u = 0; u < HOLD; ++u) {
    const int64_t e = b0 + threadIdx.x + (int64_t)u * ATD_THREADS;
    kv[u] = e < b1 ? fetch(e, true) : make_uint2(0xffffffffu, 0u);
  }
#pragma unroll
  for (int u = 0; u < HOLD; ++u)
    if (kv[u].x != 0xffffffffu) {
      const uint32_t slot = kv[u].x >> 9, i = kv[u].x & 511u;
      atomicOr(&mask[slot * ATD_MASK_WORDS + (i >> 5)], 1u << (i & 31u));
    }
  for (int64_t e = b0 + threadIdx.x + (int64_t)HOLD * ATD_THREADS; e < b1; e += ATD_THREADS) {   // (longer chunks: the rest from memory)
    const uint32_t key = fetch(e, false).x;
    const uint32_t slot = key >> 9, i = key & 511u;
    atomicOr(&mask[slot * ATD_MASK_WORDS + (i >> 5)], 1u << (i & 31u));
  }
  __syncthreads();
  // Set bits in the mask words before each word, per slot (round 5: a rank was up to ten LDS reads and popcounts; now two reads).
  // The table takes the place of `row_of`, which nobody reads once the held entries are fetched; chunks too long to be held
  // assemble their image there later and keep the loop over the words.
  const bool held = b1 - b0 <= (int64_t)HOLD * ATD_THREADS;   // no entry is ranked again below: the masks' LDS joins the image
  uint16_t* pre = reinterpret_cast<uint16_t*>(stage);        // [QBLOCK_ROWS][ATD_MASK_WORDS]
  for (int slot = threadIdx.x; slot < QBLOCK_ROWS; slot += ATD_THREADS) {   // (and the entries of every row of the block in this tile)
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < ATD_MASK_WORDS; ++w) {
      if (held) pre[slot * ATD_MASK_WORDS + w] = (uint16_t)run;
      run += __builtin_popcount(mask[slot * ATD_MASK_WORDS + w]);
    }
    len_s[slot] = (uint16_t)run;
  }
  __syncthreads();
  // rank of an entry inside its (A^T row, tile) segment = the rows of the tile before its own that hold the column
  auto rank_of = [&](uint32_t slot, uint32_t i) {
    const uint32_t* mk = mask + slot * ATD_MASK_WORDS;
    uint32_t rank = __builtin_popcount(mk[i >> 5] & ((1u << (i & 31u)) - 1u));
    if (held) return rank + (uint32_t)pre[slot * ATD_MASK_WORDS + (i >> 5)];
    for (uint32_t w = 0; w < (i >> 5); ++w) rank += __builtin_popcount(mk[w]);
    return rank;
  };
#pragma unroll
  for (int u = 0; u < HOLD; ++u) {   // the key becomes {place in the chunk (23 bits), row in the tile << 23}: the loop over the image below only places
    if (kv[u].x != 0xffffffffu) {
      const uint32_t slot = kv[u].x >> 9, i = kv[u].x & 511u;
      kv[u].x = (qoff_s[slot >> 2] + rank_of(slot, i) * 4u + (slot & 3u)) | (i << 23);
    }
    asm volatile("" ::: "memory");   // (one entry's LDS reads at a time: twelve unrolled copies in flight cost 128 VGPRs)
  }
  // The image is two halves: while one run of quads is written out (and summed), the next is assembled in the other half --
  // one barrier per run.  Slots are written exactly once: entries by the threads that hold them, the padding behind a
  // row's last entry by a thread per row.
  const uint32_t HALF = held ? (uint32_t)(MASK_WORDS_ALL / 2 + ATD_STAGE_ENT) / 2u : (uint32_t)ATD_STAGE_ENT / 2u;   // (a quad holds at most 4 x 320 entries)
  Ent* const image = held ? reinterpret_cast<Ent*>(pool) : stage;
  __syncthreads();   // (every rank is known: the image may take the masks' and the table's LDS)
  auto row_len = [&](int slot) { return (int)len_s[slot]; };
  int half = 0;
  for (int q0 = 0; q0 < nquads; half ^= 1) {
    // the next run of quads whose segments fit half the image
    int q1 = q0 + 1;
    {
      int lo = q0 + 1, hi = nquads;   // largest q1 with qoff[q1] - qoff[q0] <= HALF
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (qoff_s[mid] - qoff_s[q0] <= HALF) lo = mid; else hi = mid - 1;
      }
      q1 = __builtin_amdgcn_readfirstlane(lo);   // (every thread finds the same run: keep it in scalar registers)
    }
    Ent* st = image + (half ? HALF : 0u);
    const uint32_t o0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)qoff_s[q0]);
    const uint32_t size = (uint32_t)__builtin_amdgcn_readfirstlane((int)qoff_s[q1]) - o0;
    for (int slot = 4 * q0 + (int)threadIdx.x; slot < 4 * q1; slot += ATD_THREADS) {   // padding
      const uint32_t qo = qoff_s[slot >> 2], nsteps = (qoff_s[(slot >> 2) + 1] - qo) / 4u;
      const uint32_t o = qo - o0 + (uint32_t)(slot & 3);
#pragma clang loop vectorize(disable) unroll(disable)
      for (uint32_t k = slot < nrows ? (uint32_t)row_len(slot) : 0u; k < nsteps; ++k) st[o + 4u * k] = Ent{0u, 0.f};
    }
    auto place = [&](uint32_t slot, uint32_t i, uint32_t rank, uint32_t vbits) {
      const int q = (int)(slot >> 2);
      if (q < q0 || q >= q1) return;
      Ent x;
      x.off = i * (uint32_t)ldp_bytes;
      x.val = __uint_as_float(vbits);
      st[qoff_s[q] - o0 + rank * 4u + (slot & 3u)] = x;
    };
#pragma unroll
    for (int u = 0; u < HOLD; ++u) {   // (an empty hold has the place 2^23 - 1: never inside a run)
      const uint32_t at = (kv[u].x & 0x7fffffu) - o0;
      if (at < size) {
        Ent x;
        x.off = (kv[u].x >> 23) * (uint32_t)ldp_bytes;
        x.val = __uint_as_float(kv[u].y);
        st[at] = x;
      }
    }
    for (int64_t e = b0 + threadIdx.x + (int64_t)HOLD * ATD_THREADS; e < b1; e += ATD_THREADS) {
      const uint2 x = fetch(e, false);
      const uint32_t slot = x.x >> 9, i = x.x & 511u;
      const int q = (int)(slot >> 2);
      if (q >= q0 && q < q1) place(slot, i, rank_of(slot, i), x.y);
    }
    __syncthreads();   // (this half is complete; the other one was read out before the previous barrier)
    // (segments are multiples of 4 entries: 16-byte pieces)
    {
      const uint4* src4 = reinterpret_cast<const uint4*>(st);
      uint4* dst4 = reinterpret_cast<uint4*>(dst + o0);
      for (uint32_t i = threadIdx.x; i < size / 2; i += ATD_THREADS) dst4[i] = src4[i];
    }
    if (psum) {
      // two threads per row: the entries at even and at odd places of its segment, added in stored order, then the two halves
      const int pairs = 2 * (min(4 * q1, nrows) - 4 * q0);
      for (int pr = (int)threadIdx.x; pr < pairs; pr += ATD_THREADS) {
        const int slot = 4 * q0 + (pr >> 1), part = pr & 1;
        const int len = row_len(slot);
        const uint32_t o = qoff_s[slot >> 2] - o0 + (uint32_t)(slot & 3);
        double a = 0, b = 0;
#pragma clang loop vectorize(disable) unroll(disable)
        for (int k = part; k < len; k += 2) {
          const double v = (double)st[o + 4u * k].val;
          a += v;
          b += v * v;
        }
        a += __shfl_xor(a, 1);
        b += __shfl_xor(b, 1);
        if (part == 0) {
          const int64_t row = perm ? (int64_t)perm[row0 + slot] : (int64_t)row0 + slot;
          psum[(int64_t)t * n + row] = a;
          psq[(int64_t)t * n + row] = b;
        }
      }
    }
    q0 = q1;
  }
}

// sum[c] = the per-tile partial sums of column c added in a fixed order: sixteen runs of consecutive tiles, then the runs
__global__ void __launch_bounds__(1024)
atd_stats_reduce_kernel(const double* __restrict__ psum, const double* __restrict__ psq, int64_t n, int nct,
                        double* __restrict__ sum, double* __restrict__ sumsq) {
  __shared__ double pa[16][64], pb[16][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const int per = (nct + 15) / 16;
  double a = 0, b = 0;
  if (c < n)
    for (int t = grp * per; t < min(nct, (grp + 1) * per); ++t) {
      a += psum[(int64_t)t * n + c];
      b += psq[(int64_t)t * n + c];
    }
  pa[grp][lane] = a;
  pb[grp][lane] = b;
  __syncthreads();
  if (grp == 0 && c < n) {
    double x = 0, y = 0;
    for (int g = 0; g < 16; ++g) {
      x += pa[g][lane];
      y += pb[g][lane];
    }
    sum[c] = x;
    sumsq[c] = y;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------- host side
// A build is: the operator's geometry (one pure function), one eligibility test before anything is queued, then named
// stages on the caller's stream -- index the rows, count the chunks (the build's host exchange), publish the TiledOp, fork
// the DPP-fed sweep's tables, choose a fill, launch it.  VT = float: every route.  VT = double: the same format with
// 16-byte entries, from a CSR or a tile-major CSR; its 64-column panel rows are 512 bytes, so the geometry is that of
// 128-float panels -- `ldp` in QuadGeometry is the row length in FLOAT units.

// What build_tiled_at_direct's histogram pass hands the builder (QuadSource::FromA): S describes A^T (row offsets only),
// the entries come from A itself.  buf.misc already holds the natural quads' slot count (atd_rowlen_kernel).
struct AtDirectSrc {
  const CsrView<float>* A;
  const uint16_t* cnt16;   // [tile][column] entry counts, row stride n2
  int64_t n2;
  DevBuf* scratch;         // buckets, column map, partial sums, bucket cursors
  double* stats;           // out: sum | sumsq per column of A (may be null)
  const uint32_t* bnd;     // gather fill: ends of every (A^T row block, A row) run for `nrb_nat` natural blocks (or null)
  int64_t nrb_nat;
  const std::vector<int32_t>* blk_nat;   // ... and where those blocks start (float_blocks below)
};

namespace {

// The builder's debug switches (switches.h), read once per build.  A release library reads no environment: every member
// is a constant there.
struct BuildSwitches {
  static int number(const char* value, int otherwise) { return value ? atoi(value) : otherwise; }
  bool no_dq = dbg_on("SAPCA_NO_DQ");
  bool no_rowsort = dbg_on("SAPCA_NO_ROWSORT"), rowsort_always = dbg_on("SAPCA_ROWSORT_ALWAYS");
  bool fill_direct = dbg_on("SAPCA_FILL_DIRECT"), qf_cap_fixed = dbg_on("SAPCA_QF_CAP_FIXED");
  bool at_sort = dbg_on("SAPCA_AT_SORT");         // A/B: the transposition (radix sort) route instead of A -> A^T
  bool at_buckets = dbg_on("SAPCA_AT_BUCKETS");   // A/B: the bucket fill also where the gather fill applies (the same bytes)
  bool debug = dbg_on("SAPCA_DEBUG");
  int dq_block_rows = number(dbg_env("SAPCA_DQ_BLOCK_ROWS"), 0), split_wgs = number(dbg_env("SAPCA_SPLIT_WGS"), 0);
  int runs_seg_lds_max = number(dbg_env("SAPCA_RUNS_SEG_LDS_MAX"), 1024);   // tiles; above: the streaming fill reads its bounds from global memory
};

// Words of buf.misc (int64 each), and of the page-locked block the builder's one host exchange lands in.
enum MiscWord { kMiscMaxChunk = 0, kMiscTotal = 1, kMiscNaturalSlots = 4, kMiscDisorder = 6, kMiscWords = 8 };
// kPinMisc + w: buf.misc word w, read back as one run from word 0; the block table is staged behind it on its way up
enum PinnedWord { kPinNaturalSlots = 0, kPinMisc = 1, kPinBlocks = 8 };
static_assert(kPinMisc + kMiscDisorder < kPinBlocks, "the read-back run of buf.misc ends ahead of the staged block table");
constexpr size_t kPinBlockTable = 2 * 65536;   // block tables of up to this many (int32) entries are staged there
inline int64_t* misc_words(TiledBuffers& buf) { return buf.misc.as<int64_t>(kMiscWords); }

// The natural blocks of the gather fill: block_of(c) = (int)((float)c * scale), with the scale taken down from nrb / n until
// the last column lands in block nrb - 1.  Host and device evaluate the same IEEE single-precision product, so the table
// below IS the device's partition; blocks differ from n / nrb columns by one at most and none is empty (scale <= 1).
void float_blocks(int64_t n, int64_t nrb, std::vector<int32_t>& blk, float& scale) {
  scale = (float)nrb / (float)n;
  auto block_of = [&](int64_t c) { return (int64_t)(int)((float)(int)c * scale); };
  while (block_of(n - 1) > nrb - 1) scale = std::nextafterf(scale, 0.0f);
  blk.assign((size_t)nrb + 1, (int32_t)n);
  int64_t b = 0;
  blk[0] = 0;
  for (int64_t c = 0; c < n; ++c) {
    const int64_t bc = block_of(c);
    while (b < bc) blk[(size_t)++b] = (int32_t)c;
  }
  while (b < nrb) blk[(size_t)++b] = (int32_t)n;   // (blocks past the last column: empty; cannot happen while nrb <= n)
}

// rows per block of the DPP-fed sweep's operators, and the natural (unsorted) partition of `op_rows` rows: block count and
// the split of the tile range over workgroups
int dq_block_rows(int64_t op_rows, const BuildSwitches& sw) {
  return sw.dq_block_rows == 512 || sw.dq_block_rows == 1024 ? sw.dq_block_rows : (op_rows >= 1024 * 16 ? 1024 : 512);
}
void natural_partition(int64_t op_rows, int nct, int block_rows, const BuildSwitches& sw, int64_t& nrb, int& nsplit) {
  nrb = (op_rows + block_rows - 1) / block_rows;
  nsplit = 1;
  if (nrb >= 192) {
    nrb = round_up(nrb, 256);
  } else {
    // few row blocks (A^T): split the tile range so that (blocks x splits) lands just under a
    // multiple of the 256 CUs -- one workgroup per CU per round, no half-empty last round
    // 1024-row blocks fill a CU's LDS and registers alone: one workgroup per CU; the others run two per CU
    const int64_t split_wgs = sw.split_wgs > 0 ? sw.split_wgs : (block_rows > 512 ? 256 : 512);
    nsplit = (int)std::min<int64_t>(nct, std::max<int64_t>(1, split_wgs / nrb));
    const int64_t nrb_fit = split_wgs / nsplit;
    if (nrb_fit >= nrb && nrb_fit <= op_rows) nrb = nrb_fit;
  }
}

// workgroups of the staged fill: one per quad.  (The kernel can walk several quads per workgroup -- -DSAPCA_QF_WGS=n caps the
// grid: measured at C2 / C4 with 1024, 2048, 4096 workgroups, round 4: the same 2.0 ms preparation at C2 and +0.8 ms at C4
// (gpurun_out/r4_ab_qf.txt, r4_ab_c4.txt) -- the fill runs beside A^T's builder, which holds every wave slot of a CU while
// its workgroups are resident, so what this kernel gets are the gaps, and short-lived workgroups fill gaps best.)
inline unsigned qf_grid(int64_t nquads) {
#ifdef SAPCA_QF_WGS
  const int64_t wgs = SAPCA_QF_WGS;
#else
  const int64_t wgs = nquads;
#endif
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(nquads, wgs));
}

// ---- geometry and eligibility ----------------------------------------------------------------------------------------
// Everything about an operator's format that follows from its shape alone; every quantity has its one formula here.
struct QuadGeometry {
  int64_t rows = 0, cols = 0, nnz = 0;   // of the operator the format is for (A^T's on the A -> A^T route)
  int elem = 4;                          // bytes per value: 4 or 8
  int ldp = 0;                           // panel row length in floats
  int tc = 0, nct = 0;                   // panel rows per column tile, interleaved column tiles
  float inv_nct = 0.f;
  bool dq_candidate = false;             // the DPP-fed sweep may take it: its tile split, and 1024-row blocks where there are 16 of them
  int block_rows = 0;                    // most rows of a row block
  int stage_cap = 0;                     // most entries of a chunk the staged-entry sweep holds in LDS
  int64_t nrb = 0;                       // the natural partition: row blocks, and the split of the tile range over workgroups
  int nsplit = 1;
  bool empty() const { return rows == 0 || cols == 0 || nnz == 0; }
};

inline int tile_count(int64_t cols, int ldp) { return (int)((cols + q_tile_rows(ldp) - 1) / q_tile_rows(ldp)); }

// (an empty operator has no tiles to divide by: its partition stays unset, and eligible() refuses it)
QuadGeometry quad_geometry(int64_t rows, int64_t cols, int64_t nnz, int elem, int ldp_elems, const BuildSwitches& sw) {
  QuadGeometry g;
  g.rows = rows; g.cols = cols; g.nnz = nnz; g.elem = elem;
  g.ldp = ldp_elems * elem / 4;
  g.tc = q_tile_rows(g.ldp);
  g.nct = tile_count(cols, g.ldp);
  // (the DPP-fed sweep double-buffers the default 80 KiB tile and holds 8 or 16 row slots per lane group: f32 operators
  // with 64-column tiles keep that split, and take 1024-row blocks -- half the tile refills and barriers per entry --
  // when the operator has at least 16 of them (A^T of a tall matrix: the tile range is split over workgroups instead))
  g.dq_candidate = elem == 4 && g.ldp == 64 && !sw.no_dq;
  g.block_rows = g.dq_candidate ? dq_block_rows(rows, sw) : QWAVES * QGROUPS * q_rows_per_group(g.ldp);
  g.stage_cap = q_stage_cap(Q_TILE_BYTES, elem == 4 ? (int)sizeof(Ent) : (int)sizeof(EntD));
  if (g.empty()) return g;
  g.inv_nct = 1.0f / (float)g.nct;
  // row blocks of <= block_rows rows.  With enough rows the block count is a multiple of the 256 CUs (every
  // CU runs the same number of workgroups); with few rows (A^T) the tile range is split instead.
  natural_partition(rows, g.nct, g.block_rows, sw, g.nrb, g.nsplit);
  return g;
}

// Does this source's route build this operator?  Geometry and source only: asked before anything is queued.
bool eligible(const QuadGeometry& g, const QuadSource& src) {
  const bool f32 = g.elem == 4, tile_major = src.kind != QuadSource::Csr;
  if (g.empty()) return false;
  if (!f32 && (src.kind == QuadSource::TileMajorPacked || src.kind == QuadSource::FromA)) return false;   // f32 routes
  // float-reciprocal tile arithmetic; LDS tables of the builders
  if (g.cols >= (1 << 24) || g.nct > (tile_major ? Q_MAX_TILES_RUNS : 4096)) return false;
  // A -> A^T: 16-bit histogram counters per column of A, bit masks over a tile's rows, operators of the DPP-fed sweep
  if (src.kind == QuadSource::FromA)
    return g.rows <= ATD_MAX_COLS && g.tc <= 32 * ATD_MASK_WORDS && g.dq_candidate && g.block_rows <= QBLOCK_ROWS;
  return true;
}

// ---- stages ----------------------------------------------------------------------------------------------------------
template <typename VT>
struct Build {   // what the stages of one build share
  const CsrView<VT>& S;
  const QuadGeometry& g;
  const QuadSource& src;
  const BuildSwitches& sw;
  TiledBuffers& buf;
  hipStream_t s;
};

struct Counts {   // what counting leaves: the partition it settled on, the sizes the host needs, the tables on the device
  int64_t nrb = 0;
  int nsplit = 1, tiles_per_split = 0;
  int64_t nchunks = 0, max_chunk = 0, total = 0, mid_row0 = -1;
  bool rows_in_disorder = false;   // (A -> A^T: the histogram pass found rows of A whose columns do not ascend)
  int32_t* d_blk = nullptr;
  uint32_t* d_perm = nullptr;      // slot -> row where the rows were sorted by length; null: natural order
  uint8_t* d_steps = nullptr;
  uint32_t* d_wave_off = nullptr;
  uint32_t* d_quad_off = nullptr;
  int64_t* d_chunk = nullptr;
  int64_t* d_raw = nullptr;        // (A -> A^T) stored entries per chunk, scanned: the bucket offsets
};

// Index the rows: reads S's indices (or packed rows); queues the one kernel that writes seg[row][tile] into buf.seg -- none
// where at_stats_index left it there, none on the A -> A^T route (buf.seg holds its histogram, null is returned); no wait.
template <typename VT>
const int32_t* index_rows(const Build<VT>& b) {
  const QuadGeometry& g = b.g;
  const CsrView<VT>& S = b.S;
  if (b.src.kind == QuadSource::FromA) return nullptr;
  int32_t* d_seg = b.buf.seg.template as<int32_t>((size_t)S.rows * (g.nct + 1));
  if (b.src.kind == QuadSource::Csr) {
    hipLaunchKernelGGL(tile_hist_kernel, dim3(grid_for(S.rows, 4, 8192)), dim3(256), (size_t)4 * g.nct * sizeof(uint32_t), b.s,
                       S.ptr, S.idx, S.rows, g.nct, g.inv_nct, d_seg);
  } else if (!b.src.seg_ready) {
    hipLaunchKernelGGL(tile_index_mod_kernel, dim3(grid_for(S.rows * (int64_t)(g.nct + 1), 256, 16384)), dim3(256), 0, b.s,
                       S.ptr, S.idx, b.src.packed, S.rows, g.nct, g.inv_nct, d_seg);
  }
  return d_seg;
}

// Sort the rows by length, longest first: reads S.ptr; queues the key kernel, the radix sort and the copy of the sorted
// lengths to `sorted_len`; WAITS for the host.  Returns the slot -> row permutation (buf.perm).
// Why sort: the four rows of a quad and the quads of a wave then have similar lengths in every (interleaved) tile, which
// keeps the quad padding and the per-tile barrier wait small on matrices with skewed row lengths (cell depth, gene
// detection rate).  Blocks are cut from the sorted order with about equal entry counts (cut_blocks).
template <typename VT>
uint32_t* sort_rows_by_length(const Build<VT>& b, std::vector<uint32_t>& sorted_len) {
  const CsrView<VT>& S = b.S;
  hipStream_t s = b.s;
  uint32_t* d_len = b.buf.lens.template as<uint32_t>((size_t)2 * S.rows);
  uint32_t* d_len_sorted = d_len + S.rows;
  uint32_t* d_iota = b.buf.perm.template as<uint32_t>((size_t)2 * S.rows);
  uint32_t* d_perm = d_iota + S.rows;
  hipLaunchKernelGGL(row_len_iota_kernel, dim3(grid_for(S.rows, 256, 1 << 30)), dim3(256), 0, s, S.ptr, S.rows, d_len, d_iota);
  size_t sb = 0;
  SAPCA_HIP(rocprim::radix_sort_pairs_desc(nullptr, sb, d_len, d_len_sorted, d_iota, d_perm, (size_t)S.rows, 0u, 32u, s));
  char* tmp = static_cast<char*>(b.buf.tmp.ensure(sb + 256));
  SAPCA_HIP(rocprim::radix_sort_pairs_desc(tmp, sb, d_len, d_len_sorted, d_iota, d_perm, (size_t)S.rows, 0u, 32u, s));
  sorted_len.resize((size_t)S.rows);
  SAPCA_HIP(hipMemcpyAsync(sorted_len.data(), d_len_sorted, sorted_len.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  return d_perm;
}

// The speculation on the natural row order: reads S.ptr; queues the count of the slots the natural quads would hold (on
// the A -> A^T route atd_rowlen_kernel has left it in buf.misc) and its copy to pinned[kPinNaturalSlots]; no wait.
template <typename VT>
void queue_natural_slots(const Build<VT>& b, int64_t* pinned) {
  const CsrView<VT>& S = b.S;
  unsigned long long* d_slots = reinterpret_cast<unsigned long long*>(misc_words(b.buf)) + kMiscNaturalSlots;
  if (b.src.kind != QuadSource::FromA) {
    SAPCA_HIP(hipMemsetAsync(d_slots, 0, sizeof(unsigned long long), b.s));
    hipLaunchKernelGGL(natural_quad_slots_kernel, dim3(grid_for((S.rows + 3) / 4, 256, 1024)), dim3(256), 0, b.s, S.ptr, S.rows, d_slots);
  }
  SAPCA_HIP(hipMemcpyAsync(pinned + kPinNaturalSlots, d_slots, sizeof(unsigned long long), hipMemcpyDeviceToHost, b.s));
}

// The block table of one counting attempt (host only).  Sorted rows: a greedy cut, which also decides nrb; natural order:
// nrb equal blocks, or the column ranges the A -> A^T histogram recorded its run ends for.
std::vector<int32_t> cut_blocks(const QuadGeometry& g, const QuadSource& src, const std::vector<uint32_t>* sorted_len, int64_t& nrb) {
  std::vector<int32_t> blk;
  if (sorted_len) {
    // close a block at block_rows rows or at the per-block entry budget
    const double budget = (double)g.nnz / (double)nrb;
    blk.push_back(0);
    double acc = 0;
    int in_block = 0;
    for (int64_t r = 0; r < g.rows; ++r) {
      acc += (*sorted_len)[(size_t)r];
      ++in_block;
      const bool last = r + 1 == g.rows;
      if (last || in_block == g.block_rows || acc >= budget * (double)blk.size()) {
        blk.push_back((int32_t)(r + 1));
        in_block = 0;
      }
    }
    nrb = (int64_t)blk.size() - 1;
  } else if (src.kind == QuadSource::FromA && src.from_a->bnd && nrb == src.from_a->nrb_nat) {
    blk = *src.from_a->blk_nat;
  } else {
    blk.resize((size_t)nrb + 1);
    for (int64_t b = 0; b <= nrb; ++b) blk[(size_t)b] = (int32_t)(g.rows * b / nrb);
  }
  return blk;
}

// One counting attempt over c.nrb blocks: reads seg (A -> A^T: the histogram); queues the block table's upload,
// quad_count_kernel and the one-workgroup scan of the chunk sizes (A -> A^T: and of the stored-entry counts), then the
// read-back of largest chunk | total (| the disorder flag) into `pinned`; WAITS for the host.
template <typename VT>
void count_once(const Build<VT>& b, const int32_t* d_seg, const std::vector<int32_t>& blk, int64_t* pinned, Counts& c) {
  const int nct = b.g.nct;
  TiledBuffers& buf = b.buf;
  hipStream_t s = b.s;
  const AtDirectSrc* from_a = b.src.kind == QuadSource::FromA ? b.src.from_a : nullptr;
  c.nchunks = c.nrb * nct;
  c.mid_row0 = blk[(size_t)(c.nrb / 2)];
  c.d_blk = buf.blk.as<int32_t>((size_t)c.nrb + 1);
  c.d_steps = buf.steps.as<uint8_t>((size_t)c.nchunks * Q_BLOCK_QUADS * 2);
  c.d_wave_off = buf.wave_off.as<uint32_t>((size_t)c.nchunks * QWAVES);
  c.d_quad_off = buf.quad_off.as<uint32_t>((size_t)c.nchunks * Q_BLOCK_QUADS);
  c.d_chunk = buf.chunk_off.as<int64_t>((size_t)c.nchunks + 1);
  if (blk.size() <= kPinBlockTable) {   // (through the page-locked staging: the copy does not wait on a bounce buffer)
    std::memcpy(pinned + kPinBlocks, blk.data(), blk.size() * sizeof(int32_t));
    SAPCA_HIP(hipMemcpyAsync(c.d_blk, pinned + kPinBlocks, blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  } else {
    SAPCA_HIP(hipMemcpyAsync(c.d_blk, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  const dim3 grid((unsigned)(c.nrb * ((nct + QC_TILES - 1) / QC_TILES)));
  if (from_a) {   // (the bucket fill rebuilds the quad offsets from `steps`: none written)
    c.d_raw = buf.raw.as<int64_t>((size_t)c.nchunks + 1);
    hipLaunchKernelGGL(quad_count_kernel, grid, dim3(Q_BLOCK_QUADS), 0, s, d_seg, c.d_blk, c.d_perm, nct, reinterpret_cast<uint16_t*>(c.d_steps),
                       (uint32_t*)nullptr, c.d_wave_off, c.d_chunk, from_a->cnt16, from_a->n2, c.d_raw);
  } else {
    hipLaunchKernelGGL(quad_count_kernel, grid, dim3(Q_BLOCK_QUADS), 0, s, d_seg, c.d_blk, c.d_perm, nct, reinterpret_cast<uint16_t*>(c.d_steps),
                       c.d_quad_off, c.d_wave_off, c.d_chunk);
  }
  int64_t* d_misc = misc_words(buf);
  launch_small_scan(c.d_chunk, c.d_raw, c.nchunks, d_misc + kMiscMaxChunk, s);
  const int words = (from_a ? kMiscDisorder : kMiscTotal) + 1;
  SAPCA_HIP(hipMemcpyAsync(pinned + kPinMisc, d_misc, words * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));  // blk goes out of scope; sizes needed on the host
  if (from_a) c.rows_in_disorder = pinned[kPinMisc + kMiscDisorder] != 0;
  c.max_chunk = pinned[kPinMisc + kMiscMaxChunk];
  c.total = pinned[kPinMisc + kMiscTotal];
}

// Count the chunks: settles the partition and fills `c`.  Homogeneous rows pad little in their natural order, so the
// sort (0.2 ms per operator at C2) is skipped unless the natural quads would hold 10 % more slots than entries: that
// count comes back with the first attempt's sizes -- the natural order is assumed until then (one wait for the device
// instead of two), and a matrix that needs the sort pays for a second round of counting.  The entries of one (row block,
// tile) must fit the staged-entry sweep's LDS staging: skewed inputs (a dense cluster inside one tile) can exceed it --
// the rows per block are halved and counted again, a few times at most.  WAITS for the host once per attempt (and in the
// sort).  Returns false when the operator does not fit: the caller stays on the row kernel.
template <typename VT>
bool count_chunks(const Build<VT>& b, const int32_t* d_seg, Counts& c) {
  const QuadGeometry& g = b.g;
  int64_t* pinned = static_cast<int64_t*>(b.buf.host.ensure((kPinBlocks + kPinBlockTable / 2 + 2) * sizeof(int64_t)));
  std::vector<uint32_t> sorted_len;
  bool sort_rows = !b.sw.no_rowsort, speculate = false;
  if (sort_rows && !b.sw.rowsort_always) {
    queue_natural_slots(b, pinned);
    speculate = true;
    sort_rows = false;
  }
  if (sort_rows) c.d_perm = sort_rows_by_length(b, sorted_len);
  c.nrb = g.nrb;
  c.nsplit = g.nsplit;
  for (int attempt = 0;; ++attempt) {
    c.tiles_per_split = (g.nct + c.nsplit - 1) / c.nsplit;
    c.nsplit = (g.nct + c.tiles_per_split - 1) / c.tiles_per_split;
    const std::vector<int32_t> blk = cut_blocks(g, b.src, sort_rows ? &sorted_len : nullptr, c.nrb);
    count_once(b, d_seg, blk, pinned, c);
    if (speculate) {
      speculate = false;
      if ((double)(unsigned long long)pinned[kPinNaturalSlots] > 1.10 * (double)g.nnz) {   // the natural quads pad too much after all
        sort_rows = true;
        c.d_perm = sort_rows_by_length(b, sorted_len);
        attempt = -1;
        continue;
      }
    }
    if (b.sw.debug)
      fprintf(stderr, "sapca: build_tiled rows %lld cols %lld nrb %lld nct %d split %d max_chunk %lld (cap %d) total %lld\n",
              (long long)g.rows, (long long)g.cols, (long long)c.nrb, g.nct, c.nsplit,
              (long long)c.max_chunk, g.stage_cap, (long long)c.total);
    if (c.max_chunk <= g.stage_cap || g.dq_candidate) return true;   // the DPP-fed sweep stages no entries: nothing to fit
    if (attempt == 3 || c.nrb * 2 > g.rows) return false;
    c.nrb *= 2;
    if (c.nsplit > 1) c.nsplit = std::max(1, c.nsplit / 2);
  }
}

// Publish the TiledOp (host only): geometry, counts and the tables' addresses.  op.valid stays false until the fill is queued.
void publish(TiledOp& op, const QuadGeometry& g, const Counts& c, const void* d_ent) {
  op.rows = g.rows; op.cols = g.cols; op.ldp = g.ldp * 4 / g.elem; op.elem = g.elem; op.tc = g.tc; op.nct = g.nct;
  op.nrb = (int)c.nrb; op.block_rows = g.block_rows; op.max_chunk = c.max_chunk;
  op.nsplit = c.nsplit; op.tiles_per_split = c.tiles_per_split; op.total_entries = c.total; op.tile_bytes = Q_TILE_BYTES;
  op.mid_row0 = c.mid_row0;
  op.blk_row0 = c.d_blk; op.row_perm = c.d_perm; op.chunk_off = c.d_chunk; op.wave_off = c.d_wave_off; op.steps = c.d_steps; op.ent = d_ent;
}

// The DPP-fed sweep's tables depend on the counts only: reads the published tables; f32: queues them on buf.aux between a
// fork event on `s` and a join event the caller waits for -- ahead of the fill, behind which this small kernel would wait
// for a free CU; f64: queues them on `s` itself.  No wait.  Returns whether the DPP-fed sweep takes the operator (an f64
// operator it cannot take stays on the staged-entry sweep).
template <typename VT>
bool fork_dq_tables(TiledOp& op, TiledBuffers& buf, hipStream_t s) {
  bool dq_ok;
  op.valid = true;   // (dq_build_tables looks at it)
  if constexpr (sizeof(VT) == 4) {
    if (!buf.aux) {
      SAPCA_HIP(hipStreamCreateWithFlags(&buf.aux, hipStreamNonBlocking));
      SAPCA_HIP(hipEventCreateWithFlags(&buf.aux_fork, hipEventDisableTiming));
      SAPCA_HIP(hipEventCreateWithFlags(&buf.aux_join, hipEventDisableTiming));
    }
    SAPCA_HIP(hipEventRecord(buf.aux_fork, s));              // counts, offsets and the block table are final here
    SAPCA_HIP(hipStreamWaitEvent(buf.aux, buf.aux_fork, 0));
    dq_ok = dq_build_tables(op, buf, buf.aux);
    SAPCA_HIP(hipEventRecord(buf.aux_join, buf.aux));
  } else {
    dq_ok = dq_build_tables(op, buf, s);
  }
  op.valid = false;
  return dq_ok;
}

// Which kernel writes the entries, and the LDS image of the staged fill (entries of one quad).
enum class Fill {
  Gather,    // A -> A^T, natural blocks: every chunk reads its runs of A's rows itself
  Buckets,   // A -> A^T otherwise: A's entries scattered into per-chunk buckets first
  Runs,      // tile-major rows: streaming, a quad's run in a tile is contiguous in its rows
  Staged,    // CSR: a quad assembled in LDS, written out in contiguous runs; pads itself
  Direct     // CSR, quads too large for the image on average: one store per entry over a zeroed buffer
};
struct FillChoice { Fill fill; int qf_cap; };

FillChoice choose_fill(const QuadGeometry& g, const QuadSource& src, const Counts& c, const BuildSwitches& sw) {
  const bool f32 = g.elem == 4;
  const int64_t op_rows = g.rows, total = c.total;
  // f64 entries are 16 bytes: the LDS image holds QF_CAP_MIN of them (64 KiB), two workgroups per CU
  const int qf_cap_max = f32 ? QF_CAP_MAX : QF_CAP_MIN;
  // The image is sized to the operator's average quad + 12 % (round 5; rounds 1-4: 4096 or 6144 entries): a workgroup's LDS is
  // what limits the fill's residency (its waves sit out two memory round trips each), and C2's quads of 3 100 slots fit five
  // workgroups per CU instead of four.  A quad above the image takes the direct route inside the kernel.
  const double quad_avg = (double)total / std::max(1.0, (double)op_rows / 4.0);
  const int qf_cap_fit = (int)std::min<int64_t>(qf_cap_max, std::max<int64_t>(2048, round_up((int64_t)(1.12 * quad_avg) + 64, 256)));
  const int qf_cap = (!f32 || sw.qf_cap_fixed) ? ((double)total <= 0.85 * QF_CAP_MIN * ((double)op_rows / 4.0) ? QF_CAP_MIN : qf_cap_max) : qf_cap_fit;
  if (src.kind == QuadSource::FromA) {
    // (rows of A whose columns do not ascend -- include/sapca.h promises wrong numbers for them, not stray accesses: the run
    //  ends the histogram recorded are meaningless then, the bucket fill needs none)
    const bool gather = src.from_a->bnd != nullptr && c.d_perm == nullptr && c.nrb == src.from_a->nrb_nat && !c.rows_in_disorder && !sw.at_buckets;
    return {gather ? Fill::Gather : Fill::Buckets, qf_cap};
  }
  if (src.kind != QuadSource::Csr) return {Fill::Runs, qf_cap};
  // quads that fit the LDS image on average: staged fill
  const bool staged = !sw.fill_direct && (double)total <= 0.93 * qf_cap_max * ((double)op_rows / 4.0) && g.nct <= 768;
  return {staged ? Fill::Staged : Fill::Direct, qf_cap};
}

// A^T's entries from A (f32): reads A, the published tables and the histogram's leavings; queues the gather fill, or the
// column map, the cursors' memset, the scatter into buckets (offsets: c.d_raw) and the bucket fill; then the reduction of
// the per-tile column sums where statistics are wanted.  No wait.
void launch_fill_from_a(const QuadGeometry& g, const AtDirectSrc& a, const Counts& c, bool gather, Ent* d_ent, hipStream_t s) {
  const CsrView<float>& A = *a.A;
  const int nct = g.nct, nrb = (int)c.nrb;
  const int64_t op_rows = g.rows;
  const uint16_t* d_steps = reinterpret_cast<const uint16_t*>(c.d_steps);
  const size_t a_col = round_up((size_t)op_rows * sizeof(uint32_t), 256), a_bucket = gather ? 0 : round_up((size_t)A.nnz * sizeof(uint2), 256);
  const size_t a_part = a.stats ? round_up((size_t)nct * op_rows * sizeof(double), 256) : 0;
  char* base = static_cast<char*>(a.scratch->ensure(a_col + a_bucket + 2 * a_part + (size_t)c.nchunks * sizeof(uint32_t) + 256));
  uint32_t* d_colmap = reinterpret_cast<uint32_t*>(base);
  uint2* d_bucket = reinterpret_cast<uint2*>(base + a_col);
  double* d_psum = a.stats ? reinterpret_cast<double*>(base + a_col + a_bucket) : nullptr;
  double* d_psq = a.stats ? reinterpret_cast<double*>(base + a_col + a_bucket + a_part) : nullptr;
  if (gather) {
    hipLaunchKernelGGL(atd_fill_kernel<true>, dim3((unsigned)(8 * ((nct + 7) / 8) * nrb)), dim3(ATD_THREADS), 0, s, (const uint2*)nullptr,
                       (const int64_t*)nullptr, c.d_blk, c.d_perm, nct, g.ldp * 4, c.d_chunk, c.d_quad_off, d_steps, d_ent,
                       d_psum, d_psq, op_rows, A.idx, A.val, a.bnd, A.ptr, A.rows, g.tc, nrb);
  } else {
    hipLaunchKernelGGL(atd_colmap_kernel, dim3((unsigned)((op_rows + 255) / 256)), dim3(256), 0, s, c.d_blk, nrb, c.d_perm, op_rows,
                       d_colmap);
    uint32_t* d_cursor = reinterpret_cast<uint32_t*>(base + a_col + a_bucket + 2 * a_part);
    SAPCA_HIP(hipMemsetAsync(d_cursor, 0, (size_t)c.nchunks * sizeof(uint32_t), s));
    hipLaunchKernelGGL(atd_scatter_kernel, dim3((unsigned)std::min<int64_t>(round_up((A.rows + 3) / 4, 8), 4096)), dim3(256), 0, s, A.ptr,
                       A.idx, A.val, A.rows, nct, g.tc, d_colmap, c.d_raw, d_cursor, d_bucket);
    hipLaunchKernelGGL(atd_fill_kernel<false>, dim3((unsigned)c.nchunks), dim3(ATD_THREADS), 0, s, d_bucket, c.d_raw, c.d_blk, c.d_perm, nct, g.ldp * 4,
                       c.d_chunk, c.d_quad_off, d_steps, d_ent, d_psum, d_psq, op_rows,
                       (const int32_t*)nullptr, (const float*)nullptr, (const uint32_t*)nullptr, (const int64_t*)nullptr, (int64_t)0, g.tc, nrb);
  }
  if (a.stats)
    hipLaunchKernelGGL(atd_stats_reduce_kernel, dim3((unsigned)((op_rows + 63) / 64)), dim3(1024), 0, s, d_psum, d_psq, op_rows, nct,
                       a.stats, a.stats + op_rows);
}

// Launch the fill: reads S (or A), seg and the published tables; queues the chosen fill's kernels on `b.s`; no wait.
template <typename VT>
void launch_fill(const Build<VT>& b, const Counts& c, const int32_t* d_seg, const FillChoice& f, typename EntOf<VT>::type* d_ent) {
  typedef typename EntOf<VT>::type E;
  const QuadGeometry& g = b.g;
  const CsrView<VT>& S = b.S;
  hipStream_t s = b.s;
  const int nct = g.nct, nrb = (int)c.nrb, ldp_bytes = g.ldp * 4;
  const int nquads = nrb * Q_BLOCK_QUADS;
  switch (f.fill) {
    case Fill::Gather:
    case Fill::Buckets:
      if constexpr (sizeof(VT) == 4) launch_fill_from_a(g, *b.src.from_a, c, f.fill == Fill::Gather, d_ent, s);
      break;
    case Fill::Runs:
      if (nct <= b.sw.runs_seg_lds_max)
        hipLaunchKernelGGL((quad_fill_runs_kernel<true, VT>), dim3((unsigned)nquads), dim3(256), (size_t)4 * (nct + 1) * sizeof(int32_t), s,
                           S.ptr, S.idx, S.val, b.src.packed, d_seg, c.d_blk, c.d_perm, nct, g.inv_nct, ldp_bytes, c.d_chunk, c.d_quad_off, d_ent);
      else
        hipLaunchKernelGGL((quad_fill_runs_kernel<false, VT>), dim3((unsigned)nquads), dim3(256), 0, s,
                           S.ptr, S.idx, S.val, b.src.packed, d_seg, c.d_blk, c.d_perm, nct, g.inv_nct, ldp_bytes, c.d_chunk, c.d_quad_off, d_ent);
      break;
    case Fill::Staged: {
      const size_t fill_lds = (size_t)f.qf_cap * sizeof(E) + ((size_t)7 * nct + 1) * sizeof(uint32_t);   // up to 69.5 KiB (f32), 69.2 KiB (f64)
      static LdsAttrState attr;
      ensure_dynamic_lds(reinterpret_cast<const void*>(&quad_fill_staged_kernel<VT>), fill_lds, attr);
      hipLaunchKernelGGL(quad_fill_staged_kernel<VT>, dim3(qf_grid(nquads)), dim3(256), fill_lds, s, S.ptr, S.idx, S.val, d_seg, c.d_blk,
                         c.d_perm, nct, f.qf_cap, g.inv_nct, ldp_bytes, c.d_chunk, c.d_quad_off, d_ent, nquads);
      break;
    }
    case Fill::Direct:
      hipLaunchKernelGGL(quad_fill_kernel<VT>, dim3((unsigned)((S.rows + 3) / 4)), dim3(256), (size_t)4 * nct * sizeof(uint32_t), s,
                         S.ptr, S.idx, S.val, S.rows, c.d_blk, c.d_perm, nrb, nct, g.inv_nct, ldp_bytes, c.d_chunk, c.d_quad_off, d_ent);
      break;
  }
}

// The stages in order, for an operator eligible(g, src) accepted.  Returns false, with op.valid false, when the operator
// does not fit the staged sweeps' limits: the caller stays on the row kernel.
template <typename VT>
bool build_quads(const CsrView<VT>& S, const QuadGeometry& g, const QuadSource& src, const BuildSwitches& sw, TiledOp& op,
                 TiledBuffers& buf, hipStream_t s) {
  typedef typename EntOf<VT>::type E;
  constexpr bool f32 = sizeof(VT) == 4;
  const Build<VT> b{S, g, src, sw, buf, s};
  const int32_t* d_seg = index_rows(b);
  Counts c;
  if (!count_chunks(b, d_seg, c)) return false;
  E* d_ent = reinterpret_cast<E*>(buf.ent.ensure((size_t)(c.total + ENT_SLACK) * sizeof(E)));
  publish(op, g, c, d_ent);
  const bool dq_ok = fork_dq_tables<VT>(op, buf, s);
  if (f32 && !dq_ok && (g.block_rows > 512 || c.max_chunk > g.stage_cap)) {   // only the DPP-fed sweep reads such operators
    SAPCA_HIP(hipStreamWaitEvent(s, buf.aux_join, 0));
    return false;
  }
  const FillChoice f = choose_fill(g, src, c, sw);
  // every fill but the direct one writes its padding itself: only the slack behind the last chunk is cleared for them
  if (f.fill != Fill::Direct) SAPCA_HIP(hipMemsetAsync(d_ent + c.total, 0, (size_t)ENT_SLACK * sizeof(E), s));
  else SAPCA_HIP(hipMemsetAsync(d_ent, 0, (size_t)(c.total + ENT_SLACK) * sizeof(E), s));
  launch_fill<VT>(b, c, d_seg, f, d_ent);
  SAPCA_HIP(hipGetLastError());
  if (f32) SAPCA_HIP(hipStreamWaitEvent(s, buf.aux_join, 0));
  op.valid = true;
  return true;
}

template <typename VT>
bool build_tiled_t(const CsrView<VT>& S, int ldp_elems, TiledOp& op, TiledBuffers& buf, hipStream_t s, const QuadSource& src) {
  SAPCA_CHECK(ldp_elems == 64, SAPCA_ERR_ARG, "tiled sweep: panels must have 64 columns");
  SAPCA_CHECK(src.kind != QuadSource::FromA, SAPCA_ERR_ARG, "tiled sweep: the A -> A^T route starts in build_tiled_at_direct");
  op = TiledOp();
  const BuildSwitches sw{};
  const QuadGeometry g = quad_geometry(S.rows, S.cols, S.nnz, (int)sizeof(VT), ldp_elems, sw);
  return eligible(g, src) && build_quads<VT>(S, g, src, sw, op, buf, s);
}

}  // namespace

bool build_tiled(const CsrView<float>& S, int ldp, TiledOp& op, TiledBuffers& buf, hipStream_t s, const QuadSource& src) {
  return build_tiled_t<float>(S, ldp, op, buf, s, src);
}
bool build_tiled(const CsrView<double>& S, int ldp, TiledOp& op, TiledBuffers& buf, hipStream_t s, const QuadSource& src) {
  return build_tiled_t<double>(S, ldp, op, buf, s, src);
}

bool build_tiled_at_direct(const CsrView<float>& A, int ldp, TiledOp& op, TiledBuffers& buf, int64_t* at_ptr, double* stats,
                           DevBuf& scratch, hipStream_t s) {
  op = TiledOp();
  const BuildSwitches sw{};
  if (sw.at_sort || ldp != 64) return false;
  const int64_t m = A.rows, n = A.cols;
  const QuadGeometry g = quad_geometry(n, m, A.nnz, (int)sizeof(float), ldp, sw);   // of A^T
  QuadSource src;
  src.kind = QuadSource::FromA;
  if (!eligible(g, src)) return false;
  const int nct = g.nct, tc = g.tc;
  const int64_t n2 = round_up(n, 2);
  // entry counts per (tile of A rows, column); their column totals are A^T's row lengths
  uint16_t* cnt16 = buf.seg.as<uint16_t>((size_t)nct * n2);   // (takes the place of the per-row tile index of the other routes)
  // the natural partition of A^T's rows (the one the format takes unless its rows have to be sorted by length): the
  // histogram pass leaves the ends of every (block, A row) run for the gather fill
  const int64_t nrb_nat = g.nrb;
  uint32_t* bnd = nullptr;
  if (!sw.at_buckets && nrb_nat <= 4096) {
    // (4 (nrb + 1) bytes per row of A: 132 MB at C4 -- round 4: 264 MB of int64, cleared before every fit; the histogram pass
    //  now writes every word itself.  A table that cannot be allocated is not a failed fit: the bucket route needs none)
    try {
      bnd = buf.bounds.as<uint32_t>((size_t)(nrb_nat + 1) * (size_t)nct * tc);
    } catch (const Error&) {
      (void)hipGetLastError();
      bnd = nullptr;
    }
  }
  const size_t hist_lds = (size_t)n2 * 2;
  static LdsAttrState hist_attr;
  ensure_dynamic_lds(reinterpret_cast<const void*>(&atd_hist_kernel), hist_lds, hist_attr);
  std::vector<int32_t> blk_nat;
  float blk_scale = 0.f;
  if (bnd) float_blocks(n, nrb_nat, blk_nat, blk_scale);
  int64_t* d_disorder = misc_words(buf) + kMiscDisorder;   // (read back with the builder's one host exchange)
  unsigned long long* d_slots = reinterpret_cast<unsigned long long*>(misc_words(buf)) + kMiscNaturalSlots;   // (the natural quads' slots, likewise)
  SAPCA_HIP(hipMemsetAsync(d_disorder, 0, sizeof(int64_t), s));
  hipLaunchKernelGGL(atd_hist_kernel, dim3((unsigned)nct), dim3((size_t)n2 * 2 > 52 * 1024 ? ATD_HIST_THREADS_WIDE : ATD_HIST_THREADS),   // (above 52 KiB two workgroups share a CU: sixteen waves each)
                     hist_lds, s, A.ptr, A.idx, m, nct, tc, n2, cnt16, blk_scale, (int)nrb_nat, bnd, d_disorder, d_slots);
  hipLaunchKernelGGL(atd_rowlen_kernel, dim3((unsigned)((n + 64) / 64)), dim3(1024), 0, s, cnt16, n, n2, nct, at_ptr, d_slots);
  launch_small_scan(at_ptr, nullptr, n, nullptr, s);
  SAPCA_HIP(hipGetLastError());
  CsrView<float> At;
  At.rows = n; At.cols = m; At.nnz = A.nnz; At.ptr = at_ptr; At.idx = nullptr; At.val = nullptr;
  const AtDirectSrc from_a{&A, cnt16, n2, &scratch, stats, bnd, nrb_nat, &blk_nat};
  src.from_a = &from_a;
  return build_quads<float>(At, g, src, sw, op, buf, s);
}

void at_stats_index(const int64_t* ptr, const uint64_t* packed, int64_t rows, int64_t cols, int ldp, TiledBuffers& buf,
                    double* sum, double* sumsq, hipStream_t s) {
  if (rows == 0) return;
  const int nct = tile_count(cols, ldp);
  int32_t* d_seg = buf.seg.as<int32_t>((size_t)rows * (nct + 1));
  hipLaunchKernelGGL(at_stats_index_kernel, dim3(grid_for(rows * WAVE, 256, 4096)), dim3(256), 0, s, ptr, packed, rows, nct,
                     1.0f / (float)nct, sum, sumsq, d_seg);
  SAPCA_HIP(hipGetLastError());
}

int tiled_tile_count(int64_t cols, int ldp) { return tile_count(cols, ldp); }

}  // namespace k
}  // namespace sapca
