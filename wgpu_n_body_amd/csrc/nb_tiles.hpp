// nb_tiles.hpp -- what the passes that sum per-body terms into the cells of a 2-D grid share (nb_map.hip,
// nb_phase.hip; DESIGN.md 6f "The kernels", 6q): everything after the pass's own classify kernel has written one
// key per body, (tile << 6) | cell in the 8 x 8-cell tile, or the key of the tile past the last for a body that
// is not binned:
//   group     -- the stable sort of nb_analysis_sort.hpp on (key, body index), on the tile bits (one pass
//                up to 255 tiles, two up to 65,535, else three), so the order of a tile's list is the
//                order of the bodies;
//   lists     -- the first and last position of every tile in the sorted keys, the tiles' lists cut into
//                segments of at most `seg_len` bodies, and the segments numbered by a scan
//                (every block its 1,024 tiles, then the blocks before it added);
//   sum       -- one block of 256 threads per segment stages 256 bodies of the list at a time in LDS (the
//                cell within the tile, then the terms, field-major; the terms recomputed from the
//                gathered body by the pass's Terms).  Thread (q, c) = (tid / 64, tid % 64) adds the staged
//                bodies of cell c in quarter q in list order; the four quarters are added in order at the
//                end.  A tile of one segment is written once with plain stores; the segments of a longer
//                list go to partials, added in segment order by the combine kernel;
//   finish    -- the maximum count and the global sums of the classify kernel's slabs, in a fixed order
//                (sum_over_blocks in 32 groups).
// Cells that no body reaches are cleared beforehand.  No float atomics; the grids and the cuts depend on n, the
// grid, the segment length and the lists' lengths alone: the result is bitwise reproducible, and two passes whose
// Terms give the same doubles for the same keys give the same planes.
//
// A pass brings
//   Const  -- its constants block, passed to the kernels by value, with c[3], vc[3], center_com, w, h, tiles_x
//             and tiles;
//   Terms  -- one type per number of planes: F, kVelocity (whether a body's velocity is loaded), a device
//             constructor from (const Const &, used) -- used[0..6) the centre and velocity of centre_used --
//             and operator()(body, p, v, t) filling t[F];
//   classify -- a callable that launches its kernel: keys[i] for every body, one slab row of kTileGlobalFields
//             doubles per block of kBlock bodies, used[0..6) by block 0.
// The kernels are templates or sit in an anonymous namespace: a unit launches its own copies.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

constexpr uint32_t kTile = 8, kTileCells = kTile * kTile;  // cells per tile = the low 6 bits of a key
constexpr uint32_t kCellBits = 6;
constexpr uint32_t kTileGlobalFields = 8;  // a classify kernel's slab row
constexpr uint32_t kTileMaxBlocks = 1024;  // the maximum over the counts: grid-stride beyond
constexpr uint32_t kNoCell = 0xff;
// res: [0, 6) the centre and velocity used, then the global sums, then the maximum count
constexpr uint32_t kTileUsed = 8, kTileResMax = kTileUsed + kTileGlobalFields, kTileResDoubles = kTileResMax + 1;

// (all but the last three grow to the largest call so far)
struct TileWork {
    SortBufs<uint32_t> sort;                // the two sides of (key, body index), the histogram
    DeviceBuf<uint32_t> first, last;        // [tiles]
    DeviceBuf<uint32_t> seg_off, part_off;  // [tiles + 1]
    DeviceBuf<uint32_t> seg_tile;           // [segments possible]
    DeviceBuf<uint32_t> block_tot;          // [blocks of the segment scan][2]
    DeviceBuf<double> parts;                // [partial slots][fields + 1][64]
    DeviceBuf<double> slabs;                // [classify blocks][kTileGlobalFields]
    DeviceBuf<uint32_t> counts;             // [cells]
    DeviceBuf<double> planes;               // [fields][cells]
    DeviceBuf<uint32_t> block_max;          // [kTileMaxBlocks]
    DeviceBuf<double> res;                  // [kTileResDoubles]
    PinnedBuf<double> h_res;                // as res
};

// what a workspace's init allocates: the buffers that do not depend on the call
inline int tiles_init(TileWork &f, const char *pass) {
    if (f.block_max.reserve(kTileMaxBlocks) != hipSuccess || f.res.reserve(kTileResDoubles) != hipSuccess ||
        f.h_res.reserve(kTileResDoubles) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: cannot allocate the result workspace", pass);
        return NB_ERR_ALLOC;
    }
    return NB_OK;
}

// At least `count` elements behind b.  A failure leaves b empty and the simulator usable: the sticky error
// is cleared.
template <class T, bool kPinned>
int tiles_reserve(const char *pass, Buf<T, kPinned> &b, size_t count) {
    if (b.reserve(count) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("%s: cannot allocate %zu bytes of %s workspace", pass, sizeof(T) * count, kPinned ? "pinned" : "device");
    return NB_ERR_ALLOC;
}

inline uint32_t tiles_bits_of(uint32_t x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

#ifdef __HIPCC__

__device__ inline uint32_t segments_of(uint32_t len, uint32_t seg_len) { return (len + seg_len - 1) / seg_len; }

namespace {

// ---- lists: tile t's bodies are positions [first[t], last[t]) of the sorted keys (0, 0: none) ------
__global__ __launch_bounds__(kBlock) void tiles_bounds_kernel(const uint32_t *__restrict__ keys, uint32_t n,
                                                              uint32_t tiles, uint32_t *__restrict__ first,
                                                              uint32_t *__restrict__ last) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = keys[i] >> kCellBits;
    const uint32_t tp = i > 0 ? keys[i - 1] >> kCellBits : 0xffffffffu;
    if (t != tp) {
        if (t < tiles) first[t] = (uint32_t)i;
        if (i > 0 && tp < tiles) last[tp] = (uint32_t)i;
    }
    if (i + 1 == n && t < tiles) last[t] = n;
}

// seg_off[t] = segments of the tiles before t, seg_off[tiles] = all; part_off likewise, counting only the
// segments of tiles with more than one (they go through partials); seg_tile[g] = the tile of segment g.
// In two launches of ceil((tiles + 1) / 1024) blocks: each block scans its 1,024 tiles and leaves its two
// sums in block_tot; then every tile adds the sums of the blocks before its own and writes its segments' tile.
__global__ __launch_bounds__(kScanThreads) void tiles_segments_local_kernel(const uint32_t *__restrict__ first,
                                                                            const uint32_t *__restrict__ last,
                                                                            uint32_t tiles, uint32_t seg_len,
                                                                            uint32_t *__restrict__ seg_off,
                                                                            uint32_t *__restrict__ part_off,
                                                                            uint32_t *__restrict__ block_tot) {
    __shared__ uint32_t lds[2][2 * kScanThreads];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * kScanThreads + tid;
    const uint32_t s = t < tiles ? segments_of(last[t] - first[t], seg_len) : 0u, p = s > 1 ? s : 0u;
    uint32_t *a0 = lds[0], *b0 = lds[0] + kScanThreads, *a1 = lds[1], *b1 = lds[1] + kScanThreads;
    a0[tid] = s;
    a1[tid] = p;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {  // inclusive, Hillis-Steele, both sums at once
        b0[tid] = tid >= o ? a0[tid] + a0[tid - o] : a0[tid];
        b1[tid] = tid >= o ? a1[tid] + a1[tid - o] : a1[tid];
        __syncthreads();
        uint32_t *x = a0;
        a0 = b0;
        b0 = x;
        x = a1;
        a1 = b1;
        b1 = x;
    }
    if (t <= tiles) {
        seg_off[t] = a0[tid] - s;
        part_off[t] = a1[tid] - p;
    }
    if (tid == kScanThreads - 1) {
        block_tot[2 * blockIdx.x] = a0[tid];
        block_tot[2 * blockIdx.x + 1] = a1[tid];
    }
}

__global__ __launch_bounds__(kScanThreads) void tiles_segments_final_kernel(const uint32_t *__restrict__ first,
                                                                            const uint32_t *__restrict__ last,
                                                                            uint32_t tiles, uint32_t seg_len,
                                                                            uint32_t *__restrict__ seg_off,
                                                                            uint32_t *__restrict__ part_off,
                                                                            const uint32_t *__restrict__ block_tot,
                                                                            uint32_t *__restrict__ seg_tile,
                                                                            uint32_t seg_cap) {
    __shared__ uint32_t before[2];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * kScanThreads + tid;
    if (tid < 2) {  // (at most 65 blocks)
        uint32_t sum = 0;
        for (uint32_t b = 0; b < blockIdx.x; ++b) sum += block_tot[2 * b + tid];
        before[tid] = sum;
    }
    __syncthreads();
    if (t > tiles) return;
    const uint32_t g0 = seg_off[t] + before[0];
    seg_off[t] = g0;
    part_off[t] += before[1];
    if (t == tiles) return;
    const uint32_t g1 = g0 + segments_of(last[t] - first[t], seg_len);
    for (uint32_t g = g0; g < g1 && g < seg_cap; ++g) seg_tile[g] = t;
}

// ---- sum: one block per segment ------------------------------------------------------------------
// planes: [F][h * w]; parts: [slot][F + 1][64] doubles (the count last), slot = part_off[tile] + segment
template <class Terms, class Const>
__global__ __launch_bounds__(kBlock) void tiles_sum_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, Const k,
                                                           const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ idx,
                                                           const uint32_t *__restrict__ first,
                                                           const uint32_t *__restrict__ last,
                                                           const uint32_t *__restrict__ seg_off,
                                                           const uint32_t *__restrict__ part_off,
                                                           const uint32_t *__restrict__ seg_tile, uint32_t seg_len,
                                                           uint32_t n, uint32_t part_cap,
                                                           const double *__restrict__ used,
                                                           uint32_t *__restrict__ counts, double *__restrict__ planes,
                                                           double *__restrict__ parts) {
    constexpr uint32_t F = Terms::F;
    __shared__ double stage[F][kBlock];  // [field][staged body]; at the end [field][thread]
    __shared__ uint32_t cell_in[kBlock];  // the staged body's cell in the tile; at the end the thread's count
    const uint32_t g = blockIdx.x;
    if (g >= seg_off[k.tiles]) return;  // (uniform over the block)
    const uint32_t tid = threadIdx.x, tile = seg_tile[g];
    if (tile >= k.tiles) return;
    const uint32_t s = g - seg_off[tile];
    const uint32_t t0 = first[tile], t1 = last[tile];
    const uint32_t lo = t0 + s * seg_len, hi = t1 - lo > seg_len ? lo + seg_len : t1;
    const uint32_t nseg = segments_of(t1 - t0, seg_len);
    const Terms terms(k, used);
    const uint32_t my_cell = tid % kTileCells, q0 = tid & ~(kTileCells - 1);
    double acc[F];
    for (uint32_t f = 0; f < F; ++f) acc[f] = 0.0;
    uint32_t cnt = 0;
    for (uint32_t j0 = lo; j0 < hi; j0 += kBlock) {
        const uint32_t j = j0 + tid;
        uint32_t cell = kNoCell;
        if (j < hi) {
            const uint32_t body = idx[j];
            if (body < n) {
                cell = keys[j] & (kTileCells - 1);
                double t[F];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (Terms::kVelocity) v = vel[body];  // the mass alone needs no velocity
                terms(body, posm[body], v, t);
                for (uint32_t f = 0; f < F; ++f) stage[f][tid] = t[f];
            }
        }
        cell_in[tid] = cell;
        __syncthreads();
        for (uint32_t i = q0; i < q0 + kTileCells; ++i) {
            if (cell_in[i] == my_cell) {
                for (uint32_t f = 0; f < F; ++f) acc[f] += stage[f][i];
                ++cnt;
            }
        }
        __syncthreads();  // the staged bodies have been read
    }
    // the four quarters of every cell, in order
    for (uint32_t f = 0; f < F; ++f) stage[f][tid] = acc[f];
    cell_in[tid] = cnt;
    __syncthreads();
    if (tid >= kTileCells) return;
    double sum[F];
    for (uint32_t f = 0; f < F; ++f) {
        sum[f] = stage[f][tid];
        for (uint32_t q = kTileCells; q < kBlock; q += kTileCells) sum[f] += stage[f][q + tid];
    }
    for (uint32_t q = kTileCells; q < kBlock; q += kTileCells) cnt += cell_in[q + tid];
    if (nseg > 1) {
        const size_t slot = (size_t)part_off[tile] + s;
        if (slot >= part_cap) return;
        double *p = parts + slot * (F + 1) * kTileCells;
        for (uint32_t f = 0; f < F; ++f) p[f * kTileCells + tid] = sum[f];
        p[F * kTileCells + tid] = (double)cnt;
        return;
    }
    const uint32_t x = (tile % k.tiles_x) * kTile + tid % kTile, y = (tile / k.tiles_x) * kTile + tid / kTile;
    if (x < k.w && y < k.h) {
        const size_t cell = (size_t)y * k.w + x, cells = (size_t)k.w * k.h;
        counts[cell] = cnt;
        for (uint32_t f = 0; f < F; ++f) planes[f * cells + cell] = sum[f];
    }
}

// combine: the block of a longer list's first segment adds the list's partials in segment order
template <uint32_t F>
__global__ __launch_bounds__(kTileCells) void tiles_combine_kernel(uint32_t w, uint32_t h, uint32_t tiles_x,
                                                                   uint32_t tiles, const uint32_t *__restrict__ first,
                                                                   const uint32_t *__restrict__ last,
                                                                   const uint32_t *__restrict__ seg_off,
                                                                   const uint32_t *__restrict__ part_off,
                                                                   const uint32_t *__restrict__ seg_tile,
                                                                   uint32_t seg_len, uint32_t part_cap,
                                                                   const double *__restrict__ parts,
                                                                   uint32_t *__restrict__ counts,
                                                                   double *__restrict__ planes) {
    const uint32_t g = blockIdx.x;
    if (g >= seg_off[tiles]) return;
    const uint32_t tid = threadIdx.x, tile = seg_tile[g];
    if (tile >= tiles || g != seg_off[tile]) return;
    const uint32_t nseg = segments_of(last[tile] - first[tile], seg_len);
    if (nseg < 2 || (size_t)part_off[tile] + nseg > part_cap) return;
    const double *p = parts + (size_t)part_off[tile] * (F + 1) * kTileCells;
    double sum[F + 1];
    for (uint32_t f = 0; f <= F; ++f) sum[f] = p[f * kTileCells + tid];
    for (uint32_t s = 1; s < nseg; ++s) {
        p += (F + 1) * kTileCells;
        for (uint32_t f = 0; f <= F; ++f) sum[f] += p[f * kTileCells + tid];
    }
    const uint32_t x = (tile % tiles_x) * kTile + tid % kTile, y = (tile / tiles_x) * kTile + tid / kTile;
    if (x < w && y < h) {
        const size_t cell = (size_t)y * w + x, cells = (size_t)w * h;
        counts[cell] = (uint32_t)sum[F];  // (exact: below 2^32)
        for (uint32_t f = 0; f < F; ++f) planes[f * cells + cell] = sum[f];
    }
}

// ---- finish: the maximum count per block, then everything in a fixed order ---------------------------
__global__ __launch_bounds__(kBlock) void tiles_max_kernel(const uint32_t *__restrict__ counts, size_t cells,
                                                           uint32_t *__restrict__ block_max) {
    __shared__ uint32_t m[kBlock];
    uint32_t best = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (size_t)gridDim.x * kBlock)
        best = std::max(best, counts[i]);
    m[threadIdx.x] = best;
    __syncthreads();
    for (uint32_t o = kBlock / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) m[threadIdx.x] = std::max(m[threadIdx.x], m[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) block_max[blockIdx.x] = m[0];
}

// res[f] = sum over the classify blocks of slab element f, by sum_over_blocks in 32 groups.
// res[kTileGlobalFields] = the maximum of block_max.
__global__ __launch_bounds__(kBlock) void tiles_finish_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                              const uint32_t *__restrict__ block_max,
                                                              uint32_t max_blocks, double *__restrict__ res) {
    constexpr uint32_t kGroups = kBlock / kTileGlobalFields;
    __shared__ double pp[kGroups][kTileGlobalFields];
    __shared__ uint32_t m[kBlock];
    const uint32_t tid = threadIdx.x;
    uint32_t best = 0;
    for (uint32_t b = tid; b < max_blocks; b += kBlock) best = std::max(best, block_max[b]);
    m[tid] = best;
    const double sum = sum_over_blocks<kGroups>(slabs, blocks, kTileGlobalFields, tid % kTileGlobalFields, pp);
    if (tid < kTileGlobalFields) res[tid] = sum;
    if (tid == kBlock - 1) {
        uint32_t r = 0;
        for (uint32_t q = 0; q < kBlock; ++q) r = std::max(r, m[q]);
        res[kTileGlobalFields] = (double)r;
    }
}

template <class Terms, class Const>
int tiles_launch_sums(SimBase &sim, TileWork &w, const Const &k, const float4 *posm, const float4 *vel,
                      const uint32_t *keys, const uint32_t *idx, uint32_t seg_len, uint32_t seg_cap,
                      uint32_t part_cap) {
    const uint32_t *first = w.first, *last = w.last, *seg_off = w.seg_off, *part_off = w.part_off;
    const uint32_t *seg_tile = w.seg_tile;
    hipLaunchKernelGGL((tiles_sum_kernel<Terms, Const>), dim3(seg_cap), dim3(kBlock), 0, sim.stream, posm, vel, k, keys,
                       idx, first, last, seg_off, part_off, seg_tile, seg_len, sim.n, part_cap, w.res, w.counts,
                       w.planes, w.parts);
    NB_HIP_TRY(hipGetLastError());
    if (part_cap > 0) {
        hipLaunchKernelGGL(tiles_combine_kernel<Terms::F>, dim3(seg_cap), dim3(kTileCells), 0, sim.stream, k.w, k.h,
                           k.tiles_x, k.tiles, first, last, seg_off, part_off, seg_tile, seg_len, part_cap, w.parts,
                           w.counts, w.planes);
        NB_HIP_TRY(hipGetLastError());
    }
    return NB_OK;
}

// The pass behind its classify kernel: reserves, classifies, groups, sums, finishes, copies what is asked for and
// synchronises once.  `wide` chooses TermsWide over TermsOne (one plane).  Afterwards w.h_res holds the centre and
// velocity used, the global sums and the maximum count; the caller reports the simulator's status and its stats.
// classify(class_blocks, posm, vel, keys, slabs, used) -> NB_OK or its error.
template <class TermsOne, class TermsWide, class Const, class Classify>
int tiles_pass(SimBase &sim, TileWork &w, const char *pass, const Const &k, uint32_t seg_len, bool wide, bool com,
               Classify classify, uint32_t *counts, double *planes) {
    static_assert(TermsOne::F == 1, "the narrow terms are the mass alone");
    const uint32_t n = sim.n;
    const uint32_t fields = wide ? TermsWide::F : 1;
    const size_t cells = (size_t)k.w * k.h;
    std::memset(w.h_res, 0, sizeof(double) * kTileResDoubles);
    if (n == 0) {
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        centre_used_empty(w.h_res, com, k.c, k.vc);
        if (counts) std::memset(counts, 0, sizeof(uint32_t) * cells);
        if (planes) std::memset(planes, 0, sizeof(double) * fields * cells);
        return NB_OK;
    }
    auto reserve = [pass](auto &b, size_t count) { return tiles_reserve(pass, b, count); };
    const uint32_t class_blocks = (n + kBlock - 1) / kBlock;
    const SortShape shape = sort_shape(n);
    const uint32_t passes = (tiles_bits_of(k.tiles) + 7) / 8;  // keys' tiles run 0 .. tiles
    // segments: a tile with bodies has at most 1 + (len - 1) / seg_len; those of longer lists number
    // at most 2 (len / seg_len)
    const uint32_t seg_cap = std::min(k.tiles, n) + n / seg_len;
    const uint32_t part_cap = 2 * (n / seg_len);
    if (int rc = w.sort.reserve(n, shape, reserve)) return rc;
    if (int rc = reserve(w.first, k.tiles)) return rc;
    if (int rc = reserve(w.last, k.tiles)) return rc;
    if (int rc = reserve(w.seg_off, (size_t)k.tiles + 1)) return rc;
    if (int rc = reserve(w.part_off, (size_t)k.tiles + 1)) return rc;
    if (int rc = reserve(w.seg_tile, seg_cap)) return rc;
    const uint32_t list_blocks = (k.tiles + 1 + kScanThreads - 1) / kScanThreads;
    if (int rc = reserve(w.block_tot, (size_t)2 * list_blocks)) return rc;
    if (int rc = reserve(w.parts, std::max<size_t>(1, part_cap) * (fields + 1) * kTileCells)) return rc;
    if (int rc = reserve(w.slabs, (size_t)kTileGlobalFields * class_blocks)) return rc;
    if (int rc = reserve(w.counts, cells)) return rc;
    if (int rc = reserve(w.planes, fields * cells)) return rc;

    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    if (int rc = classify(class_blocks, posm, vel, (uint32_t *)w.sort.keys[0], (double *)w.slabs, (double *)w.res))
        return rc;
    if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, passes, kCellBits, nullptr)) return rc;
    const uint32_t *keys = w.sort.keys[passes & 1], *idx = w.sort.idx[passes & 1];
    NB_HIP_TRY(hipMemsetAsync(w.first, 0, sizeof(uint32_t) * k.tiles, sim.stream));
    NB_HIP_TRY(hipMemsetAsync(w.last, 0, sizeof(uint32_t) * k.tiles, sim.stream));
    NB_HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * cells, sim.stream));
    NB_HIP_TRY(hipMemsetAsync(w.planes, 0, sizeof(double) * fields * cells, sim.stream));
    hipLaunchKernelGGL(tiles_bounds_kernel, dim3(class_blocks), dim3(kBlock), 0, sim.stream, keys, n, k.tiles,
                       (uint32_t *)w.first, (uint32_t *)w.last);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tiles_segments_local_kernel, dim3(list_blocks), dim3(kScanThreads), 0, sim.stream,
                       (const uint32_t *)w.first, (const uint32_t *)w.last, k.tiles, seg_len, (uint32_t *)w.seg_off,
                       (uint32_t *)w.part_off, (uint32_t *)w.block_tot);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tiles_segments_final_kernel, dim3(list_blocks), dim3(kScanThreads), 0, sim.stream,
                       (const uint32_t *)w.first, (const uint32_t *)w.last, k.tiles, seg_len, (uint32_t *)w.seg_off,
                       (uint32_t *)w.part_off, (const uint32_t *)w.block_tot, (uint32_t *)w.seg_tile, seg_cap);
    NB_HIP_TRY(hipGetLastError());
    if (int rc = wide ? tiles_launch_sums<TermsWide>(sim, w, k, posm, vel, keys, idx, seg_len, seg_cap, part_cap)
                      : tiles_launch_sums<TermsOne>(sim, w, k, posm, vel, keys, idx, seg_len, seg_cap, part_cap))
        return rc;
    const uint32_t max_blocks = (uint32_t)std::min<size_t>(kTileMaxBlocks, (cells + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(tiles_max_kernel, dim3(max_blocks), dim3(kBlock), 0, sim.stream, (const uint32_t *)w.counts,
                       cells, (uint32_t *)w.block_max);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tiles_finish_kernel, dim3(1), dim3(kBlock), 0, sim.stream, (const double *)w.slabs,
                       class_blocks, (const uint32_t *)w.block_max, max_blocks, w.res + kTileUsed);
    NB_HIP_TRY(hipGetLastError());
    NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(double) * kTileResDoubles, hipMemcpyDeviceToHost, sim.stream));
    if (counts)
        NB_HIP_TRY(hipMemcpyAsync(counts, w.counts, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, sim.stream));
    if (planes)
        NB_HIP_TRY(hipMemcpyAsync(planes, w.planes, sizeof(double) * fields * cells, hipMemcpyDeviceToHost,
                                  sim.stream));
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    return NB_OK;
}

}  // namespace

#endif  // __HIPCC__

}  // namespace nb
