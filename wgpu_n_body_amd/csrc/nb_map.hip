// nb_map.hip -- nb_sim_map: per-cell mass and velocity moments of a simulator's current state on a 2-D
// grid (include/nbody.h "Projected maps"; no reference counterpart).
//
// A map has up to 2^22 cells, so the per-block slab of nb_radial.hip (256 bins) does not carry over.
// The bodies are grouped by 8 x 8-cell tile instead, stably, and every tile's list is summed in LDS:
//   classify  -- one thread per body over the float4 SoA state (SimBase::diag_state): fp64, no
//                contraction, the cell by comparisons against the edges lo + i * size.  Writes one key per
//                body, (tile << 6) | cell in the tile, or the key of the tile past the last for a body
//                that is outside or non-finite.  The global sums (class counts, masses) go through
//                per-block slabs (block_row, nb_analysis.hpp) and a fixed-order finish;
//   group     -- the stable sort of nb_analysis_sort.hpp on (key, body index), on the tile bits (one pass
//                up to 255 tiles, two up to 65,535, else three), so the order of a tile's list is the
//                order of the bodies;
//   lists     -- the first and last position of every tile in the sorted keys, the tiles' lists cut into
//                segments of at most "map_segment_len" bodies, and the segments numbered by a scan
//                (every block its 1,024 tiles, then the blocks before it added);
//   sum       -- one block of 256 threads per segment stages 256 bodies of the list at a time in LDS (the
//                cell within the tile, then the terms, field-major; the terms recomputed from the
//                gathered body, 32 B).  Thread (q, c) = (tid / 64, tid % 64) adds the staged bodies of
//                cell c in quarter q in list order; the four quarters are added in order at the end.  A
//                tile of one segment is written once with plain stores; the segments of a longer list
//                go to partials, added in segment order by the combine kernel;
//   finish    -- the maximum count and the global sums, in a fixed order (sum_over_blocks in 32 groups).
// Cells that no body reaches are cleared beforehand.  Without NB_MAP_VELOCITY only the mass is formed,
// staged and summed.  With NB_MAP_CENTER_COM the moments pass of nb_diag.hip runs first on the same
// stream and the threads divide its sums into the centre themselves: no host round trip.
// No float atomics; the grids and the cuts depend on n, the grid, the segment length and the lists'
// lengths alone: the result is bitwise reproducible.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kTile = 8, kTileCells = kTile * kTile;  // cells per tile = the low 6 bits of a key
constexpr uint32_t kCellBits = 6;
constexpr uint32_t kGlobalFields = 8;     // see GlobalField
constexpr uint32_t kMaxFields = 6;        // planes with NB_MAP_VELOCITY
constexpr uint32_t kMaxBlocks = 1024;     // the maximum over the counts: grid-stride beyond
constexpr uint32_t kNoCell = 0xff;
// res: [0, 6) the centre and velocity used, then the global sums, then the maximum count
constexpr uint32_t kUsed = 8, kResMax = kUsed + kGlobalFields, kResDoubles = kResMax + 1;

enum GlobalField { kGBinned = 0, kGOutside, kGBad, kGBinnedMass, kGOutsideMass, kGMass, kGLive };

struct MapConst {
    double c[3], vc[3], n[3], e1[3], e2[3];
    double xlo, xhi, ylo, yhi, dlo, dhi, dx, dy;
    uint32_t w, h, tiles_x, tiles;
    uint32_t center_com;
};

// The cell of coordinate a among `cells` cells of size d from lo, hi the last edge: the i with
// edge(i) <= a < edge(i + 1), edge(i) = lo + i * d below `cells` and hi at it.  lo <= a < hi is known.
// A division guesses, the comparisons decide.
__device__ inline uint32_t cell_of(double a, double lo, double d, uint32_t cells) {
#pragma clang fp contract(off)
    const double g = (a - lo) / d;
    uint32_t i = g >= (double)(cells - 1) ? cells - 1 : (uint32_t)g;  // (g >= 0)
    while (i > 0 && a < lo + (double)i * d) --i;
    while (i + 1 < cells && a >= lo + (double)(i + 1) * d) ++i;
    return i;
}

// One body by the rule of include/nbody.h: true when it is binned, then *key = (tile << 6) | cell in tile
__device__ inline bool classify(float4 p, const MapConst &k, const double (&c)[3], uint32_t *key) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    const double a = (dx * k.e1[0] + dy * k.e1[1]) + dz * k.e1[2];
    const double b = (dx * k.e2[0] + dy * k.e2[1]) + dz * k.e2[2];
    const double h = (dx * k.n[0] + dy * k.n[1]) + dz * k.n[2];
    if (!(a >= k.xlo && a < k.xhi && b >= k.ylo && b < k.yhi && h >= k.dlo && h < k.dhi)) return false;
    const uint32_t i = cell_of(a, k.xlo, k.dx, k.w), j = cell_of(b, k.ylo, k.dy, k.h);
    const uint32_t tile = (j / kTile) * k.tiles_x + i / kTile;
    *key = (tile << kCellBits) | ((j % kTile) * kTile + i % kTile);
    return true;
}

// The terms of a body: F = 1 the mass, F = 6 mass, m ua, m ub, m w, (m w) w, m |u|^2
template <uint32_t F>
__device__ inline void terms(float4 p, float4 v, const MapConst &k, const double *vc, double (&t)[F]) {
#pragma clang fp contract(off)
    const double m = p.w;
    t[0] = m;
    if constexpr (F > 1) {
        const double ux = (double)v.x - vc[0], uy = (double)v.y - vc[1], uz = (double)v.z - vc[2];
        const double ua = (ux * k.e1[0] + uy * k.e1[1]) + uz * k.e1[2];
        const double ub = (ux * k.e2[0] + uy * k.e2[1]) + uz * k.e2[2];
        const double w = (ux * k.n[0] + uy * k.n[1]) + uz * k.n[2];
        t[1] = m * ua;
        t[2] = m * ub;
        t[3] = m * w;
        t[4] = (m * w) * w;
        t[5] = m * ((ux * ux + uy * uy) + uz * uz);
    }
}

// ---- classify: keys[i] for every body, one slab of kGlobalFields doubles per block -----------------
// mom: the finished moments of nb_diag.hip (NB_MAP_CENTER_COM) or null.  Block 0 also writes the centre
// and velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kThreads) void map_classify_kernel(const float4 *__restrict__ posm,
                                                                const float4 *__restrict__ vel, uint32_t n,
                                                                MapConst k, const double *__restrict__ mom,
                                                                uint32_t *__restrict__ keys,
                                                                double *__restrict__ slabs, double *__restrict__ used) {
    __shared__ double part[kThreads / kWave][kGlobalFields];
    const uint32_t tid = threadIdx.x;
    double c[3], vc[3];
    centre_used(k.c, k.vc, k.center_com, mom, used, c, vc);
    double glob[kGLive];
    for (uint32_t f = 0; f < kGLive; ++f) glob[f] = 0.0;
    const size_t i = (size_t)blockIdx.x * kThreads + tid;
    if (i < n) {
        const float4 p = posm[i], v = vel[i];
        uint32_t key = k.tiles << kCellBits;  // the tile past the last: not binned
        if (!body_ok(p, v)) {
            glob[kGBad] = 1.0;
        } else {
            const double m = p.w;
            glob[kGMass] = m;
            if (classify(p, k, c, &key)) {
                glob[kGBinned] = 1.0;
                glob[kGBinnedMass] = m;
            } else {
                glob[kGOutside] = 1.0;
                glob[kGOutsideMass] = m;
            }
        }
        keys[i] = key;
    }
    block_row<kGlobalFields, kGLive>(glob, part, slabs + (size_t)blockIdx.x * kGlobalFields);
}

// ---- lists: tile t's bodies are positions [first[t], last[t]) of the sorted keys (0, 0: none) ------
__global__ __launch_bounds__(kThreads) void map_bounds_kernel(const uint32_t *__restrict__ keys, uint32_t n,
                                                              uint32_t tiles, uint32_t *__restrict__ first,
                                                              uint32_t *__restrict__ last) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = keys[i] >> kCellBits;
    const uint32_t tp = i > 0 ? keys[i - 1] >> kCellBits : 0xffffffffu;
    if (t != tp) {
        if (t < tiles) first[t] = (uint32_t)i;
        if (i > 0 && tp < tiles) last[tp] = (uint32_t)i;
    }
    if (i + 1 == n && t < tiles) last[t] = n;
}

__device__ inline uint32_t segments_of(uint32_t len, uint32_t seg_len) { return (len + seg_len - 1) / seg_len; }

// seg_off[t] = segments of the tiles before t, seg_off[tiles] = all; part_off likewise, counting only the
// segments of tiles with more than one (they go through partials); seg_tile[g] = the tile of segment g.
// In two launches of ceil((tiles + 1) / 1024) blocks: each block scans its 1,024 tiles and leaves its two
// sums in block_tot; then every tile adds the sums of the blocks before its own and writes its segments' tile.
__global__ __launch_bounds__(kScanThreads) void map_segments_local_kernel(const uint32_t *__restrict__ first,
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

__global__ __launch_bounds__(kScanThreads) void map_segments_final_kernel(const uint32_t *__restrict__ first,
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
template <uint32_t F>
__global__ __launch_bounds__(kThreads) void map_sum_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, MapConst k,
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
    __shared__ double stage[F][kThreads];  // [field][staged body]; at the end [field][thread]
    __shared__ uint32_t cell_in[kThreads];  // the staged body's cell in the tile; at the end the thread's count
    const uint32_t g = blockIdx.x;
    if (g >= seg_off[k.tiles]) return;  // (uniform over the block)
    const uint32_t tid = threadIdx.x, tile = seg_tile[g];
    if (tile >= k.tiles) return;
    const uint32_t s = g - seg_off[tile];
    const uint32_t t0 = first[tile], t1 = last[tile];
    const uint32_t lo = t0 + s * seg_len, hi = t1 - lo > seg_len ? lo + seg_len : t1;
    const uint32_t nseg = segments_of(t1 - t0, seg_len);
    double vc[3];
    for (int a = 0; a < 3; ++a) vc[a] = used[3 + a];
    const uint32_t my_cell = tid % kTileCells, q0 = tid & ~(kTileCells - 1);
    double acc[F];
    for (uint32_t f = 0; f < F; ++f) acc[f] = 0.0;
    uint32_t cnt = 0;
    for (uint32_t j0 = lo; j0 < hi; j0 += kThreads) {
        const uint32_t j = j0 + tid;
        uint32_t cell = kNoCell;
        if (j < hi) {
            const uint32_t body = idx[j];
            if (body < n) {
                cell = keys[j] & (kTileCells - 1);
                double t[F];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (F > 1) v = vel[body];  // the mass alone needs no velocity
                terms<F>(posm[body], v, k, vc, t);
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
        for (uint32_t q = kTileCells; q < kThreads; q += kTileCells) sum[f] += stage[f][q + tid];
    }
    for (uint32_t q = kTileCells; q < kThreads; q += kTileCells) cnt += cell_in[q + tid];
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
__global__ __launch_bounds__(kTileCells) void map_combine_kernel(MapConst k, const uint32_t *__restrict__ first,
                                                                 const uint32_t *__restrict__ last,
                                                                 const uint32_t *__restrict__ seg_off,
                                                                 const uint32_t *__restrict__ part_off,
                                                                 const uint32_t *__restrict__ seg_tile,
                                                                 uint32_t seg_len, uint32_t part_cap,
                                                                 const double *__restrict__ parts,
                                                                 uint32_t *__restrict__ counts,
                                                                 double *__restrict__ planes) {
    const uint32_t g = blockIdx.x;
    if (g >= seg_off[k.tiles]) return;
    const uint32_t tid = threadIdx.x, tile = seg_tile[g];
    if (tile >= k.tiles || g != seg_off[tile]) return;
    const uint32_t nseg = segments_of(last[tile] - first[tile], seg_len);
    if (nseg < 2 || (size_t)part_off[tile] + nseg > part_cap) return;
    const double *p = parts + (size_t)part_off[tile] * (F + 1) * kTileCells;
    double sum[F + 1];
    for (uint32_t f = 0; f <= F; ++f) sum[f] = p[f * kTileCells + tid];
    for (uint32_t s = 1; s < nseg; ++s) {
        p += (F + 1) * kTileCells;
        for (uint32_t f = 0; f <= F; ++f) sum[f] += p[f * kTileCells + tid];
    }
    const uint32_t x = (tile % k.tiles_x) * kTile + tid % kTile, y = (tile / k.tiles_x) * kTile + tid / kTile;
    if (x < k.w && y < k.h) {
        const size_t cell = (size_t)y * k.w + x, cells = (size_t)k.w * k.h;
        counts[cell] = (uint32_t)sum[F];  // (exact: below 2^32)
        for (uint32_t f = 0; f < F; ++f) planes[f * cells + cell] = sum[f];
    }
}

// ---- finish: the maximum count per block, then everything in a fixed order ---------------------------
__global__ __launch_bounds__(kThreads) void map_max_kernel(const uint32_t *__restrict__ counts, size_t cells,
                                                           uint32_t *__restrict__ block_max) {
    __shared__ uint32_t m[kThreads];
    uint32_t best = 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += (size_t)gridDim.x * kThreads)
        best = std::max(best, counts[i]);
    m[threadIdx.x] = best;
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) m[threadIdx.x] = std::max(m[threadIdx.x], m[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) block_max[blockIdx.x] = m[0];
}

// res[f] = sum over the classify blocks of slab element f, by sum_over_blocks in 32 groups.
// res[kGlobalFields] = the maximum of block_max.
__global__ __launch_bounds__(kThreads) void map_finish_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                              const uint32_t *__restrict__ block_max,
                                                              uint32_t max_blocks, double *__restrict__ res) {
    constexpr uint32_t kGroups = kThreads / kGlobalFields;
    __shared__ double pp[kGroups][kGlobalFields];
    __shared__ uint32_t m[kThreads];
    const uint32_t tid = threadIdx.x;
    uint32_t best = 0;
    for (uint32_t b = tid; b < max_blocks; b += kThreads) best = std::max(best, block_max[b]);
    m[tid] = best;
    const double sum = sum_over_blocks<kGroups>(slabs, blocks, kGlobalFields, tid % kGlobalFields, pp);
    if (tid < kGlobalFields) res[tid] = sum;
    if (tid == kThreads - 1) {
        uint32_t r = 0;
        for (uint32_t q = 0; q < kThreads; ++q) r = std::max(r, m[q]);
        res[kGlobalFields] = (double)r;
    }
}

uint32_t bits_of(uint32_t x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

}  // namespace

struct MapWork : Workspace {  // (all but the last three grow to the largest call so far)
    SortBufs<uint32_t> sort;                // the two sides of (key, body index), the histogram
    DeviceBuf<uint32_t> first, last;        // [tiles]
    DeviceBuf<uint32_t> seg_off, part_off;  // [tiles + 1]
    DeviceBuf<uint32_t> seg_tile;           // [segments possible]
    DeviceBuf<uint32_t> block_tot;          // [blocks of the segment scan][2]
    DeviceBuf<double> parts;                // [partial slots][fields + 1][64]
    DeviceBuf<double> slabs;                // [classify blocks][kGlobalFields]
    DeviceBuf<uint32_t> counts;             // [cells]
    DeviceBuf<double> planes;               // [fields][cells]
    DeviceBuf<uint32_t> block_max;          // [kMaxBlocks]
    DeviceBuf<double> res;                  // [kResDoubles]
    PinnedBuf<double> h_res;                // as res
};

namespace {

// At least `count` elements behind b.  A failure leaves b empty and the simulator usable: the sticky error
// is cleared.
template <class T>
int map_reserve(DeviceBuf<T> &b, size_t count) {
    if (b.reserve(count) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("map: cannot allocate %zu bytes of device workspace", sizeof(T) * count);
    return NB_ERR_ALLOC;
}

template <uint32_t F>
int launch_sums(SimBase &sim, MapWork &w, const MapConst &k, const float4 *posm, const float4 *vel, const uint32_t *keys,
                const uint32_t *idx, uint32_t seg_len, uint32_t seg_cap, uint32_t part_cap) {
    const uint32_t *first = w.first, *last = w.last, *seg_off = w.seg_off, *part_off = w.part_off;
    const uint32_t *seg_tile = w.seg_tile;
    hipLaunchKernelGGL(map_sum_kernel<F>, dim3(seg_cap), dim3(kThreads), 0, sim.stream, posm, vel, k, keys, idx, first,
                       last, seg_off, part_off, seg_tile, seg_len, sim.n, part_cap, w.res, w.counts, w.planes, w.parts);
    NB_HIP_TRY(hipGetLastError());
    if (part_cap > 0) {
        hipLaunchKernelGGL(map_combine_kernel<F>, dim3(seg_cap), dim3(kTileCells), 0, sim.stream, k, first, last,
                           seg_off, part_off, seg_tile, seg_len, part_cap, w.parts, w.counts, w.planes);
        NB_HIP_TRY(hipGetLastError());
    }
    return NB_OK;
}

}  // namespace

int sim_map(SimBase &sim, const nb_map_params &params, const MapPlan &plan, uint32_t *counts, double *planes,
            nb_map_stats *stats) {
    if (int rc = analysis_begin(sim, "map")) return rc;
    if (!counts && !planes && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    MapWork *work = nullptr;
    if (int rc = workspace(sim, kWorkMap, &work, [](MapWork &f) {
            if (f.block_max.reserve(kMaxBlocks) != hipSuccess || f.res.reserve(kResDoubles) != hipSuccess ||
                f.h_res.reserve(kResDoubles) != hipSuccess) {
                (void)hipGetLastError();
                set_error("map: cannot allocate the result workspace");
                return NB_ERR_ALLOC;
            }
            return NB_OK;
        }))
        return rc;
    MapWork &w = *work;
    const uint32_t n = sim.n, width = params.width, height = params.height;
    const bool com = (params.flags & NB_MAP_CENTER_COM) != 0, velocity = (params.flags & NB_MAP_VELOCITY) != 0;
    const uint32_t fields = velocity ? kMaxFields : 1;
    const size_t cells = (size_t)width * height;

    MapConst k{};
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
        k.n[a] = plan.n[a];
        k.e1[a] = plan.e1[a];
        k.e2[a] = plan.e2[a];
    }
    k.xlo = params.x_range[0];
    k.xhi = params.x_range[1];
    k.ylo = params.y_range[0];
    k.yhi = params.y_range[1];
    k.dlo = params.depth_range[0];
    k.dhi = params.depth_range[1];
    k.dx = plan.dx;
    k.dy = plan.dy;
    k.w = width;
    k.h = height;
    k.tiles_x = (width + kTile - 1) / kTile;
    k.tiles = k.tiles_x * ((height + kTile - 1) / kTile);
    k.center_com = com;

    std::memset(w.h_res, 0, sizeof(double) * kResDoubles);
    if (n > 0) {
        const uint32_t seg_len = (uint32_t)sim.map_segment_len;
        const uint32_t class_blocks = (n + kThreads - 1) / kThreads;
        const SortShape shape = sort_shape(n);
        const uint32_t passes = (bits_of(k.tiles) + 7) / 8;  // keys' tiles run 0 .. tiles
        // segments: a tile with bodies has at most 1 + (len - 1) / seg_len; those of longer lists number
        // at most 2 (len / seg_len)
        const uint32_t seg_cap = std::min(k.tiles, n) + n / seg_len;
        const uint32_t part_cap = 2 * (n / seg_len);
        if (int rc = w.sort.reserve(n, shape, [](auto &b, size_t count) { return map_reserve(b, count); })) return rc;
        if (int rc = map_reserve(w.first, k.tiles)) return rc;
        if (int rc = map_reserve(w.last, k.tiles)) return rc;
        if (int rc = map_reserve(w.seg_off, (size_t)k.tiles + 1)) return rc;
        if (int rc = map_reserve(w.part_off, (size_t)k.tiles + 1)) return rc;
        if (int rc = map_reserve(w.seg_tile, seg_cap)) return rc;
        const uint32_t list_blocks = (k.tiles + 1 + kScanThreads - 1) / kScanThreads;
        if (int rc = map_reserve(w.block_tot, (size_t)2 * list_blocks)) return rc;
        if (int rc = map_reserve(w.parts, std::max<size_t>(1, part_cap) * (fields + 1) * kTileCells))
            return rc;
        if (int rc = map_reserve(w.slabs, (size_t)kGlobalFields * class_blocks)) return rc;
        if (int rc = map_reserve(w.counts, cells)) return rc;
        if (int rc = map_reserve(w.planes, fields * cells)) return rc;

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        hipLaunchKernelGGL(map_classify_kernel, dim3(class_blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, mom,
                           w.sort.keys[0], w.slabs, w.res);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, passes, kCellBits, nullptr)) return rc;
        const uint32_t *keys = w.sort.keys[passes & 1], *idx = w.sort.idx[passes & 1];
        NB_HIP_TRY(hipMemsetAsync(w.first, 0, sizeof(uint32_t) * k.tiles, sim.stream));
        NB_HIP_TRY(hipMemsetAsync(w.last, 0, sizeof(uint32_t) * k.tiles, sim.stream));
        NB_HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * cells, sim.stream));
        NB_HIP_TRY(hipMemsetAsync(w.planes, 0, sizeof(double) * fields * cells, sim.stream));
        hipLaunchKernelGGL(map_bounds_kernel, dim3(class_blocks), dim3(kThreads), 0, sim.stream, keys, n, k.tiles,
                           w.first, w.last);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(map_segments_local_kernel, dim3(list_blocks), dim3(kScanThreads), 0, sim.stream,
                           w.first, w.last, k.tiles, seg_len, w.seg_off, w.part_off, w.block_tot);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(map_segments_final_kernel, dim3(list_blocks), dim3(kScanThreads), 0, sim.stream,
                           w.first, w.last, k.tiles, seg_len, w.seg_off, w.part_off, w.block_tot, w.seg_tile,
                           seg_cap);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = velocity ? launch_sums<kMaxFields>(sim, w, k, posm, vel, keys, idx, seg_len, seg_cap, part_cap)
                              : launch_sums<1>(sim, w, k, posm, vel, keys, idx, seg_len, seg_cap, part_cap))
            return rc;
        const uint32_t max_blocks = (uint32_t)std::min<size_t>(kMaxBlocks, (cells + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(map_max_kernel, dim3(max_blocks), dim3(kThreads), 0, sim.stream, w.counts, cells,
                           w.block_max);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(map_finish_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, class_blocks,
                           w.block_max, max_blocks, w.res + kUsed);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(double) * kResDoubles, hipMemcpyDeviceToHost, sim.stream));
        if (counts)
            NB_HIP_TRY(hipMemcpyAsync(counts, w.counts, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, sim.stream));
        if (planes)
            NB_HIP_TRY(hipMemcpyAsync(planes, w.planes, sizeof(double) * fields * cells, hipMemcpyDeviceToHost,
                                      sim.stream));
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    } else {
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        centre_used_empty(w.h_res, com, k.c, k.vc);
        if (counts) std::memset(counts, 0, sizeof(uint32_t) * cells);
        if (planes) std::memset(planes, 0, sizeof(double) * fields * cells);
    }
    if (int rc = sim.diag_status()) return rc;

    if (stats) {
        const double *used = w.h_res, *g = w.h_res + kUsed;
        nb_map_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = (uint64_t)g[kGBad];
        o.binned_count = (uint64_t)g[kGBinned];
        o.outside_count = (uint64_t)g[kGOutside];
        o.binned_mass = g[kGBinnedMass];
        o.outside_mass = g[kGOutsideMass];
        o.mass = g[kGMass];
        for (int a = 0; a < 3; ++a) {
            o.center[a] = used[a];
            o.velocity[a] = used[3 + a];
            o.n_hat[a] = plan.n[a];
            o.e1[a] = plan.e1[a];
            o.e2[a] = plan.e2[a];
        }
        o.width = width;
        o.height = height;
        o.flags = params.flags;
        o.max_count = (uint32_t)w.h_res[kResMax];
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
