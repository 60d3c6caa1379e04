// nb_fof.hpp -- what the passes that start from the friends-of-friends groups share (nb_fof.hip: nb_sim_fof itself;
// nb_bound.hip: nb_sim_bound), and what every group finder shares (nb_hop.hip: nb_sim_hop): the plan and the integer
// results of the group finder on the device, its workspace, the parts of it that only enqueue, and the work-item table
// over lists of unequal length.
#pragma once

#include <algorithm>
#include <functional>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

// The plan and the integer results of a call, on the device.  Written by single threads or integer atomics.
struct FofInfo {
    double lo[3];
    double h;
    unsigned long long total;      // cells of the grid = the key of a body that does not count
    unsigned long long nx, ny, nz;
    unsigned long long grouped_bodies, largest;  // largest: count << 32 | ~label
    uint32_t status;               // 1: refused, too many cells on an axis
    uint32_t n_ok, ncells;
    uint32_t passes[2];            // sort passes in use: the cell keys', the rows'
    uint32_t components, groups, rows;  // rows = min(groups, capacity): the key past the last row
    uint32_t row_bodies;           // bodies of the rows below `rows`
};

struct FofWork : Workspace {  // (all but the last two grow to the largest call so far)
    SortBufs<unsigned long long> sort;      // the two sides of both sorts, the histogram
    DeviceBuf<double> slabs;                // [bounds blocks][kBoundFields]
    DeviceBuf<uint32_t> flags, excl;        // [n]: what a scan reads and writes
    DeviceBuf<uint32_t> block_tot;          // [scan blocks + 1]: the blocks' sums, then the sum of all
    DeviceBuf<unsigned long long> cell_key; // [n]
    DeviceBuf<uint32_t> cell_start;         // [n + 1]
    DeviceBuf<uint32_t> boxes;              // [n][6]
    DeviceBuf<float4> spos;                 // [n]: positions in sorted order
    DeviceBuf<uint32_t> parent, labels, count, row_of, group_of;  // [n]
    DeviceBuf<uint32_t> row_start;          // [rows possible + 1]
    DeviceBuf<double> runs;                 // [run slots][kTerms]
    DeviceBuf<nb_fof_group> rows;           // [rows possible]
    PinnedBuf<uint32_t> h_labels, h_group_of;  // [n]: staged, so that a refused call leaves the outputs alone
    PinnedBuf<nb_fof_group> h_rows;
    DeviceBuf<FofInfo> info;                // [1]
    PinnedBuf<FofInfo> h_info;              // [1]
};

// The most catalogue rows a call can have: those the caller has room for, and those n bodies can make.
inline uint32_t fof_rows_cap(uint32_t n, size_t group_capacity, uint32_t min_members) {
    return (uint32_t)std::min<size_t>(group_capacity, n / min_members);
}

// nb_fof.hip: the group finder's workspace (made by the first call), and the pass itself enqueued on the
// simulator's stream with no synchronisation and no copy to the host (n > 0; the device is bound; params checked
// by fof_check_params).  Afterwards, in stream order, on the device: w.info; w.labels; w.group_of (want_group_of
// or rows_cap > 0); and for rows_cap > 0 the rows' label and count in w.rows (their nine sums too when `sums`),
// w.row_start[0 .. rows], and the bodies of the rows sorted stably by row -- every row's members in ascending body
// index -- on side info->passes[1] & 1 of w.sort.idx.  After a refusal (info->status) none of them is defined.
int fof_work(SimBase &sim, FofWork **out);
int fof_enqueue(SimBase &sim, FofWork &w, const nb_fof_params &params, uint32_t rows_cap, bool want_group_of,
                bool sums);
// The part of the pass from "labels, sizes, rows" onwards, which every group finder shares (nb_hop.hip calls it with
// its own forest): parent[i] is NB_FOF_NONE for a body of no group, else a body of i's group nearer its root, the
// root pointing at itself.  It resolves w.labels, sizes the groups and makes the catalogue exactly as described
// above; w.info must hold status 0 and zeroed integer results, and fof_catalogue_reserve(w, n, rows_cap) must have
// succeeded before anything of the call was enqueued.
int fof_catalogue_reserve(FofWork &w, uint32_t n, uint32_t rows_cap);
int fof_catalogue_enqueue(SimBase &sim, FofWork &w, const uint32_t *parent, uint32_t min_members, uint32_t rows_cap,
                          bool want_group_of, bool sums);
// the error of a refused plan (info->status), reported after the call's synchronisation
int fof_refused(const nb_fof_params &params);
int fof_refused(const char *pass, double link);
// The stages of the pass before its union, which every finder on the cell grid shares (nb_fof6.hip calls them with
// its own union behind): bounds, plan and key, the sort, the cell table (w.cell_key, w.cell_start, info->ncells),
// w.flags[p] = the cell of sorted position p, the positions gathered in sorted order (w.spos), w.parent[i] = the first
// body of i's cell (NB_FOF_NONE for a body that does not count) and, with use_boxes, the cells' position boxes
// (w.boxes).  The sorted body indices are on side info->passes[0] & 1 of w.sort.idx.  It reserves what it writes and,
// by fof_catalogue_reserve, what the catalogue needs.
int fof_cells_enqueue(SimBase &sim, FofWork &w, double link, uint32_t rows_cap, uint32_t use_boxes);
// work items of a union kernel over the chunks of the occupied cells (item_chunk below); 0 and an error when n bodies
// are more than one call takes
uint32_t fof_union_items(const SimBase &sim, const char *pass);
// The host sequence of a finder on the cell grid, around the kernels `enqueue` puts on the stream (they end with
// fof_catalogue_enqueue): the preamble, the workspace and the pinned staging, the copies, the one synchronisation,
// the refusal of a plan, and the outputs and stats of nb_sim_fof, written only by a call that succeeds.
using FofEnqueue = std::function<int(FofWork &w, uint32_t rows_cap, bool want_group_of)>;
int fof_call(SimBase &sim, const char *pass, double link, uint32_t min_members, const FofEnqueue &enqueue,
             uint32_t *labels, uint32_t *group_of, nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats);

#ifdef __HIPCC__

// the order-preserving encoding of a finite float as an unsigned integer
__device__ inline uint32_t ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float unordered(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// boxes[6 c + a] of cell c raised to the six encodings e of a body (a < 3: ~ordered(x_a), the minimum complemented;
// else ordered(x_a)) by integer atomic maxima.  A full wave whose lanes share one cell sends one lane's six atomics.
__device__ inline void box_raise(uint32_t *__restrict__ boxes, uint32_t c, uint32_t (&e)[6]) {
    const unsigned long long active = __ballot(true);
    const int first = __ffsll((long long)active) - 1;
    const uint32_t c0 = __shfl(c, first);
    if (__ballot(c != c0) == 0ull && active == ~0ull) {
        for (int o = 32; o > 0; o >>= 1)
            for (int a = 0; a < 6; ++a) e[a] = std::max(e[a], (uint32_t)__shfl_xor(e[a], o));
        if (threadIdx.x % kWave == 0)
            for (int a = 0; a < 6; ++a) atomicMax(&boxes[(size_t)6 * c + a], e[a]);
    } else {
        for (int a = 0; a < 6; ++a) atomicMax(&boxes[(size_t)6 * c + a], e[a]);
    }
}
// per axis the gap between the boxes of cells c and nb and their farthest extent, in binary64 (exact differences of
// binary32 numbers, rounded once)
__device__ inline void box_gap_far(const uint32_t *__restrict__ boxes, uint32_t c, uint32_t nb, double (&gap)[3],
                                   double (&far)[3]) {
    for (int a = 0; a < 3; ++a) {
        const double alo = unordered(~boxes[(size_t)6 * c + a]), ahi = unordered(boxes[(size_t)6 * c + 3 + a]);
        const double blo = unordered(~boxes[(size_t)6 * nb + a]), bhi = unordered(boxes[(size_t)6 * nb + 3 + a]);
        gap[a] = fmax(0.0, fmax(blo - ahi, alo - bhi));
        far[a] = fmax(bhi - alo, ahi - blo);
    }
}

// ---- the lock-free forest ------------------------------------------------------------------------------
__device__ inline uint32_t load_parent(const uint32_t *parent, uint32_t i) {
    return __atomic_load_n(parent + i, __ATOMIC_RELAXED);
}
// parent[x] < x unless x is a root: the walk ends
__device__ inline uint32_t find_root(const uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = load_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}
// ... and on the way points every second node at its grandparent (path halving).  Only a node that is not a
// root is written, with a smaller ancestor of its own tree, and a node never becomes a root again: the
// exchange in unite, which expects a root, is not disturbed, and parent[x] < x holds on.
__device__ inline uint32_t find_root_halving(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = load_parent(parent, x);
        if (p == x) return x;
        const uint32_t g = load_parent(parent, p);
        if (g != p) __atomic_store_n(parent + x, g, __ATOMIC_RELAXED);
        x = g;
    }
}
// Hook the larger root under the smaller.  A failed exchange means another thread hooked that root first:
// find both roots again.  Nothing waits on another thread.
__device__ inline void unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_root_halving(parent, a);
        b = find_root_halving(parent, b);
        if (a == b) return;
        const uint32_t hi = std::max(a, b), lo = std::min(a, b);
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
        a = hi;
        b = lo;
    }
}

constexpr uint32_t kFofNeighbours = 62;  // forward neighbours within +-2 cells per axis: (5^3 - 1) / 2

// The cell table's entry of the l-th forward neighbour (l < kFofNeighbours) of occupied cell c within +-2 cells per axis, in
// (z, y, x) order after (0, 0, 0); false when it is outside the grid or holds no body.
__device__ inline bool forward_neighbour(const FofInfo *__restrict__ info,
                                         const unsigned long long *__restrict__ cell_key, uint32_t ncells, uint32_t c,
                                         uint32_t l, uint32_t *nb) {
    const unsigned long long nx = info->nx, ny = info->ny, nz = info->nz, key = cell_key[c];
    const long long cx = (long long)(key % nx), cy = (long long)((key / nx) % ny), cz = (long long)(key / (nx * ny));
    const uint32_t t = l + kFofNeighbours + 1;
    const long long ox = (long long)(t % 5) - 2, oy = (long long)((t / 5) % 5) - 2, oz = (long long)(t / 25) - 2;
    const long long x = cx + ox, y = cy + oy, z = cz + oz;
    if (!(x >= 0 && x < (long long)nx && y >= 0 && y < (long long)ny && z >= 0 && z < (long long)nz)) return false;
    const unsigned long long want = ((unsigned long long)z * ny + (unsigned long long)y) * nx + (unsigned long long)x;
    uint32_t lo = c + 1, hi = ncells;  // (a forward neighbour has a larger key)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cell_key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    if (!(lo < ncells && cell_key[lo] == want)) return false;
    *nb = lo;
    return true;
}

// The list of work item g among lists l = 0 .. count - 1 of positions [start[l], start[l + 1]), cut into chunks
// of len: list l owns the items start[l] / len + l onwards, which are at least its chunks.  False for an item
// no list owns.  *a0, *a1: the chunk's positions; *s: its number in the list.
__device__ inline bool item_chunk(const uint32_t *__restrict__ start, uint32_t count, uint32_t len, uint32_t g,
                                  uint32_t *l_out, uint32_t *s_out, uint32_t *a0, uint32_t *a1) {
    if (count == 0) return false;
    uint32_t lo = 0, hi = count;  // start[0] / len + 0 = 0 <= g
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((unsigned long long)start[mid] / len + mid <= g) lo = mid;
        else hi = mid;
    }
    const uint32_t s = g - (start[lo] / len + lo);
    const unsigned long long first = (unsigned long long)start[lo] + (unsigned long long)s * len;
    const uint32_t end = start[lo + 1];
    if (first >= end) return false;
    *l_out = lo;
    *s_out = s;
    *a0 = (uint32_t)first;
    *a1 = (uint32_t)std::min<unsigned long long>(end, first + len);
    return true;
}

// the first run slot of row r: rows before it hold at most start / 64 + r runs
__device__ inline size_t run_slot(uint32_t start, uint32_t r) { return (size_t)start / kWave + r; }

#endif  // __HIPCC__

}  // namespace nb
