// nb_fof.hpp -- what the passes that start from the friends-of-friends groups share (nb_fof.hip: nb_sim_fof itself;
// nb_bound.hip: nb_sim_bound), and what every group finder shares (nb_hop.hip: nb_sim_hop): the plan and the integer
// results of the group finder on the device, its workspace, the parts of it that only enqueue, and the work-item table
// over lists of unequal length.
#pragma once

#include <algorithm>

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

#ifdef __HIPCC__

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
