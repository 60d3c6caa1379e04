// nb_fof.hip -- nb_sim_fof: the friends-of-friends groups of a simulator's current state (include/nbody.h
// "Friends-of-friends groups"; no reference counterpart).
//
// Bodies i != j are friends iff d2 <= link * link in binary64; a group is a connected component of that
// graph, its label the smallest body index in it.  The graph is fixed by the state, so the partition is
// unique and everything integer here is exact, whatever order the threads ran in.
//   bounds  -- the per-axis minimum and maximum of the counted bodies (body_ok) and their number over the float4
//              SoA state (SimBase::diag_state), by the bounds pass of nb_analysis_sort.hpp; the one block that
//              finishes them makes the plan on the device: the grid's origin, the cells per axis of side
//              h = (link / sqrt(3)) (1 - 2^-20), the key bits in use -- or the refusal of a state that needs
//              more than 2^21 cells on an axis.  Every later kernel reads the plan; after a refusal they all
//              return at once.  No host round trip;
//   key     -- one 64-bit linear cell key per body, (cz ny + cy) nx + cx, or the key past the last cell
//              for a body that does not count;
//   sort    -- the stable sort of nb_analysis_sort.hpp on (key, body index).  Eight passes are enqueued, those
//              the plan does not need (passes[0]; all of them after a refusal) return at once, and the sorted
//              arrays are on side passes[0] & 1.  A cell's bodies end up consecutive and in body order;
//   cells   -- the occupied cells (key, start) from neighbouring keys and a scan, every body's position
//              gathered in sorted order, parent[i] = the first body of i's cell -- all bodies of a cell are
//              friends without a test (the cell's diagonal is below link) -- and the cells' bounding boxes by
//              integer atomic minima and maxima of the order-preserving encoding of a float;
//   union   -- one wave per chunk of at most "fof_chunk_len" bodies of an occupied cell A.  Lane l looks
//              up the l-th of the 62 forward neighbours within +-2 cells per axis by binary search in the
//              cell table and classes it by the boxes: apart (nearest corners beyond link), all friends
//              (farthest corners within link), or to be tested.  A neighbour whose representative already
//              shares A's root is skipped; otherwise the pairs of A x B are tested by the rule, lanes over
//              A's bodies, until a wave ballot finds a hit; then the roots are united lock-free by
//              atomicCAS(&parent[max], max, min), retried on failure.  No locks, no waiting on other threads;
//   labels  -- every body follows parent to its root, which hooking to the smaller makes the component's
//              smallest index; component sizes by integer atomics on the root;
//   rows    -- roots with count >= min_members flagged and scanned into catalogue rows, group_of, and the
//              integer stats by integer atomics;
//   sums    -- (only when the catalogue is asked for) the grouped bodies sorted stably by row, then one
//              wave per chunk of a row's list: runs of 64 members by the fixed butterfly, one slot per run;
//              then 16 lanes per row add the row's runs in order.  The chunk length decides who adds a run,
//              never in which order: the sums do not depend on it.
// No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kMaxPasses = 8;       // a 64-bit key
constexpr uint32_t kTerms = 9;           // the sums of a catalogue row
constexpr uint32_t kRowLanes = 16;       // lanes per row of the combine kernel
constexpr uint32_t kNeighbours = kFofNeighbours;
constexpr double kMaxCells = (double)NB_FOF_MAX_CELLS_PER_AXIS;

__host__ __device__ inline uint32_t bits_of(unsigned long long x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

// One block: the bounds into the plan.  A refusal leaves no sort pass to run (passes[1] stays 0: the rows' plan
// returns first); every other kernel tests status itself.
__global__ __launch_bounds__(kThreads) void fof_plan_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                            double h, FofInfo *__restrict__ info) {
    double lo[3], hi[3];
    FofInfo o{};
    if (!bounds_finish(slabs, blocks, lo, hi, &o.n_ok)) return;
    o.h = h;
    if (o.n_ok > 0) {
        unsigned long long cells[3];
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = lo[a];
            const double c = floor((hi[a] - lo[a]) / h) + 1.0;
            if (!(c <= kMaxCells)) o.status = 1;
            cells[a] = o.status ? 0ull : (unsigned long long)c;
        }
        o.nx = cells[0];
        o.ny = cells[1];
        o.nz = cells[2];
        o.total = o.status ? 0ull : o.nx * o.ny * o.nz;  // (at most 2^63)
    }
    o.passes[0] = o.status ? 0u : std::max(1u, (bits_of(o.total) + 7) / 8);  // keys run 0 .. total
    *info = o;
}

// ---- key ------------------------------------------------------------------------------------------
// The cell of coordinate x on an axis of `cells` cells from lo: floor((x - lo) / h), x >= lo
__device__ inline unsigned long long cell_of(float x, double lo, double h, unsigned long long cells) {
    const double q = floor(((double)x - lo) / h);
    const unsigned long long c = (unsigned long long)q;
    return c < cells ? c : cells - 1;  // (q < cells by the plan's own division; the clamp never binds)
}

__global__ __launch_bounds__(kThreads) void fof_key_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, uint32_t n,
                                                           const FofInfo *__restrict__ info,
                                                           unsigned long long *__restrict__ keys) {
    if (info->status) return;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i];
    unsigned long long key = info->total;
    if (body_ok(p, vel[i])) {
        const unsigned long long cx = cell_of(p.x, info->lo[0], info->h, info->nx);
        const unsigned long long cy = cell_of(p.y, info->lo[1], info->h, info->ny);
        const unsigned long long cz = cell_of(p.z, info->lo[2], info->h, info->nz);
        key = (cz * info->ny + cy) * info->nx + cx;
    }
    keys[i] = key;
}

// ---- scans over n elements: kScanThreads elements per block, then the blocks' sums by one block --------
// excl[i] = flags before i in i's block; block_tot[b] = the flags of block b
__global__ __launch_bounds__(kScanThreads) void fof_scan_local_kernel(const FofInfo *__restrict__ info,
                                                                      const uint32_t *__restrict__ flags, uint32_t n,
                                                                      uint32_t *__restrict__ excl,
                                                                      uint32_t *__restrict__ block_tot) {
    if (info->status) return;
    __shared__ uint32_t lds[2 * kScanThreads];
    const uint32_t tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * kScanThreads + tid;
    const uint32_t s = i < n ? flags[i] : 0u;
    uint32_t *a = lds, *b = lds + kScanThreads;
    a[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {
        b[tid] = tid >= o ? a[tid] + a[tid - o] : a[tid];
        __syncthreads();
        uint32_t *t = a;
        a = b;
        b = t;
    }
    if (i < n) excl[i] = a[tid] - s;
    if (tid == kScanThreads - 1) block_tot[blockIdx.x] = a[tid];
}

// block_tot scanned in place (exclusive); the sum of all to *total
__global__ __launch_bounds__(kScanThreads) void fof_scan_blocks_kernel(const FofInfo *__restrict__ info,
                                                                       uint32_t *__restrict__ block_tot,
                                                                       uint32_t blocks, uint32_t *__restrict__ total) {
    if (info->status) return;
    __shared__ uint32_t lds[2 * kScanThreads];
    const uint32_t t = block_scan_runs(block_tot, blocks, lds);
    if (threadIdx.x == 0) *total = t;
}

__device__ inline uint32_t scanned(const uint32_t *excl, const uint32_t *block_tot, size_t i) {
    return excl[i] + block_tot[i / kScanThreads];
}

// ---- cells ----------------------------------------------------------------------------------------
// flags[p] = 1 where a cell starts in the sorted keys
__global__ __launch_bounds__(kThreads) void fof_heads_kernel(const FofInfo *__restrict__ info,
                                                             const unsigned long long *__restrict__ k0,
                                                             const unsigned long long *__restrict__ k1, uint32_t n,
                                                             uint32_t *__restrict__ flags) {
    if (info->status) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const unsigned long long *keys = info->passes[0] & 1 ? k1 : k0;
    const unsigned long long key = keys[p];
    flags[p] = key < info->total && (p == 0 || keys[p - 1] != key);
}

// the cell table: cell_key[c], cell_start[c] for the c-th occupied cell, cell_start[ncells] = counted bodies;
// flags[p] becomes the cell of sorted position p
__global__ __launch_bounds__(kThreads) void fof_cells_kernel(const FofInfo *__restrict__ info,
                                                             const unsigned long long *__restrict__ k0,
                                                             const unsigned long long *__restrict__ k1, uint32_t n,
                                                             const uint32_t *__restrict__ excl,
                                                             const uint32_t *__restrict__ block_tot,
                                                             uint32_t *__restrict__ flags,
                                                             unsigned long long *__restrict__ cell_key,
                                                             uint32_t *__restrict__ cell_start) {
    if (info->status) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= info->n_ok) return;
    const unsigned long long *keys = info->passes[0] & 1 ? k1 : k0;
    const uint32_t head = flags[p], c = scanned(excl, block_tot, p) + head - 1;
    if (head) {
        cell_key[c] = keys[p];
        cell_start[c] = (uint32_t)p;
    }
    if (p + 1 == info->n_ok) cell_start[c + 1] = info->n_ok;
    flags[p] = c;
}

// parent, the gathered positions and the cells' boxes.  boxes[6 c + a]: a < 3 the maximum of ~ordered(x_a)
// (the minimum, complemented), else the maximum of ordered(x_a); cleared to 0 beforehand.
__global__ __launch_bounds__(kThreads) void fof_parent_kernel(FofInfo *__restrict__ info,
                                                              const float4 *__restrict__ posm,
                                                              const uint32_t *__restrict__ i0p,
                                                              const uint32_t *__restrict__ i1p, uint32_t n,
                                                              const uint32_t *__restrict__ cell_of_pos,
                                                              const uint32_t *__restrict__ cell_start,
                                                              const uint32_t *__restrict__ block_tot_total,
                                                              float4 *__restrict__ spos, uint32_t *__restrict__ parent,
                                                              uint32_t *__restrict__ boxes, uint32_t use_boxes) {
    if (info->status) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p == 0) info->ncells = *block_tot_total;
    if (p >= n) return;
    const uint32_t *idx = info->passes[0] & 1 ? i1p : i0p;
    const uint32_t body = idx[p];
    if (p >= info->n_ok) {
        parent[body] = NB_FOF_NONE;
        return;
    }
    const uint32_t c = cell_of_pos[p];
    parent[body] = idx[cell_start[c]];
    const float4 q = posm[body];
    spos[p] = q;
    if (!use_boxes) return;
    uint32_t e[6] = {~ordered(q.x), ~ordered(q.y), ~ordered(q.z), ordered(q.x), ordered(q.y), ordered(q.z)};
    box_raise(boxes, c, e);
}

// ---- union ----------------------------------------------------------------------------------------
// the rule of include/nbody.h
__device__ inline bool friends(float4 p, float4 q, double b2) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    return (dx * dx + dy * dy) + dz * dz <= b2;
}

__global__ __launch_bounds__(kWave) void fof_union_kernel(const FofInfo *__restrict__ info,
                                                          const unsigned long long *__restrict__ cell_key,
                                                          const uint32_t *__restrict__ cell_start,
                                                          const uint32_t *__restrict__ boxes,
                                                          const uint32_t *__restrict__ i0p,
                                                          const uint32_t *__restrict__ i1p,
                                                          const float4 *__restrict__ spos, uint32_t *parent,
                                                          uint32_t len, double b2, uint32_t use_boxes) {
#pragma clang fp contract(off)
    if (info->status) return;
    const uint32_t ncells = info->ncells, lane = threadIdx.x;
    uint32_t c, s, a0, a1;
    if (!item_chunk(cell_start, ncells, len, blockIdx.x, &c, &s, &a0, &a1)) return;  // (uniform over the wave)
    const uint32_t *idx = info->passes[0] & 1 ? i1p : i0p;
    const uint32_t rep_a = idx[cell_start[c]];

    // lane l: the l-th forward neighbour, its place in the cell table and its class by the boxes
    uint32_t nb = 0, cls = 0;  // 0 none or apart, 1 test the pairs, 2 all friends
    if (lane < kNeighbours) {
        if (forward_neighbour(info, cell_key, ncells, c, lane, &nb)) {
            cls = 1;
            if (use_boxes) {
                // per axis the gap between the boxes and their farthest extent; the pair rule's own
                // operations on them bound every pair's d2 from below and from above (rounding is monotone)
                double gap[3], far[3];
                box_gap_far(boxes, c, nb, gap, far);
                if ((gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2] > b2) cls = 0;
                else if ((far[0] * far[0] + far[1] * far[1]) + far[2] * far[2] <= b2) cls = 2;
            }
        }
    }
    // all friends: united by the cell's first chunk alone
    unsigned long long direct = __ballot(cls == 2), test = __ballot(cls == 1);
    if (s != 0) direct = 0ull;
    while (direct) {
        const int l = __ffsll((long long)direct) - 1;
        direct &= direct - 1;
        const uint32_t b = __shfl(nb, l);
        if (lane == 0) unite(parent, rep_a, idx[cell_start[b]]);
    }
    while (test) {
        const int l = __ffsll((long long)test) - 1;
        test &= test - 1;
        const uint32_t b = __shfl(nb, l);
        const uint32_t rep_b = idx[cell_start[b]];
        uint32_t same = 0;
        if (lane == 0) same = find_root_halving(parent, rep_a) == find_root_halving(parent, rep_b);
        if (__shfl(same, 0)) continue;
        const uint32_t b0 = cell_start[b], b1 = cell_start[b + 1];
        bool hit = false;
        for (uint32_t a = a0; a < a1 && !hit; a += kWave) {
            const bool valid = a + lane < a1;
            const float4 pa = spos[valid ? a + lane : a];
            for (uint32_t j = b0; j < b1; ++j) {
                const float4 pb = spos[j];
                if (__ballot(valid && friends(pa, pb, b2))) {
                    hit = true;
                    break;
                }
            }
        }
        if (hit && lane == 0) unite(parent, rep_a, rep_b);
    }
}

// ---- labels, component sizes ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fof_label_kernel(const FofInfo *__restrict__ info,
                                                             const uint32_t *__restrict__ parent, uint32_t n,
                                                             uint32_t *__restrict__ labels, uint32_t *__restrict__ count) {
    if (info->status) return;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t r = parent[i];
    if (r != NB_FOF_NONE) r = find_root(parent, (uint32_t)i);
    labels[i] = r;
    // the lanes that share the first counted lane's root send one atomic (a large component: most of the wave)
    const bool counted = r != NB_FOF_NONE;
    const unsigned long long any = __ballot(counted);
    if (!any) return;
    const uint32_t r0 = __shfl(r, __ffsll((long long)any) - 1);
    const unsigned long long same = __ballot(counted && r == r0);
    if (counted && r != r0) atomicAdd(&count[r], 1u);
    if (threadIdx.x % kWave == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&count[r0], (uint32_t)__popcll(same));
}

// flags[i] = 1 for the root of a catalogued component; the integer stats
__global__ __launch_bounds__(kThreads) void fof_roots_kernel(FofInfo *__restrict__ info,
                                                             const uint32_t *__restrict__ labels,
                                                             const uint32_t *__restrict__ count, uint32_t n,
                                                             uint32_t min_members, uint32_t *__restrict__ flags) {
    if (info->status) return;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool root = i < n && labels[i] == (uint32_t)i;
    const uint32_t cnt = root ? count[i] : 0u;
    const bool listed = root && cnt >= min_members;
    if (i < n) flags[i] = listed;
    // one lane per wave sends the wave's share: integers, so the order is irrelevant
    const unsigned long long roots = __ballot(root);
    if (!roots) return;
    unsigned long long bodies = listed ? cnt : 0u;
    unsigned long long largest = root ? ((unsigned long long)cnt << 32) | (uint32_t)~(uint32_t)i : 0ull;
    for (int o = 32; o > 0; o >>= 1) {
        bodies += __shfl_xor(bodies, o);
        largest = std::max(largest, (unsigned long long)__shfl_xor(largest, o));
    }
    if (threadIdx.x % kWave == 0) {
        atomicAdd(&info->components, (uint32_t)__popcll(roots));
        if (bodies) atomicAdd(&info->grouped_bodies, bodies);
        atomicMax(&info->largest, largest);
    }
}

// the key past the last row and the passes of the sort by row
__global__ void fof_rows_plan_kernel(FofInfo *__restrict__ info, uint32_t capacity) {
    if (info->status) return;
    info->rows = std::min(info->groups, capacity);
    info->passes[1] = std::max(1u, (bits_of(info->rows) + 7) / 8);
}

// row_of[i] = the row of root i (NB_FOF_NONE for every other body); label and count of the rows below `rows`
__global__ __launch_bounds__(kThreads) void fof_rows_kernel(const FofInfo *__restrict__ info,
                                                            const uint32_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ excl,
                                                            const uint32_t *__restrict__ block_tot,
                                                            const uint32_t *__restrict__ count, uint32_t n,
                                                            uint32_t *__restrict__ row_of,
                                                            nb_fof_group *__restrict__ rows) {
    if (info->status) return;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t row = NB_FOF_NONE;
    if (flags[i]) {
        row = scanned(excl, block_tot, i);
        if (rows && row < info->rows) {
            rows[row].label = (uint32_t)i;
            rows[row].count = count[i];
        }
    }
    row_of[i] = row;
}

// group_of, and (keys non-null) the key of the sort by row: the row, or `rows` for a body of none below it
__global__ __launch_bounds__(kThreads) void fof_group_of_kernel(const FofInfo *__restrict__ info,
                                                                const uint32_t *__restrict__ labels,
                                                                const uint32_t *__restrict__ row_of, uint32_t n,
                                                                uint32_t *__restrict__ group_of,
                                                                unsigned long long *__restrict__ keys) {
    if (info->status) return;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t label = labels[i], row = label == NB_FOF_NONE ? NB_FOF_NONE : row_of[label];
    group_of[i] = row;
    if (keys) keys[i] = row < info->rows ? row : info->rows;
}

// ---- sums -----------------------------------------------------------------------------------------
// row_start[r] = the first sorted position of row r, row_start[rows] = the bodies of all rows
__global__ __launch_bounds__(kThreads) void fof_row_start_kernel(const FofInfo *__restrict__ info,
                                                                 const unsigned long long *__restrict__ k0,
                                                                 const unsigned long long *__restrict__ k1, uint32_t n,
                                                                 uint32_t *__restrict__ row_start) {
    if (info->status) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const unsigned long long *keys = info->passes[1] & 1 ? k1 : k0;
    const unsigned long long key = keys[p], rows = info->rows;
    if (key < rows) {
        if (p == 0 || keys[p - 1] != key) row_start[key] = (uint32_t)p;
        if (p + 1 == n || keys[p + 1] >= rows) row_start[rows] = (uint32_t)(p + 1);
    }
}

// the terms of a member
__device__ inline void terms(float4 p, float4 v, double (&t)[kTerms]) {
#pragma clang fp contract(off)
    const double m = p.w, x = p.x, y = p.y, z = p.z, vx = v.x, vy = v.y, vz = v.z;
    t[0] = m;
    t[1] = m * x;
    t[2] = m * y;
    t[3] = m * z;
    t[4] = m * vx;
    t[5] = m * vy;
    t[6] = m * vz;
    t[7] = m * ((x * x + y * y) + z * z);
    t[8] = m * ((vx * vx + vy * vy) + vz * vz);
}

// One wave per chunk of a row's list: every run of 64 members (from the row's start) through the butterfly
// into its slot.
__global__ __launch_bounds__(kWave) void fof_sum_kernel(const FofInfo *__restrict__ info,
                                                        const float4 *__restrict__ posm,
                                                        const float4 *__restrict__ vel,
                                                        const uint32_t *__restrict__ i0p,
                                                        const uint32_t *__restrict__ i1p,
                                                        const uint32_t *__restrict__ row_start, uint32_t len,
                                                        double *__restrict__ runs) {
    if (info->status) return;
    const uint32_t lane = threadIdx.x;
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, info->rows, len, blockIdx.x, &r, &s, &a0, &a1)) return;
    const uint32_t *idx = info->passes[1] & 1 ? i1p : i0p;
    const uint32_t start = row_start[r];
    for (uint32_t a = a0; a < a1; a += kWave) {  // (len is a multiple of 64: a - start too)
        double t[kTerms];
        for (uint32_t f = 0; f < kTerms; ++f) t[f] = 0.0;
        if (a + lane < a1) {
            const uint32_t body = idx[a + lane];
            terms(posm[body], vel[body], t);
        }
        for (uint32_t f = 0; f < kTerms; ++f) t[f] = wave_sum(t[f]);
        if (lane < kTerms) {
            double mine = t[0];
            for (uint32_t f = 1; f < kTerms; ++f) mine = lane == f ? t[f] : mine;
            runs[(run_slot(start, r) + (a - start) / kWave) * kTerms + lane] = mine;
        }
    }
}

// 16 lanes per row, lane f < 9 adds term f of the row's runs in order
__global__ __launch_bounds__(kThreads) void fof_combine_kernel(const FofInfo *__restrict__ info,
                                                               const uint32_t *__restrict__ row_start,
                                                               const double *__restrict__ runs,
                                                               nb_fof_group *__restrict__ rows) {
    if (info->status) return;
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t f = (uint32_t)(g % kRowLanes);
    const size_t r = g / kRowLanes;
    if (r >= info->rows || f >= kTerms) return;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start;
    const double *p = runs + run_slot(start, (uint32_t)r) * kTerms + f;
    double sum = 0.0;
    for (uint32_t q = 0; q < (count + kWave - 1) / kWave; ++q) sum += p[(size_t)q * kTerms];
    (&rows[r].mass)[f] = sum;
}

}  // namespace

static_assert(sizeof(nb_fof_group) == 8 + 8 * kTerms && offsetof(nb_fof_group, mass) == 8, "nine doubles after the header");

namespace {

template <class B>
int fof_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("fof: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

int enqueue_scan(SimBase &sim, FofWork &w, uint32_t scan_blocks, uint32_t *total) {
    hipLaunchKernelGGL(fof_scan_local_kernel, dim3(scan_blocks), dim3(kScanThreads), 0, sim.stream, w.info, w.flags,
                       sim.n, w.excl, w.block_tot);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fof_scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, sim.stream, w.info, w.block_tot,
                       scan_blocks, total);
    NB_HIP_TRY(hipGetLastError());
    return NB_OK;
}

}  // namespace

static double fof_cell_side(double link) { return (link / std::sqrt(3.0)) * (1.0 - 0x1p-20); }

int fof_work(SimBase &sim, FofWork **out) {
    return workspace(sim, kWorkFof, out, [](FofWork &f) {
        if (f.info.reserve(1) != hipSuccess || f.h_info.reserve(1) != hipSuccess) {
            (void)hipGetLastError();
            set_error("fof: cannot allocate the result workspace");
            return NB_ERR_ALLOC;
        }
        return NB_OK;
    });
}

int fof_refused(const char *pass, double link) {
    set_error("%s: link %g needs more than %u cells on an axis over this state's extent: it is below the "
              "resolution of binary32 coordinates there",
              pass, link, NB_FOF_MAX_CELLS_PER_AXIS);
    return NB_ERR_INVALID;
}
int fof_refused(const nb_fof_params &params) { return fof_refused("fof", params.link); }

int fof_catalogue_reserve(FofWork &w, uint32_t n, uint32_t rows_cap) {
    const SortShape shape = sort_shape(n);
    const uint32_t scan_blocks = (n + kScanThreads - 1) / kScanThreads;
    const size_t run_slots = (size_t)n / kWave + rows_cap + 1;
    if (int rc = w.sort.reserve(n, shape, [](auto &b, size_t count) { return fof_reserve(b, count); })) return rc;
    if (int rc = fof_reserve(w.flags, n)) return rc;
    if (int rc = fof_reserve(w.excl, n)) return rc;
    if (int rc = fof_reserve(w.block_tot, (size_t)scan_blocks + 1)) return rc;
    if (int rc = fof_reserve(w.labels, n)) return rc;
    if (int rc = fof_reserve(w.count, n)) return rc;
    if (int rc = fof_reserve(w.row_of, n)) return rc;
    if (int rc = fof_reserve(w.group_of, n)) return rc;
    if (rows_cap > 0) {
        if (int rc = fof_reserve(w.row_start, (size_t)rows_cap + 1)) return rc;
        if (int rc = fof_reserve(w.runs, run_slots * kTerms)) return rc;
        if (int rc = fof_reserve(w.rows, rows_cap)) return rc;
    }
    return NB_OK;
}

int fof_catalogue_enqueue(SimBase &sim, FofWork &w, const uint32_t *parent, uint32_t min_members, uint32_t rows_cap,
                          bool want_group_of, bool sums) {
    const uint32_t n = sim.n;
    const uint32_t len = (uint32_t)sim.fof_chunk_len;
    const unsigned long long sum_items = (unsigned long long)n / len + rows_cap + 1;
    const uint32_t blocks = (n + kThreads - 1) / kThreads;
    const uint32_t scan_blocks = (n + kScanThreads - 1) / kScanThreads;
    const SortShape shape = sort_shape(n);
    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    FofInfo *info = w.info;
    const auto &keys = w.sort.keys;  // both sides go to the kernels: the plan says where the sorted arrays are
    const auto &idx = w.sort.idx;
    // labels, sizes, rows
    NB_HIP_TRY(hipMemsetAsync(w.count, 0, sizeof(uint32_t) * n, sim.stream));
    hipLaunchKernelGGL(fof_label_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, parent, n, w.labels,
                       w.count);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fof_roots_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, w.labels, w.count, n,
                       min_members, w.flags);
    NB_HIP_TRY(hipGetLastError());
    if (int rc = enqueue_scan(sim, w, scan_blocks, &info->groups)) return rc;
    hipLaunchKernelGGL(fof_rows_plan_kernel, dim3(1), dim3(1), 0, sim.stream, info, rows_cap);
    NB_HIP_TRY(hipGetLastError());
    nb_fof_group *rows = rows_cap > 0 ? (nb_fof_group *)w.rows : nullptr;
    hipLaunchKernelGGL(fof_rows_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, w.flags, w.excl,
                       w.block_tot, w.count, n, w.row_of, rows);
    NB_HIP_TRY(hipGetLastError());
    if (want_group_of || rows_cap > 0) {
        hipLaunchKernelGGL(fof_group_of_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, w.labels, w.row_of,
                           n, w.group_of, rows_cap > 0 ? (unsigned long long *)keys[0] : nullptr);
        NB_HIP_TRY(hipGetLastError());
    }
    if (rows_cap > 0) {  // the catalogue's sums
        if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, (bits_of(rows_cap) + 7) / 8, 0, &info->passes[1]))
            return rc;
        hipLaunchKernelGGL(fof_row_start_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, keys[0],
                           keys[1], n, w.row_start);
        NB_HIP_TRY(hipGetLastError());
        if (sums) {
            hipLaunchKernelGGL(fof_sum_kernel, dim3((uint32_t)sum_items), dim3(kWave), 0, sim.stream, info, posm,
                               vel, idx[0], idx[1], w.row_start, len, w.runs);
            NB_HIP_TRY(hipGetLastError());
            const uint32_t combine_blocks = (uint32_t)(((size_t)rows_cap * kRowLanes + kThreads - 1) / kThreads);
            hipLaunchKernelGGL(fof_combine_kernel, dim3(combine_blocks), dim3(kThreads), 0, sim.stream, info,
                               w.row_start, w.runs, rows);
            NB_HIP_TRY(hipGetLastError());
        }
    }
    return NB_OK;
}

uint32_t fof_union_items(const SimBase &sim, const char *pass) {
    const unsigned long long items = (unsigned long long)sim.n / (uint32_t)sim.fof_chunk_len + sim.n + 1;
    if (items > 0x7fffffffull) {
        set_error("%s: %u bodies are more than one call takes", pass, sim.n);
        return 0;
    }
    return (uint32_t)items;
}

int fof_cells_enqueue(SimBase &sim, FofWork &w, double link, uint32_t rows_cap, uint32_t use_boxes) {
    const uint32_t n = sim.n;
    const double h = fof_cell_side(link);
    const uint32_t blocks = (n + kThreads - 1) / kThreads;
    const uint32_t scan_blocks = (n + kScanThreads - 1) / kScanThreads;
    const SortShape shape = sort_shape(n);
    if (int rc = fof_catalogue_reserve(w, n, rows_cap)) return rc;
    if (int rc = fof_reserve(w.slabs, (size_t)kBoundFields * blocks)) return rc;
    if (int rc = fof_reserve(w.cell_key, n)) return rc;
    if (int rc = fof_reserve(w.cell_start, (size_t)n + 1)) return rc;
    if (int rc = fof_reserve(w.boxes, (size_t)6 * n)) return rc;
    if (int rc = fof_reserve(w.spos, n)) return rc;
    if (int rc = fof_reserve(w.parent, n)) return rc;

    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    FofInfo *info = w.info;
    const auto &keys = w.sort.keys;  // both sides go to the kernels: the plan says where the sorted arrays are
    const auto &idx = w.sort.idx;
    uint32_t *scan_total = w.block_tot + scan_blocks;
    hipLaunchKernelGGL(bounds_kernel<>, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, w.slabs);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fof_plan_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, blocks, h, info);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fof_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, info, keys[0]);
    NB_HIP_TRY(hipGetLastError());
    if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, kMaxPasses, 0, &info->passes[0])) return rc;
    // the cell table
    hipLaunchKernelGGL(fof_heads_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, keys[0], keys[1], n,
                       w.flags);
    NB_HIP_TRY(hipGetLastError());
    if (int rc = enqueue_scan(sim, w, scan_blocks, scan_total)) return rc;
    hipLaunchKernelGGL(fof_cells_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, keys[0], keys[1], n,
                       w.excl, w.block_tot, w.flags, w.cell_key, w.cell_start);
    NB_HIP_TRY(hipGetLastError());
    if (use_boxes) NB_HIP_TRY(hipMemsetAsync(w.boxes, 0, sizeof(uint32_t) * 6 * n, sim.stream));
    hipLaunchKernelGGL(fof_parent_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, posm, idx[0], idx[1],
                       n, w.flags, w.cell_start, scan_total, w.spos, w.parent, w.boxes, use_boxes);
    NB_HIP_TRY(hipGetLastError());
    return NB_OK;
}

int fof_enqueue(SimBase &sim, FofWork &w, const nb_fof_params &params, uint32_t rows_cap, bool want_group_of,
                bool sums) {
    const double b2 = params.link * params.link;  // (positive and finite: fof_check_params)
    const uint32_t len = (uint32_t)sim.fof_chunk_len, use_boxes = (uint32_t)sim.fof_cell_boxes;
    const uint32_t union_items = fof_union_items(sim, "fof");
    if (!union_items) return NB_ERR_UNSUPPORTED;
    if (int rc = fof_cells_enqueue(sim, w, params.link, rows_cap, use_boxes)) return rc;
    const auto &idx = w.sort.idx;
    hipLaunchKernelGGL(fof_union_kernel, dim3(union_items), dim3(kWave), 0, sim.stream, w.info, w.cell_key,
                       w.cell_start, w.boxes, idx[0], idx[1], w.spos, w.parent, len, b2, use_boxes);
    NB_HIP_TRY(hipGetLastError());
    return fof_catalogue_enqueue(sim, w, w.parent, params.min_members, rows_cap, want_group_of, sums);
}

int fof_call(SimBase &sim, const char *pass, double link, uint32_t min_members, const FofEnqueue &enqueue,
             uint32_t *labels, uint32_t *group_of, nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats) {
    if (int rc = analysis_begin(sim, pass)) return rc;
    if (!groups) group_capacity = 0;
    if (!labels && !group_of && !groups && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n;
    const double h = fof_cell_side(link);
    // the most rows there can be, and those the caller has room for
    const uint32_t rows_cap = fof_rows_cap(n, group_capacity, min_members);
    FofWork *work = nullptr;
    if (int rc = fof_work(sim, &work)) return rc;
    FofWork &w = *work;
    FofInfo &res = *static_cast<FofInfo *>(w.h_info);
    std::memset(&res, 0, sizeof res);
    res.h = h;  // (largest = 0: count 0, label NB_FOF_NONE)

    if (n > 0) {
        if (labels)
            if (int rc = fof_reserve(w.h_labels, n)) return rc;
        if (group_of)
            if (int rc = fof_reserve(w.h_group_of, n)) return rc;
        if (rows_cap > 0)
            if (int rc = fof_reserve(w.h_rows, rows_cap)) return rc;
        if (int rc = enqueue(w, rows_cap, group_of != nullptr)) return rc;
        NB_HIP_TRY(hipMemcpyAsync(w.h_info, w.info, sizeof(FofInfo), hipMemcpyDeviceToHost, sim.stream));
        if (labels)
            NB_HIP_TRY(hipMemcpyAsync(w.h_labels, w.labels, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (group_of)
            NB_HIP_TRY(hipMemcpyAsync(w.h_group_of, w.group_of, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (rows_cap > 0)
            NB_HIP_TRY(hipMemcpyAsync(w.h_rows, w.rows, sizeof(nb_fof_group) * rows_cap, hipMemcpyDeviceToHost,
                                      sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (res.status) return fof_refused(pass, link);
    if (n > 0) {
        if (labels) std::memcpy(labels, w.h_labels, sizeof(uint32_t) * n);
        if (group_of) std::memcpy(group_of, w.h_group_of, sizeof(uint32_t) * n);
        if (res.rows > 0) std::memcpy(groups, w.h_rows, sizeof(nb_fof_group) * res.rows);
    }
    if (stats) {
        nb_fof_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - res.n_ok;
        o.components = res.components;
        o.groups = res.groups;
        o.grouped_bodies = res.grouped_bodies;
        o.largest_count = (uint32_t)(res.largest >> 32);
        o.largest_label = ~(uint32_t)res.largest;
        o.cells[0] = (uint32_t)res.nx;
        o.cells[1] = (uint32_t)res.ny;
        o.cells[2] = (uint32_t)res.nz;
        o.cell_side = h;
        *stats = o;
    }
    return NB_OK;
}

int sim_fof(SimBase &sim, const nb_fof_params &params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
            size_t group_capacity, nb_fof_stats *stats) {
    return fof_call(
        sim, "fof", params.link, params.min_members,
        [&](FofWork &w, uint32_t rows_cap, bool want_group_of) {
            return fof_enqueue(sim, w, params, rows_cap, want_group_of, true);
        },
        labels, group_of, groups, group_capacity, stats);
}

}  // namespace nb
