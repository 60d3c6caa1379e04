// nb_fof6.hip -- nb_fof6_sim: the phase-space groups of a simulator's current state, friends-of-friends in position
// and velocity (include/nbody.h "Phase-space groups"; no reference counterpart).
//
// Bodies i != j are friends iff d2 <= b2 and d2 v2 + u2 b2 <= b2 v2 in binary64; a group is a connected component
// of that graph, its label the smallest body index in it.  The graph is fixed by the state, so the partition is
// unique and everything integer here is exact, whatever order the threads ran in.
//   bounds .. cells -- nb_fof.hip's own stages on the position grid of side (link / sqrt(3)) (1 - 2^-20)
//              (fof_cells_enqueue): the sort, the cell table, the gathered positions, the cells' position boxes;
//   gather  -- the velocities in sorted order next to them, parent[i] = i (the bodies of a cell satisfy clause 1
//              without a test, but not clause 2: they are no longer one component), and the cells' velocity boxes in
//              their own buffer, by the same integer encoding and the same shortcut for a wave of one cell;
//   union   -- one wave per chunk of at most "fof_chunk_len" bodies of an occupied cell A.  Lane l < 62 looks up the
//              l-th forward neighbour, lane 62 stands for A itself, and each classes its cell pair by evaluating both
//              clauses on the boxes: apart, all friends, or to be tested.  The pairs of a pair to be tested are all
//              tested, lanes over A's bodies, every lane against every body of B (of A: every later body).  A hit
//              is united lock-free unless the lane's remembered root is the other body's root already; nothing ends
//              the loop over B early -- see union6_kernel;
//   labels .. sums -- fof_catalogue_enqueue (nb_fof.hpp), exactly as nb_sim_fof's.
// No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kSelf = kFofNeighbours;  // the lane that stands for the pair (A, A)

struct Fof6Work : Workspace {  // (both grow to the largest call so far)
    DeviceBuf<float4> svel;     // [n]: velocities in sorted order, next to FofWork::spos
    DeviceBuf<uint32_t> vboxes; // [n][6]: the cells' velocity boxes, encoded as FofWork::boxes
};

// parent, the gathered velocities and the cells' velocity boxes (cleared to 0 beforehand)
__global__ __launch_bounds__(kThreads) void fof6_gather_kernel(const FofInfo *__restrict__ info,
                                                               const float4 *__restrict__ vel,
                                                               const uint32_t *__restrict__ i0p,
                                                               const uint32_t *__restrict__ i1p, uint32_t n,
                                                               const uint32_t *__restrict__ cell_of_pos,
                                                               float4 *__restrict__ svel, uint32_t *__restrict__ parent,
                                                               uint32_t *__restrict__ vboxes, uint32_t use_boxes) {
    if (info->status) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t *idx = info->passes[0] & 1 ? i1p : i0p;
    const uint32_t body = idx[p];
    if (p >= info->n_ok) {
        parent[body] = NB_FOF_NONE;
        return;
    }
    parent[body] = body;
    const float4 v = vel[body];
    svel[p] = v;
    if (!use_boxes) return;
    uint32_t e[6] = {~ordered(v.x), ~ordered(v.y), ~ordered(v.z), ordered(v.x), ordered(v.y), ordered(v.z)};
    box_raise(vboxes, cell_of_pos[p], e);
}

// the squared length of a difference, in the rule's own operations
__device__ inline double sq3(double x, double y, double z) {
#pragma clang fp contract(off)
    return (x * x + y * y) + z * z;
}
// the two clauses of include/nbody.h on d2 and u2
__device__ inline bool clauses(double d2, double u2, double b2, double v2, double rhs) {
#pragma clang fp contract(off)
    return d2 <= b2 && (d2 * v2 + u2 * b2) <= rhs;
}
__device__ inline bool friends6(float4 p, float4 pv, float4 q, float4 qv, double b2, double v2, double rhs) {
#pragma clang fp contract(off)
    const double d2 = sq3((double)p.x - (double)q.x, (double)p.y - (double)q.y, (double)p.z - (double)q.z);
    const double u2 = sq3((double)pv.x - (double)qv.x, (double)pv.y - (double)qv.y, (double)pv.z - (double)qv.z);
    return clauses(d2, u2, b2, v2, rhs);
}

// One wave per chunk [a0, a1) of the sorted positions of cell c.
//
// Classes.  Every |difference| of a pair (i in A, j in B) lies, per axis, between the gap of the two boxes and their
// farthest extent; the differences are exact differences of binary32 numbers rounded once to binary64, rounding is
// monotone, and d2, u2 and d2 v2 + u2 b2 are sums of products of non-negative numbers, non-decreasing in every
// |difference| under monotone rounding.  So the rule's expressions on the gaps bound every pair's from below and on
// the farthest extents from above: a clause that fails on the gaps fails for every pair (apart), both clauses on the
// farthest extents hold for every pair (all friends).  For (A, A) the gaps are 0: never apart.
//
// All friends.  Every body of A is a friend of every body of B, so the bodies of both are one component: every chunk
// unites its own bodies with B's first body, and the cell's first chunk unites B's bodies with A's first.  For
// (A, A) every chunk unites its bodies with A's first.
//
// To be tested.  Every pair is tested once: (i, j) with j in a forward neighbour by i's chunk, and with j in A by the
// chunk of the body that comes first in sorted order.  Termination: the loop over B runs to B's end for every lane.
// A hit between A and B says nothing about A's other bodies (a cell is no longer one component) and nothing about B's
// other bodies either, so no hit ends the loop, for the wave or for a lane.  What a hit may skip is only its own
// union: lane i remembers a body `root` that was the root of i's tree at some moment (i itself at first), so i is in
// root's component for good; when j's root, read at the hit, is that body, i and j are in one component already.
// A stale `root` only costs a union that finds nothing to do.
__global__ __launch_bounds__(kWave) void fof6_union_kernel(const FofInfo *__restrict__ info,
                                                           const unsigned long long *__restrict__ cell_key,
                                                           const uint32_t *__restrict__ cell_start,
                                                           const uint32_t *__restrict__ boxes,
                                                           const uint32_t *__restrict__ vboxes,
                                                           const uint32_t *__restrict__ i0p,
                                                           const uint32_t *__restrict__ i1p,
                                                           const float4 *__restrict__ spos,
                                                           const float4 *__restrict__ svel, uint32_t *parent,
                                                           uint32_t len, double b2, double v2, double rhs,
                                                           uint32_t use_boxes) {
#pragma clang fp contract(off)
    if (info->status) return;
    const uint32_t ncells = info->ncells, lane = threadIdx.x;
    uint32_t c, s, a0, a1;
    if (!item_chunk(cell_start, ncells, len, blockIdx.x, &c, &s, &a0, &a1)) return;  // (uniform over the wave)
    const uint32_t *idx = info->passes[0] & 1 ? i1p : i0p;
    const uint32_t rep_a = idx[cell_start[c]];

    // lane l: its cell pair, the partner's place in the cell table and the pair's class by the boxes
    uint32_t nb = c, cls = 0;  // 0 none or apart, 1 test the pairs, 2 all friends
    if (lane == kSelf || (lane < kFofNeighbours && forward_neighbour(info, cell_key, ncells, c, lane, &nb))) {
        cls = 1;
        if (use_boxes) {
            double gap[3], far[3], vgap[3], vfar[3];
            box_gap_far(boxes, c, nb, gap, far);
            box_gap_far(vboxes, c, nb, vgap, vfar);
            if (!clauses(sq3(gap[0], gap[1], gap[2]), sq3(vgap[0], vgap[1], vgap[2]), b2, v2, rhs)) cls = 0;
            else if (clauses(sq3(far[0], far[1], far[2]), sq3(vfar[0], vfar[1], vfar[2]), b2, v2, rhs)) cls = 2;
        }
    }
    unsigned long long direct = __ballot(cls == 2), test = __ballot(cls == 1);
    while (direct) {
        const int l = __ffsll((long long)direct) - 1;
        direct &= direct - 1;
        const uint32_t b = __shfl(nb, l);
        const uint32_t b0 = cell_start[b], b1 = cell_start[b + 1];
        const uint32_t rep_b = idx[b0];
        for (uint32_t a = a0 + lane; a < a1; a += kWave) unite(parent, idx[a], rep_b);
        if (s == 0 && b != c)
            for (uint32_t j = b0 + lane; j < b1; j += kWave) unite(parent, idx[j], rep_a);
    }
    while (test) {
        const int l = __ffsll((long long)test) - 1;
        test &= test - 1;
        const uint32_t b = __shfl(nb, l);
        const bool self = b == c;
        const uint32_t b1 = cell_start[b + 1];
        for (uint32_t a = a0; a < a1; a += kWave) {
            const bool valid = a + lane < a1;
            const uint32_t pi = valid ? a + lane : a;
            const float4 pa = spos[pi], va = svel[pi];
            const uint32_t body = idx[pi];
            uint32_t root = body;
            for (uint32_t j = self ? a + 1 : cell_start[b]; j < b1; ++j) {  // (uniform over the wave)
                const float4 pb = spos[j], vb = svel[j];
                if (valid && (!self || j > pi) && friends6(pa, va, pb, vb, b2, v2, rhs)) {
                    const uint32_t other = idx[j];
                    if (find_root(parent, other) != root) {
                        unite(parent, body, other);
                        root = find_root_halving(parent, body);
                    }
                }
            }
        }
    }
}

template <class B>
int fof6_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("fof6: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int sim_fof6(SimBase &sim, const nb_fof6_params &params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
             size_t group_capacity, nb_fof_stats *stats) {
    return fof_call(
        sim, "fof6", params.link, params.min_members,
        [&](FofWork &w, uint32_t rows_cap, bool want_group_of) -> int {
            const uint32_t n = sim.n;
            // (positive and finite: fof6_check_params)
            const double b2 = params.link * params.link, v2 = params.vlink * params.vlink, rhs = b2 * v2;
            const uint32_t len = (uint32_t)sim.fof_chunk_len, use_boxes = (uint32_t)sim.fof6_boxes;
            const uint32_t blocks = (n + kThreads - 1) / kThreads;
            const uint32_t union_items = fof_union_items(sim, "fof6");
            if (!union_items) return (int)NB_ERR_UNSUPPORTED;
            Fof6Work *work = nullptr;
            if (int rc = workspace(sim, kWorkFof6, &work, [](Fof6Work &) { return NB_OK; })) return rc;
            if (int rc = fof6_reserve(work->svel, n)) return rc;
            if (int rc = fof6_reserve(work->vboxes, (size_t)6 * n)) return rc;
            if (int rc = fof_cells_enqueue(sim, w, params.link, rows_cap, use_boxes)) return rc;

            const float4 *posm = nullptr, *vel = nullptr;
            sim.diag_state(&posm, &vel);
            const auto &idx = w.sort.idx;
            if (use_boxes) NB_HIP_TRY(hipMemsetAsync(work->vboxes, 0, sizeof(uint32_t) * 6 * n, sim.stream));
            hipLaunchKernelGGL(fof6_gather_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, w.info, vel, idx[0],
                               idx[1], n, w.flags, work->svel, w.parent, work->vboxes, use_boxes);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(fof6_union_kernel, dim3(union_items), dim3(kWave), 0, sim.stream, w.info, w.cell_key,
                               w.cell_start, w.boxes, work->vboxes, idx[0], idx[1], w.spos, work->svel, w.parent, len,
                               b2, v2, rhs, use_boxes);
            NB_HIP_TRY(hipGetLastError());
            return fof_catalogue_enqueue(sim, w, w.parent, params.min_members, rows_cap, want_group_of, true);
        },
        labels, group_of, groups, group_capacity, stats);
}

}  // namespace nb
