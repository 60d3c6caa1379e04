// nb_mst.hip -- nb_mst_sim: the Euclidean minimum spanning tree of the counted bodies of a simulator's current
// state, its edges in ascending order and every body's degree (include/nbody.h "Minimum spanning tree", DESIGN.md
// 6y; no reference counterpart).
//
// Pairs of counted bodies are ordered by (d2, min index, max index), d2 the dist2 of nb_knn.hpp.  The order is
// strict and total, so the tree is unique and Boruvka's rounds are deterministic, whatever order the threads ran in.
//   front end -- knn_enqueue_sorted (nb_knn.hip): bounds, plan, 63-bit Morton key, the shared sort, spos and the
//                sorted body indices.  Every counted body starts as its own component, labelled by its index;
//   search    -- one wave per sorted position, "mst_block_queries" waves a block: the counted body of another
//                component that comes first in (d2, j) -- for a fixed body i the edge order is the order of j.
//                (1) seed: the 64 positions around the body's own, which gives a finite bound where the Morton
//                    neighbours are not all of the body's own component;
//                (2) the body's own finest cell, 64 positions a time in index order; it stops once the best is
//                    (0, j) with j no larger than the last index seen (a pile of coincident bodies costs one batch),
//                    and a best d2 of 0 after it ends the search: bodies of other cells are elsewhere;
//                (3) with a finite bound, nb_knn.hpp's range of finest cells and the octree level at which it is at
//                    most "mst_span_cells" cells an axis, those cells in ascending order of their lower bound; with
//                    none, the root cell.  A cell is walked depth first on a stack in LDS: a cell whose bound
//                    exceeds the best d2 strictly is dropped (an equal bound is visited: a smaller index wins a
//                    tie), a short or finest cell is scanned, any other is split into its eight children, their
//                    runs found by binary search inside the parent's run, pushed nearest last.
//                Pruning (a), "mst_skip_runs": next[p] is the next sorted position whose label differs from p's, so
//                a run, a stretch of a run or a whole cell of the body's own component is stepped over in O(1).
//                Pruning (b), "mst_shared_bound": best_d2[component] is the smallest d2 any of its bodies has found
//                this round, an integer minimum on ordered64; a body takes it as its bound, without an index, so
//                only strictly greater values are pruned;
//   pick      -- per component the least (d2, lo, hi) by integer atomics alone: the minimum of ordered64(d2) is
//                complete after the search; the bodies that hold it take the minimum of lo << 32 | hi;
//   emit      -- every component's edge, once: of two components that chose the same edge the one with the smaller
//                label emits it, at a position from an atomic counter; the edge's ends are united in nb_fof.hpp's
//                forest (the larger root under the smaller);
//   relabel   -- label = root = the smallest index; labels and the next-different-label array in sorted order (a
//                block's first change of label, a suffix minimum over the blocks, a suffix minimum inside each);
//                the components counted;
//   rounds    -- ceil(log2 max(n, 2)) of them are enqueued up front, as a round at least halves the components and
//                c exists only on the device; the blocks of a round that finds one component left return at once;
//   sort      -- the emitted edges by the shared stable sort on lo << 32 | hi and then on ordered64(d2): all keys
//                are distinct, so the list is canonical; the degrees by integer atomics.
// No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_knn.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kPasses = kKnnPasses;
constexpr unsigned long long kNoKey = ~0ull;               // past ordered64 of every double, and every lo << 32 | hi
constexpr uint32_t kNoFlag = 0xffffffffu;
constexpr uint32_t kLeaf = 2 * kWave;                      // a cell of at most this many positions is scanned, not split
constexpr uint32_t kStack = 7 * kKnnAxisBits + 9;          // a split takes one cell and pushes at most eight
constexpr uint32_t kSuffixThreads = 1024;

// The integer results of a call, on the device.  Zeroed before the rounds; written by integer atomics or single threads.
struct MstInfo {
    uint32_t edges, reserved;
    uint32_t comps_after[NB_MST_MAX_ROUNDS];
    double d2_min, d2_max;
};

struct MstWork : Workspace {  // (all grow to the largest call so far)
    DeviceBuf<uint32_t> label, parent;         // [n] by body: the component's smallest index; the forest
    DeviceBuf<uint32_t> slab, next;            // [n] by sorted position: the label; the next position of another label
    DeviceBuf<uint32_t> first_flag;            // [blocks]: a block's first change of label, then the suffix minimum
    DeviceBuf<unsigned long long> best_d2, best_pair;  // [n] by label: ordered64(d2), lo << 32 | hi of the round
    DeviceBuf<double> cand_d2;                 // [n] by sorted position: what the search found
    DeviceBuf<uint32_t> cand_j;
    DeviceBuf<uint32_t> raw_lo, raw_hi, perm;  // [n]: the edges as emitted; the first sort's order
    DeviceBuf<unsigned long long> raw_key;     // [n]: ordered64(d2) of the edges as emitted
    DeviceBuf<uint32_t> edge_lo, edge_hi, degree;  // [n]: the outputs
    DeviceBuf<double> d2;
    PinnedBuf<uint32_t> h_edge_lo, h_edge_hi, h_degree;  // staged, so that a failed call leaves the outputs alone
    PinnedBuf<double> h_d2;
    DeviceBuf<MstInfo> info;
    PinnedBuf<MstInfo> h_info;
    PinnedBuf<KnnInfo> h_plan;
};

__device__ inline double unordered64(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & ~(1ull << 63)) : ~e;
    return __longlong_as_double((long long)u);
}

// the components a round starts from
__device__ inline uint32_t comps_before(const KnnInfo *__restrict__ plan, const MstInfo *__restrict__ mi,
                                        uint32_t round) {
    return round ? mi->comps_after[round - 1] : plan->n_ok;
}

// ---- start ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mst_start_kernel(const float4 *__restrict__ posm,
                                                             const float4 *__restrict__ vel, uint32_t n,
                                                             const KnnInfo *__restrict__ plan,
                                                             const uint32_t *__restrict__ sidx,
                                                             uint32_t *__restrict__ label, uint32_t *__restrict__ parent,
                                                             uint32_t *__restrict__ slab, uint32_t *__restrict__ next,
                                                             unsigned long long *__restrict__ best_d2,
                                                             unsigned long long *__restrict__ best_pair,
                                                             uint32_t *__restrict__ degree) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const bool ok = body_ok(posm[i], vel[i]);
    label[i] = parent[i] = ok ? (uint32_t)i : NB_MST_NONE;
    degree[i] = ok ? 0u : NB_MST_NONE;
    best_d2[i] = best_pair[i] = kNoKey;
    if (i < plan->n_ok) {  // every label differs from the next
        slab[i] = sidx[i];
        next[i] = (uint32_t)i + 1;
    }
}

// ---- search -----------------------------------------------------------------------------------------
// The edge weight: one function, so that a later change can weight the pairs otherwise.
__device__ inline double edge_weight(float4 p, float4 q) { return dist2(p, q); }

struct Cell {  // an octree cell of 2^s finest cells an axis at (cx, cy, cz), its run [b0, b1), its lower bound of d2
    double bound;
    uint32_t cx, cy, cz, s, b0, b1;
};

// A wave's query: the best (d2, j) so far, the same on every lane; bj == NB_MST_NONE: bd is a bound alone.
struct Search {
    float4 p;
    double bd;
    uint32_t bj, label, lane;
    uint32_t cs, ce;  // positions already scanned as the body's own finest cell
    bool skip, shared;
    const float4 *spos;
    const uint32_t *sidx, *slab, *next;
    unsigned long long *best_d2;
};

// the valid lanes' (d, j) against the best
__device__ inline void offer(Search &q, bool valid, double d, uint32_t j) {
    const double dm = wave_min(valid ? d : (double)INFINITY);
    if (!(dm <= q.bd)) return;
    uint32_t jm = valid && d == dm ? j : NB_MST_NONE;
    for (int o = 32; o > 0; o >>= 1) jm = std::min(jm, (uint32_t)__shfl_xor(jm, o));
    if (!before(dm, jm, q.bd, q.bj)) return;
    q.bd = dm;
    q.bj = jm;
    if (q.shared && q.lane == 0) atomicMin(q.best_d2 + q.label, ordered64(dm));
}

// a component's bound, where it is below the body's own: an index no longer goes with it
__device__ inline void take_shared(Search &q) {
    if (!q.shared) return;
    const unsigned long long sb = __atomic_load_n(q.best_d2 + q.label, __ATOMIC_RELAXED);
    if (sb < ordered64(q.bd)) {
        q.bd = unordered64(sb);
        q.bj = NB_MST_NONE;
    }
}

// The bodies of other components at sorted positions [b0, b1) against the best, 64 a time.  zero_stop: the run is
// one finest cell, its bodies in index order.  All arguments are the same on every lane.
__device__ inline void scan(Search &q, uint32_t b0, uint32_t b1, bool zero_stop) {
    uint32_t a = b0;
    while (a < b1) {
        if (a >= q.cs && a < q.ce) {
            a = q.ce;
            continue;
        }
        if (q.skip && q.slab[a] == q.label) {  // pruning (a)
            a = q.next[a];
            continue;
        }
        const uint32_t pos = a + q.lane;
        bool valid = pos < b1 && !(pos >= q.cs && pos < q.ce);
        valid = valid && q.slab[pos] != q.label;
        double d = 0.0;
        uint32_t j = 0;
        if (valid) {
            d = edge_weight(q.p, q.spos[pos]);
            j = q.sidx[pos];
        }
        offer(q, valid, d, j);
        a = (uint32_t)std::min<unsigned long long>(b1, (unsigned long long)a + kWave);
        // every unseen body of the run has a larger index than the last seen, and d2 >= 0
        if (zero_stop && q.bd == 0.0 && q.bj != NB_MST_NONE && q.bj <= q.sidx[a - 1]) break;
    }
}

// the gap on an axis between x and the cell cc of 2^s finest cells: its bodies have edge(first) <= x_j, and
// x_j < edge(last + 1) or, in the last cell of the axis, x_j <= hi
__device__ inline double axis_gap(double lo, double hi, double h, double x, uint32_t cc, uint32_t s) {
#pragma clang fp contract(off)
    const uint32_t first = cc << s, last = ((cc + 1) << s) - 1;
    const double elo = edge(lo, h, first);
    const double ehi = last >= kKnnAxisMax ? hi : edge(lo, h, last + 1);
    return fmax(0.0, fmax(elo - x, x - ehi));
}
__device__ inline double cell_bound(const KnnInfo *__restrict__ plan, double h, float4 p, uint32_t cx, uint32_t cy,
                                    uint32_t cz, uint32_t s) {
#pragma clang fp contract(off)
    const double gx = axis_gap(plan->lo[0], plan->hi[0], h, (double)p.x, cx, s);
    const double gy = axis_gap(plan->lo[1], plan->hi[1], h, (double)p.y, cy, s);
    const double gz = axis_gap(plan->lo[2], plan->hi[2], h, (double)p.z, cz, s);
    return (gx * gx + gy * gy) + gz * gz;
}

// is [b0, b1) (b0 < b1) wholly of the body's own component?
__device__ inline bool own_run(const Search &q, uint32_t b0, uint32_t b1) {
    return q.skip && q.slab[b0] == q.label && q.next[b0] >= b1;
}

// The cell `root` and everything below it, depth first, nearest child first.
__device__ inline void visit(Search &q, Cell *stack, const KnnInfo *__restrict__ plan, double h,
                             const unsigned long long *__restrict__ keys, Cell root) {
    uint32_t top = 1;
    if (q.lane == 0) stack[0] = root;
    while (top) {
        __builtin_amdgcn_wave_barrier();
        const Cell e = stack[--top];
        __builtin_amdgcn_wave_barrier();
        take_shared(q);
        if (e.bound > q.bd) continue;  // strictly: an equal bound is visited
        if (own_run(q, e.b0, e.b1)) continue;
        if (e.s == 0 || e.b1 - e.b0 <= kLeaf || top + 8 > kStack) {
            scan(q, e.b0, e.b1, false);
            continue;
        }
        // lane o < 8 (the others repeat them): child o, its run inside the parent's, its bound
        const uint32_t o = q.lane & 7u, s = e.s - 1;
        const uint32_t cx = 2 * e.cx + (o & 1u), cy = 2 * e.cy + ((o >> 1) & 1u), cz = 2 * e.cz + (o >> 2);
        const unsigned long long prefix = morton(cx, cy, cz);
        const unsigned long long klo = prefix << (3 * s), khi = (prefix + 1) << (3 * s);  // <= 2^63
        const uint32_t c0 = first_at_least(keys, e.b0, e.b1, klo), c1 = first_at_least(keys, c0, e.b1, khi);
        const double bound = cell_bound(plan, h, q.p, cx, cy, cz, s);
        const bool valid = q.lane < 8 && c1 > c0 && bound <= q.bd && !own_run(q, c0, c1);
        const uint32_t m = (uint32_t)(__ballot(valid) & 0xffull), count = (uint32_t)__popc(m);
        uint32_t rank = 0;  // the valid children before this one in (bound, o)
        for (uint32_t l = 0; l < 8; ++l) {
            const double bl = __shfl(bound, (int)l);
            rank += ((m >> l) & 1u) && (bl < bound || (bl == bound && l < q.lane)) ? 1u : 0u;
        }
        if (valid) stack[top + (count - 1 - rank)] = Cell{bound, cx, cy, cz, s, c0, c1};
        top += count;
    }
}

__global__ __launch_bounds__(kThreads) void mst_search_kernel(
    const KnnInfo *__restrict__ plan, const MstInfo *__restrict__ mi, uint32_t round,
    const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ sidx, const float4 *__restrict__ spos,
    const uint32_t *__restrict__ slab, const uint32_t *__restrict__ next, unsigned long long *__restrict__ best_d2,
    double *__restrict__ cand_d2, uint32_t *__restrict__ cand_j, uint32_t span, uint32_t skip, uint32_t shared) {
#pragma clang fp contract(off)
    __shared__ Cell stacks[kThreads / kWave][kStack];
    const uint32_t c = plan->n_ok;
    if (comps_before(plan, mi, round) <= 1) return;
    const size_t pl = (size_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (pl >= c) return;  // (uniform over the wave)
    const uint32_t p = (uint32_t)pl;
    Cell *stack = stacks[threadIdx.x / kWave];

    Search q;
    q.p = spos[p];
    q.bd = INFINITY;
    q.bj = NB_MST_NONE;
    q.label = slab[p];
    q.lane = threadIdx.x % kWave;
    q.cs = q.ce = 0;
    q.skip = skip != 0;
    q.shared = shared != 0;
    q.spos = spos;
    q.sidx = sidx;
    q.slab = slab;
    q.next = next;
    q.best_d2 = best_d2;
    take_shared(q);  // pruning (b): there is no seed guarantee, the bound starts at +inf or here

    // (1) the seed
    {
        const uint32_t w0 = p > kWave / 2 ? p - kWave / 2 : 0u;
        const uint32_t w1 = (uint32_t)std::min<size_t>(c, (size_t)w0 + kWave), pos = w0 + q.lane;
        const bool valid = pos < w1 && slab[pos] != q.label;
        double d = 0.0;
        uint32_t j = 0;
        if (valid) {
            d = edge_weight(q.p, spos[pos]);
            j = sidx[pos];
        }
        offer(q, valid, d, j);
    }
    // (2) the own finest cell, in index order, with the zero stop
    const unsigned long long key = keys[p];
    const uint32_t cs = first_at_least(keys, 0u, p, key), ce = first_at_least(keys, p + 1, c, key + 1);
    scan(q, cs, ce, true);
    q.cs = cs;
    q.ce = ce;
    const double h = plan->h;
    // bodies of other cells are elsewhere: d2 > 0; h = 0: there are none
    if (q.bd != 0.0 && h > 0.0) {
        if (!(q.bd < (double)INFINITY)) {
            visit(q, stack, plan, h, keys, Cell{0.0, 0u, 0u, 0u, kKnnAxisBits, 0u, c});
        } else {
            // (3) finest cells [tlo, thi] per axis: a body of a cell below tlo or above thi has d2 > bd
            const double x[3] = {q.p.x, q.p.y, q.p.z};
            const double rad = sqrt(q.bd);
            uint32_t tlo[3], thi[3];
            for (int a = 0; a < 3; ++a) {
                const double lo = plan->lo[a];
                uint32_t t0 = clamp_cell(floor(((x[a] - rad) - lo) / h) - 1.0);
                uint32_t t1 = clamp_cell(floor(((x[a] + rad) - lo) / h) + 1.0);
                while (t0 > 0) {  // bodies of cells below t0 have x_j < edge(t0)
                    const double e = edge(lo, h, t0), g = x[a] - e;
                    if (x[a] >= e && g * g > q.bd) break;
                    --t0;
                }
                while (t1 < kKnnAxisMax) {  // bodies of cells above t1 have x_j >= edge(t1 + 1)
                    const double e = edge(lo, h, t1 + 1), g = e - x[a];
                    if (e >= x[a] && g * g > q.bd) break;
                    ++t1;
                }
                tlo[a] = t0;
                thi[a] = t1;
            }
            uint32_t s = 0;  // the level: cells of 2^s finest cells an axis
            while (s < kKnnAxisBits &&
                   ((thi[0] >> s) - (tlo[0] >> s) >= span || (thi[1] >> s) - (tlo[1] >> s) >= span ||
                    (thi[2] >> s) - (tlo[2] >> s) >= span))
                ++s;
            const uint32_t c0[3] = {tlo[0] >> s, tlo[1] >> s, tlo[2] >> s};
            const uint32_t nx = (thi[0] >> s) - c0[0] + 1, ny = (thi[1] >> s) - c0[1] + 1,
                           nz = (thi[2] >> s) - c0[2] + 1;
            const uint32_t total = nx * ny * nz;  // at most span^3 <= 512
            for (uint32_t base = 0; base < total; base += kWave) {
                const uint32_t t = base + q.lane;
                bool pending = t < total;
                double bound = INFINITY;
                uint32_t b0 = 0, b1 = 0;
                if (pending) {
                    const uint32_t cx = c0[0] + t % nx, cy = c0[1] + (t / nx) % ny, cz = c0[2] + t / (nx * ny);
                    bound = cell_bound(plan, h, q.p, cx, cy, cz, s);
                    pending = bound <= q.bd;
                    if (pending) {
                        const unsigned long long prefix = morton(cx, cy, cz);
                        const unsigned long long klo = prefix << (3 * s), khi = (prefix + 1) << (3 * s);  // <= 2^63
                        b0 = first_at_least(keys, 0u, c, klo);
                        b1 = first_at_least(keys, b0, c, khi);
                        pending = b1 > b0;
                    }
                }
                for (;;) {  // ascending bound; an equal bound is visited: a smaller index wins a tie
                    if (__ballot(pending) == 0ull) break;
                    const double b = pending ? bound : (double)INFINITY;
                    const double least = wave_min(b);
                    if (!(least <= q.bd)) break;
                    const int l = __ffsll((long long)__ballot(pending && b == least)) - 1;
                    const uint32_t tl = base + (uint32_t)l;
                    visit(q, stack, plan, h, keys,
                          Cell{least, c0[0] + tl % nx, c0[1] + (tl / nx) % ny, c0[2] + tl / (nx * ny), s,
                               (uint32_t)__shfl(b0, l), (uint32_t)__shfl(b1, l)});
                    if ((int)q.lane == l) pending = false;
                }
            }
        }
    }
    if (q.lane == 0) {
        const bool found = q.bj != NB_MST_NONE;
        cand_d2[p] = found ? q.bd : (double)INFINITY;
        cand_j[p] = q.bj;
        if (found) atomicMin(best_d2 + q.label, ordered64(q.bd));
    }
}

// ---- pick, emit ---------------------------------------------------------------------------------------
// among the bodies that hold their component's least d2, the least lo << 32 | hi
__global__ __launch_bounds__(kThreads) void mst_pick_kernel(const KnnInfo *__restrict__ plan,
                                                            const MstInfo *__restrict__ mi, uint32_t round,
                                                            const uint32_t *__restrict__ sidx,
                                                            const uint32_t *__restrict__ slab,
                                                            const unsigned long long *__restrict__ best_d2,
                                                            const double *__restrict__ cand_d2,
                                                            const uint32_t *__restrict__ cand_j,
                                                            unsigned long long *__restrict__ best_pair) {
    if (comps_before(plan, mi, round) <= 1) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= plan->n_ok) return;
    const uint32_t j = cand_j[p];
    if (j == NB_MST_NONE) return;
    const uint32_t l = slab[p], i = sidx[p];
    if (ordered64(cand_d2[p]) != best_d2[l]) return;
    atomicMin(best_pair + l, (unsigned long long)std::min(i, j) << 32 | std::max(i, j));
}

// every component's edge, once, and its ends united
__global__ __launch_bounds__(kThreads) void mst_emit_kernel(const KnnInfo *__restrict__ plan, MstInfo *__restrict__ mi,
                                                            uint32_t round, uint32_t n,
                                                            const uint32_t *__restrict__ label,
                                                            const unsigned long long *__restrict__ best_d2,
                                                            const unsigned long long *__restrict__ best_pair,
                                                            uint32_t *__restrict__ parent, uint32_t *__restrict__ raw_lo,
                                                            uint32_t *__restrict__ raw_hi,
                                                            unsigned long long *__restrict__ raw_key) {
    if (comps_before(plan, mi, round) <= 1) return;
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n || label[r] != (uint32_t)r) return;  // (a body that is not counted has no label)
    const unsigned long long pair = best_pair[r];
    if (pair == kNoKey) return;
    const uint32_t lo = (uint32_t)(pair >> 32), hi = (uint32_t)pair;
    const uint32_t other = label[lo] == (uint32_t)r ? label[hi] : label[lo];
    const bool mutual = best_pair[other] == pair && best_d2[other] == best_d2[r];
    if (!(mutual && other < (uint32_t)r)) {
        const uint32_t slot = atomicAdd(&mi->edges, 1u);
        if (slot < n) {  // (a forest on c bodies has fewer than c edges)
            raw_lo[slot] = lo;
            raw_hi[slot] = hi;
            raw_key[slot] = best_d2[r];
        }
    }
    unite(parent, lo, hi);
}

// ---- relabel ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mst_flatten_kernel(const KnnInfo *__restrict__ plan,
                                                               const MstInfo *__restrict__ mi, uint32_t round,
                                                               uint32_t n, const uint32_t *__restrict__ parent,
                                                               uint32_t *__restrict__ label) {
    if (comps_before(plan, mi, round) <= 1) return;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || label[i] == NB_MST_NONE) return;
    label[i] = find_root(parent, (uint32_t)i);
}

// labels in sorted order, the forest flat, the round's minima reset, the components counted, and the block's first
// position whose label differs from the position before
__global__ __launch_bounds__(kThreads) void mst_relabel_kernel(const KnnInfo *__restrict__ plan,
                                                               MstInfo *__restrict__ mi, uint32_t round,
                                                               const uint32_t *__restrict__ sidx,
                                                               const uint32_t *__restrict__ label,
                                                               uint32_t *__restrict__ parent, uint32_t *__restrict__ slab,
                                                               unsigned long long *__restrict__ best_d2,
                                                               unsigned long long *__restrict__ best_pair,
                                                               uint32_t *__restrict__ first_flag) {
    if (comps_before(plan, mi, round) <= 1) return;
    __shared__ uint32_t first;
    if (threadIdx.x == 0) first = kNoFlag;
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p < plan->n_ok) {
        const uint32_t i = sidx[p], l = label[i];
        slab[p] = l;
        parent[i] = l;
        best_d2[i] = best_pair[i] = kNoKey;
        if (l == i) atomicAdd(&mi->comps_after[round], 1u);
        if (p == 0 || label[sidx[p - 1]] != l) atomicMin(&first, (uint32_t)p);
    }
    __syncthreads();
    if (threadIdx.x == 0) first_flag[blockIdx.x] = first;
}

// first_flag[b] = the least first_flag of the blocks after b, by one block
__global__ __launch_bounds__(kSuffixThreads) void mst_suffix_kernel(const KnnInfo *__restrict__ plan,
                                                                    const MstInfo *__restrict__ mi, uint32_t round,
                                                                    uint32_t *__restrict__ first_flag,
                                                                    uint32_t blocks) {
    if (comps_before(plan, mi, round) <= 1) return;
    __shared__ uint32_t sh[2][kSuffixThreads];
    const uint32_t t = threadIdx.x, per = (blocks + kSuffixThreads - 1) / kSuffixThreads;
    const size_t lo = std::min<size_t>(blocks, (size_t)t * per), hi = std::min<size_t>(blocks, lo + per);
    uint32_t m = kNoFlag;
    for (size_t b = lo; b < hi; ++b) m = std::min(m, first_flag[b]);
    uint32_t *a = sh[0], *b = sh[1];
    a[t] = m;
    __syncthreads();
    for (uint32_t o = 1; o < kSuffixThreads; o <<= 1) {  // inclusive, from the end
        b[t] = t + o < kSuffixThreads ? std::min(a[t], a[t + o]) : a[t];
        __syncthreads();
        uint32_t *s = a;
        a = b;
        b = s;
    }
    uint32_t run = t + 1 < kSuffixThreads ? a[t + 1] : kNoFlag;
    for (size_t k = hi; k > lo; --k) {
        const uint32_t f = first_flag[k - 1];
        first_flag[k - 1] = run;
        run = std::min(run, f);
    }
}

// next[p] = the first position after p whose label differs from p's, or c
__global__ __launch_bounds__(kThreads) void mst_next_kernel(const KnnInfo *__restrict__ plan,
                                                            const MstInfo *__restrict__ mi, uint32_t round,
                                                            const uint32_t *__restrict__ slab,
                                                            const uint32_t *__restrict__ first_flag,
                                                            uint32_t *__restrict__ next) {
    if (comps_before(plan, mi, round) <= 1) return;
    __shared__ uint32_t sh[2][kThreads];
    const uint32_t t = threadIdx.x, c = plan->n_ok;
    const size_t p = (size_t)blockIdx.x * kThreads + t;
    const bool flag = p < c && (p == 0 || slab[p] != slab[p - 1]);
    uint32_t *a = sh[0], *b = sh[1];
    a[t] = flag ? (uint32_t)p : kNoFlag;
    __syncthreads();
    for (uint32_t o = 1; o < kThreads; o <<= 1) {  // inclusive, from the end
        b[t] = t + o < kThreads ? std::min(a[t], a[t + o]) : a[t];
        __syncthreads();
        uint32_t *s = a;
        a = b;
        b = s;
    }
    const uint32_t inside = t + 1 < kThreads ? a[t + 1] : kNoFlag;
    if (p < c) next[p] = std::min(c, std::min(inside, first_flag[blockIdx.x]));
}

// ---- the edges in order ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mst_pair_key_kernel(uint32_t n, const MstInfo *__restrict__ mi,
                                                                const uint32_t *__restrict__ raw_lo,
                                                                const uint32_t *__restrict__ raw_hi,
                                                                unsigned long long *__restrict__ keys) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    keys[t] = t < mi->edges ? (unsigned long long)raw_lo[t] << 32 | raw_hi[t] : kNoKey;
}
__global__ __launch_bounds__(kThreads) void mst_d2_key_kernel(uint32_t n, const MstInfo *__restrict__ mi,
                                                              const uint32_t *__restrict__ order,
                                                              const unsigned long long *__restrict__ raw_key,
                                                              uint32_t *__restrict__ perm,
                                                              unsigned long long *__restrict__ keys) {
    const size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const uint32_t t = order[q];
    perm[q] = t;
    keys[q] = t < mi->edges ? raw_key[t] : kNoKey;
}
__global__ __launch_bounds__(kThreads) void mst_output_kernel(uint32_t n, MstInfo *__restrict__ mi,
                                                              const uint32_t *__restrict__ order,
                                                              const uint32_t *__restrict__ perm,
                                                              const uint32_t *__restrict__ raw_lo,
                                                              const uint32_t *__restrict__ raw_hi,
                                                              const unsigned long long *__restrict__ raw_key,
                                                              uint32_t *__restrict__ edge_lo,
                                                              uint32_t *__restrict__ edge_hi, double *__restrict__ d2,
                                                              uint32_t *__restrict__ degree) {
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t m = std::min(mi->edges, n);
    if (r >= m) return;
    const uint32_t t = perm[order[r]];
    const uint32_t lo = raw_lo[t], hi = raw_hi[t];
    const double d = unordered64(raw_key[t]);
    edge_lo[r] = lo;
    edge_hi[r] = hi;
    d2[r] = d;
    atomicAdd(degree + lo, 1u);
    atomicAdd(degree + hi, 1u);
    if (r == 0) mi->d2_min = d;
    if (r + 1 == m) mi->d2_max = d;
}

template <class B>
int mst_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("mst: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

// the rounds enqueued: ceil(log2 max(n, 2)), as a round at least halves the components
uint32_t mst_rounds(uint32_t n) {
    uint32_t r = 1;
    while (r < NB_MST_MAX_ROUNDS && (1ull << r) < n) ++r;
    return r;
}

}  // namespace

int sim_mst(SimBase &sim, const nb_mst_params &, uint32_t *edge_lo, uint32_t *edge_hi, double *d2, uint32_t *degree,
            nb_mst_stats *stats) {
    if (int rc = analysis_begin(sim, "mst")) return rc;
    if (!edge_lo && !edge_hi && !d2 && !degree && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n;
    if (n > 0x7fffffffu) {
        set_error("mst: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    KnnWork *kwork = nullptr;
    if (int rc = knn_work(sim, &kwork)) return rc;
    KnnWork &w = *kwork;
    MstWork *work = nullptr;
    if (int rc = workspace(sim, kWorkMst, &work, [](MstWork &f) {
            if (f.info.reserve(1) != hipSuccess || f.h_info.reserve(1) != hipSuccess ||
                f.h_plan.reserve(1) != hipSuccess) {
                (void)hipGetLastError();
                set_error("mst: cannot allocate the result workspace");
                return (int)NB_ERR_ALLOC;
            }
            return (int)NB_OK;
        }))
        return rc;
    MstWork &mw = *work;
    MstInfo &res = *static_cast<MstInfo *>(mw.h_info);
    KnnInfo &plan_res = *static_cast<KnnInfo *>(mw.h_plan);
    std::memset(&res, 0, sizeof res);
    std::memset(&plan_res, 0, sizeof plan_res);

    const uint32_t room = n ? n - 1 : 0;  // the edges a caller has room for
    if (n > 0) {
        const uint32_t blocks = (n + kThreads - 1) / kThreads;
        if (int rc = mst_reserve(mw.label, n)) return rc;
        if (int rc = mst_reserve(mw.parent, n)) return rc;
        if (int rc = mst_reserve(mw.slab, n)) return rc;
        if (int rc = mst_reserve(mw.next, n)) return rc;
        if (int rc = mst_reserve(mw.first_flag, blocks)) return rc;
        if (int rc = mst_reserve(mw.best_d2, n)) return rc;
        if (int rc = mst_reserve(mw.best_pair, n)) return rc;
        if (int rc = mst_reserve(mw.cand_d2, n)) return rc;
        if (int rc = mst_reserve(mw.cand_j, n)) return rc;
        if (int rc = mst_reserve(mw.raw_lo, n)) return rc;
        if (int rc = mst_reserve(mw.raw_hi, n)) return rc;
        if (int rc = mst_reserve(mw.perm, n)) return rc;
        if (int rc = mst_reserve(mw.raw_key, n)) return rc;
        if (int rc = mst_reserve(mw.edge_lo, n)) return rc;
        if (int rc = mst_reserve(mw.edge_hi, n)) return rc;
        if (int rc = mst_reserve(mw.degree, n)) return rc;
        if (int rc = mst_reserve(mw.d2, n)) return rc;
        if (edge_lo)
            if (int rc = mst_reserve(mw.h_edge_lo, n)) return rc;
        if (edge_hi)
            if (int rc = mst_reserve(mw.h_edge_hi, n)) return rc;
        if (d2)
            if (int rc = mst_reserve(mw.h_d2, n)) return rc;
        if (degree)
            if (int rc = mst_reserve(mw.h_degree, n)) return rc;
        if (int rc = knn_enqueue_sorted(sim, w)) return rc;

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        const KnnInfo *plan = w.info;
        MstInfo *mi = mw.info;
        static_assert(kPasses % 2 == 0, "the sorted arrays are on side 0");
        unsigned long long *keys = w.sort.keys[0];
        const uint32_t *sidx = w.sort.idx[0];
        const hipStream_t st = sim.stream;
        NB_HIP_TRY(hipMemsetAsync(mi, 0, sizeof(MstInfo), st));
        hipLaunchKernelGGL(mst_start_kernel, dim3(blocks), dim3(kThreads), 0, st, posm, vel, n, plan, sidx, mw.label,
                           mw.parent, mw.slab, mw.next, mw.best_d2, mw.best_pair, mw.degree);
        NB_HIP_TRY(hipGetLastError());

        const uint32_t per_block = (uint32_t)sim.mst_block_queries, span = (uint32_t)sim.mst_span_cells;
        const uint32_t skip = (uint32_t)sim.mst_skip_runs, shared = (uint32_t)sim.mst_shared_bound;
        const uint32_t rounds = mst_rounds(n);
        // one wave per sorted position; those past the counted bodies, and every block of a round that starts
        // from one component, return at once: no host round trip decides a launch
        for (uint32_t r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(mst_search_kernel, dim3((n + per_block - 1) / per_block), dim3(per_block * kWave), 0, st,
                               plan, (const MstInfo *)mi, r, (const unsigned long long *)keys, sidx,
                               (const float4 *)w.spos, (const uint32_t *)mw.slab, (const uint32_t *)mw.next,
                               (unsigned long long *)mw.best_d2, (double *)mw.cand_d2, (uint32_t *)mw.cand_j, span,
                               skip, shared);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(mst_pick_kernel, dim3(blocks), dim3(kThreads), 0, st, plan, (const MstInfo *)mi, r, sidx,
                               (const uint32_t *)mw.slab, (const unsigned long long *)mw.best_d2,
                               (const double *)mw.cand_d2, (const uint32_t *)mw.cand_j,
                               (unsigned long long *)mw.best_pair);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(mst_emit_kernel, dim3(blocks), dim3(kThreads), 0, st, plan, mi, r, n,
                               (const uint32_t *)mw.label, (const unsigned long long *)mw.best_d2,
                               (const unsigned long long *)mw.best_pair, (uint32_t *)mw.parent, (uint32_t *)mw.raw_lo,
                               (uint32_t *)mw.raw_hi, (unsigned long long *)mw.raw_key);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(mst_flatten_kernel, dim3(blocks), dim3(kThreads), 0, st, plan, (const MstInfo *)mi, r, n,
                               (const uint32_t *)mw.parent, (uint32_t *)mw.label);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(mst_relabel_kernel, dim3(blocks), dim3(kThreads), 0, st, plan, mi, r, sidx,
                               (const uint32_t *)mw.label, (uint32_t *)mw.parent, (uint32_t *)mw.slab,
                               (unsigned long long *)mw.best_d2, (unsigned long long *)mw.best_pair,
                               (uint32_t *)mw.first_flag);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(mst_suffix_kernel, dim3(1), dim3(kSuffixThreads), 0, st, plan, (const MstInfo *)mi, r,
                               (uint32_t *)mw.first_flag, blocks);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(mst_next_kernel, dim3(blocks), dim3(kThreads), 0, st, plan, (const MstInfo *)mi, r,
                               (const uint32_t *)mw.slab, (const uint32_t *)mw.first_flag, (uint32_t *)mw.next);
            NB_HIP_TRY(hipGetLastError());
        }

        // the plan is read before the sort's buffers, the front end's, are taken for the edges
        NB_HIP_TRY(hipMemcpyAsync(mw.h_plan, plan, sizeof(KnnInfo), hipMemcpyDeviceToHost, st));
        const SortShape shape = sort_shape(n);
        hipLaunchKernelGGL(mst_pair_key_kernel, dim3(blocks), dim3(kThreads), 0, st, n, (const MstInfo *)mi,
                           (const uint32_t *)mw.raw_lo, (const uint32_t *)mw.raw_hi, keys);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = enqueue_sort(st, w.sort, n, shape, kPasses, 0, nullptr)) return rc;
        hipLaunchKernelGGL(mst_d2_key_kernel, dim3(blocks), dim3(kThreads), 0, st, n, (const MstInfo *)mi, sidx,
                           (const unsigned long long *)mw.raw_key, (uint32_t *)mw.perm, keys);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = enqueue_sort(st, w.sort, n, shape, kPasses, 0, nullptr)) return rc;
        hipLaunchKernelGGL(mst_output_kernel, dim3(blocks), dim3(kThreads), 0, st, n, mi, sidx,
                           (const uint32_t *)mw.perm, (const uint32_t *)mw.raw_lo, (const uint32_t *)mw.raw_hi,
                           (const unsigned long long *)mw.raw_key, (uint32_t *)mw.edge_lo, (uint32_t *)mw.edge_hi,
                           (double *)mw.d2, (uint32_t *)mw.degree);
        NB_HIP_TRY(hipGetLastError());

        NB_HIP_TRY(hipMemcpyAsync(mw.h_info, mi, sizeof(MstInfo), hipMemcpyDeviceToHost, st));
        if (edge_lo && room)
            NB_HIP_TRY(hipMemcpyAsync(mw.h_edge_lo, mw.edge_lo, sizeof(uint32_t) * room, hipMemcpyDeviceToHost, st));
        if (edge_hi && room)
            NB_HIP_TRY(hipMemcpyAsync(mw.h_edge_hi, mw.edge_hi, sizeof(uint32_t) * room, hipMemcpyDeviceToHost, st));
        if (d2 && room) NB_HIP_TRY(hipMemcpyAsync(mw.h_d2, mw.d2, sizeof(double) * room, hipMemcpyDeviceToHost, st));
        if (degree)
            NB_HIP_TRY(hipMemcpyAsync(mw.h_degree, mw.degree, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    const uint32_t c = plan_res.n_ok, m = res.edges;
    if (m != (c ? c - 1 : 0u)) {  // (cannot happen: a spanning tree of c bodies)
        set_error("mst: %u edges for %u counted bodies", m, c);
        return NB_ERR_HIP;
    }
    if (m > 0) {
        if (edge_lo) std::memcpy(edge_lo, mw.h_edge_lo, sizeof(uint32_t) * m);
        if (edge_hi) std::memcpy(edge_hi, mw.h_edge_hi, sizeof(uint32_t) * m);
        if (d2) std::memcpy(d2, mw.h_d2, sizeof(double) * m);
    }
    if (degree && n > 0) std::memcpy(degree, mw.h_degree, sizeof(uint32_t) * n);
    if (stats) {
        nb_mst_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - c;
        o.edges = m;
        uint32_t before = c;
        for (uint32_t r = 0; r < NB_MST_MAX_ROUNDS && before > 1; ++r) {
            o.components_after[r] = before = res.comps_after[r];
            o.rounds = r + 1;
        }
        o.d2_min = res.d2_min;
        o.d2_max = res.d2_max;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = plan_res.lo[a];
            o.hi[a] = plan_res.hi[a];
        }
        o.h = plan_res.h;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
