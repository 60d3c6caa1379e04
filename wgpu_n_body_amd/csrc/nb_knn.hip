// nb_knn.hip -- nb_sim_knn: the k-th neighbour, the mass inside it and the density it gives, per body of a
// simulator's current state, and the density-weighted sums (include/nbody.h "k-nearest-neighbour density",
// DESIGN.md 6i; no reference counterpart).
//
// For a counted body i the other counted bodies are ordered by (d2(i, j), j); the k-th of them fixes r2, kth,
// mass_in and density.  The order is total (j is unique), so everything per body is unique given the state,
// whatever order the threads ran in.
//   bounds  -- the per-axis minimum and maximum of the counted bodies (body_ok) and their number c over the float4
//              SoA state (SimBase::diag_state), by the bounds pass of nb_analysis_sort.hpp; the one block that
//              finishes them makes the plan on the device: lo, hi and the side h = (largest extent) 2^-21 of
//              the finest cells.  Every later kernel reads the plan;
//   key     -- a body's cell on an axis is the q with e(q) <= x < e(q + 1), e(q) = lo + q h: found by a
//              division and then corrected by comparing x with the edges themselves, so that membership is a
//              comparison and not an arithmetic identity.  The key is the 63-bit Morton code of (qx, qy, qz),
//              or 2^63 for a body that does not count;
//   sort    -- the stable sort of nb_analysis_sort.hpp on (key, body index), all eight passes.  A cell of any
//              octree level is then a contiguous run of positions, its bodies of equal key in body order;
//   gather  -- positions and masses in sorted order; every body's outputs preset to those of a body that is
//              not counted, or of a state short of k;
//   search  -- one wave per counted body, "knn_block_queries" waves a block.  The k best (d2, j) sit one per
//              lane, ascending; a candidate that beats the k-th is inserted by a ballot and a shift.
//              (1) seed: the positions p - k .. p + k, at least k bodies, so the k-th is finite from here on;
//              (2) the body's own finest cell from its start, 64 positions a time: its bodies come in index
//                  order, so once the k-th is (0, j) with j no larger than the last index seen, nothing can
//                  beat it and the search is over (the k-zeros stop).  Coincident bodies share a cell;
//              (3) the range of finest cells per axis outside which the rule's own arithmetic on the gap to a
//                  cell edge already exceeds the k-th d2; the octree level at which that range is at most
//                  "knn_span_cells" cells an axis; each of those cells, one per lane: a lower bound of d2 from
//                  its edges, and, when the bound does not exceed the k-th d2, its run by two binary searches
//                  on key prefixes.  The runs are visited in ascending order of bound until the smallest
//                  exceeds the k-th d2 strictly; positions seen in (1) and (2) are skipped.
//              mass_in is then added over lanes 0 .. k - 2 in order, the density formed as written, and lane
//              0 stores the four results at the body's own index;
//   sums    -- over body order: the eight products of density, block_row slabs, sum_over_blocks<16>; the peak
//              by an integer maximum of the order-preserving encoding of the density, its index by an integer
//              minimum over the bodies that hold it.
// No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kPasses = 8;          // a 64-bit key; even, so the sorted arrays are on side 0
constexpr uint32_t kAxisBits = 21;
constexpr uint32_t kAxisMax = (1u << kAxisBits) - 1;       // the last finest cell of an axis
constexpr unsigned long long kKeyNone = 1ull << 63;        // past every Morton code
constexpr uint32_t kSumFields = 16, kSumLive = 9;          // the eight sums and the degenerate bodies
constexpr uint32_t kFinishGroups = 16;                     // G of sum_over_blocks
constexpr double kSphere = NB_KNN_SPHERE;                  // C = 4 pi / 3

// The plan and the reduced results of a call, on the device.  Written by single threads or integer atomics.
struct KnnInfo {
    double lo[3], hi[3];
    double h;                      // side of a finest cell; 0 when all counted bodies are at one point
    double sums[kSumFields];
    unsigned long long peak_key;   // ordered64 of the peak density, 0: none
    uint32_t n_ok, peak_index;
};

// the order-preserving encoding of a double as an unsigned integer (0.0 and -0.0 as one value); never 0
__device__ inline unsigned long long ordered64(double f) {
    if (f == 0.0) f = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(f);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__host__ inline double unordered64(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & ~(1ull << 63)) : ~e;
    double f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

__device__ inline double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// One block: the bounds into the plan.
__global__ __launch_bounds__(kThreads) void knn_plan_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                            KnnInfo *__restrict__ info) {
    double lo[3], hi[3];
    KnnInfo o{};
    if (!bounds_finish(slabs, blocks, lo, hi, &o.n_ok)) return;
    o.peak_index = NB_KNN_NONE;
    if (o.n_ok > 0) {
        double extent = 0.0;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = lo[a];
            o.hi[a] = hi[a];
            extent = fmax(extent, o.hi[a] - o.lo[a]);  // finite: a difference of binary32 values
        }
        o.h = extent * 0x1p-21;  // exact; 0 only for a state at one point
    }
    *info = o;
}

// ---- key ------------------------------------------------------------------------------------------
// the lower edge of finest cell q of an axis: non-decreasing in q (a product and a sum, each monotone)
__device__ inline double edge(double lo, double h, uint32_t q) { return lo + (double)q * h; }

__device__ inline uint32_t clamp_cell(double g) {
    return g >= (double)kAxisMax ? kAxisMax : (g > 0.0 ? (uint32_t)g : 0u);  // (NaN: 0)
}

// The finest cell of x: the q in 0 .. kAxisMax with edge(q) <= x, and x < edge(q + 1) unless q is the last.
// The division proposes, the comparisons decide; lo <= x = edge(0) side always holds.  The proposal is off by
// a cell at the most (h is at least 2^8 units in the last place of any coordinate involved), so the loops are
// short; they end in any case, q moving one way inside 0 .. kAxisMax.
__device__ inline uint32_t cell_of(float xf, double lo, double h) {
    if (!(h > 0.0)) return 0u;
    const double x = xf;
    uint32_t q = clamp_cell(floor((x - lo) / h));
    while (q > 0 && x < edge(lo, h, q)) --q;
    while (q < kAxisMax && x >= edge(lo, h, q + 1)) ++q;
    return q;
}

// bit i of x to bit 3 i
__device__ inline unsigned long long spread3(unsigned long long x) {
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ inline unsigned long long morton(uint32_t x, uint32_t y, uint32_t z) {
    return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2);
}

__global__ __launch_bounds__(kThreads) void knn_key_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, uint32_t n,
                                                           const KnnInfo *__restrict__ info,
                                                           unsigned long long *__restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i];
    unsigned long long key = kKeyNone;
    if (body_ok(p, vel[i])) {
        const double h = info->h;
        key = morton(cell_of(p.x, info->lo[0], h), cell_of(p.y, info->lo[1], h), cell_of(p.z, info->lo[2], h));
    }
    keys[i] = key;
}

// ---- gather ---------------------------------------------------------------------------------------
// spos[p] = the body at sorted position p; body i's outputs preset: not counted, or (counted) short of k --
// the search overwrites the latter when there are more than k counted bodies
__global__ __launch_bounds__(kThreads) void knn_gather_kernel(const float4 *__restrict__ posm,
                                                              const float4 *__restrict__ vel, uint32_t n,
                                                              const KnnInfo *__restrict__ info,
                                                              const uint32_t *__restrict__ sidx,
                                                              float4 *__restrict__ spos, double *__restrict__ r2,
                                                              uint32_t *__restrict__ kth, double *__restrict__ mass_in,
                                                              double *__restrict__ density) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (i < info->n_ok) spos[i] = posm[sidx[i]];
    r2[i] = body_ok(posm[i], vel[i]) ? (double)INFINITY : (double)NAN;
    kth[i] = NB_KNN_NONE;
    mass_in[i] = 0.0;
    density[i] = 0.0;
}

// ---- search ---------------------------------------------------------------------------------------
// the rule of include/nbody.h
__device__ inline double dist2(float4 p, float4 q) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline bool before(double d, uint32_t j, double kd, uint32_t kj) {
    return d < kd || (d == kd && j < kj);
}

// A wave's query: lane l < k holds the l-th best (d2, j) so far, ascending; (kd, kj) is the k-th, on every lane.
struct Query {
    float4 p;
    double ld, kd;
    uint32_t lj, kj;
    uint32_t k, lane;
};

// (cd, cj), the same on every lane and before the k-th, takes its place; the k-th falls off
__device__ inline void insert(Query &q, double cd, uint32_t cj) {
    const unsigned long long first_k = q.k == kWave ? ~0ull : (1ull << q.k) - 1ull;
    const uint32_t pos = (uint32_t)__popcll(__ballot(before(q.ld, q.lj, cd, cj)) & first_k);
    const double ud = __shfl_up(q.ld, 1);
    const uint32_t uj = __shfl_up(q.lj, 1);
    if (q.lane == pos) {
        q.ld = cd;
        q.lj = cj;
    } else if (q.lane > pos) {
        q.ld = ud;
        q.lj = uj;
    }
    q.kd = __shfl(q.ld, (int)q.k - 1);
    q.kj = __shfl(q.lj, (int)q.k - 1);
}

// lower bound of `want` in the ascending keys[lo .. hi)
__device__ inline uint32_t first_at_least(const unsigned long long *__restrict__ keys, uint32_t lo, uint32_t hi,
                                          unsigned long long want) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The bodies at sorted positions [b0, b1) against the query, 64 a time, but for the positions in [s0, s1) and
// [t0, t1).  All arguments are the same on every lane.
__device__ inline void scan_run(Query &q, const float4 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                uint32_t b0, uint32_t b1, uint32_t s0, uint32_t s1, uint32_t t0, uint32_t t1) {
    uint32_t a = b0;
    while (a < b1) {
        if (a >= t0 && a < t1) {  // (a crowded own cell inside a run: step over it)
            a = t1;
            continue;
        }
        const uint32_t pos = a + q.lane;
        const bool valid = pos < b1 && !(pos >= s0 && pos < s1) && !(pos >= t0 && pos < t1);
        double d = 0.0;
        uint32_t j = 0;
        if (valid) {
            d = dist2(q.p, spos[pos]);
            j = sidx[pos];
        }
        bool take = valid && before(d, j, q.kd, q.kj);
        unsigned long long m = __ballot(take);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            insert(q, __shfl(d, l), __shfl(j, l));
            take = take && (int)q.lane != l && before(d, j, q.kd, q.kj);
            m = __ballot(take);
        }
        a += kWave;
    }
}

__global__ __launch_bounds__(kThreads) void knn_search_kernel(const KnnInfo *__restrict__ info,
                                                              const unsigned long long *__restrict__ keys,
                                                              const uint32_t *__restrict__ sidx,
                                                              const float4 *__restrict__ spos,
                                                              const float4 *__restrict__ posm, uint32_t k,
                                                              uint32_t span, double *__restrict__ r2,
                                                              uint32_t *__restrict__ kth, double *__restrict__ mass_in,
                                                              double *__restrict__ density) {
#pragma clang fp contract(off)
    const uint32_t c = info->n_ok;
    if (c <= k) return;  // short of k: the presets stand
    const size_t pl = (size_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (pl >= c) return;  // (uniform over the wave)
    const uint32_t p = (uint32_t)pl;
    Query q;
    q.p = spos[p];
    q.ld = q.kd = INFINITY;
    q.lj = q.kj = NB_KNN_NONE;
    q.k = k;
    q.lane = threadIdx.x % kWave;

    // (1) the seed: at least k others, as c > k
    const uint32_t w0 = p > k ? p - k : 0u, w1 = (uint32_t)std::min<size_t>(c, (size_t)p + k + 1);
    scan_run(q, spos, sidx, w0, w1, p, p + 1, 0u, 0u);

    // (2) the own finest cell, in index order, with the k-zeros stop
    const unsigned long long key = keys[p];
    const uint32_t cs = first_at_least(keys, 0u, p, key), ce = first_at_least(keys, p + 1, c, key + 1);
    bool done = false;
    for (uint32_t a = cs; a < ce && !done; a += kWave) {
        const uint32_t a1 = std::min(ce, a + kWave);
        scan_run(q, spos, sidx, a, a1, w0, w1, 0u, 0u);
        done = q.kd == 0.0 && q.kj <= sidx[a1 - 1];
    }
    const double h = info->h;
    done = done || q.kd == 0.0 || !(h > 0.0);  // bodies of other cells are elsewhere: d2 > 0; h = 0: there are none

    if (!done) {
        // (3) finest cells [tlo, thi] per axis: a body of a cell below tlo or above thi has d2 > kd
        const double x[3] = {q.p.x, q.p.y, q.p.z};
        const double rad = sqrt(q.kd);
        uint32_t tlo[3], thi[3];
        for (int a = 0; a < 3; ++a) {
            const double lo = info->lo[a];
            uint32_t t0 = clamp_cell(floor(((x[a] - rad) - lo) / h) - 1.0);
            uint32_t t1 = clamp_cell(floor(((x[a] + rad) - lo) / h) + 1.0);
            while (t0 > 0) {  // bodies of cells below t0 have x_j < edge(t0)
                const double e = edge(lo, h, t0), g = x[a] - e;
                if (x[a] >= e && g * g > q.kd) break;
                --t0;
            }
            while (t1 < kAxisMax) {  // bodies of cells above t1 have x_j >= edge(t1 + 1)
                const double e = edge(lo, h, t1 + 1), g = e - x[a];
                if (e >= x[a] && g * g > q.kd) break;
                ++t1;
            }
            tlo[a] = t0;
            thi[a] = t1;
        }
        uint32_t s = 0;  // the level: cells of 2^s finest cells an axis
        while (s < kAxisBits && ((thi[0] >> s) - (tlo[0] >> s) >= span || (thi[1] >> s) - (tlo[1] >> s) >= span ||
                                 (thi[2] >> s) - (tlo[2] >> s) >= span))
            ++s;
        const uint32_t c0[3] = {tlo[0] >> s, tlo[1] >> s, tlo[2] >> s};
        const uint32_t nx = (thi[0] >> s) - c0[0] + 1, ny = (thi[1] >> s) - c0[1] + 1, nz = (thi[2] >> s) - c0[2] + 1;
        const uint32_t total = nx * ny * nz;  // at most span^3 <= 512
        for (uint32_t base = 0; base < total; base += kWave) {
            const uint32_t t = base + q.lane;
            bool pending = t < total;
            double bound = INFINITY;
            uint32_t b0 = 0, b1 = 0;
            if (pending) {
                const uint32_t cc[3] = {c0[0] + t % nx, c0[1] + (t / nx) % ny, c0[2] + t / (nx * ny)};
                double g[3];
                for (int a = 0; a < 3; ++a) {
                    // the cell's bodies have edge(first) <= x_j, and x_j < edge(last + 1) or, in the last
                    // cell of the axis, x_j <= hi
                    const uint32_t first = cc[a] << s, last = ((cc[a] + 1) << s) - 1;
                    const double elo = edge(info->lo[a], h, first);
                    const double ehi = last >= kAxisMax ? info->hi[a] : edge(info->lo[a], h, last + 1);
                    g[a] = fmax(0.0, fmax(elo - x[a], x[a] - ehi));
                }
                bound = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
                pending = bound <= q.kd;
                if (pending) {
                    const unsigned long long prefix = morton(cc[0], cc[1], cc[2]);
                    const unsigned long long klo = prefix << (3 * s), khi = (prefix + 1) << (3 * s);  // <= 2^63
                    b0 = first_at_least(keys, 0u, c, klo);
                    b1 = first_at_least(keys, b0, c, khi);
                    pending = b1 > b0;
                }
            }
            for (;;) {  // ascending bound; an equal bound is visited: a smaller index wins a tie
                const double b = pending ? bound : (double)INFINITY;
                const double least = wave_min(b);
                if (!(least <= q.kd)) break;
                const int l = __ffsll((long long)__ballot(pending && b == least)) - 1;
                scan_run(q, spos, sidx, __shfl(b0, l), __shfl(b1, l), w0, w1, cs, ce);
                if ((int)q.lane == l) pending = false;
            }
        }
    }

    // lane l < k holds the (l + 1)-th body of the order
    const double ml = q.lane + 1 < k && q.lj != NB_KNN_NONE ? (double)posm[q.lj].w : 0.0;
    double mass = 0.0;
    for (uint32_t l = 0; l + 1 < k; ++l) mass += __shfl(ml, (int)l);
    if (q.lane == 0) {
        const uint32_t body = sidx[p];
        r2[body] = q.kd;
        kth[body] = q.kj;
        mass_in[body] = mass;
        density[body] = q.kd == 0.0 ? (double)INFINITY : mass / (kSphere * (q.kd * sqrt(q.kd)));
    }
}

// ---- sums -----------------------------------------------------------------------------------------
// does body i enter the sums and the peak?  (*rho: its density; *degenerate: counted, r2 == 0)
__device__ inline bool summed(const KnnInfo *__restrict__ info, uint32_t k, float4 p, float4 v, double r2,
                              bool *degenerate) {
    *degenerate = false;
    if (info->n_ok <= k || !body_ok(p, v)) return false;
    *degenerate = r2 == 0.0;
    return r2 != 0.0 && isfinite(r2);
}

__global__ __launch_bounds__(kThreads) void knn_sum_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, uint32_t n, uint32_t k,
                                                           KnnInfo *__restrict__ info, const double *__restrict__ r2,
                                                           const double *__restrict__ density,
                                                           double *__restrict__ slabs) {
#pragma clang fp contract(off)
    __shared__ double part[kThreads / kWave][kSumFields];
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    double t[kSumLive];
    for (uint32_t f = 0; f < kSumLive; ++f) t[f] = 0.0;
    unsigned long long peak = 0ull;
    if (i < n) {
        const float4 p = posm[i], v = vel[i];
        bool degenerate;
        if (summed(info, k, p, v, r2[i], &degenerate)) {
            const double rho = density[i];
            t[0] = rho;
            t[1] = rho * (double)p.x;
            t[2] = rho * (double)p.y;
            t[3] = rho * (double)p.z;
            t[4] = rho * (double)v.x;
            t[5] = rho * (double)v.y;
            t[6] = rho * (double)v.z;
            t[7] = rho * rho;
            if (isfinite(rho)) peak = ordered64(rho);
        }
        t[8] = degenerate ? 1.0 : 0.0;
    }
    block_row<kSumFields, kSumLive>(t, part, slabs + (size_t)blockIdx.x * kSumFields);
    for (int o = 32; o > 0; o >>= 1) peak = std::max(peak, (unsigned long long)__shfl_xor(peak, o));
    if (threadIdx.x % kWave == 0 && peak) atomicMax(&info->peak_key, peak);
}

__global__ __launch_bounds__(kThreads) void knn_finish_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                              KnnInfo *__restrict__ info) {
    constexpr uint32_t kPer = kThreads / kFinishGroups;
    static_assert(kPer == kSumFields, "one column per field");
    __shared__ double pp[kFinishGroups][kPer];
    const uint32_t tid = threadIdx.x;
    const double r = sum_over_blocks<kFinishGroups>(slabs, blocks, kSumFields, tid % kPer, pp);
    if (tid < kPer) info->sums[tid] = r;
}

// the smallest index that holds the peak
__global__ __launch_bounds__(kThreads) void knn_peak_kernel(const float4 *__restrict__ posm,
                                                            const float4 *__restrict__ vel, uint32_t n, uint32_t k,
                                                            KnnInfo *__restrict__ info, const double *__restrict__ r2,
                                                            const double *__restrict__ density) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long peak = info->peak_key;
    bool degenerate;
    if (!peak || !summed(info, k, posm[i], vel[i], r2[i], &degenerate)) return;
    const double rho = density[i];
    if (isfinite(rho) && ordered64(rho) == peak) atomicMin(&info->peak_index, (uint32_t)i);
}

}  // namespace

struct KnnWork : Workspace {  // (all grow to the largest call so far)
    SortBufs<unsigned long long> sort;      // the two sides of (key, body index), the histogram
    DeviceBuf<double> slabs;                // [blocks][max(kBoundFields, kSumFields)]
    DeviceBuf<float4> spos;                 // [n]: positions and masses in sorted order
    DeviceBuf<double> r2, mass_in, density; // [n]
    DeviceBuf<uint32_t> kth;                // [n]
    PinnedBuf<double> h_r2, h_mass_in, h_density;  // [n]: staged, so that a failed call leaves the outputs alone
    PinnedBuf<uint32_t> h_kth;
    DeviceBuf<KnnInfo> info;                // [1]
    PinnedBuf<KnnInfo> h_info;              // [1]
};

namespace {

template <class B>
int knn_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("knn: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int sim_knn(SimBase &sim, const nb_knn_params &params, double *r2, uint32_t *kth, double *mass_in, double *density,
            nb_knn_stats *stats) {
    if (int rc = analysis_begin(sim, "knn")) return rc;
    if (!r2 && !kth && !mass_in && !density && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n, k = params.k;
    if (n > 0x7fffffffu) {
        set_error("knn: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    KnnWork *work = nullptr;
    if (int rc = workspace(sim, kWorkKnn, &work, [](KnnWork &f) {
            if (f.info.reserve(1) != hipSuccess || f.h_info.reserve(1) != hipSuccess) {
                (void)hipGetLastError();
                set_error("knn: cannot allocate the result workspace");
                return NB_ERR_ALLOC;
            }
            return NB_OK;
        }))
        return rc;
    KnnWork &w = *work;
    KnnInfo &res = *static_cast<KnnInfo *>(w.h_info);
    std::memset(&res, 0, sizeof res);
    res.peak_index = NB_KNN_NONE;

    if (n > 0) {
        const uint32_t blocks = (n + kThreads - 1) / kThreads;
        const SortShape shape = sort_shape(n);
        const uint32_t per_block = (uint32_t)sim.knn_block_queries, span = (uint32_t)sim.knn_span_cells;
        if (int rc = w.sort.reserve(n, shape, [](auto &b, size_t count) { return knn_reserve(b, count); })) return rc;
        if (int rc = knn_reserve(w.slabs, (size_t)std::max(kBoundFields, kSumFields) * blocks)) return rc;
        if (int rc = knn_reserve(w.spos, n)) return rc;
        if (int rc = knn_reserve(w.r2, n)) return rc;
        if (int rc = knn_reserve(w.mass_in, n)) return rc;
        if (int rc = knn_reserve(w.density, n)) return rc;
        if (int rc = knn_reserve(w.kth, n)) return rc;
        if (r2)
            if (int rc = knn_reserve(w.h_r2, n)) return rc;
        if (kth)
            if (int rc = knn_reserve(w.h_kth, n)) return rc;
        if (mass_in)
            if (int rc = knn_reserve(w.h_mass_in, n)) return rc;
        if (density)
            if (int rc = knn_reserve(w.h_density, n)) return rc;

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        KnnInfo *info = w.info;
        hipLaunchKernelGGL(bounds_kernel<>, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, w.slabs);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(knn_plan_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, blocks, info);
        NB_HIP_TRY(hipGetLastError());
        static_assert(kPasses % 2 == 0, "the sort starts from side 0 and its result is read from there");
        unsigned long long *keys = w.sort.keys[0];
        const uint32_t *sidx = w.sort.idx[0];
        hipLaunchKernelGGL(knn_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, info, keys);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, kPasses, 0, nullptr)) return rc;
        hipLaunchKernelGGL(knn_gather_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, info, sidx,
                           w.spos, w.r2, w.kth, w.mass_in, w.density);
        NB_HIP_TRY(hipGetLastError());
        // one wave per sorted position; those past the counted bodies, and all of them in a state short of k,
        // return at once: no host round trip decides the launch
        hipLaunchKernelGGL(knn_search_kernel, dim3((n + per_block - 1) / per_block), dim3(per_block * kWave), 0,
                           sim.stream, info, keys, sidx, w.spos, posm, k, span, w.r2, w.kth, w.mass_in, w.density);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(knn_sum_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, info, w.r2,
                           w.density, w.slabs);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(knn_finish_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, blocks, info);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(knn_peak_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, info, w.r2,
                           w.density);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_info, info, sizeof(KnnInfo), hipMemcpyDeviceToHost, sim.stream));
        if (r2) NB_HIP_TRY(hipMemcpyAsync(w.h_r2, w.r2, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
        if (kth) NB_HIP_TRY(hipMemcpyAsync(w.h_kth, w.kth, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (mass_in)
            NB_HIP_TRY(hipMemcpyAsync(w.h_mass_in, w.mass_in, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
        if (density)
            NB_HIP_TRY(hipMemcpyAsync(w.h_density, w.density, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (n > 0) {
        if (r2) std::memcpy(r2, w.h_r2, sizeof(double) * n);
        if (kth) std::memcpy(kth, w.h_kth, sizeof(uint32_t) * n);
        if (mass_in) std::memcpy(mass_in, w.h_mass_in, sizeof(double) * n);
        if (density) std::memcpy(density, w.h_density, sizeof(double) * n);
    }
    if (stats) {
        nb_knn_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - res.n_ok;
        o.counted = res.n_ok;
        o.degenerate = (uint64_t)res.sums[8];
        o.short_of_k = res.n_ok <= k ? res.n_ok : 0;
        o.sum_rho = res.sums[0];
        for (int a = 0; a < 3; ++a) {
            o.sum_rho_x[a] = res.sums[1 + a];
            o.sum_rho_v[a] = res.sums[4 + a];
        }
        o.sum_rho2 = res.sums[7];
        o.peak_index = res.peak_index;
        o.peak_density = res.peak_key ? unordered64(res.peak_key) : 0.0;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
