// nb_knn.hpp -- what the passes that start from the neighbour search share (nb_knn.hip: nb_sim_knn itself;
// nb_hop.hip: nb_sim_hop; nb_kinematics.hip: nb_local_kinematics_sim): the plan and the reduced results of the
// search on the device, its workspace, the part of it that only enqueues, and the device code of the search itself
// up to "lane l < k holds the (l + 1)-th body of the order", with the mass and the density that follow from it --
// every epilogue calls one search.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

constexpr uint32_t kKnnSumFields = 16;   // the eight sums and the degenerate bodies, padded to a slab row

// The plan and the reduced results of a call, on the device.  Written by single threads or integer atomics.
struct KnnInfo {
    double lo[3], hi[3];
    double h;                      // side of a finest cell; 0 when all counted bodies are at one point
    double sums[kKnnSumFields];
    unsigned long long peak_key;   // ordered64 of the peak density, 0: none
    uint32_t n_ok, peak_index;
};

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

// nb_knn.hip: the search's workspace (made by the first call), and the pass enqueued on the
// simulator's stream up to and including the search, with no synchronisation and no copy to the host (n > 0; the
// device is bound; k checked by knn_check_params).  Afterwards, in stream order, on the device: w.info (the plan
// and n_ok), the sorted (key, body index) on side 0 of w.sort, w.spos, and the four per-body arrays w.r2, w.kth,
// w.mass_in, w.density.
int knn_work(SimBase &sim, KnnWork **out);
int knn_enqueue(SimBase &sim, KnnWork &w, uint32_t k);
// ... and the same without the search kernel, for a pass that runs the search under an epilogue of its own
// (nb_kinematics.hip): afterwards w.info, the sorted (key, body index), w.spos, and the four per-body arrays at
// their presets (a body that is not counted, or a state short of k)
int knn_enqueue_sorted(SimBase &sim, KnnWork &w);

#ifdef __HIPCC__

constexpr uint32_t kKnnPasses = 8;       // a 64-bit key; even, so the sorted arrays are on side 0
constexpr uint32_t kKnnAxisBits = 21;
constexpr uint32_t kKnnAxisMax = (1u << kKnnAxisBits) - 1;    // the last finest cell of an axis

// the order-preserving encoding of a double as an unsigned integer (0.0 and -0.0 as one value); never 0
__device__ inline unsigned long long ordered64(double f) {
    if (f == 0.0) f = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(f);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

__device__ inline double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// ---- key ------------------------------------------------------------------------------------------
// the lower edge of finest cell q of an axis: non-decreasing in q (a product and a sum, each monotone)
__device__ inline double edge(double lo, double h, uint32_t q) { return lo + (double)q * h; }

__device__ inline uint32_t clamp_cell(double g) {
    return g >= (double)kKnnAxisMax ? kKnnAxisMax : (g > 0.0 ? (uint32_t)g : 0u);  // (NaN: 0)
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

// The search of sorted position p (p < c, c > k, the same on every lane of the wave): afterwards lane l < k holds
// the (l + 1)-th body of the order in (q.ld, q.lj), and (q.kd, q.kj) is the k-th on every lane.
__device__ inline void knn_search(Query &q, const KnnInfo *__restrict__ info,
                                  const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ sidx,
                                  const float4 *__restrict__ spos, uint32_t c, uint32_t p, uint32_t k,
                                  uint32_t span) {
#pragma clang fp contract(off)
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
            while (t1 < kKnnAxisMax) {  // bodies of cells above t1 have x_j >= edge(t1 + 1)
                const double e = edge(lo, h, t1 + 1), g = e - x[a];
                if (e >= x[a] && g * g > q.kd) break;
                ++t1;
            }
            tlo[a] = t0;
            thi[a] = t1;
        }
        uint32_t s = 0;  // the level: cells of 2^s finest cells an axis
        while (s < kKnnAxisBits && ((thi[0] >> s) - (tlo[0] >> s) >= span || (thi[1] >> s) - (tlo[1] >> s) >= span ||
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
                    const double ehi = last >= kKnnAxisMax ? info->hi[a] : edge(info->lo[a], h, last + 1);
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
}

// After knn_search: mass_in, added over lanes 0 .. k - 2 in order, and the density formed as written (the rule of
// include/nbody.h), the same on every lane.
__device__ inline void knn_mass_density(const Query &q, const float4 *__restrict__ posm, uint32_t k, double *mass_in,
                                        double *density) {
#pragma clang fp contract(off)
    const double ml = q.lane + 1 < k && q.lj != NB_KNN_NONE ? (double)posm[q.lj].w : 0.0;
    double mass = 0.0;
    for (uint32_t l = 0; l + 1 < k; ++l) mass += __shfl(ml, (int)l);
    *mass_in = mass;
    *density = q.kd == 0.0 ? (double)INFINITY : mass / (NB_KNN_SPHERE * (q.kd * sqrt(q.kd)));
}

#endif  // __HIPCC__

}  // namespace nb
