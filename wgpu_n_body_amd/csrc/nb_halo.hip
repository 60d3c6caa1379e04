// nb_halo.hip -- nb_sim_halo_profiles: the spherical profile of nb_sim_radial_profile about many centres in one
// call, each centre testing only the bodies of the grid cells its sphere can reach (include/nbody.h "Halo
// profiles"; no reference counterpart).
//
//   bounds  -- the per-axis minimum and maximum of the counted bodies (body_ok) and their number, by the bounds pass
//              of nb_analysis_sort.hpp; the one block that finishes them makes the plan on the device: a uniform
//              grid of side h = max(R, E / 1024), R = edges[nbins], E the largest extent, at most 1,024 cells an
//              axis.  Every later kernel reads the plan;
//   key     -- a body's cell on an axis is the q with e(q) <= x < e(q + 1), e(q) = lo + q h: proposed by a
//              division, decided by comparing x with the edges themselves (as nb_knn.hip does).  The key is the
//              linear cell id, x fastest, or the number of cells for a body that does not count;
//   sort    -- the stable sort of nb_analysis_sort.hpp on (key, body index), four passes.  A row of cells along x
//              is then one contiguous run of positions, its bodies in body order inside a cell;
//   centre  -- one thread per centre: the centre and velocity used (a body centre is read here), the range of cells
//              per axis outside which the rule's own arithmetic on the gap to a cell edge already reaches R^2, the
//              non-empty runs of that range in (iz, iy) order, their total T and the ceil(T / L) work items;
//   scan    -- one block: the exclusive prefix sum of the work items over the centres; then one thread per centre
//              names its items' centre;
//   gather  -- blocks stride over the work items.  An item walks its L candidates in tiles of 256: a thread loads
//              its candidate through the sorted index, classifies it (fp64, no contraction; the branch-free binary
//              search over the squared edges in LDS), and stages the bin and the eight terms in LDS; the tile is
//              summed per bin as nb_radial.hip does (segments of P = the power of two >= nbins, scanned in
//              candidate order).  The item writes one partial of 2 + 9 nbins doubles;
//   finish  -- per centre, every element of its partials added in item order from 0, written as the rows the caller
//              gets.
// No float atomics; the candidate sequence of a centre is a function of the state and the edges alone, so a
// centre's row does not depend on the other centres and two calls return the same bits.
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

constexpr uint32_t kThreads = kBlock;    // = candidates per tile; 4 waves per block
constexpr uint32_t kPasses = 4;          // a 32-bit key; even, so the sorted arrays are on side 0
constexpr uint32_t kMaxBins = NB_HALO_MAX_BINS;
constexpr uint32_t kEdgeSlots = 128;     // squared edges in LDS, padded with +inf for the search
constexpr uint32_t kChunk = NB_HALO_CHUNK;                 // L
constexpr uint32_t kAxisCells = NB_HALO_MAX_CELLS_PER_AXIS;
constexpr uint32_t kMaxSpan = 5;                           // cells of a centre's range on y and on z (3 but for rounding)
constexpr uint32_t kMaxRuns = kMaxSpan * kMaxSpan;
constexpr uint32_t kTerms = 8;                             // staged per candidate, see Field
constexpr uint32_t kBinFields = 9;                         // the terms and the count
constexpr uint32_t kHeadFields = 2;                        // inside_count, inside_mass
constexpr uint32_t kGatherBlocks = 2048;
constexpr uint32_t kFinishBlocks = 4096;
constexpr uint32_t kStatusSpan = 1u, kStatusItems = 2u;
constexpr uint16_t kNoBin = 0xffff;

static_assert(kChunk % kThreads == 0 && kChunk >= 1024 && kChunk <= 16384, "L is whole tiles");
static_assert(kMaxBins + 1 < kEdgeSlots, "the search covers every edge");

enum Field { kFMass = 0, kFR, kFUr, kFUr2, kFU2, kFAng /* 5..7 */, kFCount = 8 };
// the 8-byte word of nb_radial_bin a field goes to (count first; m_uphi and m_uphi2 stay 0)
__device__ inline uint32_t bin_word(uint32_t f) { return f == kFCount ? 0u : f < kFU2 ? f + 1 : f + 3; }

// The plan and the totals of a call, on the device.  Written by single threads or integer atomics.
struct HaloInfo {
    double lo[3], hi[3];
    double h;                      // side of a cell
    double r2max;                  // edges[nbins]^2
    unsigned long long tested;     // sum of T over the centres
    unsigned long long items;      // sum of the work items
    uint32_t cells[3];
    uint32_t n_ok;
    uint32_t status, pad;
};

// A centre's plan: what it uses and where its candidates are.
struct HaloCentre {
    double c[3], vc[3];
    uint32_t flags, runs;
    uint32_t start[kMaxRuns];      // first sorted position of run r
    uint32_t pre[kMaxRuns + 1];    // candidates before run r; pre[runs] = T
};

// One block: the bounds into the plan.
__global__ __launch_bounds__(kThreads) void halo_plan_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                             double radius, double r2max,
                                                             HaloInfo *__restrict__ info) {
    double lo[3], hi[3];
    HaloInfo o{};
    if (!bounds_finish(slabs, blocks, lo, hi, &o.n_ok)) return;
    o.r2max = r2max;
    o.h = radius;
    for (int a = 0; a < 3; ++a) o.cells[a] = 1;
    if (o.n_ok > 0) {
        double extent = 0.0;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = lo[a];
            o.hi[a] = hi[a];
            extent = fmax(extent, hi[a] - lo[a]);  // finite: a difference of binary32 values
        }
        o.h = fmax(radius, extent * 0x1p-10);  // > 0: radius is
        for (int a = 0; a < 3; ++a) {
            const double g = floor((hi[a] - lo[a]) / o.h) + 1.0;  // at most 1,025
            o.cells[a] = g >= (double)kAxisCells ? kAxisCells : (uint32_t)g;
        }
    }
    *info = o;
}

// ---- key ------------------------------------------------------------------------------------------
// the lower edge of cell q of an axis: non-decreasing in q (a product and a sum, each monotone)
__device__ inline double edge(double lo, double h, uint32_t q) { return lo + (double)q * h; }

__device__ inline uint32_t clamp_cell(double g, uint32_t last) {
    return g >= (double)last ? last : (g > 0.0 ? (uint32_t)g : 0u);  // (NaN: 0)
}

// The cell of x: the q in 0 .. last with edge(q) <= x, and x < edge(q + 1) unless q is the last.  The division
// proposes, the comparisons decide.
__device__ inline uint32_t cell_of(float xf, double lo, double h, uint32_t last) {
    const double x = xf;
    uint32_t q = clamp_cell(floor((x - lo) / h), last);
    while (q > 0 && x < edge(lo, h, q)) --q;
    while (q < last && x >= edge(lo, h, q + 1)) ++q;
    return q;
}

__global__ __launch_bounds__(kThreads) void halo_key_kernel(const float4 *__restrict__ posm,
                                                            const float4 *__restrict__ vel, uint32_t n,
                                                            const HaloInfo *__restrict__ info,
                                                            uint32_t *__restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i];
    const uint32_t cx = info->cells[0], cy = info->cells[1], cz = info->cells[2];
    uint32_t key = cx * cy * cz;  // past every cell
    if (body_ok(p, vel[i])) {
        const double h = info->h;
        const uint32_t qx = cell_of(p.x, info->lo[0], h, cx - 1), qy = cell_of(p.y, info->lo[1], h, cy - 1),
                       qz = cell_of(p.z, info->lo[2], h, cz - 1);
        key = (qz * cy + qy) * cx + qx;
    }
    keys[i] = key;
}

// ---- centre ---------------------------------------------------------------------------------------
// lower bound of `want` in the ascending keys[lo .. hi)
__device__ inline uint32_t first_at_least(const uint32_t *__restrict__ keys, uint32_t lo, uint32_t hi, uint32_t want) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Bodies of cells below t have x < edge(t) <= c: |fl(x - c)| >= fl(c - edge(t)) = g, and g g >= R^2 puts them at
// r2 >= R^2.  True for t = 0: there are none.
__device__ inline bool none_below(double c, double lo, double h, double r2max, uint32_t t) {
    if (t == 0) return true;
    const double e = edge(lo, h, t), g = c - e;
    return c >= e && g * g >= r2max;
}
// Bodies of cells above t have x >= edge(t + 1) >= c.  True for t = last.
__device__ inline bool none_above(double c, double lo, double h, double r2max, uint32_t t, uint32_t last) {
    if (t == last) return true;
    const double e = edge(lo, h, t + 1), g = e - c;
    return e >= c && g * g >= r2max;
}

// The cells [t0, t1] of an axis a centre at c has to look at: t0 the largest t with none_below, t1 the smallest
// with none_above (both monotone in t, so the walk from any proposal ends there).  False when the sphere lies
// wholly outside the counted bodies' bounds on this axis.
__device__ inline bool axis_range(double c, double lo, double hi, double h, uint32_t last, double r2max,
                                  uint32_t *t0_out, uint32_t *t1_out) {
    {
        const double g = c - hi;
        if (c >= hi && g * g >= r2max) return false;  // every body has x <= hi
    }
    {
        const double g = lo - c;
        if (lo >= c && g * g >= r2max) return false;  // every body has x >= lo
    }
    const double rad = sqrt(r2max);
    uint32_t t0 = clamp_cell(floor(((c - rad) - lo) / h), last);
    uint32_t t1 = clamp_cell(floor(((c + rad) - lo) / h), last);
    while (!none_below(c, lo, h, r2max, t0)) --t0;
    while (t0 < last && none_below(c, lo, h, r2max, t0 + 1)) ++t0;
    while (!none_above(c, lo, h, r2max, t1, last)) ++t1;
    while (t1 > 0 && none_above(c, lo, h, r2max, t1 - 1, last)) --t1;
    *t0_out = t0;
    *t1_out = t1;
    return t0 <= t1;
}

// centers / bodies: exactly one non-null.  velocities may be null.
__global__ __launch_bounds__(kThreads) void halo_centre_kernel(const float4 *__restrict__ posm,
                                                               const float4 *__restrict__ vel, uint32_t m,
                                                               const double *__restrict__ centers,
                                                               const uint32_t *__restrict__ bodies,
                                                               const double *__restrict__ velocities,
                                                               HaloInfo *__restrict__ info,
                                                               const uint32_t *__restrict__ keys,
                                                               HaloCentre *__restrict__ plan,
                                                               uint32_t *__restrict__ items) {
    const size_t ci = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (ci >= m) return;
    HaloCentre &o = plan[ci];
    double c[3] = {0.0, 0.0, 0.0}, vc[3] = {0.0, 0.0, 0.0};
    uint32_t flags = 0;
    if (centers) {
        for (int a = 0; a < 3; ++a) c[a] = centers[3 * ci + a];
        if (velocities)
            for (int a = 0; a < 3; ++a) vc[a] = velocities[3 * ci + a];
    } else {
        const float4 p = posm[bodies[ci]], v = vel[bodies[ci]];
        if (body_ok(p, v)) {
            c[0] = p.x, c[1] = p.y, c[2] = p.z;
            vc[0] = v.x, vc[1] = v.y, vc[2] = v.z;
            if (velocities)
                for (int a = 0; a < 3; ++a) vc[a] = velocities[3 * ci + a];
        } else {
            flags = NB_HALO_CENTER_NONFINITE;
        }
    }
    uint32_t runs = 0, total = 0;
    const uint32_t n_ok = info->n_ok;
    const double r2max = info->r2max;
    uint32_t t0[3], t1[3];
    bool any = !flags && n_ok > 0 && r2max > 0.0;
    for (int a = 0; a < 3 && any; ++a)
        any = axis_range(c[a], info->lo[a], info->hi[a], info->h, info->cells[a] - 1, r2max, &t0[a], &t1[a]);
    if (any) {
        if (t1[1] - t0[1] >= kMaxSpan || t1[2] - t0[2] >= kMaxSpan) {
            atomicOr(&info->status, kStatusSpan);  // (h >= R: cannot happen)
        } else {
            const uint32_t cx = info->cells[0], cy = info->cells[1];
            for (uint32_t iz = t0[2]; iz <= t1[2]; ++iz)
                for (uint32_t iy = t0[1]; iy <= t1[1]; ++iy) {
                    const uint32_t row = (iz * cy + iy) * cx;
                    const uint32_t b0 = first_at_least(keys, 0u, n_ok, row + t0[0]);
                    const uint32_t b1 = first_at_least(keys, b0, n_ok, row + t1[0] + 1);
                    if (b1 > b0) {
                        o.start[runs] = b0;
                        o.pre[runs] = total;
                        total += b1 - b0;
                        ++runs;
                    }
                }
        }
    }
    o.pre[runs] = total;
    o.runs = runs;
    o.flags = flags;
    for (int a = 0; a < 3; ++a) {
        o.c[a] = c[a];
        o.vc[a] = vc[a];
    }
    const uint32_t it = (total + kChunk - 1) / kChunk;
    items[ci] = it;
    if (total) {
        atomicAdd(&info->tested, (unsigned long long)total);
        atomicAdd(&info->items, (unsigned long long)it);
    }
}

// One block: first[c] = the work items before centre c, first[m] = all of them.  A total the partials have no room
// for is a refusal: the later kernels return at once.
__global__ __launch_bounds__(kScanThreads) void halo_scan_kernel(uint32_t *__restrict__ first, uint32_t m,
                                                                 uint32_t capacity, HaloInfo *__restrict__ info) {
    __shared__ uint32_t lds[2 * kScanThreads];
    if (info->items > capacity) {  // (the 32-bit scan could wrap)
        if (threadIdx.x == 0) info->status |= kStatusItems;
        return;
    }
    const uint32_t total = block_scan_runs(first, m, lds);
    if (threadIdx.x == 0) first[m] = total;
}

__global__ __launch_bounds__(kThreads) void halo_items_kernel(const uint32_t *__restrict__ first, uint32_t m,
                                                              const HaloInfo *__restrict__ info,
                                                              uint32_t *__restrict__ item_centre) {
    const size_t ci = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (ci >= m || info->status) return;
    for (uint32_t it = first[ci]; it < first[ci + 1]; ++it) item_centre[it] = (uint32_t)ci;
}

// ---- gather: one partial of kHeadFields + nbins * kBinFields doubles per work item -----------------------------
// One candidate by the rule of include/nbody.h (spherical): its class (cnt = edges at or below r2: 0 inside,
// nbins + 1 outside) and its eight terms.
__device__ inline uint32_t classify(float4 p, float4 v, const double *c, const double *vc, const double *e2,
                                    double (&term)[kTerms]) {
#pragma clang fp contract(off)
    const double m = p.w;
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    const double ux = (double)v.x - vc[0], uy = (double)v.y - vc[1], uz = (double)v.z - vc[2];
    const double r2 = (dx * dx + dy * dy) + dz * dz;
    uint32_t cnt = 0;
    for (uint32_t step = kEdgeSlots / 2; step > 0; step >>= 1)
        if (e2[cnt + step - 1] <= r2) cnt += step;
    const double r = sqrt(r2);
    double ur = 0.0;
    if (r2 != 0.0) ur = ((dx * ux + dy * uy) + dz * uz) / r;
    term[kFMass] = m;
    term[kFR] = m * r;
    term[kFUr] = m * ur;
    term[kFUr2] = (m * ur) * ur;
    term[kFU2] = m * ((ux * ux + uy * uy) + uz * uz);
    term[kFAng + 0] = m * (dy * uz - dz * uy);
    term[kFAng + 1] = m * (dz * ux - dx * uz);
    term[kFAng + 2] = m * (dx * uy - dy * ux);
    return cnt;
}

__global__ __launch_bounds__(kThreads) void halo_gather_kernel(const float4 *__restrict__ posm,
                                                               const float4 *__restrict__ vel,
                                                               const uint32_t *__restrict__ sidx,
                                                               const HaloInfo *__restrict__ info,
                                                               const HaloCentre *__restrict__ plan,
                                                               const uint32_t *__restrict__ first,
                                                               const uint32_t *__restrict__ item_centre,
                                                               uint32_t m, uint32_t nbins, uint32_t p2,
                                                               const double *__restrict__ e2g,
                                                               double *__restrict__ partials) {
    __shared__ double e2[kEdgeSlots];
    __shared__ double stage[kBinFields][kThreads];  // [term][candidate of the tile]; at the end [field][thread]
    __shared__ uint16_t bin_of[kThreads];
    __shared__ double part[kThreads / kWave][kHeadFields];
    __shared__ uint32_t run_start[kMaxRuns], run_pre[kMaxRuns + 1];
    __shared__ double cen[6];
    if (info->status) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = tid; j < kEdgeSlots; j += kThreads) e2[j] = j <= nbins ? e2g[j] : INFINITY;
    const uint32_t my_bin = tid & (p2 - 1), seg0 = tid & ~(p2 - 1);
    const uint32_t n_items = first[m], elems = kHeadFields + nbins * kBinFields;

    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t ci = item_centre[item];
        const HaloCentre &hc = plan[ci];
        const uint32_t runs = hc.runs;
        if (tid < runs) run_start[tid] = hc.start[tid];
        if (tid <= runs) run_pre[tid] = hc.pre[tid];
        if (tid < 3) cen[tid] = hc.c[tid];
        else if (tid < 6) cen[tid] = hc.vc[tid - 3];
        __syncthreads();
        const uint32_t total = run_pre[runs];
        const uint32_t o0 = (item - first[ci]) * kChunk, o1 = std::min(total, o0 + kChunk);  // (o0 < total)

        double acc[kBinFields];
        for (uint32_t f = 0; f < kBinFields; ++f) acc[f] = 0.0;
        double head[kHeadFields] = {0.0, 0.0};

        // this thread's candidates are o0 + tid, o0 + tid + 256, ...: the run only moves forward
        uint32_t run = 0;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p;
        auto fetch = [&](uint32_t ord) {
            if (ord < o1) {
                while (ord >= run_pre[run + 1]) ++run;
                const uint32_t i = sidx[run_start[run] + (ord - run_pre[run])];
                p = posm[i];
                v = vel[i];
            }
        };
        fetch(o0 + tid);
        for (uint32_t o = o0; o < o1; o += kThreads) {
            uint16_t b = kNoBin;
            if (o + tid < o1) {
                double term[kTerms];
                const uint32_t cnt = classify(p, v, cen, cen + 3, e2, term);
                if (cnt == 0) {
                    head[0] += 1.0;
                    head[1] += term[kFMass];
                } else if (cnt <= nbins) {
                    b = (uint16_t)(cnt - 1);
                    for (uint32_t f = 0; f < kTerms; ++f) stage[f][tid] = term[f];
                }
            }
            bin_of[tid] = b;
            __syncthreads();
            fetch(o + kThreads + tid);  // the next tile's loads fly while this one is summed
            for (uint32_t j = seg0; j < seg0 + p2; ++j) {
                if (bin_of[j] == my_bin) {
                    for (uint32_t f = 0; f < kTerms; ++f) acc[f] += stage[f][j];
                    acc[kFCount] += 1.0;
                }
            }
            __syncthreads();  // the tile has been read
        }

        // what is not binned through the waves; then the segments of every bin, in order
        for (uint32_t f = 0; f < kBinFields; ++f) stage[f][tid] = acc[f];
        double *row = partials + (size_t)item * elems;
        block_row<kHeadFields, kHeadFields>(head, part, row);
        if (tid < nbins) {
            for (uint32_t f = 0; f < kBinFields; ++f) {
                double s = stage[f][tid];
                for (uint32_t q = p2; q < kThreads; q += p2) s += stage[f][q + tid];
                row[kHeadFields + tid * kBinFields + f] = s;
            }
        }
        __syncthreads();  // the item's LDS has been read
    }
}

// ---- finish: a centre's partials added in item order, into the rows the caller gets ----------------------------
__global__ __launch_bounds__(kThreads) void halo_finish_kernel(const HaloInfo *__restrict__ info,
                                                               const HaloCentre *__restrict__ plan,
                                                               const uint32_t *__restrict__ first, uint32_t m,
                                                               uint32_t nbins, const double *__restrict__ partials,
                                                               nb_halo_head *__restrict__ heads,
                                                               nb_radial_bin *__restrict__ bins) {
    if (info->status) return;
    const uint32_t tid = threadIdx.x, elems = kHeadFields + nbins * kBinFields;
    for (uint32_t ci = blockIdx.x; ci < m; ci += gridDim.x) {
        const uint32_t i0 = first[ci], i1 = first[ci + 1];
        unsigned long long *words = reinterpret_cast<unsigned long long *>(bins + (size_t)ci * nbins);
        for (uint32_t e = tid; e < elems; e += kThreads) {
            double s = 0.0;
            for (uint32_t it = i0; it < i1; ++it) s += partials[(size_t)it * elems + e];
            if (e == 0) {
                heads[ci].inside_count = (uint32_t)s;
            } else if (e == 1) {
                heads[ci].inside_mass = s;
            } else {
                const uint32_t b = (e - kHeadFields) / kBinFields, f = (e - kHeadFields) % kBinFields;
                unsigned long long *w = words + (size_t)b * 11 + bin_word(f);
                *w = f == kFCount ? (unsigned long long)s : (unsigned long long)__double_as_longlong(s);
            }
        }
        for (uint32_t b = tid; b < nbins; b += kThreads) {  // m_uphi, m_uphi2: 0 as in spherical mode
            words[(size_t)b * 11 + 5] = 0ull;
            words[(size_t)b * 11 + 6] = 0ull;
        }
        if (tid < 3) heads[ci].center[tid] = plan[ci].c[tid];
        else if (tid < 6) heads[ci].velocity[tid - 3] = plan[ci].vc[tid - 3];
        else if (tid == 6) heads[ci].flags = plan[ci].flags;
    }
}

uint32_t pow2_at_least(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

size_t round_up(size_t x, size_t to) { return (x + to - 1) / to * to; }

}  // namespace

static_assert(sizeof(nb_radial_bin) == 88, "halo_finish_kernel writes nb_radial_bin as 11 words");

struct HaloWork : Workspace {  // (all grow to the largest call so far)
    SortBufs<uint32_t> sort;          // the two sides of (key, body index), the histogram
    DeviceBuf<double> slabs;          // [blocks][kBoundFields]
    DeviceBuf<double> in;             // squared edges [kEdgeSlots], then centres or velocities [m][3] each
    DeviceBuf<uint32_t> in_bodies;    // [m]
    DeviceBuf<HaloCentre> plan;       // [m]
    DeviceBuf<uint32_t> first;        // [m + 1]
    DeviceBuf<uint32_t> item_centre;  // [capacity]
    DeviceBuf<double> partials;       // [capacity][2 + 9 nbins]
    DeviceBuf<unsigned char> out;     // HaloInfo (padded), heads [m], bins [m][nbins]
    PinnedBuf<double> h_in;
    PinnedBuf<uint32_t> h_bodies;
    PinnedBuf<unsigned char> h_out;
};

namespace {

template <class B>
int halo_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("halo_profiles: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int sim_halo_profiles(SimBase &sim, const nb_halo_params &params, nb_halo_head *heads, nb_radial_bin *bins,
                      nb_halo_stats *stats) {
    if (int rc = analysis_begin(sim, "halo_profiles")) return rc;
    const uint32_t n = sim.n, nbins = params.nbins;
    const uint32_t m = (uint32_t)params.m;
    if (n > 0x7fffffffu) {
        set_error("halo_profiles: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    if (params.bodies)
        for (uint32_t j = 0; j < m; ++j)
            if (params.bodies[j] >= n) {
                set_error("halo_profiles: bodies[%u] = %u is not a body of %u", j, params.bodies[j], n);
                return NB_ERR_INVALID;
            }
    HaloWork *work = nullptr;
    if (int rc = workspace(sim, kWorkHalo, &work, [](HaloWork &) { return NB_OK; })) return rc;
    HaloWork &w = *work;

    nb_halo_stats st{};
    st.step_num = sim.step_num;
    st.n = n;
    st.centers = m;
    const bool launch = n > 0 && m > 0;
    const size_t heads_at = round_up(sizeof(HaloInfo), 64), bins_at = heads_at + sizeof(nb_halo_head) * (size_t)m;
    if (launch) {
        const uint32_t blocks = (n + kThreads - 1) / kThreads, cblocks = (m + kThreads - 1) / kThreads;
        const SortShape shape = sort_shape(n);
        // sum over the centres of ceil(T / L) <= m + floor(sum of T / L) <= m + floor(m n / L): room for one item a
        // centre, whatever m is, and for NB_HALO_EXTRA_ITEMS more
        const uint64_t bound = (uint64_t)m + (uint64_t)m * n / kChunk;
        const uint32_t capacity = (uint32_t)std::min<uint64_t>(bound, (uint64_t)m + NB_HALO_EXTRA_ITEMS);
        const uint32_t elems = kHeadFields + nbins * kBinFields;
        const size_t out_bytes = bins_at + sizeof(nb_radial_bin) * (size_t)m * nbins;
        const size_t copy_bytes = bins ? out_bytes : heads ? bins_at : sizeof(HaloInfo);
        const size_t in_count = kEdgeSlots + 6 * (size_t)m;
        if (int rc = w.sort.reserve(n, shape, [](auto &b, size_t count) { return halo_reserve(b, count); })) return rc;
        if (int rc = halo_reserve(w.slabs, (size_t)kBoundFields * blocks)) return rc;
        if (int rc = halo_reserve(w.in, in_count)) return rc;
        if (int rc = halo_reserve(w.h_in, in_count)) return rc;
        if (int rc = halo_reserve(w.in_bodies, m)) return rc;
        if (int rc = halo_reserve(w.h_bodies, m)) return rc;
        if (int rc = halo_reserve(w.plan, m)) return rc;
        if (int rc = halo_reserve(w.first, (size_t)m + 1)) return rc;
        if (int rc = halo_reserve(w.item_centre, capacity)) return rc;
        if (int rc = halo_reserve(w.partials, (size_t)capacity * elems)) return rc;
        if (int rc = halo_reserve(w.out, out_bytes)) return rc;
        if (int rc = halo_reserve(w.h_out, copy_bytes)) return rc;

        double *h_in = w.h_in, *d_in = w.in;
        for (uint32_t j = 0; j <= nbins; ++j) h_in[j] = params.edges[j] * params.edges[j];
        const double *d_centers = nullptr, *d_vel = nullptr;
        const uint32_t *d_bodies = nullptr;
        size_t used = kEdgeSlots;
        if (params.centers) {
            std::memcpy(h_in + used, params.centers, sizeof(double) * 3 * m);
            d_centers = d_in + used;
            used += 3 * (size_t)m;
        } else {
            std::memcpy(w.h_bodies, params.bodies, sizeof(uint32_t) * m);
            NB_HIP_TRY(hipMemcpyAsync(w.in_bodies, w.h_bodies, sizeof(uint32_t) * m, hipMemcpyHostToDevice, sim.stream));
            d_bodies = w.in_bodies;
        }
        if (params.velocities) {
            std::memcpy(h_in + used, params.velocities, sizeof(double) * 3 * m);
            d_vel = d_in + used;
            used += 3 * (size_t)m;
        }
        NB_HIP_TRY(hipMemcpyAsync(d_in, h_in, sizeof(double) * used, hipMemcpyHostToDevice, sim.stream));

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        unsigned char *out = w.out;
        HaloInfo *info = reinterpret_cast<HaloInfo *>(out);
        nb_halo_head *d_heads = reinterpret_cast<nb_halo_head *>(out + heads_at);
        nb_radial_bin *d_bins = reinterpret_cast<nb_radial_bin *>(out + bins_at);
        hipLaunchKernelGGL(bounds_kernel<>, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, w.slabs);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(halo_plan_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, blocks,
                           params.edges[nbins], h_in[nbins], info);
        NB_HIP_TRY(hipGetLastError());
        static_assert(kPasses % 2 == 0, "the sort starts from side 0 and its result is read from there");
        uint32_t *keys = w.sort.keys[0];
        const uint32_t *sidx = w.sort.idx[0];
        hipLaunchKernelGGL(halo_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, info, keys);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, kPasses, 0, nullptr)) return rc;
        hipLaunchKernelGGL(halo_centre_kernel, dim3(cblocks), dim3(kThreads), 0, sim.stream, posm, vel, m, d_centers,
                           d_bodies, d_vel, info, keys, w.plan, w.first);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(halo_scan_kernel, dim3(1), dim3(kScanThreads), 0, sim.stream, w.first, m, capacity, info);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(halo_items_kernel, dim3(cblocks), dim3(kThreads), 0, sim.stream, w.first, m, info,
                           w.item_centre);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(halo_gather_kernel, dim3(std::min(capacity, kGatherBlocks)), dim3(kThreads), 0, sim.stream,
                           posm, vel, sidx, info, w.plan, w.first, w.item_centre, m, nbins, pow2_at_least(nbins), d_in,
                           w.partials);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(halo_finish_kernel, dim3(std::min(m, kFinishBlocks)), dim3(kThreads), 0, sim.stream, info,
                           w.plan, w.first, m, nbins, w.partials, d_heads, d_bins);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_out, out, copy_bytes, hipMemcpyDeviceToHost, sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;

    if (launch) {
        const unsigned char *h_out = w.h_out;
        HaloInfo res;
        std::memcpy(&res, h_out, sizeof res);
        if (res.status & kStatusSpan) {
            set_error("halo_profiles: a centre's cell range is wider than %u cells", kMaxSpan);
            return NB_ERR_UNSUPPORTED;
        }
        if (res.status & kStatusItems) {
            set_error("halo_profiles: %llu work items of %u candidates are more than one call takes (%u centres + %u): "
                      "use fewer centres a call or a smaller edges[nbins]",
                      res.items, kChunk, m, NB_HALO_EXTRA_ITEMS);
            return NB_ERR_UNSUPPORTED;
        }
        if (heads) std::memcpy(heads, h_out + heads_at, sizeof(nb_halo_head) * (size_t)m);
        if (bins) std::memcpy(bins, h_out + bins_at, sizeof(nb_radial_bin) * (size_t)m * nbins);
        st.nonfinite = n - res.n_ok;
        st.tested = res.tested;
        st.items = res.items;
        for (int a = 0; a < 3; ++a) st.cells[a] = res.cells[a];
    } else if (m > 0) {  // no bodies: every row is empty (a body centre was refused above: no index is < 0)
        if (bins) std::memset(bins, 0, sizeof(nb_radial_bin) * (size_t)m * nbins);
        if (heads)
            for (uint32_t j = 0; j < m; ++j) {
                nb_halo_head hd{};
                for (int a = 0; a < 3; ++a) {
                    hd.center[a] = params.centers[3 * (size_t)j + a];
                    hd.velocity[a] = params.velocities ? params.velocities[3 * (size_t)j + a] : 0.0;
                }
                heads[j] = hd;
            }
    }
    if (stats) *stats = st;
    return NB_OK;
}

}  // namespace nb
