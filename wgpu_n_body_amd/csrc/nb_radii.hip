// nb_radii.hip -- nb_group_radii_sim: the exact mass radii, the extent and the peak of the circular-velocity curve of
// every row of a caller's assignment of bodies to rows (include/nbody.h "Group radii"; no reference
// counterpart).
//
// The front end (nb_assign.hpp) leaves the counted members sorted by row, each row's list in ascending body index,
// with position and mass gathered into that order.  Then, with no host round trip:
//   centre   -- only when the caller gave none: round 0 of nb_sim_group_shapes restated -- runs of 64 positions
//               through the fixed butterfly into run slots, a block per row adds the slots in order from 0, a wave
//               per field;
//   key      -- one thread per position: r2 about the row's centre, its bit pattern the 64-bit key; a position past
//               the members gets the largest key;
//   sort     -- nb_analysis_sort.hpp twice: the 64-bit key, then the row on assign_passes(m) digits.  Both are
//               stable, so a row's members end in (r2, body index) order at the row's own positions;
//   gather   -- r2, mass and body index into that order;
//   totals   -- one wave per chunk of 4,096 ranks: the sequential sum of every run of 64 (a 64-step read-lane
//               loop), the runs' totals T added in order: the chunk's total and the two terms it is made of;
//   prefix   -- one wave per row: A, the running sum of the totals of the chunks before, 64 chunks a batch through
//               the same read-lane loop, and the row's mass;
//   cross    -- one wave per chunk again: M(s) = (A + B) + C rebuilt per rank, the first rank of the chunk at
//               which each fraction is reached (wave ballots, integer minima) and the chunk's largest M / r (a
//               value and rank pair, ties to the smaller rank);
//   rows     -- one wave per row: the minima and the maximum over the row's chunks, the row;
//   scatter  -- rank and M from the sorted order back to body order.
// The grids depend on n and m alone.  Integer atomics only (the front end's); every value leaves by a vector store.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_assign.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kChunk = NB_RADII_CHUNK;  // ranks of a chunk: 64 runs of 64
constexpr uint32_t kComFields = 4;           // mass, m x, m y, m z
constexpr uint32_t kMaxF = NB_RADII_MAX_FRACTIONS;

static_assert(kChunk == kWave * kWave, "a chunk is one wave of runs of one wave");
static_assert(kMaxF <= kWave, "a fraction per lane");

// a chunk of a row between the kernels: slot = the work item of item_chunk(row_start, m, kChunk, ...)
struct RadiiChunk {
    double b_last, t_last;  // B and T of the chunk's last run: total = b_last + t_last
    double total;
    double a;               // A: the totals of the row's chunks before, in order
    double vx;              // the chunk's largest M / r ...
    uint32_t vrank;         // ... and its rank in the row (NB_FOF_NONE: no candidate)
    uint32_t pad;
    uint32_t cross[kMaxF];  // the first rank of the chunk with M >= f mass (NB_FOF_NONE: none)
};

// lane j's value on every lane (j uniform)
__device__ inline double lane_value(double v, uint32_t j) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// lane l: v_0 + v_1 + ... + v_l, added left to right starting from v_0 alone
__device__ inline double run_inclusive(double v, uint32_t lane) {
    double acc = lane_value(v, 0), mine = acc;
#pragma unroll
    for (uint32_t j = 1; j < kWave; ++j) {
        acc += lane_value(v, j);
        mine = lane == j ? acc : mine;
    }
    return mine;
}

// lane l: carry + v_0 + ... + v_(l - 1), added left to right starting from carry; *carry: the sum through v_63
__device__ inline double run_exclusive(double v, uint32_t lane, double *carry) {
    double acc = *carry, mine = acc;
#pragma unroll
    for (uint32_t j = 0; j < kWave; ++j) {
        mine = lane == j ? acc : mine;
        acc += lane_value(v, j);
    }
    *carry = acc;
    return mine;
}

// C of every rank of a chunk's run k (lane = rank - first rank of the run; an absent rank adds +0 after the last
// member) and, on every lane, T = C at the run's last member
__device__ inline double run_scan(const double *__restrict__ ms, uint32_t first, uint32_t a1, uint32_t lane,
                                  double *t) {
    const uint32_t p = first + lane;
    const double c = run_inclusive(p < a1 ? ms[p] : 0.0, lane);
    *t = lane_value(c, std::min(kWave, a1 - first) - 1);
    return c;
}

// ---- centre: round 0 of nb_sim_group_shapes (nb_shape.hip: shape_sum_kernel about c = 0 with R = +inf) ------
__global__ __launch_bounds__(kWave) void radii_com_sum_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                              const float4 *__restrict__ gpos,
                                                              double *__restrict__ runs) {
#pragma clang fp contract(off)
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, m, kChunk, blockIdx.x, &r, &s, &a0, &a1)) return;
    const uint32_t lane = threadIdx.x, start = row_start[r];
    for (uint32_t a = a0; a < a1; a += kWave) {
        const uint32_t p = a + lane;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < a1) x = gpos[p];
        const double mass = x.w;
        const double dx = (double)x.x - 0.0, dy = (double)x.y - 0.0, dz = (double)x.z - 0.0;
        const bool in = p < a1;
        const double t0 = wave_sum(in ? mass : 0.0), t1 = wave_sum(in ? mass * dx : 0.0),
                     t2 = wave_sum(in ? mass * dy : 0.0), t3 = wave_sum(in ? mass * dz : 0.0);
        if (lane < kComFields) {
            const double mine = lane == 0 ? t0 : lane == 1 ? t1 : lane == 2 ? t2 : t3;
            runs[(run_slot(start, r) + (a - start) / kWave) * kComFields + lane] = mine;
        }
    }
}

// one block per row, wave f its field f (mass, m x, m y, m z): the run slots added in order from 0, 64 slots a batch
// through read-lane, the next batch's loads in flight meanwhile; c = md / mass
__global__ __launch_bounds__(kComFields * kWave) void radii_com_row_kernel(const uint32_t *__restrict__ row_start,
                                                                           const double *__restrict__ runs,
                                                                           double *__restrict__ centre) {
#pragma clang fp contract(off)
    __shared__ double total[kComFields];
    const uint32_t r = blockIdx.x, lane = threadIdx.x % kWave, f = threadIdx.x / kWave;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nruns = (count + kWave - 1) / kWave;
    const double *p = runs + run_slot(start, r) * kComFields + f;
    double sum = 0.0;
    double next = lane < nruns ? p[(size_t)lane * kComFields] : 0.0;
    for (uint32_t k0 = 0; k0 < nruns; k0 += kWave) {
        const double v = next;
        const uint32_t ahead = k0 + kWave + lane;
        next = ahead < nruns ? p[(size_t)ahead * kComFields] : 0.0;
        if (nruns - k0 >= kWave) {
#pragma unroll
            for (uint32_t j = 0; j < kWave; ++j) sum += lane_value(v, j);
        } else {
            for (uint32_t j = 0; j < nruns - k0; ++j) sum += lane_value(v, j);
        }
    }
    if (lane == 0) total[f] = sum;
    __syncthreads();
    if (threadIdx.x < 3) centre[3 * (size_t)r + threadIdx.x] = total[1 + threadIdx.x] / total[0];  // (no member: 0 / 0)
}

// ---- key: r2 of every member about its row's centre --------------------------------------------------------
__global__ __launch_bounds__(kThreads) void radii_key_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                             uint32_t n, const uint32_t *__restrict__ row_of,
                                                             const float4 *__restrict__ gpos,
                                                             const double *__restrict__ centre,
                                                             uint64_t *__restrict__ keys) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    uint64_t key = ~0ull;  // past the members: stays at the end
    if (p < row_start[m]) {
        const double *c = centre + 3 * (size_t)row_of[p];
        const float4 x = gpos[p];
        const double dx = (double)x.x - c[0], dy = (double)x.y - c[1], dz = (double)x.z - c[2];
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        key = (uint64_t)__double_as_longlong(r2);
    }
    keys[p] = key;
}

// the row key of every position of the r2 order (m past the members, as the front end left it)
__global__ __launch_bounds__(kThreads) void radii_row_key_kernel(uint32_t n, const uint32_t *__restrict__ row_of,
                                                                 const uint32_t *__restrict__ by_r2,
                                                                 uint32_t *__restrict__ keys) {
    const size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (q < n) keys[q] = row_of[by_r2[q]];
}

// ---- gather: (row, r2, body) order ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void radii_gather_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                                const uint32_t *__restrict__ by_row,
                                                                const uint32_t *__restrict__ by_r2,
                                                                const uint64_t *__restrict__ r2_keys,
                                                                const uint32_t *__restrict__ idx,
                                                                const float4 *__restrict__ gpos,
                                                                double *__restrict__ r2s, double *__restrict__ ms,
                                                                uint32_t *__restrict__ body) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= row_start[m]) return;
    const uint32_t q = by_row[s], p = by_r2[q];
    r2s[s] = __longlong_as_double((long long)r2_keys[q]);
    ms[s] = (double)gpos[p].w;
    body[s] = idx[p];
}

// ---- totals ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void radii_totals_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                             const double *__restrict__ ms,
                                                             RadiiChunk *__restrict__ chunks) {
#pragma clang fp contract(off)
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, m, kChunk, blockIdx.x, &r, &s, &a0, &a1)) return;
    const uint32_t lane = threadIdx.x;
    double b = 0.0, b_last = 0.0, t_last = 0.0;  // B(k) = B(k - 1) + T(k - 1) from 0
    for (uint32_t first = a0; first < a1; first += kWave) {
        double t;
        (void)run_scan(ms, first, a1, lane, &t);
        b_last = b;
        t_last = t;
        b += t;
    }
    if (lane == 0) {
        RadiiChunk &c = chunks[blockIdx.x];
        c.b_last = b_last;
        c.t_last = t_last;
        c.total = b_last + t_last;
    }
}

// ---- prefix: one wave per row ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void radii_prefix_kernel(const uint32_t *__restrict__ row_start,
                                                             RadiiChunk *__restrict__ chunks,
                                                             double *__restrict__ row_mass) {
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nch = (count + kChunk - 1) / kChunk;
    RadiiChunk *mine = chunks + ((size_t)start / kChunk + r);
    if (count == 0) {
        if (lane == 0) row_mass[r] = 0.0;
        return;
    }
    double carry = 0.0;
    for (uint32_t c0 = 0; c0 < nch; c0 += kWave) {
        const uint32_t c = c0 + lane;
        const double a = run_exclusive(c < nch ? mine[c].total : 0.0, lane, &carry);
        if (c < nch) mine[c].a = a;
        if (c == nch - 1) row_mass[r] = (a + mine[c].b_last) + mine[c].t_last;
    }
}

// ---- cross: M per rank, the crossings and the v_max candidate of a chunk -------------------------------------
struct Fractions {
    double f[kMaxF];
};

__device__ inline bool better(double xa, uint32_t ra, double xb, uint32_t rb) {  // a before b
    return ra != NB_FOF_NONE && (rb == NB_FOF_NONE || xa > xb || (xa == xb && ra < rb));
}

__global__ __launch_bounds__(kWave) void radii_cross_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                            const double *__restrict__ ms,
                                                            const double *__restrict__ r2s,
                                                            const double *__restrict__ row_mass, Fractions fr,
                                                            uint32_t nf, uint32_t vmax_skip,
                                                            RadiiChunk *__restrict__ chunks,
                                                            double *__restrict__ enclosed) {
#pragma clang fp contract(off)
    uint32_t r, sc, a0, a1;
    if (!item_chunk(row_start, m, kChunk, blockIdx.x, &r, &sc, &a0, &a1)) return;
    const uint32_t lane = threadIdx.x, start = row_start[r];
    RadiiChunk &ch = chunks[blockIdx.x];
    const double a = ch.a, mass = row_mass[r];
    double frac = 0.0;  // lane f: fraction f and its threshold
#pragma unroll
    for (uint32_t f = 0; f < kMaxF; ++f) frac = lane == f ? fr.f[f] : frac;
    const double thr = frac * mass;
    uint32_t found = NB_FOF_NONE;  // lane f: the chunk's first rank at or past thr

    double b = 0.0;  // B of the run: the T of the chunk's runs before, in order from 0
    double best_x = 0.0;
    uint32_t best_rank = NB_FOF_NONE;
    for (uint32_t first = a0; first < a1; first += kWave) {
        double t;
        const double c = run_scan(ms, first, a1, lane, &t);
        const uint32_t p = first + lane, rank = p - start;
        const bool live = p < a1;
        const double big_m = (a + b) + c;
        b += t;
        if (live && enclosed) enclosed[p] = big_m;
        for (uint32_t f = 0; f < nf; ++f) {
            const unsigned long long hit = __ballot(live && big_m >= lane_value(thr, f));
            if (hit && lane == f && found == NB_FOF_NONE) found = (first - start) + (uint32_t)__builtin_ctzll(hit);
        }
        if (live && rank >= vmax_skip) {
            const double r2 = r2s[p];
            if (r2 > 0.0) {
                const double x = big_m / sqrt(r2);
                if (x == x && (best_rank == NB_FOF_NONE || x > best_x)) {  // (a NaN is passed over)
                    best_x = x;
                    best_rank = rank;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ox = __shfl_xor(best_x, o);
        const uint32_t orank = __shfl_xor(best_rank, o);
        if (better(ox, orank, best_x, best_rank)) {
            best_x = ox;
            best_rank = orank;
        }
    }
    if (lane < kMaxF) ch.cross[lane] = found;
    if (lane == 0) {
        ch.vx = best_x;
        ch.vrank = best_rank;
    }
}

// ---- rows: one wave per row -------------------------------------------------------------------------------------
// lane l takes the row's chunks l, l + 64, ...; minima and the best pair are exact in any order
__global__ __launch_bounds__(kWave) void radii_rows_kernel(const uint32_t *__restrict__ row_start,
                                                           const RadiiChunk *__restrict__ chunks,
                                                           const double *__restrict__ centre,
                                                           const double *__restrict__ row_mass,
                                                           const double *__restrict__ r2s,
                                                           const uint32_t *__restrict__ body, uint32_t nf,
                                                           nb_radii_group *__restrict__ rows) {
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nch = (count + kChunk - 1) / kChunk;
    const RadiiChunk *mine = chunks + ((size_t)start / kChunk + r);
    double vx = 0.0;
    uint32_t vrank = NB_FOF_NONE, cross[kMaxF];
#pragma unroll
    for (uint32_t f = 0; f < kMaxF; ++f) cross[f] = NB_FOF_NONE;
    for (uint32_t c = lane; c < nch; c += kWave) {
        const RadiiChunk &ch = mine[c];
        if (better(ch.vx, ch.vrank, vx, vrank)) {
            vx = ch.vx;
            vrank = ch.vrank;
        }
#pragma unroll
        for (uint32_t f = 0; f < kMaxF; ++f) cross[f] = min(cross[f], ch.cross[f]);
    }
    uint32_t s = NB_FOF_NONE;  // lane f: the crossing of fraction f
    for (int o = 32; o > 0; o >>= 1) {
        const double ox = __shfl_xor(vx, o);
        const uint32_t orank = __shfl_xor(vrank, o);
        if (better(ox, orank, vx, vrank)) {
            vx = ox;
            vrank = orank;
        }
    }
#pragma unroll
    for (uint32_t f = 0; f < kMaxF; ++f) {
        uint32_t v = cross[f];
        for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
        s = lane == f ? v : s;
    }
    const double nan = __builtin_nan("");
    nb_radii_group &o = rows[r];
    if (lane < kMaxF) {
        if (lane >= nf) s = NB_FOF_NONE;
        o.radius[lane] = s != NB_FOF_NONE ? sqrt(r2s[start + s]) : nan;
        o.index[lane] = s != NB_FOF_NONE ? body[start + s] : NB_FOF_NONE;
    }
    if (lane != 0) return;
    o.count = count;
    for (int a = 0; a < 3; ++a) o.center[a] = centre[3 * (size_t)r + a];
    o.mass = row_mass[r];
    o.r_min = count ? sqrt(r2s[start]) : nan;
    o.r_max = count ? sqrt(r2s[start + count - 1]) : nan;
    o.vc2_max = vrank != NB_FOF_NONE ? vx : nan;
    o.r_vmax = vrank != NB_FOF_NONE ? sqrt(r2s[start + vrank]) : nan;
    o.vmax_index = vrank != NB_FOF_NONE ? body[start + vrank] : NB_FOF_NONE;
}

// ---- scatter: the sorted order back to body order ----------------------------------------------------------
__global__ __launch_bounds__(kThreads) void radii_fill_kernel(uint32_t n, uint32_t *__restrict__ rank_of,
                                                              double *__restrict__ enclosed_of) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    rank_of[i] = NB_FOF_NONE;
    enclosed_of[i] = __builtin_nan("");
}

// (the lists are well formed whatever group_of holds: a value that is no row has the key m, and the host refuses)
__global__ __launch_bounds__(kThreads) void radii_scatter_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                                 const uint32_t *__restrict__ row_of,
                                                                 const uint32_t *__restrict__ body,
                                                                 const double *__restrict__ enclosed,
                                                                 uint32_t *__restrict__ rank_of,
                                                                 double *__restrict__ enclosed_of) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= row_start[m]) return;
    const uint32_t b = body[s];
    rank_of[b] = (uint32_t)s - row_start[row_of[s]];
    enclosed_of[b] = enclosed[s];
}

}  // namespace

struct RadiiWork : Workspace {  // (all grow to the largest call so far)
    AssignBufs assign;
    SortBufs<uint64_t> by_r2;        // the r2 keys and the list positions
    SortBufs<uint32_t> by_row;       // the row keys and the positions of the r2 order
    DeviceBuf<double> centre;        // [m][3]
    DeviceBuf<double> runs;          // [run slots][kComFields]: the centre's sums
    DeviceBuf<double> r2s, ms;       // [n]: in (row, r2, body) order
    DeviceBuf<uint32_t> body;        // [n]
    DeviceBuf<double> enclosed;      // [n]: M, in the same order
    DeviceBuf<RadiiChunk> chunks;    // [n / 4096 + m + 1]
    DeviceBuf<double> row_mass;      // [m]
    DeviceBuf<nb_radii_group> rows;  // [m]
    DeviceBuf<uint32_t> rank_of;     // [n]: in body order
    DeviceBuf<double> enclosed_of;   // [n]
    PinnedBuf<double> h_centre;
    PinnedBuf<nb_radii_group> h_rows;  // staged, so that a refused call leaves the outputs alone
    PinnedBuf<uint32_t> h_rank_of;
    PinnedBuf<double> h_enclosed_of;
};

namespace {

template <class B>
int radii_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("group_radii: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

// the row of a call over no bodies
nb_radii_group empty_row(const double *c) {
    nb_radii_group o{};
    const double nan = std::nan("");
    for (int a = 0; a < 3; ++a) o.center[a] = c ? c[a] : nan;
    o.r_min = o.r_max = o.vc2_max = o.r_vmax = nan;
    o.vmax_index = NB_FOF_NONE;
    for (uint32_t f = 0; f < kMaxF; ++f) {
        o.radius[f] = nan;
        o.index[f] = NB_FOF_NONE;
    }
    return o;
}

}  // namespace

int sim_group_radii(SimBase &sim, const nb_radii_params &params, const uint32_t *group_of, size_t m_in,
                    const double *centers, nb_radii_group *rows_out, uint32_t *rank_of, double *enclosed_of,
                    nb_radii_stats *stats) {
    if (int rc = analysis_begin(sim, "group_radii")) return rc;
    const uint32_t n = sim.n, m = (uint32_t)m_in;
    const uint64_t items64 = (uint64_t)n / kChunk + m + 1;
    if (n > 0x7fffffffu || items64 > 0x7fffffffu) {
        set_error("group_radii: %u bodies in %u rows are more than one call takes", n, m);
        return NB_ERR_UNSUPPORTED;
    }
    RadiiWork *work = nullptr;
    if (int rc = workspace(sim, kWorkRadii, &work, [](RadiiWork &) { return (int)NB_OK; })) return rc;
    RadiiWork &w = *work;
    AssignBufs &ab = w.assign;
    const bool launch = n > 0 && m > 0, per_body = rank_of || enclosed_of;

    if (n > 0) {
        const auto reserve = [](auto &b, size_t count) { return radii_reserve(b, count); };
        if (int rc = ab.reserve(n, m, reserve)) return rc;
        const SortShape shape = sort_shape(n);
        if (launch) {
            if (int rc = w.by_r2.reserve(n, shape, reserve)) return rc;
            if (int rc = w.by_row.reserve(n, shape, reserve)) return rc;
            if (int rc = radii_reserve(w.centre, 3 * (size_t)m)) return rc;
            if (int rc = radii_reserve(w.h_centre, 3 * (size_t)m)) return rc;
            if (!centers)
                if (int rc = radii_reserve(w.runs, ((size_t)n / kWave + m + 1) * kComFields)) return rc;
            if (int rc = radii_reserve(w.r2s, n)) return rc;
            if (int rc = radii_reserve(w.ms, n)) return rc;
            if (int rc = radii_reserve(w.body, n)) return rc;
            if (per_body)
                if (int rc = radii_reserve(w.enclosed, n)) return rc;
            if (int rc = radii_reserve(w.chunks, (size_t)items64)) return rc;
            if (int rc = radii_reserve(w.row_mass, m)) return rc;
            if (int rc = radii_reserve(w.rows, m)) return rc;
            if (int rc = radii_reserve(w.h_rows, m)) return rc;
        }
        if (per_body) {
            if (int rc = radii_reserve(w.rank_of, n)) return rc;
            if (int rc = radii_reserve(w.enclosed_of, n)) return rc;
            if (int rc = radii_reserve(w.h_rank_of, n)) return rc;
            if (int rc = radii_reserve(w.h_enclosed_of, n)) return rc;
        }
        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        if (int rc = assign_enqueue(sim.stream, ab, group_of, n, m, posm, vel)) return rc;
        const uint32_t blocks = (n + kThreads - 1) / kThreads;
        if (per_body) {
            hipLaunchKernelGGL(radii_fill_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, n,
                               (uint32_t *)w.rank_of, (double *)w.enclosed_of);
            NB_HIP_TRY(hipGetLastError());
        }
        if (launch) {
            const uint32_t *row_start = ab.row_start;
            const uint32_t items = (uint32_t)items64;
            double *centre = w.centre;
            if (centers) {
                std::memcpy(w.h_centre, centers, sizeof(double) * 3 * m);
                NB_HIP_TRY(hipMemcpyAsync(centre, w.h_centre, sizeof(double) * 3 * m, hipMemcpyHostToDevice,
                                          sim.stream));
            } else {
                hipLaunchKernelGGL(radii_com_sum_kernel, dim3(items), dim3(kWave), 0, sim.stream, row_start, m,
                                   (const float4 *)ab.gpos, (double *)w.runs);
                NB_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(radii_com_row_kernel, dim3(m), dim3(kComFields * kWave), 0, sim.stream, row_start,
                                   (const double *)w.runs, centre);
                NB_HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(radii_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, row_start, m, n,
                               ab.rows(), (const float4 *)ab.gpos, (const double *)centre,
                               (uint64_t *)w.by_r2.keys[0]);
            NB_HIP_TRY(hipGetLastError());
            constexpr uint32_t kKeyPasses = 8;  // (even: the r2 order ends on side 0)
            if (int rc = enqueue_sort(sim.stream, w.by_r2, n, shape, kKeyPasses, 0, nullptr)) return rc;
            hipLaunchKernelGGL(radii_row_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, n, ab.rows(),
                               (const uint32_t *)w.by_r2.idx[0], (uint32_t *)w.by_row.keys[0]);
            NB_HIP_TRY(hipGetLastError());
            const uint32_t row_passes = assign_passes(m), side = row_passes & 1;
            if (int rc = enqueue_sort(sim.stream, w.by_row, n, shape, row_passes, 0, nullptr)) return rc;
            hipLaunchKernelGGL(radii_gather_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, row_start, m,
                               (const uint32_t *)w.by_row.idx[side], (const uint32_t *)w.by_r2.idx[0],
                               (const uint64_t *)w.by_r2.keys[0], ab.idx(), (const float4 *)ab.gpos,
                               (double *)w.r2s, (double *)w.ms, (uint32_t *)w.body);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(radii_totals_kernel, dim3(items), dim3(kWave), 0, sim.stream, row_start, m,
                               (const double *)w.ms, (RadiiChunk *)w.chunks);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(radii_prefix_kernel, dim3(m), dim3(kWave), 0, sim.stream, row_start,
                               (RadiiChunk *)w.chunks, (double *)w.row_mass);
            NB_HIP_TRY(hipGetLastError());
            Fractions fr{};
            for (uint32_t f = 0; f < params.nf; ++f) fr.f[f] = params.fractions[f];
            hipLaunchKernelGGL(radii_cross_kernel, dim3(items), dim3(kWave), 0, sim.stream, row_start, m,
                               (const double *)w.ms, (const double *)w.r2s, (const double *)w.row_mass, fr, params.nf,
                               params.vmax_skip, (RadiiChunk *)w.chunks, per_body ? (double *)w.enclosed : nullptr);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(radii_rows_kernel, dim3(m), dim3(kWave), 0, sim.stream, row_start,
                               (const RadiiChunk *)w.chunks, (const double *)centre,
                               (const double *)w.row_mass, (const double *)w.r2s, (const uint32_t *)w.body, params.nf,
                               (nb_radii_group *)w.rows);
            NB_HIP_TRY(hipGetLastError());
            if (per_body) {
                hipLaunchKernelGGL(radii_scatter_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, row_start, m, (const uint32_t *)w.by_row.keys[side],
                                   (const uint32_t *)w.body, (const double *)w.enclosed, (uint32_t *)w.rank_of,
                                   (double *)w.enclosed_of);
                NB_HIP_TRY(hipGetLastError());
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_rows, w.rows, sizeof(nb_radii_group) * m, hipMemcpyDeviceToHost, sim.stream));
        }
        if (rank_of)
            NB_HIP_TRY(hipMemcpyAsync(w.h_rank_of, w.rank_of, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (enclosed_of)
            NB_HIP_TRY(hipMemcpyAsync(w.h_enclosed_of, w.enclosed_of, sizeof(double) * n, hipMemcpyDeviceToHost,
                                      sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(ab.h_info, ab.info, sizeof(AssignInfo), hipMemcpyDeviceToHost, sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;

    nb_radii_stats st{};
    st.step_num = sim.step_num;
    st.n = n;
    st.rows = m;
    const nb_radii_group *h_rows = nullptr;
    if (n > 0) {
        const AssignInfo res = *static_cast<const AssignInfo *>(ab.h_info);
        if (res.invalid) {
            set_error("group_radii: group_of[%u] = %u is neither NB_FOF_NONE nor a row below %u (%u such values)",
                      res.first_invalid, group_of[res.first_invalid], m, res.invalid);
            return NB_ERR_INVALID;
        }
        st.members = res.members;  // (0 for m == 0: there is no list)
        st.nonfinite_members = res.nonfinite;
        if (rank_of) std::memcpy(rank_of, w.h_rank_of, sizeof(uint32_t) * n);
        if (enclosed_of) std::memcpy(enclosed_of, w.h_enclosed_of, sizeof(double) * n);
        if (launch) h_rows = w.h_rows;
    }
    for (uint32_t r = 0; r < m; ++r) {
        const nb_radii_group g = h_rows ? h_rows[r] : empty_row(centers ? centers + 3 * (size_t)r : nullptr);
        if (rows_out) rows_out[r] = g;
        st.empty += g.count == 0;
    }
    if (stats) *stats = st;
    return NB_OK;
}

}  // namespace nb
