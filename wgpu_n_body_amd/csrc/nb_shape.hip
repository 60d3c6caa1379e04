// nb_shape.hip -- nb_sim_group_shapes: the shape tensor, the principal axes and the angular momentum of every row
// of a caller's assignment of bodies to rows, iterated inside a deforming ellipsoid (include/nbody.h "Group shapes",
// DESIGN.md 6n; no reference counterpart).
//
// The front end (nb_assign.hpp) leaves the counted members sorted by row -- position p of a member is its place in
// its row's list for the whole call -- with position, mass and velocity gathered into that order.  Then, with no
// host round trip:
//   init     -- one thread per row: the centre, frame velocity and radius the caller gave, the unit ellipsoid; a
//               row with no member is EMPTY at once;
//   sum      -- the hot path, one launch per round.  One wave per chunk of a row's list (item_chunk): every lane
//               rotates its member into the ellipsoid's frame, tests it and forms its 23 terms (the count and the 22
//               sums; +0 for a member that is not selected: masking, the positions never move), and each run of 64
//               positions goes through the butterfly into its run slot.  Round 0 is the same kernel with the radius
//               +inf about c = 0 or V = 0: its sums are the members' first moments, for a centre or a frame
//               velocity the caller did not give;
//   update   -- 32 lanes per row: lane f adds field f of the row's run slots in order, lane 0 then diagonalises
//               (nb_shape.hpp), decides the verdict and writes the next ellipsoid, or the finished row.  A finished
//               row raises its status and the counter: the later blocks of the row return at once, and every
//               block returns before any look-up once the counter has reached m;
//   scatter  -- selected_of from list order back to body order.
// All max_iter rounds are enqueued up front; the grids depend on n, m and the tuning alone.  Integer atomics only.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_assign.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_shape.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kFields = 23;    // the count, then the 22 sums in nb_shape_group's order
constexpr uint32_t kRowLanes = 32;  // lanes of the update per row: one per field, and idle ones
constexpr uint32_t kRowsPerBlock = kThreads / kRowLanes;
constexpr uint32_t kShaped = NB_SHAPE_CONVERGED | NB_SHAPE_UNCONVERGED;  // a row with a shape

static_assert(kFields <= kRowLanes && kWave % kRowLanes == 0, "a row's lanes lie in one wave");
static_assert(offsetof(nb_shape_group, mass) + (kFields - 1) * sizeof(double) == offsetof(nb_shape_group, lambda),
              "the 22 sums are consecutive doubles");

struct ShapeInfo {
    uint32_t finished;  // rows with a status
    uint32_t pad;
};

// a row between the rounds
struct ShapeRow {
    double c[3], v[3];  // centre and frame velocity
    double radius;      // R
    double q, s;        // of the round to come
    double e[9];        // its axes, e[3 k + j] = component j of axis k
    uint32_t status, pad;
};

__device__ inline bool all_done(const AssignInfo *ai, const ShapeInfo *si, uint32_t m) {
    return ai->invalid || __atomic_load_n(&si->finished, __ATOMIC_RELAXED) >= m;
}

__device__ inline void write_row(nb_shape_group *out, const ShapeRow &st, uint32_t count, uint32_t iterations,
                                 const double *sums, const double *lambda, const double *axes, double q, double s) {
    nb_shape_group o{};
    const double nan = __builtin_nan("");
    o.count = count;
    o.selected = sums ? (uint32_t)sums[0] : 0u;
    o.iterations = iterations;
    o.status = st.status;
    o.radius = st.radius;
    for (int a = 0; a < 3; ++a) {
        o.center[a] = st.c[a];
        o.velocity[a] = st.v[a];
        o.lambda[a] = lambda ? lambda[a] : nan;
    }
    for (int a = 0; a < 9; ++a) o.axes[a] = axes ? axes[a] : nan;
    double *dst = &o.mass;
    for (uint32_t f = 1; f < kFields; ++f) dst[f - 1] = sums ? sums[f] : 0.0;
    o.q = q;
    o.s = s;
    *out = o;
}

// ---- init ----------------------------------------------------------------------------------------------
// centers, velocities, radius: null for what the caller did not give (c = 0 and V = 0 then stand for round 0)
__global__ __launch_bounds__(kThreads) void shape_init_kernel(const AssignInfo *__restrict__ ai,
                                                              ShapeInfo *__restrict__ si,
                                                              const uint32_t *__restrict__ row_start, uint32_t m,
                                                              const double *__restrict__ centers,
                                                              const double *__restrict__ velocities,
                                                              const double *__restrict__ radius,
                                                              ShapeRow *__restrict__ rs,
                                                              nb_shape_group *__restrict__ rows) {
    if (ai->invalid) return;
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= m) return;
    ShapeRow st{};
    for (int a = 0; a < 3; ++a) {
        st.c[a] = centers ? centers[3 * r + a] : 0.0;
        st.v[a] = velocities ? velocities[3 * r + a] : 0.0;
        st.e[4 * a] = 1.0;
    }
    st.radius = radius ? radius[r] : INFINITY;
    st.q = st.s = 1.0;
    if (row_start[r + 1] == row_start[r]) {  // no member: no centre of mass either
        const double nan = __builtin_nan("");
        for (int a = 0; a < 3; ++a) {
            if (!centers) st.c[a] = nan;
            if (!velocities) st.v[a] = nan;
        }
        st.status = NB_SHAPE_EMPTY;
        write_row(&rows[r], st, 0u, 0u, nullptr, nullptr, nullptr, nan, nan);
        atomicAdd(&si->finished, 1u);
    }
    rs[r] = st;
}

// ---- sum: the hot path ---------------------------------------------------------------------------------
// kReduced: w = 1 / rho2 on the terms of T.  kMark: sel[p] = whether position p was selected, for selected_of.
template <bool kReduced, bool kMark>
__global__ __launch_bounds__(kWave) void shape_sum_kernel(const AssignInfo *__restrict__ ai,
                                                          const ShapeInfo *__restrict__ si,
                                                          const uint32_t *__restrict__ row_start, uint32_t m,
                                                          uint32_t chunk_len, const ShapeRow *__restrict__ rs,
                                                          const float4 *__restrict__ gpos,
                                                          const float4 *__restrict__ gvel, uint32_t round0,
                                                          unsigned char *__restrict__ sel,
                                                          double *__restrict__ runs) {
#pragma clang fp contract(off)
    if (all_done(ai, si, m)) return;
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, m, chunk_len, blockIdx.x, &r, &s, &a0, &a1)) return;
    const ShapeRow &st = rs[r];
    if (st.status) return;
    const uint32_t lane = threadIdx.x, start = row_start[r];
    const double cx = st.c[0], cy = st.c[1], cz = st.c[2], vx = st.v[0], vy = st.v[1], vz = st.v[2];
    const double big = round0 ? INFINITY : st.radius;
    const double ax1 = big, ax2 = big * st.q, ax3 = big * st.s;
    const double e0 = st.e[0], e1 = st.e[1], e2 = st.e[2], e3 = st.e[3], e4 = st.e[4], e5 = st.e[5], e6 = st.e[6],
                 e7 = st.e[7], e8 = st.e[8];
    for (uint32_t a = a0; a < a1; a += kWave) {  // (chunk_len is a multiple of 64: a - start too)
        const uint32_t p = a + lane;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), v = x;  // an absent position: never selected
        if (p < a1) {
            x = gpos[p];
            v = gvel[p];
        }
        const double mass = x.w;
        const double dx = (double)x.x - cx, dy = (double)x.y - cy, dz = (double)x.z - cz;
        const double ux = (double)v.x - vx, uy = (double)v.y - vy, uz = (double)v.z - vz;
        const double y1 = (e0 * dx + e1 * dy) + e2 * dz, y2 = (e3 * dx + e4 * dy) + e5 * dz,
                     y3 = (e6 * dx + e7 * dy) + e8 * dz;
        const double z1 = y1 / ax1, z2 = y2 / ax2, z3 = y3 / ax3;
        const double rho2 = (z1 * z1 + z2 * z2) + z3 * z3;
        const bool in = p < a1 && rho2 <= 1.0;  // (a NaN is not selected)
        double wm = mass;
        if (kReduced) wm = rho2 == 0.0 ? 0.0 : (1.0 / rho2) * mass;
        const double mdx = mass * dx, mdy = mass * dy, mdz = mass * dz;
        const double mux = mass * ux, muy = mass * uy, muz = mass * uz;
        const double wdx = wm * dx, wdy = wm * dy, wdz = wm * dz;
        double t[kFields] = {1.0,
                             mass,
                             mdx,
                             mdy,
                             mdz,
                             mux,
                             muy,
                             muz,
                             wdx * dx,
                             wdx * dy,
                             wdx * dz,
                             wdy * dy,
                             wdy * dz,
                             wdz * dz,
                             mux * ux,
                             mux * uy,
                             mux * uz,
                             muy * uy,
                             muy * uz,
                             muz * uz,
                             mass * (dy * uz - dz * uy),
                             mass * (dz * ux - dx * uz),
                             mass * (dx * uy - dy * ux)};
#pragma unroll
        for (uint32_t f = 0; f < kFields; ++f) t[f] = wave_sum(in ? t[f] : 0.0);
        if (lane < kFields) {
            double mine = t[0];
#pragma unroll
            for (uint32_t f = 1; f < kFields; ++f) mine = lane == f ? t[f] : mine;
            runs[(run_slot(start, r) + (a - start) / kWave) * kFields + lane] = mine;
        }
        if (kMark && p < a1) sel[p] = in;
    }
}

// ---- update: the verdict of round t (t = 0: the centre and the frame velocity of round 0) ---------------
__global__ __launch_bounds__(kThreads) void shape_update_kernel(const AssignInfo *__restrict__ ai,
                                                                ShapeInfo *__restrict__ si,
                                                                const uint32_t *__restrict__ row_start, uint32_t m,
                                                                const double *__restrict__ runs,
                                                                ShapeRow *__restrict__ rs,
                                                                nb_shape_group *__restrict__ rows, uint32_t t,
                                                                uint32_t com_centre, uint32_t com_velocity,
                                                                uint32_t max_iter, uint32_t min_members, double tol) {
#pragma clang fp contract(off)
    if (all_done(ai, si, m)) return;
    const size_t r = (size_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kRowLanes;
    if (r >= m) return;
    if (rs[r].status) return;  // (a row's 32 lanes leave together)
    const uint32_t f = threadIdx.x % kRowLanes;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nruns = (count + kWave - 1) / kWave;
    double mine = 0.0;
    if (f < kFields) {
        const double *p = runs + run_slot(start, (uint32_t)r) * kFields + f;
        for (uint32_t k = 0; k < nruns; ++k) mine += p[(size_t)k * kFields];
    }
    double sum[kFields];
    const int base = (int)((threadIdx.x % kWave) & ~(kRowLanes - 1));
#pragma unroll
    for (uint32_t k = 0; k < kFields; ++k) sum[k] = __shfl(mine, base + (int)k);
    if (f != 0) return;

    ShapeRow st = rs[r];
    if (t == 0) {
        for (int a = 0; a < 3; ++a) {
            if (com_centre) st.c[a] = sum[2 + a] / sum[1];
            if (com_velocity) st.v[a] = sum[5 + a] / sum[1];
        }
        rs[r] = st;
        return;
    }
    double lambda[3], axes[9];
    shape_eigen(&sum[8], lambda, axes);
    const double nan = __builtin_nan("");
    double q = nan, s = nan;
    const bool shaped = (uint32_t)sum[0] >= min_members && lambda[2] > 0.0 && isfinite(lambda[0]) &&
                        isfinite(lambda[1]) && isfinite(lambda[2]);
    if (!shaped) {
        st.status = NB_SHAPE_DEGENERATE;
    } else {
        q = sqrt(lambda[1] / lambda[0]);
        s = sqrt(lambda[2] / lambda[0]);
        if (st.radius == INFINITY) {
            st.status = NB_SHAPE_CONVERGED;
        } else {
            const double delta = fmax(fabs(q - st.q) / q, fabs(s - st.s) / s);
            if (t >= 2 && delta < tol) st.status = NB_SHAPE_CONVERGED;
            else if (t == max_iter) st.status = NB_SHAPE_UNCONVERGED;
        }
    }
    if (st.status) {
        write_row(&rows[r], st, count, t, sum, lambda, axes, q, s);
        atomicAdd(&si->finished, 1u);
    } else {
        st.q = q;
        st.s = s;
        for (int a = 0; a < 9; ++a) st.e[a] = axes[a];
    }
    rs[r] = st;
}

// ---- scatter: list order back to body order ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void shape_fill_kernel(uint32_t n, uint32_t *__restrict__ selected_of) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) selected_of[i] = NB_FOF_NONE;
}

__global__ __launch_bounds__(kThreads) void shape_scatter_kernel(const AssignInfo *__restrict__ ai,
                                                                 const uint32_t *__restrict__ row_start, uint32_t m,
                                                                 const uint32_t *__restrict__ idx,
                                                                 const uint32_t *__restrict__ row_of,
                                                                 const ShapeRow *__restrict__ rs,
                                                                 const unsigned char *__restrict__ sel,
                                                                 uint32_t *__restrict__ selected_of) {
    if (ai->invalid) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= row_start[m]) return;
    const uint32_t r = row_of[p];
    if (sel[p] && (rs[r].status & kShaped)) selected_of[idx[p]] = r;
}

}  // namespace

struct ShapeWork : Workspace {  // (all grow to the largest call so far)
    AssignBufs assign;
    DeviceBuf<double> in;               // centres, velocities [m][3] each, radii [m]
    DeviceBuf<double> runs;             // [run slots][kFields]
    DeviceBuf<ShapeRow> rs;             // [m]
    DeviceBuf<nb_shape_group> rows;     // [m]
    DeviceBuf<unsigned char> sel;       // [n]: in list order
    DeviceBuf<uint32_t> selected_of;    // [n]: in body order
    DeviceBuf<ShapeInfo> info;          // [1]
    PinnedBuf<double> h_in;
    PinnedBuf<nb_shape_group> h_rows;   // staged, so that a refused call leaves the outputs alone
    PinnedBuf<uint32_t> h_selected_of;
};

namespace {

template <class B>
int shape_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("group_shapes: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

template <bool kReduced>
void launch_sum(SimBase &sim, ShapeWork &w, uint32_t items, uint32_t m, bool mark, uint32_t round0) {
    const AssignBufs &ab = w.assign;
    if (mark)
        hipLaunchKernelGGL((shape_sum_kernel<kReduced, true>), dim3(items), dim3(kWave), 0, sim.stream,
                           (const AssignInfo *)ab.info, (const ShapeInfo *)w.info, (const uint32_t *)ab.row_start, m,
                           (uint32_t)sim.shape_chunk_len, (const ShapeRow *)w.rs, (const float4 *)ab.gpos,
                           (const float4 *)ab.gvel, round0, (unsigned char *)w.sel, (double *)w.runs);
    else
        hipLaunchKernelGGL((shape_sum_kernel<kReduced, false>), dim3(items), dim3(kWave), 0, sim.stream,
                           (const AssignInfo *)ab.info, (const ShapeInfo *)w.info, (const uint32_t *)ab.row_start, m,
                           (uint32_t)sim.shape_chunk_len, (const ShapeRow *)w.rs, (const float4 *)ab.gpos,
                           (const float4 *)ab.gvel, round0, (unsigned char *)w.sel, (double *)w.runs);
}

// the row of a call over no bodies
nb_shape_group empty_row(const double *c, const double *v, double radius) {
    nb_shape_group o{};
    const double nan = std::nan("");
    o.status = NB_SHAPE_EMPTY;
    o.radius = radius;
    for (int a = 0; a < 3; ++a) {
        o.center[a] = c ? c[a] : nan;
        o.velocity[a] = v ? v[a] : nan;
        o.lambda[a] = nan;
    }
    for (int a = 0; a < 9; ++a) o.axes[a] = nan;
    o.q = o.s = nan;
    return o;
}

}  // namespace

void shape_eigen_host(const double t[6], double lambda[3], double axes[9]) { shape_eigen(t, lambda, axes); }

int sim_group_shapes(SimBase &sim, const nb_shape_params &params, const uint32_t *group_of, size_t m_in,
                     const double *centers, const double *velocities, const double *radius, nb_shape_group *rows_out,
                     uint32_t *selected_of, nb_shape_stats *stats) {
    if (int rc = analysis_begin(sim, "group_shapes")) return rc;
    const uint32_t n = sim.n, m = (uint32_t)m_in;
    const uint32_t chunk = (uint32_t)sim.shape_chunk_len;
    const uint64_t items64 = (uint64_t)n / chunk + m + 1;
    if (n > 0x7fffffffu || items64 > 0x7fffffffu) {
        set_error("group_shapes: %u bodies in %u rows are more than one call takes", n, m);
        return NB_ERR_UNSUPPORTED;
    }
    ShapeWork *work = nullptr;
    if (int rc = workspace(sim, kWorkShape, &work, [](ShapeWork &f) { return shape_reserve(f.info, 1); })) return rc;
    ShapeWork &w = *work;
    AssignBufs &ab = w.assign;
    const bool launch = n > 0 && m > 0;

    if (n > 0) {
        const auto reserve = [](auto &b, size_t count) { return shape_reserve(b, count); };
        if (int rc = ab.reserve(n, m, reserve)) return rc;
        if (launch) {
            if (int rc = shape_reserve(w.in, 7 * (size_t)m)) return rc;
            if (int rc = shape_reserve(w.h_in, 7 * (size_t)m)) return rc;
            if (int rc = shape_reserve(w.runs, ((size_t)n / kWave + m + 1) * kFields)) return rc;
            if (int rc = shape_reserve(w.rs, m)) return rc;
            if (int rc = shape_reserve(w.rows, m)) return rc;
            if (int rc = shape_reserve(w.h_rows, m)) return rc;
            if (selected_of)
                if (int rc = shape_reserve(w.sel, n)) return rc;
        }
        if (selected_of) {
            if (int rc = shape_reserve(w.selected_of, n)) return rc;
            if (int rc = shape_reserve(w.h_selected_of, n)) return rc;
        }
        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        if (int rc = assign_enqueue(sim.stream, ab, group_of, n, m, posm, vel)) return rc;
        const uint32_t blocks = (n + kThreads - 1) / kThreads;
        if (selected_of) {
            hipLaunchKernelGGL(shape_fill_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, n,
                               (uint32_t *)w.selected_of);
            NB_HIP_TRY(hipGetLastError());
        }
        if (launch) {
            double *h_in = w.h_in, *d_in = w.in;
            const double *d_centers = nullptr, *d_vel = nullptr, *d_radius = nullptr;
            size_t used = 0;
            if (centers) {
                std::memcpy(h_in + used, centers, sizeof(double) * 3 * m);
                d_centers = d_in + used;
                used += 3 * (size_t)m;
            }
            if (velocities) {
                std::memcpy(h_in + used, velocities, sizeof(double) * 3 * m);
                d_vel = d_in + used;
                used += 3 * (size_t)m;
            }
            if (radius) {
                std::memcpy(h_in + used, radius, sizeof(double) * m);
                d_radius = d_in + used;
                used += m;
            }
            if (used) NB_HIP_TRY(hipMemcpyAsync(d_in, h_in, sizeof(double) * used, hipMemcpyHostToDevice, sim.stream));
            NB_HIP_TRY(hipMemsetAsync(w.info, 0, sizeof(ShapeInfo), sim.stream));

            const AssignInfo *ai = ab.info;
            const uint32_t *row_start = ab.row_start;
            const uint32_t items = (uint32_t)items64, row_blocks = (m + kThreads - 1) / kThreads,
                           update_blocks = (m + kRowsPerBlock - 1) / kRowsPerBlock;
            const bool reduced = (params.flags & NB_SHAPE_REDUCED) != 0, mark = selected_of != nullptr;
            hipLaunchKernelGGL(shape_init_kernel, dim3(row_blocks), dim3(kThreads), 0, sim.stream, ai,
                               (ShapeInfo *)w.info, row_start, m, d_centers, d_vel, d_radius, (ShapeRow *)w.rs,
                               (nb_shape_group *)w.rows);
            NB_HIP_TRY(hipGetLastError());
            for (uint32_t t = centers && velocities ? 1 : 0; t <= params.max_iter; ++t) {
                if (reduced) launch_sum<true>(sim, w, items, m, mark, t == 0);
                else launch_sum<false>(sim, w, items, m, mark, t == 0);
                NB_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(shape_update_kernel, dim3(update_blocks), dim3(kThreads), 0, sim.stream, ai,
                                   (ShapeInfo *)w.info, row_start, m, (const double *)w.runs, (ShapeRow *)w.rs,
                                   (nb_shape_group *)w.rows, t, centers ? 0u : 1u, velocities ? 0u : 1u,
                                   params.max_iter, params.min_members, params.tol);
                NB_HIP_TRY(hipGetLastError());
            }
            if (selected_of) {
                hipLaunchKernelGGL(shape_scatter_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, ai, row_start, m,
                                   ab.idx(), ab.rows(), (const ShapeRow *)w.rs, (const unsigned char *)w.sel,
                                   (uint32_t *)w.selected_of);
                NB_HIP_TRY(hipGetLastError());
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_rows, w.rows, sizeof(nb_shape_group) * m, hipMemcpyDeviceToHost, sim.stream));
        }
        if (selected_of)
            NB_HIP_TRY(hipMemcpyAsync(w.h_selected_of, w.selected_of, sizeof(uint32_t) * n, hipMemcpyDeviceToHost,
                                      sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(ab.h_info, ab.info, sizeof(AssignInfo), hipMemcpyDeviceToHost, sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;

    nb_shape_stats st{};
    st.step_num = sim.step_num;
    st.n = n;
    st.rows = m;
    const nb_shape_group *h_rows = nullptr;
    if (n > 0) {
        const AssignInfo res = *static_cast<const AssignInfo *>(ab.h_info);
        if (res.invalid) {
            set_error("group_shapes: group_of[%u] = %u is neither NB_FOF_NONE nor a row below %u (%u such values)",
                      res.first_invalid, group_of[res.first_invalid], m, res.invalid);
            return NB_ERR_INVALID;
        }
        st.members = res.members;  // (0 for m == 0: there is no list)
        st.nonfinite_members = res.nonfinite;
        if (selected_of) std::memcpy(selected_of, w.h_selected_of, sizeof(uint32_t) * n);
        if (launch) h_rows = w.h_rows;
    }
    for (uint32_t r = 0; r < m; ++r) {
        const nb_shape_group g = h_rows ? h_rows[r]
                                        : empty_row(centers ? centers + 3 * (size_t)r : nullptr,
                                                    velocities ? velocities + 3 * (size_t)r : nullptr,
                                                    radius ? radius[r] : INFINITY);
        if (rows_out) rows_out[r] = g;
        st.converged += g.status == NB_SHAPE_CONVERGED;
        st.unconverged += g.status == NB_SHAPE_UNCONVERGED;
        st.degenerate += g.status == NB_SHAPE_DEGENERATE;
        st.empty += g.status == NB_SHAPE_EMPTY;
        st.rounds_max = std::max(st.rounds_max, g.iterations);
    }
    if (stats) *stats = st;
    return NB_OK;
}

}  // namespace nb
