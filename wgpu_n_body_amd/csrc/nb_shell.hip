// nb_shell.hip -- nb_shell_modes_sim: the spherical-harmonic sums of a simulator's current state per radial shell
// about a centre (include/nbody.h "Shell modes"; no reference counterpart).
//
// The frame of nb_modes.hip with another rule per body: one streaming classification, the shared sort, and per-list
// sums in a fixed order, with no host round trip:
//   key      -- one thread per body: the spherical r2 of nb_radial.hip about the centre (the explicit one, or the
//               diagnostics' centre of mass divided on the device), the branch-free binary search over the squared
//               edges in LDS; the key is 0 inside, k + 1 for bin k, nbins + 1 outside, nbins + 2 for a body that
//               does not count;
//   sort     -- nb_analysis_sort.hpp on as many 8-bit digits as nbins + 2 has: stable, so every list is in ascending
//               body index; then nb_assign.hpp's row starts and gather (position, velocity);
//   sums     -- the hot kernel.  A block of four waves owns a chunk of 4,096 places of one list (item_chunk), a wave
//               a run of 64 places at a time: it evaluates the direction once per body, loops over m outside and l
//               inside, carries c_m, s_m and the two live Q of the Legendre recurrence (with rates their dots too),
//               and sends every term through the butterfly as it is formed, so only a handful of partials are live;
//               field f of the run goes to LDS.  Then thread f adds the chunk's runs of field f left to right.  Every
//               body in one bin is n / 4,096 blocks, not one thread;
//   rows     -- one wave per list, lane f adds the chunks of field f left to right.
// The grids depend on n and nbins alone.  No atomics at all: the counts are differences of row starts.
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
constexpr uint32_t kWaves = kThreads / kWave;
constexpr uint32_t kChunk = NB_SHELL_CHUNK;  // places of a chunk: 64 runs of 64
constexpr uint32_t kRuns = kChunk / kWave;
constexpr uint32_t kMaxBins = NB_SHELL_MAX_BINS;
constexpr uint32_t kMaxRows = kMaxBins + 2;  // inside, the bins, outside
constexpr uint32_t kMaxFields = kWave;       // the sums, their rates, then mu r and mu u_r: one lane each
constexpr uint32_t kEdgeSlots = 512;         // squared edges in LDS, padded with +inf for the search
constexpr uint32_t kUsed = 8;                // res[0..6): the centre and velocity used; the rows from res[kUsed]

constexpr uint32_t shell_fields(uint32_t lmax, bool rates) { return (lmax + 1) * (lmax + 1) * (rates ? 2u : 1u) + 2u; }

static_assert(kChunk == kWave * kWave, "a chunk is 64 runs of one wave");
static_assert(shell_fields(NB_SHELL_MAX_L, false) <= kMaxFields && shell_fields(NB_SHELL_MAX_L_RATES, true) <= kMaxFields,
              "a field per lane: (lmax + 1)^2 (1 + rates) + 2 <= 64 sets the two limits of lmax");
static_assert(kMaxBins + 1 < kEdgeSlots, "the search covers every edge and ends in the padding");

struct ShellConst {
    double c[3], vc[3];         // explicit centre and velocity (center_com: not read)
    double n[3], e1[3], e2[3];  // axis_frame of the caller's axis
    uint32_t nbins, lmax, center_com;
};

__device__ inline bool row_is_bin(uint32_t r, uint32_t nbins) { return r >= 1 && r <= nbins; }

// d and the spherical r2 of nb_radial.hip's rule
__device__ inline double sphere_r2(float4 p, const double (&c)[3], double (&d)[3]) {
#pragma clang fp contract(off)
    d[0] = (double)p.x - c[0];
    d[1] = (double)p.y - c[1];
    d[2] = (double)p.z - c[2];
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

__device__ inline double dot3(const double (&a)[3], const double (&b)[3]) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// ---- key: one thread per body ------------------------------------------------------------------------------------
// mom: the finished moments of nb_diag.hip (center_com) or null.  e2g: nbins + 1 squared edges.  Block 0 also writes
// the centre and velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kThreads) void shell_key_kernel(const float4 *__restrict__ posm,
                                                             const float4 *__restrict__ vel, uint32_t n, ShellConst k,
                                                             const double *__restrict__ mom,
                                                             const double *__restrict__ e2g,
                                                             uint32_t *__restrict__ keys, double *__restrict__ used) {
    __shared__ double e2[kEdgeSlots];
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = tid; j < kEdgeSlots; j += kThreads) e2[j] = j <= k.nbins ? e2g[j] : INFINITY;
    double c[3], vc[3];
    centre_used(k.c, k.vc, k.center_com, mom, used, c, vc);
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kThreads + tid;
    if (i >= n) return;
    const float4 p = posm[i];
    uint32_t key = k.nbins + 2;
    if (body_ok(p, vel[i])) {
        double d[3];
        const double r2 = sphere_r2(p, c, d);
        uint32_t cnt = 0;  // edges at or below r2 (a NaN r2 -- a NaN centre -- is below every edge)
        for (uint32_t step = kEdgeSlots / 2; step > 0; step >>= 1)
            if (e2[cnt + step - 1] <= r2) cnt += step;
        key = min(cnt, k.nbins + 1);  // (only an infinite r2 reaches the padding)
    }
    keys[i] = key;
}

// ---- sums: one block per chunk of a list ----------------------------------------------------------------------------
// chunks[item][F]: item = the work item of item_chunk(row_start, nbins + 2, kChunk, ...), F = shell_fields(lmax, rates).
// One lane of the wave stores a run's total of a field: the butterfly leaves it in every lane.
template <bool kRates>
__global__ __launch_bounds__(kThreads) void shell_sum_kernel(const uint32_t *__restrict__ row_start,
                                                             const float4 *__restrict__ gpos,
                                                             const float4 *__restrict__ gvel, ShellConst k,
                                                             const double *__restrict__ used,
                                                             double *__restrict__ chunks) {
#pragma clang fp contract(off)
    __shared__ double run_total[kRuns][kMaxFields];
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, k.nbins + 2, kChunk, blockIdx.x, &r, &s, &a0, &a1)) return;  // (uniform over the block)
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const bool bin = row_is_bin(r, k.nbins);
    const uint32_t nk = (k.lmax + 1) * (k.lmax + 1), fields = shell_fields(k.lmax, kRates);
    const uint32_t llim = bin ? k.lmax : 0, live_fields = bin ? fields : 1;  // inside and outside: sum mu alone
    double c[3], vc[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = used[a];
        vc[a] = used[3 + a];
    }
    const uint32_t nruns = (a1 - a0 + kWave - 1) / kWave;
    for (uint32_t run = wave; run < nruns; run += kWaves) {
        double *total = run_total[run];
        const uint32_t p = a0 + run * kWave + lane;
        const bool live = p < a1;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), v = x;
        if (live) {
            x = gpos[p];
            v = gvel[p];
        }
        const double mu = x.w;
        double d[3];
        const double r2 = sphere_r2(x, c, d);
        const double u[3] = {(double)v.x - vc[0], (double)v.y - vc[1], (double)v.z - vc[2]};
        const double big_r = sqrt(r2);
        const bool centre = r2 == 0.0;  // counts in (0, 0) alone: every other term of it is +0
        double zeta = 0.0, alpha = 0.0, beta = 0.0, ur = 0.0;
        if (!centre) {
            zeta = dot3(d, k.n) / big_r;
            alpha = dot3(d, k.e1) / big_r;
            beta = dot3(d, k.e2) / big_r;
            ur = dot3(u, d) / big_r;
        }
        double zeta_d = 0.0, alpha_d = 0.0, beta_d = 0.0;
        if (kRates && !centre) {
            zeta_d = (dot3(u, k.n) - ur * zeta) / big_r;
            alpha_d = (dot3(u, k.e1) - ur * alpha) / big_r;
            beta_d = (dot3(u, k.e2) - ur * beta) / big_r;
        }
        const bool higher = live && !centre;  // (an absent place adds +0, whatever its terms would be)
        double cm = 1.0, sm = 0.0, cd = 0.0, sd = 0.0, qmm = 1.0;
        for (uint32_t m = 0; m <= llim; ++m) {
            if (m > 1) qmm = qmm * (double)(2 * m - 1);  // (2m - 1)!!, exact
            double q1 = 0.0, q2 = 0.0, qd1 = 0.0, qd2 = 0.0;  // Q_(l-1)^m, Q_(l-2)^m and their rates
            for (uint32_t l = m; l <= llim; ++l) {
                double q = qmm, qd = 0.0;
                if (l > m) {
                    const double f1 = (double)(2 * l - 1), f2 = (double)(l + m - 1), den = (double)(l - m);
                    q = ((f1 * zeta) * q1 - f2 * q2) / den;
                    if (kRates) qd = (f1 * (zeta_d * q1 + zeta * qd1) - f2 * qd2) / den;
                }
                const uint32_t i = l * l + (m ? 2 * m - 1 : 0);
                const bool on = l == 0 ? live : higher;
                const double tc = wave_sum(on ? mu * (q * cm) : 0.0);
                if (lane == 0) total[i] = tc;
                if (m) {
                    const double ts = wave_sum(on ? mu * (q * sm) : 0.0);
                    if (lane == 0) total[i + 1] = ts;
                }
                if (kRates) {
                    const double tdc = wave_sum(higher ? mu * (qd * cm + q * cd) : 0.0);
                    if (lane == 0) total[nk + i] = tdc;
                    if (m) {
                        const double tds = wave_sum(higher ? mu * (qd * sm + q * sd) : 0.0);
                        if (lane == 0) total[nk + i + 1] = tds;
                    }
                }
                q2 = q1;
                q1 = q;
                qd2 = qd1;
                qd1 = qd;
            }
            const double cn = cm * alpha - sm * beta, sn = sm * alpha + cm * beta;
            if (kRates) {
                const double cdn = (cd * alpha + cm * alpha_d) - (sd * beta + sm * beta_d);
                const double sdn = (sd * alpha + sm * alpha_d) + (cd * beta + cm * beta_d);
                cd = cdn;
                sd = sdn;
            }
            cm = cn;
            sm = sn;
        }
        if (bin) {
            const double t0 = wave_sum(live ? mu * big_r : 0.0), t1 = wave_sum(live ? mu * ur : 0.0);
            if (lane < 2) total[fields - 2 + lane] = lane == 0 ? t0 : t1;
        }
    }
    __syncthreads();
    if (tid < live_fields) {
        double sum = 0.0;
        for (uint32_t j = 0; j < nruns; ++j) sum += run_total[j][tid];
        chunks[(size_t)blockIdx.x * fields + tid] = sum;
    }
}

// ---- rows: one wave per list, lane f its field f ----------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void shell_rows_kernel(const uint32_t *__restrict__ row_start, uint32_t nbins,
                                                           uint32_t fields, const double *__restrict__ chunks,
                                                           double *__restrict__ rows) {
    const uint32_t r = blockIdx.x, f = threadIdx.x;
    if (f >= fields) return;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nch = (count + kChunk - 1) / kChunk;
    const double *mine = chunks + ((size_t)start / kChunk + r) * fields + f;
    double sum = 0.0;
    if (f < (row_is_bin(r, nbins) ? fields : 1u)) {
        constexpr uint32_t kBatch = 8;  // loads in flight; the additions stay in order
        uint32_t c = 0;
        for (; c + kBatch <= nch; c += kBatch) {
            double v[kBatch];
#pragma unroll
            for (uint32_t j = 0; j < kBatch; ++j) v[j] = mine[(size_t)(c + j) * fields];
#pragma unroll
            for (uint32_t j = 0; j < kBatch; ++j) sum += v[j];
        }
        for (; c < nch; ++c) sum += mine[(size_t)c * fields];
    }
    rows[(size_t)r * fields + f] = sum;
}

}  // namespace

struct ShellWork : Workspace {  // (all grow to the largest call so far)
    SortBufs<uint32_t> sort;        // the two sides of (key, body index), the histogram
    DeviceBuf<uint32_t> row_start;  // [kMaxRows + 1]
    DeviceBuf<AssignInfo> info;     // [1]: assign_rows_kernel's count of the counted bodies
    DeviceBuf<float4> gpos, gvel;   // [n]: in list order
    DeviceBuf<double> chunks;       // [n / 4096 + rows + 1][fields]
    DeviceBuf<double> res;          // [kUsed + kMaxRows * kMaxFields]
    DeviceBuf<double> e2;           // [kMaxBins + 1] squared edges
    PinnedBuf<double> h_res;        // as res
    PinnedBuf<double> h_e2;         // as e2
    PinnedBuf<uint32_t> h_row_start;  // as row_start
};

namespace {

template <class B>
int shell_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("shell_modes: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int sim_shell_modes(SimBase &sim, const nb_shell_params &params, nb_shell_head *out, nb_shell_bin *bins,
                    double *coef) {
    if (int rc = analysis_begin(sim, "shell_modes")) return rc;
    const uint32_t n = sim.n, nbins = params.nbins, lmax = params.lmax, rows = nbins + 2;
    const bool rates = (params.flags & NB_SHELL_RATES) != 0;
    const uint32_t fields = shell_fields(lmax, rates);
    const uint64_t items64 = (uint64_t)n / kChunk + rows + 1;
    if (n > 0x7fffffffu) {
        set_error("shell_modes: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    if (fields > kMaxFields) {  // (shell_check_params has passed it)
        set_error("shell_modes: lmax = %u needs %u fields, a wave has %u lanes", lmax, fields, kMaxFields);
        return NB_ERR_INVALID;
    }
    ShellWork *work = nullptr;
    if (int rc = workspace(sim, kWorkShell, &work, [](ShellWork &f) {
            if (int rc = shell_reserve(f.row_start, kMaxRows + 1)) return rc;
            if (int rc = shell_reserve(f.info, 1)) return rc;
            if (int rc = shell_reserve(f.res, kUsed + (size_t)kMaxRows * kMaxFields)) return rc;
            if (int rc = shell_reserve(f.e2, kMaxBins + 1)) return rc;
            if (int rc = shell_reserve(f.h_res, kUsed + (size_t)kMaxRows * kMaxFields)) return rc;
            if (int rc = shell_reserve(f.h_e2, kMaxBins + 1)) return rc;
            return shell_reserve(f.h_row_start, kMaxRows + 1);
        }))
        return rc;
    ShellWork &w = *work;
    const bool com = (params.flags & NB_SHELL_CENTER_COM) != 0;

    ShellConst k{};
    k.nbins = nbins;
    k.lmax = lmax;
    k.center_com = com;
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
    }
    if (!axis_frame(params.axis, k.n, k.e1, k.e2)) {  // (shell_check_params has passed it)
        set_error("shell_modes: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    for (uint32_t j = 0; j <= nbins; ++j) w.h_e2[j] = params.edges[j] * params.edges[j];

    const size_t res_count = kUsed + (size_t)rows * fields;
    std::memset(w.h_res, 0, sizeof(double) * res_count);
    std::memset(w.h_row_start, 0, sizeof(uint32_t) * (rows + 1));
    if (n > 0) {
        const auto reserve = [](auto &b, size_t count) { return shell_reserve(b, count); };
        const SortShape shape = sort_shape(n);
        if (int rc = w.sort.reserve(n, shape, reserve)) return rc;
        if (int rc = shell_reserve(w.gpos, n)) return rc;
        if (int rc = shell_reserve(w.gvel, n)) return rc;
        if (int rc = shell_reserve(w.chunks, (size_t)items64 * fields)) return rc;
        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        NB_HIP_TRY(hipMemcpyAsync(w.e2, w.h_e2, sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, sim.stream));
        const uint32_t blocks = (n + kThreads - 1) / kThreads, items = (uint32_t)items64;
        hipLaunchKernelGGL(shell_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, mom,
                           (const double *)w.e2, (uint32_t *)w.sort.keys[0], (double *)w.res);
        NB_HIP_TRY(hipGetLastError());
        const uint32_t passes = assign_passes(rows), side = passes & 1;  // (the largest key is `rows`)
        if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, passes, 0, nullptr)) return rc;
        uint32_t *row_start = w.row_start;
        hipLaunchKernelGGL(assign_rows_kernel, dim3(rows / kBlock + 1), dim3(kBlock), 0, sim.stream,
                           (const uint32_t *)w.sort.keys[side], n, rows, row_start, (AssignInfo *)w.info);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(assign_gather_kernel, dim3(blocks), dim3(kBlock), 0, sim.stream, (const uint32_t *)row_start,
                           rows, (const uint32_t *)w.sort.idx[side], posm, vel, (float4 *)w.gpos, (float4 *)w.gvel);
        NB_HIP_TRY(hipGetLastError());
        if (rates)
            hipLaunchKernelGGL(shell_sum_kernel<true>, dim3(items), dim3(kThreads), 0, sim.stream,
                               (const uint32_t *)row_start, (const float4 *)w.gpos, (const float4 *)w.gvel, k,
                               (const double *)w.res, (double *)w.chunks);
        else
            hipLaunchKernelGGL(shell_sum_kernel<false>, dim3(items), dim3(kThreads), 0, sim.stream,
                               (const uint32_t *)row_start, (const float4 *)w.gpos, (const float4 *)w.gvel, k,
                               (const double *)w.res, (double *)w.chunks);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(shell_rows_kernel, dim3(rows), dim3(kWave), 0, sim.stream, (const uint32_t *)row_start, nbins,
                           fields, (const double *)w.chunks, (double *)w.res + kUsed);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(double) * res_count, hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(w.h_row_start, w.row_start, sizeof(uint32_t) * (rows + 1), hipMemcpyDeviceToHost,
                                  sim.stream));
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    } else {
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        centre_used_empty(w.h_res, com, k.c, k.vc);
    }
    if (int rc = sim.diag_status()) return rc;

    const double *used = w.h_res, *row = w.h_res + kUsed;
    const uint32_t *start = w.h_row_start;
    nb_shell_head o{};
    o.step_num = sim.step_num;
    o.n = n;
    o.nonfinite = n - start[rows];
    o.inside_count = start[1] - start[0];
    o.outside_count = start[rows] - start[rows - 1];
    o.inside_mass = row[0];
    o.outside_mass = row[(size_t)(rows - 1) * fields];
    double mass = o.inside_mass;
    for (uint32_t j = 0; j < nbins; ++j) {
        const double *f = row + (size_t)(j + 1) * fields;
        mass += f[0];
        nb_shell_bin b{};
        b.count = start[j + 2] - start[j + 1];
        b.m_r = f[fields - 2];
        b.m_ur = f[fields - 1];
        bins[j] = b;
        std::memcpy(coef + (size_t)j * (fields - 2), f, sizeof(double) * (fields - 2));
    }
    o.mass = mass + o.outside_mass;
    for (int a = 0; a < 3; ++a) {
        o.center[a] = used[a];
        o.velocity[a] = used[3 + a];
        o.axis[a] = k.n[a];
        o.e1[a] = k.e1[a];
        o.e2[a] = k.e2[a];
    }
    o.nbins = nbins;
    o.lmax = lmax;
    o.flags = params.flags;
    *out = o;
    return NB_OK;
}

}  // namespace nb
