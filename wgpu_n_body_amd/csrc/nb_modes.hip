// nb_modes.hip -- nb_disc_modes_sim: the azimuthal Fourier sums of a simulator's current state per annulus about an
// axis (include/nbody.h "Disc modes"; no reference counterpart).
//
// One streaming classification, the shared sort, and per-list sums in a fixed order, with no host round trip:
//   key      -- one thread per body: the cylindrical r2 of nb_radial.hip about the centre (the explicit one, or the
//               diagnostics' centre of mass divided on the device), a branch-free binary search over the squared
//               edges in LDS; the key is 0 inside, k + 1 for bin k, nbins + 1 outside, nbins + 2 for a body that
//               does not count;
//   sort     -- nb_analysis_sort.hpp on as many 8-bit digits as nbins + 2 has, known on the host: stable, so every
//               list is in ascending body index; then nb_assign.hpp's row starts and gather (position, velocity);
//   sums     -- the hot kernel.  A block of four waves owns a chunk of 4,096 places of one list (item_chunk), a wave
//               a run of 64 places at a time: it evaluates the rule once per body, loops over m with the
//               recurrence and carries the six terms of the mode through the butterfly, so no more than six
//               partials are live; lane f keeps field f of the run in LDS.  Then thread f adds the chunk's runs
//               of field f left to right.  Every body in one bin is n / 4,096 blocks, not one thread;
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
constexpr uint32_t kChunk = NB_MODES_CHUNK;  // places of a chunk: 64 runs of 64
constexpr uint32_t kRuns = kChunk / kWave;
constexpr uint32_t kMaxBins = NB_MODES_MAX_BINS;
constexpr uint32_t kMaxRows = kMaxBins + 2;  // inside, the bins, outside
constexpr uint32_t kTerms = NB_MODES_FIELDS;
constexpr uint32_t kMaxFields = kTerms * (NB_MODES_MAX_M + 1) + 2;  // the modes, then mu R and (mu h) h
constexpr uint32_t kEdgeSlots = 512;  // squared edges in LDS, padded with +inf for the search
constexpr uint32_t kUsed = 8;         // res[0..6): the centre and velocity used; the rows from res[kUsed]

static_assert(kChunk == kWave * kWave && kMaxFields <= kWave, "a chunk is 64 runs of one wave; a field per lane");
static_assert(kMaxBins + 1 < kEdgeSlots, "the search covers every edge and ends in the padding");

struct ModesConst {
    double c[3], vc[3];          // explicit centre and velocity (center_com: not read)
    double n[3], e1[3], e2[3];   // axis_frame of the caller's axis
    uint32_t nbins, mmax, center_com;
};

// the fields of a list's row: a bin has all of them, inside and outside mode 0 alone
__device__ inline bool row_is_bin(uint32_t r, uint32_t nbins) { return r >= 1 && r <= nbins; }

// d, and the height h and the cylindrical r2 of nb_radial.hip's rule; q = d - h n
__device__ inline double plane_r2(float4 p, const double (&c)[3], const ModesConst &k, double (&q)[3], double *h_out) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    const double h = (dx * k.n[0] + dy * k.n[1]) + dz * k.n[2];
    q[0] = dx - h * k.n[0];
    q[1] = dy - h * k.n[1];
    q[2] = dz - h * k.n[2];
    *h_out = h;
    return (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
}

// ---- key: one thread per body ------------------------------------------------------------------------------------
// mom: the finished moments of nb_diag.hip (center_com) or null.  e2g: nbins + 1 squared edges.  Block 0 also writes
// the centre and velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kThreads) void modes_key_kernel(const float4 *__restrict__ posm,
                                                             const float4 *__restrict__ vel, uint32_t n, ModesConst k,
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
        double q[3], h;
        const double r2 = plane_r2(p, c, k, q, &h);
        uint32_t cnt = 0;  // edges at or below r2 (a NaN r2 -- a NaN centre -- is below every edge)
        for (uint32_t step = kEdgeSlots / 2; step > 0; step >>= 1)
            if (e2[cnt + step - 1] <= r2) cnt += step;
        key = min(cnt, k.nbins + 1);  // (only an infinite r2 reaches the padding)
    }
    keys[i] = key;
}

// ---- sums: one block per chunk of a list ----------------------------------------------------------------------------
// chunks[item][F]: item = the work item of item_chunk(row_start, nbins + 2, kChunk, ...), F = 6 (mmax + 1) + 2
__global__ __launch_bounds__(kThreads) void modes_sum_kernel(const uint32_t *__restrict__ row_start,
                                                             const float4 *__restrict__ gpos,
                                                             const float4 *__restrict__ gvel, ModesConst k,
                                                             const double *__restrict__ used,
                                                             double *__restrict__ chunks) {
#pragma clang fp contract(off)
    __shared__ double run_total[kRuns][kMaxFields];
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, k.nbins + 2, kChunk, blockIdx.x, &r, &s, &a0, &a1)) return;  // (uniform over the block)
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const bool bin = row_is_bin(r, k.nbins);
    const uint32_t mlim = bin ? k.mmax : 0, fields = kTerms * (k.mmax + 1) + 2, live_fields = bin ? fields : kTerms;
    double c[3], vc[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = used[a];
        vc[a] = used[3 + a];
    }
    const uint32_t nruns = (a1 - a0 + kWave - 1) / kWave;
    for (uint32_t run = wave; run < nruns; run += kWaves) {
        const uint32_t p = a0 + run * kWave + lane;
        const bool live = p < a1;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), v = x;
        if (live) {
            x = gpos[p];
            v = gvel[p];
        }
        const double mu = x.w;
        double q[3], h;
        const double r2 = plane_r2(x, c, k, q, &h);
        const double ux = (double)v.x - vc[0], uy = (double)v.y - vc[1], uz = (double)v.z - vc[2];
        const double a = (q[0] * k.e1[0] + q[1] * k.e1[1]) + q[2] * k.e1[2];
        const double b = (q[0] * k.e2[0] + q[1] * k.e2[1]) + q[2] * k.e2[2];
        const double ua = (ux * k.e1[0] + uy * k.e1[1]) + uz * k.e1[2];
        const double ub = (ux * k.e2[0] + uy * k.e2[1]) + uz * k.e2[2];
        const double big_r = sqrt(r2);
        double c1 = 0.0, s1 = 0.0, w = 0.0;
        if (r2 != 0.0) {
            c1 = a / big_r;
            s1 = b / big_r;
            w = (a * ub - b * ua) / r2;
        }
        const double muw = mu * w, muh = mu * h;
        double cm = 1.0, sm = 0.0;
        for (uint32_t m = 0; m <= mlim; ++m) {  // (an absent place adds +0, whatever its terms would be)
            const double t0 = wave_sum(live ? mu * cm : 0.0), t1 = wave_sum(live ? mu * sm : 0.0);
            const double t2 = wave_sum(live ? muw * cm : 0.0), t3 = wave_sum(live ? muw * sm : 0.0);
            const double t4 = wave_sum(live ? muh * cm : 0.0), t5 = wave_sum(live ? muh * sm : 0.0);
            if (lane < kTerms)
                run_total[run][kTerms * m + lane] =
                    lane == 0 ? t0 : lane == 1 ? t1 : lane == 2 ? t2 : lane == 3 ? t3 : lane == 4 ? t4 : t5;
            const double cn = cm * c1 - sm * s1, sn = sm * c1 + cm * s1;
            cm = cn;
            sm = sn;
        }
        if (bin) {
            const double t0 = wave_sum(live ? mu * big_r : 0.0), t1 = wave_sum(live ? muh * h : 0.0);
            if (lane < 2) run_total[run][fields - 2 + lane] = lane == 0 ? t0 : t1;
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
__global__ __launch_bounds__(kWave) void modes_rows_kernel(const uint32_t *__restrict__ row_start, uint32_t nbins,
                                                           uint32_t fields, const double *__restrict__ chunks,
                                                           double *__restrict__ rows) {
    const uint32_t r = blockIdx.x, f = threadIdx.x;
    if (f >= fields) return;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nch = (count + kChunk - 1) / kChunk;
    const double *mine = chunks + ((size_t)start / kChunk + r) * fields + f;
    double sum = 0.0;
    if (f < (row_is_bin(r, nbins) ? fields : kTerms)) {
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

struct ModesWork : Workspace {  // (all grow to the largest call so far)
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
int modes_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("disc_modes: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int sim_disc_modes(SimBase &sim, const nb_modes_params &params, nb_modes_head *out, nb_modes_bin *bins,
                   double *modes) {
    if (int rc = analysis_begin(sim, "disc_modes")) return rc;
    const uint32_t n = sim.n, nbins = params.nbins, mmax = params.mmax, rows = nbins + 2;
    const uint32_t fields = kTerms * (mmax + 1) + 2;
    const uint64_t items64 = (uint64_t)n / kChunk + rows + 1;
    if (n > 0x7fffffffu) {
        set_error("disc_modes: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    ModesWork *work = nullptr;
    if (int rc = workspace(sim, kWorkModes, &work, [](ModesWork &f) {
            if (int rc = modes_reserve(f.row_start, kMaxRows + 1)) return rc;
            if (int rc = modes_reserve(f.info, 1)) return rc;
            if (int rc = modes_reserve(f.res, kUsed + (size_t)kMaxRows * kMaxFields)) return rc;
            if (int rc = modes_reserve(f.e2, kMaxBins + 1)) return rc;
            if (int rc = modes_reserve(f.h_res, kUsed + (size_t)kMaxRows * kMaxFields)) return rc;
            if (int rc = modes_reserve(f.h_e2, kMaxBins + 1)) return rc;
            return modes_reserve(f.h_row_start, kMaxRows + 1);
        }))
        return rc;
    ModesWork &w = *work;
    const bool com = (params.flags & NB_MODES_CENTER_COM) != 0;

    ModesConst k{};
    k.nbins = nbins;
    k.mmax = mmax;
    k.center_com = com;
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
    }
    if (!axis_frame(params.axis, k.n, k.e1, k.e2)) {  // (modes_check_params has passed it)
        set_error("disc_modes: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    for (uint32_t j = 0; j <= nbins; ++j) w.h_e2[j] = params.edges[j] * params.edges[j];

    const size_t res_count = kUsed + (size_t)rows * fields;
    std::memset(w.h_res, 0, sizeof(double) * res_count);
    std::memset(w.h_row_start, 0, sizeof(uint32_t) * (rows + 1));
    if (n > 0) {
        const auto reserve = [](auto &b, size_t count) { return modes_reserve(b, count); };
        const SortShape shape = sort_shape(n);
        if (int rc = w.sort.reserve(n, shape, reserve)) return rc;
        if (int rc = modes_reserve(w.gpos, n)) return rc;
        if (int rc = modes_reserve(w.gvel, n)) return rc;
        if (int rc = modes_reserve(w.chunks, (size_t)items64 * fields)) return rc;
        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        NB_HIP_TRY(hipMemcpyAsync(w.e2, w.h_e2, sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, sim.stream));
        const uint32_t blocks = (n + kThreads - 1) / kThreads, items = (uint32_t)items64;
        hipLaunchKernelGGL(modes_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, mom,
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
        hipLaunchKernelGGL(modes_sum_kernel, dim3(items), dim3(kThreads), 0, sim.stream, (const uint32_t *)row_start,
                           (const float4 *)w.gpos, (const float4 *)w.gvel, k, (const double *)w.res,
                           (double *)w.chunks);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(modes_rows_kernel, dim3(rows), dim3(kWave), 0, sim.stream, (const uint32_t *)row_start, nbins,
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
    nb_modes_head o{};
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
        mass += f[NB_MODES_C];
        nb_modes_bin b{};
        b.count = start[j + 2] - start[j + 1];
        b.m_r = f[fields - 2];
        b.m_h2 = f[fields - 1];
        bins[j] = b;
        std::memcpy(modes + (size_t)j * (fields - 2), f, sizeof(double) * (fields - 2));
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
    o.mmax = mmax;
    o.flags = params.flags;
    *out = o;
    return NB_OK;
}

}  // namespace nb
