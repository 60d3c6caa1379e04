// nb_radial.hip -- nb_sim_radial_profile: per-shell mass and velocity moments of a simulator's current
// state (include/nbody.h "Radial profiles"; no reference counterpart).
//
// One streaming pass over the float4 SoA state the simulator hands out (SimBase::diag_state), then one
// fixed-order finish:
//   bins    -- blocks of 256 threads stride over tiles of 256 bodies.  A thread classifies its body (fp64,
//              no contraction; a branch-free binary search over the squared edges in LDS), adds what is
//              not binned (inside, outside, non-finite, total mass, shape) to its own registers, and
//              stages the bin index and the body's ten fp64 terms in LDS.  Then the tile is summed per
//              bin: with P = the power of two >= nbins, thread (s, b) = (tid / P, tid % P) scans the P
//              staged bodies of segment s in body order and adds those of bin b to its registers.  At
//              nbins = 256 a thread scans the whole tile for its bin; at nbins = 1 every thread owns one
//              body, so bodies that all fall into one bin still sum in parallel.  At the end the block
//              adds its 256 / P segments per bin in order and writes one slab (what is not binned: block_row,
//              nb_analysis.hpp);
//   finish  -- every element of the slab is summed over the blocks in a fixed order (sum_over_blocks in
//              16 groups).
// With NB_RADIAL_CENTER_COM the moments pass of nb_diag.hip runs first on the same stream and the
// threads divide its sums into the centre themselves: no host round trip.
// No float atomics, and the grid depends on n and nbins alone: the result is bitwise reproducible.
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;    // = bodies per tile; 4 waves per block
constexpr uint32_t kMaxBins = NB_RADIAL_MAX_BINS;
constexpr uint32_t kEdgeSlots = 512;     // squared edges in LDS, padded with +inf for the search
constexpr uint32_t kBinFields = 11;      // see BinField
constexpr uint32_t kGlobalFields = 16;   // see GlobalField
constexpr uint32_t kBlockBins = 65536;   // grid cap: blocks * P <= this (slabs <= 5.9 MB)
constexpr uint32_t kMaxBlocks = 1024;
constexpr uint32_t kMaxElems = kGlobalFields + kMaxBins * kBinFields;
constexpr uint32_t kUsed = 8;            // res[0..6): the centre and velocity used; sums from res[kUsed]
constexpr uint16_t kNoBin = 0xffff;

enum BinField { kBMass = 0, kBR, kBUr, kBUr2, kBUphi, kBUphi2, kBU2, kBAng, kBCount = 10 };
enum GlobalField { kGInCount = 0, kGOutCount, kGBad, kGInMass, kGOutMass, kGMass, kGShape /* 6..11 */, kGLive = 12 };

struct RadialConst {
    double c[3], vc[3], axis[3];  // axis: the unit vector (cylindrical)
    uint32_t nbins, p2;           // p2 = P
    uint32_t cylindrical, center_com;
};

// One body by the rule of include/nbody.h: its class (cnt = edges at or below r2: 0 inside, nbins + 1
// outside), its ten bin terms and its six shape terms.
__device__ inline uint32_t classify(float4 p, float4 v, const RadialConst &k, const double (&c)[3],
                                    const double (&vc)[3], const double *e2, double (&term)[kBCount],
                                    double (&shape)[6]) {
#pragma clang fp contract(off)
    const double m = p.w;
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    const double ux = (double)v.x - vc[0], uy = (double)v.y - vc[1], uz = (double)v.z - vc[2];
    double qx = dx, qy = dy, qz = dz;  // what the radius is taken of
    if (k.cylindrical) {
        const double h = (dx * k.axis[0] + dy * k.axis[1]) + dz * k.axis[2];
        qx = dx - h * k.axis[0];
        qy = dy - h * k.axis[1];
        qz = dz - h * k.axis[2];
    }
    const double r2 = (qx * qx + qy * qy) + qz * qz;
    uint32_t cnt = 0;  // edges at or below r2 (a NaN r2 -- a NaN centre -- is below every edge)
    for (uint32_t step = kEdgeSlots / 2; step > 0; step >>= 1)
        if (e2[cnt + step - 1] <= r2) cnt += step;
    const double r = sqrt(r2);
    double ur = 0.0, uphi = 0.0;
    if (r2 != 0.0) {
        ur = ((qx * ux + qy * uy) + qz * uz) / r;
        if (k.cylindrical) {
            const double wx = qy * uz - qz * uy, wy = qz * ux - qx * uz, wz = qx * uy - qy * ux;
            uphi = ((k.axis[0] * wx + k.axis[1] * wy) + k.axis[2] * wz) / r;
        }
    }
    term[kBMass] = m;
    term[kBR] = m * r;
    term[kBUr] = m * ur;
    term[kBUr2] = (m * ur) * ur;
    term[kBUphi] = m * uphi;
    term[kBUphi2] = (m * uphi) * uphi;
    term[kBU2] = m * ((ux * ux + uy * uy) + uz * uz);
    term[kBAng + 0] = m * (dy * uz - dz * uy);
    term[kBAng + 1] = m * (dz * ux - dx * uz);
    term[kBAng + 2] = m * (dx * uy - dy * ux);
    shape[0] = (m * dx) * dx;
    shape[1] = (m * dy) * dy;
    shape[2] = (m * dz) * dz;
    shape[3] = (m * dx) * dy;
    shape[4] = (m * dx) * dz;
    shape[5] = (m * dy) * dz;
    return cnt;
}

// ---- bins: one slab of kGlobalFields + nbins * kBinFields doubles per block ----------------
// mom: the finished moments of nb_diag.hip (NB_RADIAL_CENTER_COM) or null.  e2g: nbins + 1 squared edges.
// Block 0 also writes the centre and velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kThreads) void radial_bins_kernel(const float4 *__restrict__ posm,
                                                               const float4 *__restrict__ vel, uint32_t n,
                                                               RadialConst k, const double *__restrict__ mom,
                                                               const double *__restrict__ e2g,
                                                               double *__restrict__ slabs, double *__restrict__ used) {
    __shared__ double e2[kEdgeSlots];
    __shared__ double stage[kBinFields][kThreads];  // [field][body of the tile]; at the end [field][thread]
    __shared__ uint16_t bin_of[kThreads];
    __shared__ double part[kThreads / kWave][kGlobalFields];
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = tid; j < kEdgeSlots; j += kThreads) e2[j] = j <= k.nbins ? e2g[j] : INFINITY;
    double c[3], vc[3];
    centre_used(k.c, k.vc, k.center_com, mom, used, c, vc);
    __syncthreads();

    const uint32_t my_bin = tid & (k.p2 - 1), seg0 = tid & ~(k.p2 - 1);  // this thread's bin and first staged body
    double acc[kBinFields];
    for (uint32_t f = 0; f < kBinFields; ++f) acc[f] = 0.0;
    double glob[kGLive];
    for (uint32_t f = 0; f < kGLive; ++f) glob[f] = 0.0;

    const uint32_t n_tiles = (n + kThreads - 1) / kThreads;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p;
    {
        const size_t i = (size_t)blockIdx.x * kThreads + tid;
        if (i < n) {
            p = posm[i];
            v = vel[i];
        }
    }
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t i = (size_t)t * kThreads + tid;
        uint16_t b = kNoBin;
        if (i < n) {
            if (!body_ok(p, v)) {
                glob[kGBad] += 1.0;
            } else {
                double term[kBCount], shape[6];
                const uint32_t cnt = classify(p, v, k, c, vc, e2, term, shape);
                glob[kGMass] += term[kBMass];
                if (cnt > k.nbins) {
                    glob[kGOutCount] += 1.0;
                    glob[kGOutMass] += term[kBMass];
                } else {
                    for (int a = 0; a < 6; ++a) glob[kGShape + a] += shape[a];
                    if (cnt == 0) {
                        glob[kGInCount] += 1.0;
                        glob[kGInMass] += term[kBMass];
                    } else {
                        b = (uint16_t)(cnt - 1);
                        for (uint32_t f = 0; f < kBCount; ++f) stage[f][tid] = term[f];
                    }
                }
            }
        }
        bin_of[tid] = b;
        __syncthreads();
        {  // the next tile's loads fly while this one is summed
            const size_t in = ((size_t)t + gridDim.x) * kThreads + tid;
            if (in < n) {
                p = posm[in];
                v = vel[in];
            }
        }
        for (uint32_t j = seg0; j < seg0 + k.p2; ++j) {
            if (bin_of[j] == my_bin) {
                for (uint32_t f = 0; f < kBCount; ++f) acc[f] += stage[f][j];
                acc[kBCount] += 1.0;
            }
        }
        __syncthreads();  // the tile has been read
    }

    // what is not binned, by the last 16 threads (the last wave: busy with the bins only at nbins > 192); then
    // the segments of every bin, in order
    for (uint32_t f = 0; f < kBinFields; ++f) stage[f][tid] = acc[f];
    double *slab = slabs + (size_t)blockIdx.x * (kGlobalFields + k.nbins * kBinFields);
    block_row<kGlobalFields, kGLive>(glob, part, slab, kThreads - kGlobalFields);
    if (tid < k.nbins) {
        for (uint32_t f = 0; f < kBinFields; ++f) {
            double s = stage[f][tid];
            for (uint32_t q = k.p2; q < kThreads; q += k.p2) s += stage[f][q + tid];
            slab[kGlobalFields + tid * kBinFields + f] = s;
        }
    }
}

// ---- finish: res[e] = sum over the blocks of slab element e, in a fixed order -----------------
// block x owns elements 16 x .. 16 x + 15, summed by sum_over_blocks in 16 groups.
__global__ __launch_bounds__(kThreads) void radial_finish_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                                 uint32_t elems, double *__restrict__ res) {
    constexpr uint32_t kPer = 16, kGroups = kThreads / kPer;
    __shared__ double pp[kGroups][kPer];
    const uint32_t tid = threadIdx.x, e = blockIdx.x * kPer + tid % kPer;
    const double r = sum_over_blocks<kGroups>(slabs, blocks, elems, e, pp);
    if (tid < kPer && e < elems) res[e] = r;
}

uint32_t pow2_at_least(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace

struct RadialWork : Workspace {
    DeviceBuf<double> slabs;  // [blocks][kGlobalFields + nbins * kBinFields], blocks * P <= kBlockBins
    DeviceBuf<double> res;    // [kUsed + kMaxElems]
    DeviceBuf<double> e2;     // [kMaxBins + 1] squared edges
    PinnedBuf<double> h_res;  // as res
    PinnedBuf<double> h_e2;   // as e2
};

int sim_radial_profile(SimBase &sim, const nb_radial_params &params, nb_radial_profile *out, nb_radial_bin *bins) {
    if (int rc = analysis_begin(sim, "radial_profile")) return rc;
    RadialWork *work = nullptr;
    if (int rc = workspace(sim, kWorkRadial, &work, [](RadialWork &f) {
            // the largest slab set: P = 1 has kMaxBlocks blocks of 16 + 11 doubles, P = 256 has 256 of 16 + 2816
            NB_HIP_TRY(f.slabs.reserve((size_t)kBlockBins * kBinFields + (size_t)kMaxBlocks * kGlobalFields));
            NB_HIP_TRY(f.res.reserve(kUsed + kMaxElems));
            NB_HIP_TRY(f.e2.reserve(kMaxBins + 1));
            NB_HIP_TRY(f.h_res.reserve(kUsed + kMaxElems));
            NB_HIP_TRY(f.h_e2.reserve(kMaxBins + 1));
            return NB_OK;
        }))
        return rc;
    RadialWork &w = *work;
    const uint32_t n = sim.n, nbins = params.nbins;
    const bool cyl = (params.flags & NB_RADIAL_CYLINDRICAL) != 0, com = (params.flags & NB_RADIAL_CENTER_COM) != 0;

    RadialConst k{};
    k.nbins = nbins;
    k.p2 = pow2_at_least(nbins);
    k.cylindrical = cyl;
    k.center_com = com;
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
    }
    if (cyl) {
#pragma clang fp contract(off)
        const double *ax = params.axis;
        const double len = std::sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
        for (int a = 0; a < 3; ++a) k.axis[a] = ax[a] / len;
    }
    for (uint32_t j = 0; j <= nbins; ++j) w.h_e2[j] = params.edges[j] * params.edges[j];

    const uint32_t elems = kGlobalFields + nbins * kBinFields;
    std::memset(w.h_res, 0, sizeof(double) * (kUsed + elems));
    if (n > 0) {
        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        NB_HIP_TRY(hipMemcpyAsync(w.e2, w.h_e2, sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, sim.stream));
        const uint32_t n_tiles = (n + kThreads - 1) / kThreads;
        const uint32_t blocks = std::min(std::min(kMaxBlocks, kBlockBins / k.p2), n_tiles);
        hipLaunchKernelGGL(radial_bins_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, mom,
                           w.e2, w.slabs, w.res);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(radial_finish_kernel, dim3((elems + 15) / 16), dim3(kThreads), 0, sim.stream, w.slabs,
                           blocks, elems, w.res + kUsed);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(double) * (kUsed + elems), hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    } else {
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        centre_used_empty(w.h_res, com, k.c, k.vc);
    }
    if (int rc = sim.diag_status()) return rc;

    const double *used = w.h_res, *g = w.h_res + kUsed, *b = g + kGlobalFields;
    nb_radial_profile o{};
    o.step_num = sim.step_num;
    o.n = n;
    o.nonfinite = (uint64_t)g[kGBad];
    o.inside_count = (uint64_t)g[kGInCount];
    o.outside_count = (uint64_t)g[kGOutCount];
    o.inside_mass = g[kGInMass];
    o.outside_mass = g[kGOutMass];
    o.mass = g[kGMass];
    for (int a = 0; a < 3; ++a) {
        o.center[a] = used[a];
        o.velocity[a] = used[3 + a];
        o.axis[a] = k.axis[a];
    }
    for (int a = 0; a < 6; ++a) o.shape[a] = g[kGShape + a];
    o.nbins = nbins;
    o.flags = params.flags;
    for (uint32_t j = 0; j < nbins; ++j) {
        const double *f = b + (size_t)j * kBinFields;
        nb_radial_bin r{};
        r.count = (uint64_t)f[kBCount];
        r.mass = f[kBMass];
        r.m_r = f[kBR];
        r.m_ur = f[kBUr];
        r.m_ur2 = f[kBUr2];
        r.m_uphi = f[kBUphi];
        r.m_uphi2 = f[kBUphi2];
        r.m_u2 = f[kBU2];
        for (int a = 0; a < 3; ++a) r.ang[a] = f[kBAng + a];
        bins[j] = r;
    }
    *out = o;
    return NB_OK;
}

}  // namespace nb
