// nb_analysis.hpp -- what the analysis passes over a simulator's current state share (nb_diag.hip,
// nb_render.hip, nb_radial.hip, nb_field.hip, nb_map.hip, nb_fof.hip, nb_knn.hip):
//   host    -- the buffers a workspace is made of, the workspace of a pass behind its slot of SimBase, the
//              preamble of every entry point, and the centre a pass over no bodies reports;
//   device  -- the predicate that decides which bodies count, the fixed-order reductions that make the sums
//              bitwise reproducible (wave, block, blocks), and the centre a pass uses.
// The device part only adds, takes maxima and divides: there is nothing to contract, so it is the same
// arithmetic in the units built with -ffp-contract=off and in those built without.  The terms that are summed
// stay in their units, whose contraction setting is part of their specification.
// What only the passes that sort their bodies by a spatial key share (nb_map.hip, nb_fof.hip, nb_knn.hip) -- the
// radix sort and, for the last two, the bounds of the counted bodies -- is in nb_analysis_sort.hpp, on top of this.
#pragma once

#include <cmath>
#include <memory>
#include <utility>

#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

// A buffer of `count` T on the device (or, kPinned, in pinned host memory) that grows to the largest request
// so far.  Move-only; the destructor frees.  The conversion to T * is deliberate: a buffer is passed to kernels and
// copies as the pointer it stands for.  It owns that pointer: never delete or free what the conversion gives.
template <class T, bool kPinned>
class Buf {
   public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf &operator=(Buf &&o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~Buf() { release(); }

    // At least `count` elements; a request no larger than the capacity allocates nothing, a larger one frees
    // and reallocates (the contents are not kept).  A failure leaves the buffer empty.
    hipError_t reserve(size_t count) {
        if (count <= cap_) return hipSuccess;
        release();
        const hipError_t e = kPinned ? hipHostMalloc((void **)&p_, sizeof(T) * count, hipHostMallocDefault)
                                     : hipMalloc((void **)&p_, sizeof(T) * count);
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        cap_ = count;
        return hipSuccess;
    }
    operator T *() const { return p_; }

   private:
    void release() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    T *p_ = nullptr;
    size_t cap_ = 0;
};
template <class T>
using DeviceBuf = Buf<T, false>;
template <class T>
using PinnedBuf = Buf<T, true>;

// Slot k's workspace (a W : Workspace), created by the first call that needs it: init(W &) allocates what
// does not depend on the call and returns NB_OK or its error.  A workspace whose init fails is dropped:
// the slot holds a complete workspace or none.
template <class W, class Init>
int workspace(SimBase &sim, WorkSlot k, W **out, Init init) {
    if (!sim.work[k]) {
        auto fresh = std::make_unique<W>();
        if (int rc = init(*fresh)) return rc;
        sim.work[k] = std::move(fresh);
    }
    *out = static_cast<W *>(sim.work[k].get());
    return NB_OK;
}

// The preamble of every analysis entry point: a pass reads the whole state, so a shard is refused; then the
// simulator's device is bound.  A pass that checks the simulator's parameters does so between the two.
inline int refuse_sharded(const SimBase &sim, const char *name) {
    if (sim.place.world <= 1) return NB_OK;
    set_error("%s: not available on a sharded simulator (placement world %d > 1)", name, sim.place.world);
    return NB_ERR_UNSUPPORTED;
}
inline int analysis_begin(const SimBase &sim, const char *name) {
    if (int rc = refuse_sharded(sim, name)) return rc;
    return sim.bind_device();
}

// used[0..6) of a pass over no bodies (centre_used below never ran): the explicit centre and velocity, or
// NaN for the centre of no mass
inline void centre_used_empty(double *used, bool com, const double *c, const double *vc) {
    for (int a = 0; a < 3; ++a) {
        used[a] = com ? std::nan("") : c[a];
        used[3 + a] = com ? std::nan("") : vc[a];
    }
}

#ifdef __HIPCC__

constexpr uint32_t kBlock = 256;  // threads of every kernel that calls block_row or sum_over_blocks: 4 waves

__device__ inline bool finite4(float4 p) {
    return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w);
}

// a body counts when its position, mass and velocity are all finite
__device__ inline bool body_ok(float4 p, float4 v) {
    return finite4(p) && isfinite(v.x) && isfinite(v.y) && isfinite(v.z);
}

// fixed-order wave reductions (xor butterfly: every lane ends with the same, order-fixed result)
__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// a and b of field f combined: bit f of kMaxMask names a field reduced by fmax; every other, and every f >= 32,
// is summed
template <uint32_t kMaxMask>
__device__ inline double reduce2(double a, double b, uint32_t f) {
    if constexpr (kMaxMask == 0)
        return a + b;
    else
        return f < 32 && ((kMaxMask >> f) & 1u) ? fmax(a, b) : a + b;
}

// One slab row of F doubles per block from per-thread partials: v[f] through the wave butterfly, lane 0 of
// every wave into part[wave][f], then thread first + f combines the four waves in order and writes row[f].
// Fields [kLive, F) of the row are written as 0.  One barrier: LDS the caller wrote before the call may be
// read after it.
template <uint32_t F, uint32_t kLive, uint32_t kMaxMask = 0>
__device__ inline void block_row(double (&v)[kLive], double (*part)[F], double *row, uint32_t first = 0) {
    static_assert(kLive <= F && F <= 32, "a row of at most 32 fields");
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if constexpr (kMaxMask == 0) {
        for (uint32_t f = 0; f < kLive; ++f) v[f] = wave_sum(v[f]);
    } else {  // unrolled, so that the choice per field is made at compile time and the butterflies are independent
#pragma unroll
        for (uint32_t f = 0; f < kLive; ++f) v[f] = (kMaxMask >> f) & 1u ? wave_max(v[f]) : wave_sum(v[f]);
    }
    if (lane == 0)
        for (uint32_t f = 0; f < kLive; ++f) part[wave][f] = v[f];
    __syncthreads();
    const uint32_t f = threadIdx.x - first;
    if (f < F) {  // (threads first .. first + F - 1)
        double s = 0.0;
        if (f < kLive) {
            s = part[0][f];
            for (uint32_t w = 1; w < kBlock / kWave; ++w) s = reduce2<kMaxMask>(s, part[w][f], f);
        }
        row[f] = s;
    }
}

// The fixed-order sum over the blocks' rows (`elems` doubles each) by one block in G groups: thread (c, g) =
// (tid % (256 / G), tid / (256 / G)) combines element e -- its column's, by the caller's rule -- of rows g,
// g + G, ...; then the G partials of a column in order.  Threads tid < 256 / G return their column's result
// (0 for e >= elems).  The order of the additions is the result, so G belongs to the caller's specification.
// kMaxMask names elements below 32.  One barrier, as in block_row.
template <uint32_t G, uint32_t kMaxMask = 0>
__device__ inline double sum_over_blocks(const double *__restrict__ slabs, uint32_t blocks, uint32_t elems,
                                         uint32_t e, double (*pp)[kBlock / G]) {
    constexpr uint32_t kPer = kBlock / G;
    const uint32_t tid = threadIdx.x, g = tid / kPer;
    double s = 0.0;  // (a field reduced by fmax is >= 0)
    if (e < elems)
        for (uint32_t b = g; b < blocks; b += G) s = reduce2<kMaxMask>(s, slabs[(size_t)b * elems + e], e);
    pp[g][tid % kPer] = s;
    __syncthreads();
    if (tid < kPer) {
        s = pp[0][tid];
        for (uint32_t q = 1; q < G; ++q) s = reduce2<kMaxMask>(s, pp[q][tid], e);
    }
    return s;
}

// The centre c and velocity vc a pass uses: the explicit ones, or (center_com) `com` and `momentum / mass`
// exactly as sim_diagnostics forms them, from the finished moments of diag_enqueue_moments.  Thread 0 of
// block 0 also writes them to used[0..6).
__device__ inline void centre_used(const double (&c_in)[3], const double (&vc_in)[3], uint32_t center_com,
                                   const double *__restrict__ mom, double *__restrict__ used, double (&c)[3],
                                   double (&vc)[3]) {
    for (int a = 0; a < 3; ++a) {
        c[a] = c_in[a];
        vc[a] = vc_in[a];
    }
    if (center_com) {
        const double mass = mom[kDiagResMass];
        for (int a = 0; a < 3; ++a) {
            c[a] = mom[kDiagResMX + a] / mass;
            vc[a] = mom[kDiagResMV + a] / mass;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int a = 0; a < 3; ++a) {
            used[a] = c[a];
            used[3 + a] = vc[a];
        }
}

#endif  // __HIPCC__

}  // namespace nb
