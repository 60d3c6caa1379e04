// nb_analysis_sort.hpp -- what the analysis passes that sort their bodies by a spatial key share (nb_map.hip,
// nb_fof.hip, nb_knn.hip, nb_hop.hip; DESIGN.md 6g "The sort", "The bounds"):
//   the sort    -- a stable LSD radix sort of (key, index), 8 bits a pass, on 32- or 64-bit keys: its shape
//                  (chunks, histogram), its two sides, its three kernels and the loop that enqueues them;
//   the bounds  -- the per-axis minimum and maximum of the counted bodies and their number: the slab kernel and
//                  the finish inside a caller's one-block plan kernel.
// Integer work, maxima and a sum of small integers: there is nothing to contract, so it is the same arithmetic in
// units built with -ffp-contract=off and in those built without.  Every kernel sits in an anonymous namespace:
// a unit launches its own copy, at internal linkage like the unit's other kernels.
#pragma once

#include <cstddef>
#include <cstdint>

namespace nb {

// ---- the shape of a sort over n elements: plain host arithmetic, usable without HIP -------------------------
constexpr uint32_t kRadix = 256;         // 8 bits of the key per sort pass
constexpr uint32_t kSortBlocks = 2048;   // at most this many chunks (one wave each) per sort pass
constexpr uint32_t kSortChunkStep = 64;  // a chunk is whole wave-loads (kWave, checked below)
constexpr uint32_t kSortChunkMin = 256;

// Chunk b = elements [b * chunk, (b + 1) * chunk) of a pass's input, one wave each: chunks of a multiple of 64
// elements, at least 256, at most kSortBlocks of them.  hist: [256][blocks] counts, then the 256 digit totals.
struct SortShape {
    uint32_t chunk, blocks;
    size_t hist_size() const { return (size_t)kRadix * ((size_t)blocks + 1); }
    size_t totals_at() const { return (size_t)kRadix * blocks; }
};
inline SortShape sort_shape(uint32_t n) {
    const uint64_t per = ((uint64_t)n + kSortBlocks - 1) / kSortBlocks;
    const uint64_t stepped = (per + kSortChunkStep - 1) / kSortChunkStep * kSortChunkStep;
    const uint32_t chunk = (uint32_t)(stepped > kSortChunkMin ? stepped : kSortChunkMin);
    return {chunk, (uint32_t)(((uint64_t)n + chunk - 1) / chunk)};
}

}  // namespace nb

#ifdef __HIPCC__

#include <algorithm>
#include <cmath>

#include "nb_analysis.hpp"
#include "nb_common.hpp"

namespace nb {

static_assert(kSortChunkStep == kWave, "a chunk is whole wave-loads");
constexpr uint32_t kScanThreads = 1024;  // the one-block scans
constexpr uint32_t kBoundFields = 8, kBoundLive = 7;  // max(-x, -y, -z, x, y, z), counted bodies
constexpr uint32_t kBoundMax = 0x3f;

// The sort's buffers in a pass's workspace.  reserve(buffer, count) is the pass's own: it words the pass's error.
template <class K>
struct SortBufs {
    DeviceBuf<K> keys[2];        // [n] each: the two sides
    DeviceBuf<uint32_t> idx[2];  // [n] each
    DeviceBuf<uint32_t> hist;    // SortShape::hist_size()
    template <class Reserve>
    int reserve(uint32_t n, const SortShape &shape, Reserve reserve) {
        for (int s = 0; s < 2; ++s) {
            if (int rc = reserve(keys[s], (size_t)n)) return rc;
            if (int rc = reserve(idx[s], (size_t)n)) return rc;
        }
        return reserve(hist, shape.hist_size());
    }
};

// An exclusive scan of v[0 .. count) in place by one block of kScanThreads, thread t owning a run of `per`
// elements; returns the sum of all of them.
__device__ inline uint32_t block_scan_runs(uint32_t *v, uint32_t count, uint32_t *lds /* [2][kScanThreads] */) {
    const uint32_t tid = threadIdx.x, per = (count + kScanThreads - 1) / kScanThreads;
    const size_t lo = std::min<size_t>(count, (size_t)tid * per), hi = std::min<size_t>(count, lo + per);
    uint32_t s = 0;
    for (size_t i = lo; i < hi; ++i) s += v[i];
    uint32_t *a = lds, *b = lds + kScanThreads;
    a[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {  // inclusive, Hillis-Steele
        b[tid] = tid >= o ? a[tid] + a[tid - o] : a[tid];
        __syncthreads();
        uint32_t *t = a;
        a = b;
        b = t;
    }
    uint32_t run = a[tid] - s;  // exclusive
    const uint32_t total = a[kScanThreads - 1];
    for (size_t i = lo; i < hi; ++i) {
        const uint32_t x = v[i];
        v[i] = run;
        run += x;
    }
    __syncthreads();
    return total;
}

// Thread 0 of a one-block kernel of kBlock threads gets the bounds_kernel slabs finished: lo, hi per axis and the
// number of counted bodies (lo, hi meaningless when that is 0); true on thread 0 alone.  Every thread calls it.
// Maxima and a sum of small integers: exact in any order.
__device__ inline bool bounds_finish(const double *__restrict__ slabs, uint32_t blocks, double (&lo)[3],
                                     double (&hi)[3], uint32_t *n_ok) {
    __shared__ double red[kBoundLive][kBlock];
    const uint32_t tid = threadIdx.x;
    double v[kBoundLive];
    for (uint32_t f = 0; f < 6; ++f) v[f] = -INFINITY;  // (not sum_over_blocks: its columns start at 0, -x is negative)
    v[6] = 0.0;
    for (uint32_t b = tid; b < blocks; b += kBlock) {
        const double *row = slabs + (size_t)b * kBoundFields;
        for (uint32_t f = 0; f < 6; ++f) v[f] = fmax(v[f], row[f]);
        v[6] += row[6];
    }
    for (uint32_t f = 0; f < kBoundLive; ++f) red[f][tid] = v[f];
    __syncthreads();
    for (uint32_t o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o) {
            for (uint32_t f = 0; f < 6; ++f) red[f][tid] = fmax(red[f][tid], red[f][tid + o]);
            red[6][tid] += red[6][tid + o];
        }
        __syncthreads();
    }
    if (tid != 0) return false;
    for (int a = 0; a < 3; ++a) {
        lo[a] = -red[a][0];
        hi[a] = red[3 + a][0];
    }
    *n_ok = (uint32_t)red[6][0];
    return true;
}

namespace {

// ---- the bounds: one slab row of kBoundFields doubles per block of kBlock bodies ----------------------------
// (a template only so that a unit that never launches it, nb_map.hip, emits no copy)
template <int = 0>
__global__ __launch_bounds__(kBlock) void bounds_kernel(const float4 *__restrict__ posm,
                                                        const float4 *__restrict__ vel, uint32_t n,
                                                        double *__restrict__ slabs) {
    __shared__ double part[kBlock / kWave][kBoundFields];
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    double v[kBoundLive];
    for (uint32_t f = 0; f < 6; ++f) v[f] = -INFINITY;
    v[6] = 0.0;
    if (i < n) {
        const float4 p = posm[i];
        if (body_ok(p, vel[i])) {
            v[0] = -(double)p.x;
            v[1] = -(double)p.y;
            v[2] = -(double)p.z;
            v[3] = p.x;
            v[4] = p.y;
            v[5] = p.z;
            v[6] = 1.0;
        }
    }
    block_row<kBoundFields, kBoundLive, kBoundMax>(v, part, slabs + (size_t)blockIdx.x * kBoundFields);
}

// ---- the sort: one pass, digit = (key >> shift) & 255 -------------------------------------------------------
// A pass runs iff limit is null or pass < *limit: a device plan (nb_fof.hip) skips the passes its keys do not
// need, and all of them after a refusal, without a host round trip.
__device__ inline bool sort_pass_runs(const uint32_t *__restrict__ limit, uint32_t pass) {
    return !limit || pass < *limit;
}

// count: hist[d * blocks + b] = elements of chunk b with digit d
template <class K>
__global__ __launch_bounds__(kWave) void sort_count_kernel(const K *__restrict__ keys, uint32_t n, uint32_t chunk,
                                                           uint32_t shift, uint32_t *__restrict__ hist,
                                                           const uint32_t *__restrict__ limit, uint32_t pass) {
    if (!sort_pass_runs(limit, pass)) return;
    __shared__ uint32_t cnt[kRadix];
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < kRadix; d += kWave) cnt[d] = 0;
    __syncthreads();
    const size_t lo = (size_t)blockIdx.x * chunk, hi = std::min<size_t>(n, lo + chunk);
    for (size_t i = lo + lane; i < hi; i += kWave) atomicAdd(&cnt[(uint32_t)(keys[i] >> shift) & (kRadix - 1)], 1u);
    __syncthreads();
    for (uint32_t d = lane; d < kRadix; d += kWave) hist[(size_t)d * gridDim.x + blockIdx.x] = cnt[d];
}

// scan: block d scans the row of digit d over the chunks in place and writes the row's sum to totals[d]; the
// scatter adds the digits below itself
__global__ __launch_bounds__(kScanThreads) void sort_scan_kernel(uint32_t *__restrict__ hist, uint32_t blocks,
                                                                 uint32_t *__restrict__ totals,
                                                                 const uint32_t *__restrict__ limit, uint32_t pass) {
    if (!sort_pass_runs(limit, pass)) return;
    __shared__ uint32_t lds[2 * kScanThreads];
    const uint32_t total = block_scan_runs(hist + (size_t)blockIdx.x * blocks, blocks, lds);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// scatter: element i of chunk b goes to (elements with a lower digit) + offs[d * blocks + b] + (elements of the
// chunk before i with digit d): the rank inside a chunk by wave ballots in element order, so the sort is stable
// and no atomic reserves a place.  idx_in null: the identity (the first pass).
template <class K>
__global__ __launch_bounds__(kWave) void sort_scatter_kernel(const K *__restrict__ key_in,
                                                             const uint32_t *__restrict__ idx_in,
                                                             K *__restrict__ key_out, uint32_t *__restrict__ idx_out,
                                                             uint32_t n, uint32_t chunk, uint32_t shift,
                                                             const uint32_t *__restrict__ offs,
                                                             const uint32_t *__restrict__ totals,
                                                             const uint32_t *__restrict__ limit, uint32_t pass) {
    if (!sort_pass_runs(limit, pass)) return;
    __shared__ uint32_t base[kRadix];
    const uint32_t lane = threadIdx.x;
    {  // lane l owns digits 4 l .. 4 l + 3: an exclusive scan of the 256 totals, four a lane, then over the wave
        constexpr uint32_t kPer = kRadix / kWave;
        uint32_t t[kPer], sum = 0;
        for (uint32_t q = 0; q < kPer; ++q) {
            t[q] = totals[lane * kPer + q];
            sum += t[q];
        }
        uint32_t inc = sum;
        for (uint32_t o = 1; o < kWave; o <<= 1) {
            const uint32_t y = __shfl_up(inc, o);
            if (lane >= o) inc += y;
        }
        uint32_t run = inc - sum;
        for (uint32_t q = 0; q < kPer; ++q) {
            const uint32_t d = lane * kPer + q;
            base[d] = run + offs[(size_t)d * gridDim.x + blockIdx.x];
            run += t[q];
        }
    }
    __syncthreads();
    const size_t lo = (size_t)blockIdx.x * chunk, hi = std::min<size_t>(n, lo + chunk);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (size_t i0 = lo; i0 < hi; i0 += kWave) {
        const size_t i = i0 + lane;
        const bool valid = i < hi;
        const K key = valid ? key_in[i] : K(0);
        const uint32_t src = valid ? (idx_in ? idx_in[i] : (uint32_t)i) : 0u;
        const uint32_t d = (uint32_t)(key >> shift) & (kRadix - 1);
        unsigned long long same = __ballot(valid);  // the valid lanes with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below), group = (uint32_t)__popcll(same);
        const uint32_t pos = base[d] + rank;
        __syncthreads();
        if (valid && rank + 1 == group) base[d] += group;  // one lane per digit present
        __syncthreads();
        if (valid && pos < n) {
            key_out[pos] = key;
            idx_out[pos] = src;
        }
    }
}

// Passes 0 .. count - 1 of the stable sort of (keys[0], identity), pass p on the digit at first_shift + 8 p.  Pass
// p reads side p & 1 and writes the other: after `passes` passes that ran the sorted arrays are on side passes & 1
// -- count & 1 where every pass runs (limit null), else what the device plan behind `limit` says.
template <class K>
int enqueue_sort(hipStream_t stream, const SortBufs<K> &b, uint32_t n, const SortShape &shape, uint32_t count,
                 uint32_t first_shift, const uint32_t *limit) {
    uint32_t *hist = b.hist, *totals = hist + shape.totals_at();
    for (uint32_t pass = 0; pass < count; ++pass) {
        const int in = pass & 1, out = in ^ 1;
        const uint32_t shift = first_shift + 8 * pass;
        hipLaunchKernelGGL(sort_count_kernel<K>, dim3(shape.blocks), dim3(kWave), 0, stream, (const K *)b.keys[in], n,
                           shape.chunk, shift, hist, limit, pass);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sort_scan_kernel, dim3(kRadix), dim3(kScanThreads), 0, stream, hist, shape.blocks, totals,
                           limit, pass);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sort_scatter_kernel<K>, dim3(shape.blocks), dim3(kWave), 0, stream, (const K *)b.keys[in],
                           pass ? (const uint32_t *)b.idx[in] : nullptr, (K *)b.keys[out], (uint32_t *)b.idx[out], n,
                           shape.chunk, shift, (const uint32_t *)hist, (const uint32_t *)totals, limit, pass);
        NB_HIP_TRY(hipGetLastError());
    }
    return NB_OK;
}

}  // namespace

}  // namespace nb

#endif  // __HIPCC__
