// nb_tree_sort.hpp -- part of the nb_tree.hip translation unit: included there, inside its
// namespace nb { namespace {, and never compiled on its own.
// stages 1-3e: bound, Morton keys, radix sort / counting sort / fix-ups of the ties.

// ---- 1. bound -----------------------------------------------------------------------------------
// max over bodies and axes of |coord|, never below 1.0 (rayon reduce identity [1.0;3],
// tree.rs:427-433).  Non-negative floats order like their bit patterns -> atomicMax on u32.
__global__ __launch_bounds__(256) void bound_kernel(const float4 *__restrict__ posm, uint32_t n,
                                                    uint32_t *bound_bits) {
    __shared__ float s_m[4];
    float m = 1.0f;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = posm[i];
        m = fmaxf(m, fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    // one atomic per workgroup: thousands of atomics on one word serialise (~12 ns each)
    if (threadIdx.x == 0)
        atomicMax(bound_bits, __float_as_uint(fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]))));
}

// The walk kernels also accumulate the NEXT step's bound from the positions they write, so a steady-state
// step needs neither bound_kernel nor a memset: morton_kernel takes the maximum of the slots (and of 1.0).
// A wave whose bodies stay inside the unit cube has nothing to say (the bound is never below 1.0,
// tree.rs:427-433); the others add their maximum to one of 1,024 slots -- 64 cache lines -- with an atomic
// nobody waits for.  (Round 2 read the slot first, "skip the atomic when not above": a device-scope load of one
// of FOUR lines by every wave, in its prologue and waited for -- the lines' channel served ~300 waves per us
// chip-wide, and a wave of a 32,768-body walk spent 8 us (up to 27) between its launch and its first batch.)
constexpr uint32_t kBoundSlots = 1024;
__device__ __forceinline__ void publish_bound(uint32_t *__restrict__ slots, uint32_t key, float m) {
    const uint32_t bits = __float_as_uint(m);  // non-negative floats order like their bit patterns
    if (bits > 0x3f800000u) atomicMax(slots + (key & (kBoundSlots - 1u)), bits);
}

// (see morton_kernel) the cell of a coordinate at the finest level, and its 21 bits spread to every third bit
__device__ __forceinline__ uint32_t cell_21(float x, float inv_h) {
    const int t = (int)__builtin_ceilf(x * inv_h) + (1 << 20) - 1;
    return (uint32_t)min(max(t, 0), (1 << 21) - 1);
}
__device__ __forceinline__ uint64_t spread_21(uint32_t v) {
    // the low 11 and the high 10 bits separately, in 32-bit arithmetic: bit i -> bit 3 i
    auto spread = [](uint32_t x) {  // x < 2^11
        x = (x | (x << 16)) & 0x070000ffu;
        x = (x | (x << 8)) & 0x0700f00fu;
        x = (x | (x << 4)) & 0x430c30c3u;
        x = (x | (x << 2)) & 0x49249249u;
        return x;
    };
    return (uint64_t)spread(v & 0x7ffu) | ((uint64_t)spread(v >> 11) << 33);
}

// ---- 2. keys ------------------------------------------------------------------------------------
// One workgroup per sort tile: the keys, and the tile's histogram of the first digit (saves the
// first pass its histogram launch).
// bound_src: where the root cube's half width comes from -- scalars[0] (bound_kernel / the LET
// maximum; n_src = 1) or the kBoundSlots words accumulated by the previous step's walk (n_src =
// kBoundSlots); it is republished in scalars[0].
__global__ __launch_bounds__(2 * kSortThreads) void morton_kernel(const float4 *__restrict__ posm, uint32_t n,
                                                              const uint32_t *__restrict__ bound_src,
                                                              uint32_t n_src, uint32_t *__restrict__ bound_bits,
                                                              uint64_t *__restrict__ keys,
                                                              uint32_t *__restrict__ idx,
                                                              uint32_t *__restrict__ hist, uint32_t nblocks,
                                                              uint32_t items, uint32_t hist_shift,
                                                              uint32_t hist_bins, uint32_t *__restrict__ key_hi,
                                                              uint32_t key_descent_only) {
    // key_hi (the radix passes sort 32-bit high words paired with indices, section 3e): the high word of
    // every key beside the key, and no identity index array -- the first pass makes it up.
    // (blockDim.x * items bodies = a sort tile: a workgroup leaves the tile's histogram of the digit the
    // FIRST radix pass sorts by -- hist_bins values at bit hist_shift; the counting sort of small
    // problems needs no histogram and takes items = 1: more, shorter workgroups)
    __shared__ uint32_t s_hist[kSortMaxBins];
    for (uint32_t b = threadIdx.x; b < kSortMaxBins; b += blockDim.x) s_hist[b] = 0;
    __syncthreads();
    uint32_t bmax;
    if (n_src > 1u) {  // the slots of the previous walk: a share per thread, the maximum through LDS
        __shared__ uint32_t s_bmax[2 * kSortThreads / 64];
        uint32_t mine = 0;
        for (uint32_t k = threadIdx.x; k < n_src; k += blockDim.x) mine = max(mine, bound_src[k]);
        mine = (uint32_t)wave_max_to_lane63((int)mine);  // (bit patterns of non-negative floats: positive as int)
        if ((threadIdx.x & 63u) == 63u) s_bmax[threadIdx.x >> 6] = mine;
        __syncthreads();
        bmax = 0;
        for (uint32_t w = 0; w < blockDim.x / 64u; ++w) bmax = max(bmax, s_bmax[w]);
    } else {
        bmax = bound_src[0];
    }
    const float bound = fmaxf(1.0f, __uint_as_float(bmax));  // never below 1.0, tree.rs:427-433
    if (blockIdx.x == 0 && threadIdx.x == 0 && bound_src != bound_bits) *bound_bits = __float_as_uint(bound);
    const float root_w = bound * 2.0f;  // root width, tree.rs:465
    // The quarter widths of the 21 levels, width / 4 (shift_node_center) with width halved per level: exact powers
    // of two times root_w, i.e. root_w's bit pattern with its exponent lowered -- wave-uniform integers the scalar
    // unit computes, where `w / 4.0f; w = w / 2.0f` cost two vector multiplies per level and body.
    const uint32_t root_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(root_w));
    const bool pow2_root = (root_bits & 0x007fffffu) == 0u && !key_descent_only;
    const float inv_h = __uint_as_float((275u - (root_bits >> 23)) << 23);  // 2^21 / root_w for a power of two
    // (the loads of a tile's bodies first, all in flight together: one body after the other the
    // kernel waited out eight memory latencies per thread)
    float4 pv[kSortItems];
#pragma unroll
    for (uint32_t c = 0; c < kSortItems; ++c) {
        const uint32_t i = (blockIdx.x * items + c) * blockDim.x + threadIdx.x;
        if (c < items && i < n) pv[c] = posm[i];
    }
#pragma unroll
    for (uint32_t c = 0; c < kSortItems; ++c) {
        const uint32_t i = (blockIdx.x * items + c) * blockDim.x + threadIdx.x;
        if (c >= items || i >= n) break;
        const float4 p = pv[c];
        uint64_t key = 0;
        if (pow2_root) {
            // root_w a power of two (every state inside the unit cube: bound = 1.0): the centres of the descent
            // below are multiples of root_w / 2^22 below root_w / 2 -- at most 21 significant bits, exact in fp32 --
            // so its 21 strict comparisons spell the binary digits of ceil((x + root_w / 2) / h) - 1, h = root_w /
            // 2^21 the finest cell (a body ON a cell boundary belongs below it; x = -root_w / 2 gives all zeros).
            // x / h is an exact scaling, its ceiling an exact integer of at most 21 bits: three instructions per
            // axis and a bit interleave instead of 21 dependent levels of compare, select, add.
            key = spread_21(cell_21(p.x, inv_h)) | (spread_21(cell_21(p.y, inv_h)) << 1) | (spread_21(cell_21(p.z, inv_h)) << 2);
        } else {
            float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
            for (int l = 0; l < kLevels; ++l) {
#pragma clang fp contract(off)
                const uint32_t bx = p.x > cx, by = p.y > cy, bz = p.z > cz;  // decide_octant, strict >
                key = (key << 3) | (uint64_t)(bx | (by << 1) | (bz << 2));
                const float q = __uint_as_float(root_bits - ((uint32_t)(l + 2) << 23));  // (root_w / 2^l) / 4, exactly
                cx = cx + (bx ? q : -q);  // shift_node_center
                cy = cy + (by ? q : -q);
                cz = cz + (bz ? q : -q);
            }
        }
        keys[i] = key;
        if (key_hi) key_hi[i] = (uint32_t)(key >> 32);
        else idx[i] = i;
        if (hist) atomicAdd(&s_hist[(uint32_t)(key >> hist_shift) & (hist_bins - 1u)], 1u);
    }
    __syncthreads();
    if (hist)
        for (uint32_t b = threadIdx.x; b < hist_bins; b += blockDim.x) hist[b * nblocks + blockIdx.x] = s_hist[b];  // bin-major
}

// ---- 3. radix sort (LSD, digits of W bits, pairs) ------------------------------------------------
// A block owns a tile of kSortThreads * ITEMS elements; wave w owns the contiguous sub-range
// [w*64*ITEMS, (w+1)*64*ITEMS) of it, read in ITEMS chunks of 64 -- so "wave, chunk, lane" order
// IS the input order, which is what makes the per-wave ranking below stable.
// (Counting the tile histograms of digit p + 1 inside the scatter of pass p, with one global atomic
// per element where it lands, was measured and dropped: 47 instead of 12 us per scatter at 2^20
// bodies, 10.8 instead of 5 + 5 at 8,192 -- profiles/r02_sort_experiments.txt.)
// (ITEMS elements per thread of a 2 x kSortThreads workgroup: the tile of the scatter, whatever its order inside)
template <uint32_t ITEMS, typename KeyT = uint64_t>
__global__ __launch_bounds__(2 * kSortThreads) void radix_hist_kernel(
    const KeyT *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t bins, uint32_t *__restrict__ hist,
    uint32_t nblocks) {
    constexpr uint32_t THREADS = 2u * kSortThreads;
    __shared__ uint32_t s_hist[kSortMaxBins];
    for (uint32_t b = threadIdx.x; b < kSortMaxBins; b += THREADS) s_hist[b] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (THREADS * ITEMS) + threadIdx.x;
#pragma unroll
    for (uint32_t c = 0; c < ITEMS; ++c) {
        const uint32_t i = base + c * THREADS;
        if (i < n) atomicAdd(&s_hist[(uint32_t)(keys[i] >> shift) & (bins - 1u)], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += THREADS) hist[b * nblocks + blockIdx.x] = s_hist[b];  // bin-major
}

// One workgroup per bin: exclusive scan of that bin's per-block counts; the bin total goes to
// totals[bin].  (rows of `nblocks` entries; used with 256 bins by the sort and 22 by the ids.)
__global__ __launch_bounds__(256) void bin_scan_kernel(uint32_t *__restrict__ hist,
                                                       uint32_t nblocks,
                                                       uint32_t *__restrict__ totals) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_carry;
    uint32_t *row = hist + (size_t)blockIdx.x * nblocks;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t base = 0; base < nblocks; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? row[i] : 0u;
        const uint32_t x = wave_scan_u32(v);  // inclusive scan within the wave
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        uint32_t off = s_carry;
        for (uint32_t w = 0; w < wave; ++w) off += s_wave[w];
        if (i < nblocks) row[i] = off + x - v;
        __syncthreads();
        if (threadIdx.x == 255) s_carry = off + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = s_carry;
}

// exclusive scan over the workgroup of one value per thread
__device__ __forceinline__ uint32_t sort_scan_block(uint32_t v, uint32_t *s_w) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t x = wave_scan_u32(v);
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t w = 0; w < wave; ++w) off += s_w[w];
    __syncthreads();
    return off + x - v;
}

// SCAN_INLINE (few tiles: the launch-bound small problems): `hist` holds the raw per-tile counts
// and every block sums its digit rows itself -- thread t adds up its rows -- which saves the
// bin_scan launch of the pass.  Thread t looks after the digits [t PER, (t + 1) PER).
// THREADS x ITEMS elements = a sort tile (2,048-element tiles run as 512 threads x 4: twice the waves per SIMD
// of 256 x 8 for a kernel that is a chain of LDS round trips and barriers).
// KeyT = uint32_t: the high words of the keys (section 3e) -- 8-byte instead of 12-byte elements; vals_in = null:
// the values are the positions themselves (the first pass: no identity array is ever written or read).
template <int W, uint32_t THREADS, uint32_t ITEMS, bool SCAN_INLINE, typename KeyT = uint64_t>
__global__ __launch_bounds__(THREADS) void radix_scatter_kernel(
    const KeyT *__restrict__ keys_in, const uint32_t *__restrict__ vals_in,
    KeyT *__restrict__ keys_out, uint32_t *__restrict__ vals_out, uint32_t n, uint32_t shift,
    const uint32_t *__restrict__ hist, const uint32_t *__restrict__ totals, uint32_t nblocks) {
    constexpr uint32_t NB = 1u << W, PER = (NB + THREADS - 1u) / THREADS, TILE = THREADS * ITEMS, NWV = THREADS / 64u;
    __shared__ uint32_t s_cnt[NWV][NB];  // per-wave running digit counts -> exclusive wave offsets
    __shared__ uint32_t s_base[NB];    // global start of each digit + this block's offset in it
    __shared__ uint32_t s_tile[NB], s_w[NWV];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t b0 = threadIdx.x * PER;  // my digits: b0 .. b0 + PER - 1 (none if b0 >= NB)
    for (uint32_t w = 0; w < NWV; ++w)
        for (uint32_t b = threadIdx.x; b < NB; b += THREADS) s_cnt[w][b] = 0;
    {   // exclusive scan of the digit totals (tiny; every block redoes it)
        uint32_t t[PER], mine[PER], sum = 0;  // digit total over all tiles; the tiles before this one
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            const uint32_t d = b0 + q;
            t[q] = mine[q] = 0u;
            if (d < NB) {
                if (SCAN_INLINE) {
                    const uint32_t *row = hist + (size_t)d * nblocks;
                    for (uint32_t b = 0; b < nblocks; ++b) {
                        const uint32_t v = row[b];
                        mine[q] += b < blockIdx.x ? v : 0u;
                        t[q] += v;
                    }
                } else {
                    t[q] = totals[d];
                    mine[q] = hist[d * nblocks + blockIdx.x];
                }
            }
            sum += t[q];
        }
        uint32_t run = sort_scan_block(sum, s_w);
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            if (b0 + q < NB) s_base[b0 + q] = run + mine[q];
            run += t[q];
        }
    }
    __syncthreads();

    const uint32_t base = blockIdx.x * TILE + wave * (64 * ITEMS);
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    KeyT key[ITEMS];
    uint32_t val[ITEMS], local[ITEMS];
#pragma unroll
    for (uint32_t c = 0; c < ITEMS; ++c) {
        const uint32_t i = base + c * 64 + lane;
        const bool valid = i < n;
        key[c] = valid ? keys_in[i] : (KeyT)~(KeyT)0;
        val[c] = !valid ? 0u : vals_in ? vals_in[i] : i;
        const uint32_t d = (uint32_t)(key[c] >> shift) & (NB - 1u);
        // lanes holding the same digit (ballot match over the W digit bits)
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < W; ++b) {
            const uint64_t bal = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? bal : ~bal;
        }
        const uint32_t rank = __popcll(peers & lt_mask);
        const uint32_t before = valid ? s_cnt[wave][d] : 0u;  // same address for all peers
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) s_cnt[wave][d] = before + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        local[c] = before + rank;
    }
    __syncthreads();
    {   // per digit: exclusive prefix over the waves and the digit's count in this tile; then the
        // exclusive scan of the tile's digit counts: where each digit's run starts inside the tile
        uint32_t cnt[PER], sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            cnt[q] = 0;
            if (b0 + q < NB) {
                uint32_t o = 0;
                for (uint32_t w = 0; w < NWV; ++w) {
                    const uint32_t t = s_cnt[w][b0 + q];
                    s_cnt[w][b0 + q] = o;
                    o += t;
                }
                cnt[q] = o;
            }
            sum += cnt[q];
        }
        uint32_t run = sort_scan_block(sum, s_w);
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            if (b0 + q < NB) s_tile[b0 + q] = run;
            run += cnt[q];
        }
    }
    __syncthreads();
    // Stage the tile in LDS in digit order, then write it out with consecutive threads on
    // consecutive elements: each digit's run lands in global memory as one contiguous, coalesced
    // stream instead of 64 scattered 8-byte stores per wave instruction.
    __shared__ KeyT s_key[TILE];
    __shared__ uint32_t s_val[TILE];
#pragma unroll
    for (uint32_t c = 0; c < ITEMS; ++c) {
        const uint32_t i = base + c * 64 + lane;
        if (i < n) {
            const uint32_t d = (uint32_t)(key[c] >> shift) & (NB - 1u);
            const uint32_t pos = s_tile[d] + s_cnt[wave][d] + local[c];
            s_key[pos] = key[c];
            s_val[pos] = val[c];
        }
    }
    __syncthreads();
    const uint32_t tile_n = min(TILE, n - blockIdx.x * TILE);
#pragma unroll
    for (uint32_t c = 0; c < ITEMS; ++c) {
        const uint32_t j = c * THREADS + threadIdx.x;
        if (j < tile_n) {
            const KeyT k = s_key[j];
            const uint32_t d = (uint32_t)(k >> shift) & (NB - 1u);
            const uint32_t dst = s_base[d] + (j - s_tile[d]);
            keys_out[dst] = k;
            vals_out[dst] = s_val[j];
        }
    }
}

// ---- 3c. small problems: the whole sort in ONE launch, by counting ------------------------------
// Up to kRankSortMax bodies a step is bound by its chain of dependent launches (a trivial kernel
// costs ~4.3 us end to end; the radix sort is sixteen of them), not by work.  There the sorted
// position of a body is simply COUNTED: rank(i) = #{ j : (key_j, j) < (key_i, i) } -- the all-pairs
// pattern of the force kernel, on integers: N^2 64-bit compares (6.7e7 at 8,192 bodies, a few
// microseconds on 1,024 SIMDs), ties broken by source index exactly as the stable radix sort breaks
// them.  A workgroup owns 64 bodies; its 16 waves split the j range, each staging its slice in LDS;
// (key_j, j) < (key_i, i) is evaluated as key_j < key_i + [j < i], one compare per pair once a
// wave's j slice lies entirely below or above its bodies.
// (measured per runner.step(), theta 0.75: 8,192 bodies 77.0 us counted / 80.6 radix; 12,288: 84.8 / 84.9;
// 16,384: 93.7 / 89.1 -- the two-pass high-word radix sort with its thread-per-body fix-up takes over there)
constexpr uint32_t kRankSortMax = 12288;
constexpr uint32_t kRankWaves = 16;
constexpr int kRankUnroll = 32;

// (Two workgroups per tile with a ticket for the last to add up and scatter, and the j slices staged
// in LDS instead of read through the scalar cache, were both measured slower.)
__global__ __launch_bounds__(64 * kRankWaves) void rank_sort_kernel(const uint64_t *__restrict__ keys, uint32_t n,
                                                                    uint64_t *__restrict__ keys_out,
                                                                    uint32_t *__restrict__ order) {
    __shared__ uint32_t s_cnt[kRankWaves][64];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t i0 = blockIdx.x * 64u, i = i0 + lane;
    const uint64_t ki = i < n ? keys[i] : ~0ull;
    const uint32_t per = (n + kRankWaves - 1u) / kRankWaves;
    const uint32_t j_lo = min(wave * per, n), j_hi = min(j_lo + per, n);
    uint32_t count = 0;
    // (kRankUnroll keys per round of scalar loads -- wave-uniform addresses go through the scalar
    // cache; a round costs one load latency, so the rounds are made long)
#define NB_COUNT_RANGE(A, B, CMP)                                   \
    {                                                               \
        const uint64_t *kp = keys + (A), *ke = keys + (B);          \
        for (; kp + kRankUnroll <= ke; kp += kRankUnroll) {         \
            uint64_t kk[kRankUnroll];                               \
            _Pragma("unroll") for (int u = 0; u < kRankUnroll; ++u) kk[u] = kp[u]; \
            _Pragma("unroll") for (int u = 0; u < kRankUnroll; ++u) count += (kk[u] CMP ki) ? 1u : 0u; \
        }                                                           \
        for (; kp < ke; ++kp) count += (*kp CMP ki) ? 1u : 0u;      \
    }
    // j below the workgroup's bodies: (key_j, j) < (key_i, i)  <=>  key_j <= key_i
    const uint32_t below_end = min(j_hi, i0);
    if (j_lo < below_end) NB_COUNT_RANGE(j_lo, below_end, <=)
    // the workgroup's own 64 bodies: per-lane tie-break
    const uint32_t own_lo = max(j_lo, i0), own_hi = min(j_hi, min(i0 + 64u, n));
    for (uint32_t j = own_lo; j < own_hi; ++j) {
        const uint64_t kj = keys[j];
        count += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
    }
    // j above: key_j < key_i
    const uint32_t above_lo = max(j_lo, min(i0 + 64u, n));
    if (above_lo < j_hi) NB_COUNT_RANGE(above_lo, j_hi, <)
#undef NB_COUNT_RANGE
    s_cnt[wave][lane] = count;
    __syncthreads();
    if (wave == 0u && i < n) {
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t w = 0; w < kRankWaves; ++w) rank += s_cnt[w][lane];
        keys_out[rank] = ki;
        order[rank] = i;
    }
}

// ---- 3d. large problems: radix passes over the HIGH digits only, then a fix-up of the ties --------
// With N bodies in a cube, two bodies share the top 8 P bits of their keys only if they sit in the
// same cell of level ~8P/3: for P = 4 that is one of 2^31 cells, so after four stable passes over
// bits 32..62 all but a few hundred of a million uniform bodies are already in their final place,
// and the others form short RUNS of equal high bits (in source-index order, the passes being
// stable) that only need sorting among themselves by the low bits.  That replaces the four low
// passes (12 launches) by one: runs_fix_kernel finds the runs and sorts each in
// place -- a wave per run of <= 64 bodies (rank by counting, keys exchanged by shuffles), a
// workgroup per longer run (counting against the whole run, out of place into the idle ping-pong
// buffer, then copied back).  Any input is sorted correctly; a dense cluster just costs O(L^2)
// compares for a run of L.  The result is the stable full-key order, bit for bit the 8-pass sort's.
constexpr uint32_t kRunWave = 64;

constexpr uint32_t kRunItems = 1;  // positions per thread: a workgroup looks at 256 consecutive positions
// A run longer than this is not ranked by counting (L^2 compares by one workgroup: a dense core of 10^5..10^6
// bodies inside a root cube that a few escapers have stretched -- the normal late state of a gravitational
// run -- would take seconds to minutes) but radix-sorted on its low bits by the workgroup: O(L) per digit.
constexpr uint32_t kRunCountMax = 1024;
// The host's part (TreeSim::wait): the longest run of a step comes back through the status words, and the
// next steps sort one more high digit per kRunBoostAbove exceeded -- the fix-up then sees short runs again;
// `probe` tells it when the extra digits can go.  Speed only: every path gives the stable full-key order.
constexpr uint32_t kRunBoostAbove = 1024, kRunProbeSpan = 512;

// The run [start, start + len) of keys that tie on their high bits, sorted in place by the low `low_bits`
// bits, stably, by one workgroup of 256: LSD radix, 8 bits per pass, between the run's own slots in
// (keys, vals) and in (alt_keys, alt_vals).  A pass = a histogram sweep, a scan of the 256 counts, and a
// scatter sweep in chunks of 256 -- a thread per element, ranked among the chunk's equal digits by wave
// ballots and per-wave counts (the scheme of radix_scatter_kernel).  Digits on which the whole run agrees
// are skipped.
__device__ void run_radix_sort(uint64_t *keys, uint32_t *vals, uint64_t *alt_keys, uint32_t *alt_vals, uint32_t start,
                               uint32_t len, uint32_t low_bits, uint32_t *s_hist, uint32_t (*s_wcnt)[256], uint32_t *s_w,
                               uint32_t *s_flag) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint64_t *ks = keys + start, *kd = alt_keys + start;
    uint32_t *vs = vals + start, *vd = alt_vals + start;
    bool in_alt = false;
    for (uint32_t sh = 0; sh < low_bits; sh += 8u) {
        const uint32_t dmask = low_bits - sh >= 8u ? 255u : (1u << (low_bits - sh)) - 1u;
        s_hist[tid] = 0u;
        for (uint32_t w = 0; w < 4u; ++w) s_wcnt[w][tid] = 0u;
        if (tid == 0u) *s_flag = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < len; i += 256u) atomicAdd(&s_hist[(uint32_t)(ks[i] >> sh) & dmask], 1u);
        __syncthreads();
        const uint32_t mine = s_hist[tid];
        if (mine == len) *s_flag = 1u;  // every key of the run has this digit: nothing moves
        const uint32_t base = sort_scan_block(mine, s_w);  // (syncs: s_flag is visible after it)
        if (*s_flag) {
            __syncthreads();
            continue;
        }
        s_hist[tid] = base;  // from here on: where the next key with digit tid goes
        __syncthreads();
        for (uint32_t c0 = 0; c0 < len; c0 += 256u) {
            const uint32_t i = c0 + tid;
            const bool valid = i < len;
            const uint64_t key = valid ? ks[i] : 0ull;
            const uint32_t val = valid ? vs[i] : 0u;
            const uint32_t d = (uint32_t)(key >> sh) & dmask;
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (int bb = 0; bb < 8; ++bb) {
                const uint64_t bal = __ballot((d >> bb) & 1u);
                peers &= ((d >> bb) & 1u) ? bal : ~bal;
            }
            const uint32_t rank = (uint32_t)__popcll(peers & lt_mask);
            if (valid && rank == 0u) s_wcnt[wave][d] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (valid) {
                uint32_t off = s_hist[d] + rank;
                for (uint32_t w = 0; w < wave; ++w) off += s_wcnt[w][d];
                kd[off] = key;
                vd[off] = val;
            }
            __syncthreads();
            {   // thread t looks after digit t: advance its base, clear the chunk's counts
                uint32_t t = 0u;
                for (uint32_t w = 0; w < 4u; ++w) {
                    t += s_wcnt[w][tid];
                    s_wcnt[w][tid] = 0u;
                }
                s_hist[tid] += t;
            }
            __syncthreads();
        }
        __threadfence_block();
        __syncthreads();
        uint64_t *tk = ks; ks = kd; kd = tk;
        uint32_t *tv = vs; vs = vd; vd = tv;
        in_alt = !in_alt;
    }
    if (in_alt) {  // an odd number of passes moved: the sorted run sits in the alternate buffers
        for (uint32_t i = tid; i < len; i += 256u) {
            kd[i] = ks[i];
            vd[i] = vs[i];
        }
        __threadfence_block();
    }
    __syncthreads();
}

// One launch (it was two -- a kernel listing the runs with aggregated atomics, a kernel sorting them -- and
// the lists needed no more than LDS): a workgroup finds the runs that START among its 256 positions and
// sorts them, short ones (< 64 bodies) a wave each, longer ones one after the other with all its threads.
// (A neighbouring workgroup may still be looking for its run starts while this one already permutes a run:
// it only ever compares the HIGH bits of a key, which a permutation inside a run does not change at any
// position, and an aligned 64-bit load sees one key or the other.)
// stat[0]: the longest run met (atomicMax; the launch of the step before zeroed it: stat_clear = the word
// of the other parity).  stat[2], with probe_bits != 0: set if some run of keys that tie on all but their low
// probe_bits bits is longer than kRunProbeSpan -- what the fix-up would meet with one high digit less.
// (The high-word sort has its own fix-up, a thread per body: runs_rank_kernel, section 3e.)
__global__ __launch_bounds__(256) void runs_fix_kernel(uint64_t *keys, uint32_t *__restrict__ vals,
                                                       uint64_t *__restrict__ alt_keys, uint32_t *__restrict__ alt_vals,
                                                       uint32_t n, uint32_t low_bits, uint32_t probe_bits,
                                                       uint32_t *__restrict__ stat, uint32_t *__restrict__ stat_clear) {
    __shared__ uint32_t s_short[256 * kRunItems], s_long[256 * kRunItems / kRunWave + 1], s_n[3];
    __shared__ uint32_t s_hist[256], s_wcnt[4][256], s_w[4], s_flag;
    // the bits a run ties on, and the coarser ones the probe looks at
    auto high = [&](uint32_t k) -> uint64_t { return keys[k] >> low_bits; };
    auto coarse = [&](uint32_t k) -> uint64_t { return keys[k] >> probe_bits; };
    uint64_t *const run_keys = keys;
    if (threadIdx.x < 3u) s_n[threadIdx.x] = 0u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) stat_clear[0] = stat_clear[2] = stat_clear[4] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t c = 0; c < kRunItems; ++c) {
        const uint32_t k = (blockIdx.x * kRunItems + c) * 256u + threadIdx.x;
        if (k + 1u < n) {
            const uint64_t hi = high(k);
            const bool first = k == 0u || high(k - 1u) != hi;
            if (first && high(k + 1u) == hi) {
                // sorted by the high bits: if the body 64 places on still shares them, so do all in between
                if (k + kRunWave < n && high(k + kRunWave) == hi) s_long[atomicAdd(&s_n[1], 1u)] = k;
                else s_short[atomicAdd(&s_n[0], 1u)] = k;
            }
            if (probe_bits && k + kRunProbeSpan < n && coarse(k + kRunProbeSpan) == coarse(k)) s_n[2] = 1u;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u && s_n[2]) atomicMax(&stat[2], 1u);
    const uint32_t lane = threadIdx.x & 63u, n_short = s_n[0], n_long = s_n[1];
    // short runs: one wave each (the order in which the lists were filled does not matter: the runs are disjoint)
    for (uint32_t r = threadIdx.x >> 6; r < n_short; r += 4u) {
        const uint32_t start = s_short[r];
        const uint64_t hi = high(start);
        const uint32_t pos = start + lane;
        const bool in = pos < n && high(min(pos, n - 1u)) == hi;   // (a run is < 64 long here)
        const uint32_t len = (uint32_t)__popcll(__ballot(in));
        const uint64_t ki = in ? keys[pos] : ~0ull;
        const uint32_t vi = in ? vals[pos] : 0u;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < len; ++j) {
            const uint64_t kj = ((uint64_t)(uint32_t)__shfl((int)(ki >> 32), (int)j) << 32) |
                                (uint32_t)__shfl((int)(uint32_t)ki, (int)j);
            rank += (kj < ki || (kj == ki && j < lane)) ? 1u : 0u;
        }
        __builtin_amdgcn_wave_barrier();
        if (in) {
            keys[start + rank] = ki;
            vals[start + rank] = vi;
        }
    }
    // long runs: the whole workgroup, one after the other
    for (uint32_t r = 0; r < n_long; ++r) {
        const uint32_t start = s_long[r];
        const uint64_t hi = high(start);
        uint32_t lo_s = start + kRunWave, hi_s = n;   // first position past the run: binary search
        while (lo_s < hi_s) {
            const uint32_t mid = lo_s + ((hi_s - lo_s) >> 1);
            if (high(mid) == hi) lo_s = mid + 1u; else hi_s = mid;
        }
        const uint32_t len = lo_s - start;
        if (threadIdx.x == 0u) atomicMax(&stat[0], len);
        if (len > kRunCountMax) {
            run_radix_sort(run_keys, vals, alt_keys, alt_vals, start, len, low_bits, s_hist, s_wcnt, s_w, &s_flag);
            continue;
        }
        for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
            const uint64_t ki = run_keys[start + i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < len; ++j) {
                const uint64_t kj = run_keys[start + j];
                rank += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
            }
            alt_keys[start + rank] = ki;
            alt_vals[start + rank] = vals[start + i];
        }
        __threadfence_block();
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
            run_keys[start + i] = alt_keys[start + i];
            vals[start + i] = alt_vals[start + i];
        }
        __syncthreads();
    }
}

// ---- 3e. the fix-up of the high-word sort, a thread per body ----------------------------------------------
// After the passes over (high word, index) the array is sorted by the top bits and every body is either alone
// with its high bits or in a run of ties.  Here EVERY body finds its final place by itself: a singleton
// copies its index across; a body in a run shorter than 64 looks left and right for the run's ends on the
// sorted high words, fetches the full keys of the run's members through their indices and counts how many
// come before it -- (key, place in the run) order, the stable order of the full-key sort.  The result goes OUT
// OF PLACE (vals_out), so no body waits for another: where a quarter of the bodies sit in runs of two or
// three -- one radix pass less than runs_fix_kernel's wave-per-run scheme could afford -- this costs what a
// copy of the index array costs plus a few gathers.  Runs of 64 or more (clustered input) are left to the
// workgroup that holds their first body, as in runs_fix_kernel: ranked by counting up to kRunCountMax, radix-
// sorted beyond, and copied to vals_out.  stat / probe: as runs_fix_kernel.
constexpr uint32_t kRankItems = 1;  // positions per thread (4: -10 us at 4,000,000 bodies, +8 us at 131,072 where most bodies sit in runs)
__global__ __launch_bounds__(256) void runs_rank_kernel(const uint32_t *__restrict__ khi, const uint64_t *__restrict__ keys,
                                                        uint32_t *vals_in, uint32_t *vals_out, uint64_t *run_keys,
                                                        uint64_t *alt_keys, uint32_t n, uint32_t low_bits,
                                                        uint32_t probe_bits, uint32_t *__restrict__ stat,
                                                        uint32_t *__restrict__ stat_clear) {
    __shared__ uint32_t s_long[kRankItems * 256 / kRunWave + 1], s_n[2];
    __shared__ uint32_t s_hist[256], s_wcnt[4][256], s_w[4], s_flag;
    const uint32_t hs = low_bits - 32u;
    if (threadIdx.x < 2u) s_n[threadIdx.x] = 0u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) stat_clear[0] = stat_clear[2] = stat_clear[4] = 0u;
    __syncthreads();
    // kRankItems rounds of 256 consecutive positions per workgroup; what every position needs first -- its high
    // word, its neighbours', its index -- is fetched for all rounds together (independent loads in flight
    // together: the kernel is a chain of short dependent loads otherwise)
    uint32_t hw_[kRankItems], hl_[kRankItems], hr_[kRankItems], val_[kRankItems];
#pragma unroll
    for (uint32_t c = 0; c < kRankItems; ++c) {
        const uint32_t k = (blockIdx.x * kRankItems + c) * 256u + threadIdx.x;
        hw_[c] = k < n ? khi[k] : 0u;
        hl_[c] = k > 0u && k < n ? khi[k - 1u] : 0u;
        hr_[c] = k + 1u < n ? khi[k + 1u] : 0u;
        val_[c] = k < n ? vals_in[k] : 0u;
    }
#pragma unroll
    for (uint32_t c = 0; c < kRankItems; ++c) {
        const uint32_t k = (blockIdx.x * kRankItems + c) * 256u + threadIdx.x;
        if (k >= n) continue;
        const uint32_t hw = hw_[c], hi = hw >> hs;
        const bool left = k > 0u && (hl_[c] >> hs) == hi, right = k + 1u < n && (hr_[c] >> hs) == hi;
        if (!left && !right) {
            vals_out[k] = val_[c];
        } else {
            uint32_t s = k, e = k + 1u;  // the run [s, e), as far as it matters: up to kRunWave places either way
            while (s > 0u && k - s < kRunWave && (khi[s - 1u] >> hs) == hi) --s;
            while (e < n && e - s < kRunWave && (khi[e] >> hs) == hi) ++e;
            if (e - s >= kRunWave) {  // a long run: its first body's workgroup sorts it
                if (!left) s_long[atomicAdd(&s_n[0], 1u)] = k;
            } else {
                const uint32_t mine = val_[c];
                const uint64_t ki = keys[mine];
                uint32_t rank = 0u;
                for (uint32_t j = s; j < e; ++j) {
                    const uint64_t kj = keys[vals_in[j]];
                    rank += (kj < ki || (kj == ki && j < k)) ? 1u : 0u;
                }
                vals_out[s + rank] = mine;
            }
        }
        // (the probe of this kernel COUNTS: bodies whose run, with one digit less, would be a long one)
        if (probe_bits && k + kRunWave < n && (khi[k + kRunWave] >> (probe_bits - 32u)) == (hw >> (probe_bits - 32u)))
            atomicAdd(&s_n[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0u && s_n[1]) atomicAdd(&stat[2], s_n[1]);
    const uint32_t n_long = s_n[0];
    for (uint32_t r = 0; r < n_long; ++r) {
        const uint32_t start = s_long[r];
        const uint32_t hi = khi[start] >> hs;
        uint32_t lo_s = start + kRunWave, hi_s = n;   // first position past the run: binary search
        while (lo_s < hi_s) {
            const uint32_t mid = lo_s + ((hi_s - lo_s) >> 1);
            if ((khi[mid] >> hs) == hi) lo_s = mid + 1u; else hi_s = mid;
        }
        const uint32_t len = lo_s - start;
        if (threadIdx.x == 0u) {
            atomicMax(&stat[0], len);
            atomicAdd(&stat[4], len);  // bodies that took this slow path
        }
        for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) run_keys[start + i] = keys[vals_in[start + i]];
        __threadfence_block();
        __syncthreads();
        if (len > kRunCountMax) {
            run_radix_sort(run_keys, vals_in, alt_keys, vals_out, start, len, low_bits, s_hist, s_wcnt, s_w, &s_flag);
            for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) vals_out[start + i] = vals_in[start + i];
            __syncthreads();
            continue;
        }
        for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
            const uint64_t ki = run_keys[start + i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < len; ++j) {
                const uint64_t kj = run_keys[start + j];
                rank += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
            }
            vals_out[start + rank] = vals_in[start + i];
        }
        __syncthreads();
    }
}
