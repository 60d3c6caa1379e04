// nb_tree_wave.hpp -- part of the nb_tree.hip translation unit: included there, inside its
// namespace nb { namespace {, and never compiled on its own.
// constants, the leapfrog kick / drift and the wave-level scans by DPP.

constexpr int kLevels = 21;            // 3 x 21 = 63 key bits
constexpr int kMaxDepth = kLevels + 1;  // leaves can sit at depth 1..21 (+1 guard)
// bodies per thread of a sort tile: 4 up to kSortSmallMax bodies (more, smaller workgroups: build
// -13 us at 131,072 bodies, -5 at 524,288), 8 beyond (half the histogram rows: -14 us at 2^20, -40 at 2^21)
constexpr uint32_t kSortThreads = 256, kSortItems = 8, kSortItemsSmall = 4, kSortSmallMax = 786432;
constexpr uint32_t kSortBits = 8, kSortWideBits = 9, kSortMaxBins = 1u << kSortWideBits;  // digit widths (the kernels take 7..9)
#ifndef NB_SORT_INLINE_BLOCKS
#define NB_SORT_INLINE_BLOCKS 32
#endif
constexpr uint32_t kSortInlineScanBlocks = NB_SORT_INLINE_BLOCKS;  // up to 32,768 bodies the scatter scans the tile counts itself (-6 %)
// wave-level stack of sibling groups (16 B each, 3 KiB per wave): a depth-first walk pushes at
// most 8 groups per level and pops one, so 7 x 21 + 1 = 148 entries is the most it can hold
constexpr uint32_t kWalkStack = 192;

__device__ __forceinline__ float kick(float v, float a, float dt) {
#pragma clang fp contract(off)
    return v + (a * dt) / 2.0f;  // tree.wgsl:105,108
}
__device__ __forceinline__ float drift(float x, float v, float dt) {
#pragma clang fp contract(off)
    return x + v * dt;  // tree.wgsl:106
}

// ---- wave-level scans by DPP (no LDS round trip) ---------------------------------------------------
#define NB_DPP(old, src, ctrl, row_mask) \
    ((uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(src), (ctrl), (row_mask), 0xf, false))

// inclusive prefix sum over the 64 lanes (row_shr within the 16-lane rows, then the row totals)
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t x) {
    x += NB_DPP(0, x, 0x111, 0xf);  // row_shr:1
    x += NB_DPP(0, x, 0x112, 0xf);  // row_shr:2
    x += NB_DPP(0, x, 0x114, 0xf);  // row_shr:4
    x += NB_DPP(0, x, 0x118, 0xf);  // row_shr:8
    x += NB_DPP(0, x, 0x142, 0xa);  // row_bcast:15 -> rows 1 and 3
    x += NB_DPP(0, x, 0x143, 0xc);  // row_bcast:31 -> rows 2 and 3
    return x;
}

// minimum / maximum over the 64 lanes (the same DPP steps; a lane without a source keeps its own value): in lane 63
__device__ __forceinline__ int wave_min_to_lane63(int v) {
    uint32_t x = (uint32_t)v;
#define NB_STEPM(ctrl, row_mask) x = (uint32_t)min((int)x, (int)NB_DPP(x, x, ctrl, row_mask))
    NB_STEPM(0x111, 0xf); NB_STEPM(0x112, 0xf); NB_STEPM(0x114, 0xf); NB_STEPM(0x118, 0xf);
    NB_STEPM(0x142, 0xa); NB_STEPM(0x143, 0xc);
#undef NB_STEPM
    return (int)x;
}
__device__ __forceinline__ int wave_max_to_lane63(int v) {
    uint32_t x = (uint32_t)v;
#define NB_STEPM(ctrl, row_mask) x = (uint32_t)max((int)x, (int)NB_DPP(x, x, ctrl, row_mask))
    NB_STEPM(0x111, 0xf); NB_STEPM(0x112, 0xf); NB_STEPM(0x114, 0xf); NB_STEPM(0x118, 0xf);
    NB_STEPM(0x142, 0xa); NB_STEPM(0x143, 0xc);
#undef NB_STEPM
    return (int)x;
}

// ... of binary64 values (the moment sums): the two halves move by DPP, the add is a v_add_f64.  Lanes without a
// source in a step add +0.0.  Twelve VALU instructions per step instead of two LDS-crossbar shuffles
// (ds_bpermute) and their ~60-cycle round trip: the scans of cells_a / cells_c were chains of those.
__device__ __forceinline__ double wave_scan_f64(double v) {
    uint32_t lo = (uint32_t)__double_as_longlong(v), hi = (uint32_t)((unsigned long long)__double_as_longlong(v) >> 32);
#define NB_STEP64(ctrl, row_mask)                                                                        \
    {                                                                                                    \
        const uint32_t l2 = NB_DPP(0, lo, ctrl, row_mask), h2 = NB_DPP(0, hi, ctrl, row_mask);           \
        const double s = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)) +        \
                         __longlong_as_double((long long)(((unsigned long long)h2 << 32) | l2));         \
        lo = (uint32_t)__double_as_longlong(s);                                                          \
        hi = (uint32_t)((unsigned long long)__double_as_longlong(s) >> 32);                              \
    }
    NB_STEP64(0x111, 0xf);
    NB_STEP64(0x112, 0xf);
    NB_STEP64(0x114, 0xf);
    NB_STEP64(0x118, 0xf);
    NB_STEP64(0x142, 0xa);
    NB_STEP64(0x143, 0xc);
#undef NB_STEP64
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
