// nb_smooth.hip -- nb_sim_smooth_map: the smoothed image of a simulator's current state, every body spread
// over the pixels of a 2-D grid with a kernel of its own radius (include/nbody.h "Smoothed maps", DESIGN.md 6j;
// no reference counterpart).
//
// A gather, not a scatter: the pixels of an 8 x 8 tile (one lane of a wave each) walk the list of the bodies
// whose support can touch the tile and decide themselves, by the rule's one comparison, which of them they take.
//   count     -- one thread per body (the float4 SoA state of SimBase::diag_state and the caller's s[]): fp64,
//                no contraction; the body's class, and the clipped rectangle of tiles its bounding square can
//                touch, widened so that rounding can never drop a reaching pixel (tile_rect).  A tile that turns
//                out untouched costs a list entry and adds nothing;
//   offsets   -- an exclusive scan of the bodies' tile counts: every block of 1,024 bodies, then the blocks.
//                The total E is the one number the host reads before the end: the entry buffers are sized by it,
//                not by n (E > NB_SMOOTH_MAX_ENTRIES is refused there, with nothing written);
//   emit      -- one thread per entry finds its body in the offsets (two binary searches) and writes the tile
//                key and the body index: the entries are in body order, a body's tiles in row-major order;
//   group     -- the stable sort of nb_analysis_sort.hpp on the tile key.  Its first pass numbers the entries
//                itself, so the sorted index is an entry's position and the body is read through it;
//   lists     -- first and last position of every tile and the lists cut into segments of at most
//                "smooth_segment_len" entries, numbered by a scan, exactly as nb_map.hip cuts its lists;
//   sum       -- one block of 256 threads per segment stages 256 entries at a time in LDS (a, b, s2, K / s2, m and
//                the velocity terms, recomputed from the gathered body).  Thread (q, c) = (tid / 64, tid % 64)
//                walks quarter q's 64 staged bodies in list order for pixel c; a quarter is a wave, and one ballot
//                per staged body tells whether any pixel took it (hit[], the exact `deposited`).  The quarters
//                are added in order; a one-segment tile is stored directly, longer lists go through partials that
//                the combine kernel adds in segment order.  Pixels of a border tile outside the grid are masked;
//   finish    -- the bodies' classes and masses through per-block slabs, the maximum count and the sum of the
//                counts, all in a fixed order.
// No float atomics; the cuts depend on n, the grid, s, the segment length and the lists' lengths alone: the
// result is bitwise reproducible.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kTile = 8, kTilePixels = kTile * kTile;  // one pixel a lane
constexpr uint32_t kGlobalFields = 8;                       // see GlobalField
constexpr uint32_t kMaxFields = 6;                          // planes with NB_SMOOTH_VELOCITY
constexpr uint32_t kMaxBlocks = 1024;                       // of the pass over the counts: grid-stride beyond
// res: [0, 6) the centre and velocity used, then the global sums, the maximum count, the sum of the counts
constexpr uint32_t kUsed = 8, kResMax = kUsed + kGlobalFields, kResPairs = kResMax + 1, kResDoubles = kResPairs + 1;
static_assert(kTilePixels == kWave, "a quarter of the sum block is one wave: the ballot below");

enum GlobalField { kGBad = 0, kGBadS, kGRaised, kGLowered, kGSkipped, kGDeposited, kGMass, kGDepositedMass };
enum BodyClass : uint32_t { kClsEligible = 1, kClsBad = 2, kClsBadS = 4, kClsRaised = 8, kClsLowered = 16 };

struct SmoothConst {
    double c[3], vc[3], n[3], e1[3], e2[3];
    double xlo, xhi, ylo, yhi, dlo, dhi, dx, dy, s_min, s_max;
    uint32_t w, h, tiles_x, tiles_y, tiles;
    uint32_t center_com;
};

// What the rule forms of a body before any pixel is looked at
struct Placed {
    double a, b, h, s_eff;
};

__device__ inline Placed place(float4 p, double s, const SmoothConst &k, const double (&c)[3]) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    Placed o;
    o.a = (dx * k.e1[0] + dy * k.e1[1]) + dz * k.e1[2];
    o.b = (dx * k.e2[0] + dy * k.e2[1]) + dz * k.e2[2];
    o.h = (dx * k.n[0] + dy * k.n[1]) + dz * k.n[2];
    o.s_eff = s < k.s_min ? k.s_min : (s > k.s_max ? k.s_max : s);  // (a NaN stays)
    return o;
}

// The pixels [*i0, *i1] of one axis whose centre can lie within s of a: false when there is none.  Centre i is
// lo + (i + 1/2) d up to a few ulps of the window's bounds, so the pixels are those with (a - s - lo) / d - 1/2 <
// i < (a + s - lo) / d - 1/2.  The range is taken a whole pixel wider on either side than floor() of the
// quotients, after the interval itself has been widened by 2^-50 of every magnitude that went into it: far
// more than the roundings of the sum, the quotient and the centres can move it.  Never used to decide: the
// sum's comparison does.
__device__ inline bool pixel_range(double a, double s, double lo, double hi, double d, uint32_t cells, uint32_t *i0,
                                   uint32_t *i1) {
    const double e = 0x1p-50 * (((fabs(a) + s) + fabs(lo)) + fabs(hi));
    const double g0 = floor((((a - s) - e) - lo) / d) - 1.0, g1 = floor((((a + s) + e) - lo) / d) + 1.0;
    if (!(g1 >= 0.0) || !(g0 <= (double)(cells - 1))) return false;  // (a NaN: none)
    *i0 = g0 <= 0.0 ? 0u : (uint32_t)g0;
    *i1 = g1 >= (double)(cells - 1) ? cells - 1 : (uint32_t)g1;
    return true;
}

// rect = (first tile column, first tile row, columns, rows) of the tiles a body can touch; false: none
__device__ inline bool tile_rect(const Placed &b, const SmoothConst &k, uint32_t (&rect)[4]) {
    if (!(b.h >= k.dlo && b.h < k.dhi)) return false;
    uint32_t i0, i1, j0, j1;
    if (!pixel_range(b.a, b.s_eff, k.xlo, k.xhi, k.dx, k.w, &i0, &i1)) return false;
    if (!pixel_range(b.b, b.s_eff, k.ylo, k.yhi, k.dy, k.h, &j0, &j1)) return false;
    rect[0] = i0 / kTile;
    rect[1] = j0 / kTile;
    rect[2] = i1 / kTile - rect[0] + 1;
    rect[3] = j1 / kTile - rect[1] + 1;
    return true;
}

// ---- count: cls[i], rect[i] and ntiles[i] for every body ----------------------------------------------------
// mom: the finished moments of nb_diag.hip (NB_SMOOTH_CENTER_COM) or null.  Block 0 also writes the centre and
// velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kThreads) void smooth_count_kernel(const float4 *__restrict__ posm,
                                                                const float4 *__restrict__ vel,
                                                                const double *__restrict__ s, uint32_t n,
                                                                SmoothConst k, const double *__restrict__ mom,
                                                                uint32_t *__restrict__ cls, uint2 *__restrict__ rects,
                                                                uint32_t *__restrict__ ntiles,
                                                                double *__restrict__ used) {
    double c[3], vc[3];
    centre_used(k.c, k.vc, k.center_com, mom, used, c, vc);
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i], v = vel[i];
    const double si = s[i];
    uint32_t klass = 0, count = 0, rect[4] = {0, 0, 0, 0};
    if (!body_ok(p, v)) {
        klass = kClsBad;
    } else if (si != si) {
        klass = kClsBadS;
    } else {
        klass = kClsEligible | (si < k.s_min ? kClsRaised : 0u) | (si > k.s_max ? kClsLowered : 0u);
        if (tile_rect(place(p, si, k, c), k, rect)) count = rect[2] * rect[3];
    }
    cls[i] = klass;
    rects[i] = make_uint2(rect[0] | (rect[1] << 16), rect[2] | (rect[3] << 16));
    ntiles[i] = count;
}

// ---- offsets: off[i] = the tiles of the bodies of i's block of 1,024 before i; block_tot[b] the block's ------
__global__ __launch_bounds__(kScanThreads) void smooth_offsets_local_kernel(const uint32_t *__restrict__ ntiles,
                                                                            uint32_t n, uint32_t *__restrict__ off,
                                                                            uint32_t *__restrict__ block_tot) {
    __shared__ uint32_t lds[2 * kScanThreads];
    const uint32_t tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * kScanThreads + tid;
    const uint32_t x = i < n ? ntiles[i] : 0u;  // (at most 2^18 each: a block's sum is below 2^32)
    uint32_t *a = lds, *b = lds + kScanThreads;
    a[tid] = x;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {  // inclusive, Hillis-Steele
        b[tid] = tid >= o ? a[tid] + a[tid - o] : a[tid];
        __syncthreads();
        uint32_t *t = a;
        a = b;
        b = t;
    }
    if (i < n) off[i] = a[tid] - x;
    if (tid == kScanThreads - 1) block_tot[blockIdx.x] = a[tid];
}

// ... and block_base[b] = the tiles of the blocks before b, block_base[blocks] = *total = all of them, in 64 bits:
// one block, thread t owning a run of blocks
__global__ __launch_bounds__(kScanThreads) void smooth_offsets_blocks_kernel(const uint32_t *__restrict__ block_tot,
                                                                             uint32_t blocks,
                                                                             unsigned long long *__restrict__ block_base,
                                                                             unsigned long long *__restrict__ total) {
    __shared__ unsigned long long lds[2 * kScanThreads];
    const uint32_t tid = threadIdx.x, per = (blocks + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = std::min(blocks, tid * per), hi = std::min(blocks, lo + per);
    unsigned long long s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += block_tot[i];
    unsigned long long *a = lds, *b = lds + kScanThreads;
    a[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {
        b[tid] = tid >= o ? a[tid] + a[tid - o] : a[tid];
        __syncthreads();
        unsigned long long *t = a;
        a = b;
        b = t;
    }
    unsigned long long run = a[tid] - s;
    for (uint32_t i = lo; i < hi; ++i) {
        block_base[i] = run;
        run += block_tot[i];
    }
    if (tid == kScanThreads - 1) {
        block_base[blocks] = a[tid];
        *total = a[tid];
    }
}

// ---- emit: entry e = (tile key, body), one thread each ------------------------------------------------------
// The body of entry e is the last one whose offset is <= e among those with tiles: first its block of 1,024 in
// block_base, then its place in the block's offsets.
__global__ __launch_bounds__(kThreads) void smooth_emit_kernel(const uint32_t *__restrict__ off,
                                                               const unsigned long long *__restrict__ block_base,
                                                               const uint2 *__restrict__ rects, uint32_t n,
                                                               uint32_t blocks, uint32_t entries, uint32_t tiles_x,
                                                               uint32_t tiles, uint32_t *__restrict__ keys,
                                                               uint32_t *__restrict__ entry_body) {
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= entries) return;
    uint32_t lo = 0, hi = blocks;  // the last block with block_base <= e (block_base[0] = 0): in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (block_base[mid] <= e) lo = mid; else hi = mid;
    }
    const uint32_t local = (uint32_t)(e - block_base[lo]);
    const uint32_t first = lo * kScanThreads;
    uint32_t l = first, h = std::min<uint32_t>(n, first + kScanThreads);
    while (h - l > 1) {
        const uint32_t mid = l + (h - l) / 2;
        if (off[mid] <= local) l = mid; else h = mid;
    }
    // (bodies without tiles share their successor's offset: the last of equal offsets is the one with tiles)
    const uint2 r = rects[l];
    const uint32_t tx0 = r.x & 0xffffu, ty0 = r.x >> 16, nx = r.y & 0xffffu, q = local - off[l];
    if (nx == 0 || q >= nx * (r.y >> 16)) return;  // (cannot happen: the offsets were made from these counts)
    const uint32_t tile = (ty0 + q / nx) * tiles_x + tx0 + q % nx;
    keys[e] = tile < tiles ? tile : tiles - 1;
    entry_body[e] = l;
}

// ---- lists: tile t's entries are positions [first[t], last[t]) of the sorted keys (0, 0: none) ---------------
__global__ __launch_bounds__(kThreads) void smooth_bounds_kernel(const uint32_t *__restrict__ keys, uint32_t entries,
                                                                 uint32_t tiles, uint32_t *__restrict__ first,
                                                                 uint32_t *__restrict__ last) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= entries) return;
    const uint32_t t = keys[i];
    const uint32_t tp = i > 0 ? keys[i - 1] : 0xffffffffu;
    if (t != tp) {
        if (t < tiles) first[t] = (uint32_t)i;
        if (i > 0 && tp < tiles) last[tp] = (uint32_t)i;
    }
    if (i + 1 == entries && t < tiles) last[t] = entries;
}

__device__ inline uint32_t segments_of(uint32_t len, uint32_t seg_len) { return (len + seg_len - 1) / seg_len; }

// seg_off[t] = segments of the tiles before t, seg_off[tiles] = all; part_off likewise, counting only the
// segments of tiles with more than one (they go through partials); seg_tile[g] = the tile of segment g.  Two
// launches of ceil((tiles + 1) / 1024) blocks, as in nb_map.hip.
__global__ __launch_bounds__(kScanThreads) void smooth_segments_local_kernel(const uint32_t *__restrict__ first,
                                                                             const uint32_t *__restrict__ last,
                                                                             uint32_t tiles, uint32_t seg_len,
                                                                             uint32_t *__restrict__ seg_off,
                                                                             uint32_t *__restrict__ part_off,
                                                                             uint32_t *__restrict__ block_tot) {
    __shared__ uint32_t lds[2][2 * kScanThreads];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * kScanThreads + tid;
    const uint32_t s = t < tiles ? segments_of(last[t] - first[t], seg_len) : 0u, p = s > 1 ? s : 0u;
    uint32_t *a0 = lds[0], *b0 = lds[0] + kScanThreads, *a1 = lds[1], *b1 = lds[1] + kScanThreads;
    a0[tid] = s;
    a1[tid] = p;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {  // inclusive, Hillis-Steele, both sums at once
        b0[tid] = tid >= o ? a0[tid] + a0[tid - o] : a0[tid];
        b1[tid] = tid >= o ? a1[tid] + a1[tid - o] : a1[tid];
        __syncthreads();
        uint32_t *x = a0;
        a0 = b0;
        b0 = x;
        x = a1;
        a1 = b1;
        b1 = x;
    }
    if (t <= tiles) {
        seg_off[t] = a0[tid] - s;
        part_off[t] = a1[tid] - p;
    }
    if (tid == kScanThreads - 1) {
        block_tot[2 * blockIdx.x] = a0[tid];
        block_tot[2 * blockIdx.x + 1] = a1[tid];
    }
}

__global__ __launch_bounds__(kScanThreads) void smooth_segments_final_kernel(const uint32_t *__restrict__ first,
                                                                             const uint32_t *__restrict__ last,
                                                                             uint32_t tiles, uint32_t seg_len,
                                                                             uint32_t *__restrict__ seg_off,
                                                                             uint32_t *__restrict__ part_off,
                                                                             const uint32_t *__restrict__ block_tot,
                                                                             uint32_t *__restrict__ seg_tile,
                                                                             uint32_t seg_cap) {
    __shared__ uint32_t before[2];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * kScanThreads + tid;
    if (tid < 2) {  // (at most 67 blocks)
        uint32_t sum = 0;
        for (uint32_t b = 0; b < blockIdx.x; ++b) sum += block_tot[2 * b + tid];
        before[tid] = sum;
    }
    __syncthreads();
    if (t > tiles) return;
    const uint32_t g0 = seg_off[t] + before[0];
    seg_off[t] = g0;
    part_off[t] += before[1];
    if (t == tiles) return;
    const uint32_t g1 = g0 + segments_of(last[t] - first[t], seg_len);
    for (uint32_t g = g0; g < g1 && g < seg_cap; ++g) seg_tile[g] = t;
}

// ---- sum: one block per segment ------------------------------------------------------------------------------
// What is staged of an entry's body: a, b, s2 = s_eff s_eff (0: no body, nothing is below it), ks = K / s2, m,
// and with F = 6 ua, ub, w, u2 = (ux ux + uy uy) + uz uz.
template <uint32_t F>
constexpr uint32_t staged_fields() {
    return F > 1 ? 9 : 5;
}
enum Staged { kSA = 0, kSB, kSS2, kSKs, kSM, kSUa, kSUb, kSW, kSU2 };

// planes: [F][h * w]; parts: [slot][F + 1][64] doubles (the count last), slot = part_off[tile] + segment
template <uint32_t F>
__global__ __launch_bounds__(kThreads) void smooth_sum_kernel(const float4 *__restrict__ posm,
                                                              const float4 *__restrict__ vel,
                                                              const double *__restrict__ s, SmoothConst k,
                                                              const double *__restrict__ xc,
                                                              const double *__restrict__ yc,
                                                              const uint32_t *__restrict__ idx,
                                                              const uint32_t *__restrict__ entry_body,
                                                              const uint32_t *__restrict__ first,
                                                              const uint32_t *__restrict__ last,
                                                              const uint32_t *__restrict__ seg_off,
                                                              const uint32_t *__restrict__ part_off,
                                                              const uint32_t *__restrict__ seg_tile, uint32_t seg_len,
                                                              uint32_t n, uint32_t entries, uint32_t part_cap,
                                                              const double *__restrict__ used,
                                                              uint32_t *__restrict__ hit, uint32_t *__restrict__ counts,
                                                              double *__restrict__ planes, double *__restrict__ parts) {
#pragma clang fp contract(off)
    constexpr uint32_t S = staged_fields<F>();
    static_assert(S >= F, "the staging area also carries the quarters' sums");
    __shared__ double stage[S][kThreads];   // [staged field][staged body]; at the end [plane][thread]
    __shared__ uint32_t body_in[kThreads];  // the staged body; at the end the thread's count
    const uint32_t g = blockIdx.x;
    if (g >= seg_off[k.tiles]) return;  // (uniform over the block)
    const uint32_t tid = threadIdx.x, tile = seg_tile[g];
    if (tile >= k.tiles) return;
    const uint32_t sg = g - seg_off[tile];
    const uint32_t t0 = first[tile], t1 = last[tile];
    const uint32_t lo = t0 + sg * seg_len, hi = t1 - lo > seg_len ? lo + seg_len : t1;
    const uint32_t nseg = segments_of(t1 - t0, seg_len);
    double c[3], vc[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = used[a];
        vc[a] = used[3 + a];
    }
    const uint32_t pix = tid % kTilePixels, q0 = tid & ~(kTilePixels - 1);
    const uint32_t x = (tile % k.tiles_x) * kTile + pix % kTile, y = (tile / k.tiles_x) * kTile + pix / kTile;
    const bool on_grid = x < k.w && y < k.h;
    const double px = on_grid ? xc[x] : 0.0, py = on_grid ? yc[y] : 0.0;
    double acc[F];
    for (uint32_t f = 0; f < F; ++f) acc[f] = 0.0;
    uint32_t cnt = 0;
    for (uint32_t j0 = lo; j0 < hi; j0 += kThreads) {
        const uint32_t j = j0 + tid;
        double st[S];
        for (uint32_t f = 0; f < S; ++f) st[f] = 0.0;
        uint32_t body = 0;
        if (j < hi) {
            const uint32_t e = idx[j];
            if (e < entries) body = entry_body[e];
            if (e < entries && body < n) {
                const float4 p = posm[body];
                const Placed b = place(p, s[body], k, c);
                const double s2 = b.s_eff * b.s_eff;
                st[kSA] = b.a;
                st[kSB] = b.b;
                st[kSS2] = s2;
                st[kSKs] = NB_SMOOTH_K / s2;
                st[kSM] = (double)p.w;
                if constexpr (F > 1) {
                    const float4 v = vel[body];
                    const double ux = (double)v.x - vc[0], uy = (double)v.y - vc[1], uz = (double)v.z - vc[2];
                    st[kSUa] = (ux * k.e1[0] + uy * k.e1[1]) + uz * k.e1[2];
                    st[kSUb] = (ux * k.e2[0] + uy * k.e2[1]) + uz * k.e2[2];
                    st[kSW] = (ux * k.n[0] + uy * k.n[1]) + uz * k.n[2];
                    st[kSU2] = (ux * ux + uy * uy) + uz * uz;
                }
            } else {
                body = 0;
            }
        }
        for (uint32_t f = 0; f < S; ++f) stage[f][tid] = st[f];
        body_in[tid] = body;
        __syncthreads();
        const uint32_t staged = std::min(hi - j0, kThreads);  // (uniform over the block)
        const uint32_t i1 = std::min(q0 + kTilePixels, staged);
        for (uint32_t i = q0; i < i1; ++i) {  // (uniform over the wave)
            const double s2 = stage[kSS2][i];
            const double da = px - stage[kSA][i], db = py - stage[kSB][i];
            const double r2 = da * da + db * db;
            const bool reach = on_grid && r2 < s2;
            if (__ballot(reach) != 0ull && pix == 0) hit[body_in[i]] = 1u;  // (s2 > 0: a real body)
            if (reach) {
                const double t = 1.0 - r2 / s2;
                const double wgt = stage[kSKs][i] * (t * t);
                const double wm = stage[kSM][i] * wgt;
                acc[0] += wm;
                if constexpr (F > 1) {
                    const double w = stage[kSW][i];
                    acc[1] += wm * stage[kSUa][i];
                    acc[2] += wm * stage[kSUb][i];
                    acc[3] += wm * w;
                    acc[4] += (wm * w) * w;
                    acc[5] += wm * stage[kSU2][i];
                }
                ++cnt;
            }
        }
        __syncthreads();  // the staged bodies have been read
    }
    // the four quarters of every pixel, in order
    for (uint32_t f = 0; f < F; ++f) stage[f][tid] = acc[f];
    body_in[tid] = cnt;
    __syncthreads();
    if (tid >= kTilePixels) return;
    double sum[F];
    for (uint32_t f = 0; f < F; ++f) {
        sum[f] = stage[f][tid];
        for (uint32_t q = kTilePixels; q < kThreads; q += kTilePixels) sum[f] += stage[f][q + tid];
    }
    for (uint32_t q = kTilePixels; q < kThreads; q += kTilePixels) cnt += body_in[q + tid];
    if (nseg > 1) {
        const size_t slot = (size_t)part_off[tile] + sg;
        if (slot >= part_cap) return;
        double *p = parts + slot * (F + 1) * kTilePixels;
        for (uint32_t f = 0; f < F; ++f) p[f * kTilePixels + tid] = sum[f];
        p[F * kTilePixels + tid] = (double)cnt;
        return;
    }
    if (on_grid) {
        const size_t cell = (size_t)y * k.w + x, cells = (size_t)k.w * k.h;
        counts[cell] = cnt;
        for (uint32_t f = 0; f < F; ++f) planes[f * cells + cell] = sum[f];
    }
}

// combine: the block of a longer list's first segment adds the list's partials in segment order
template <uint32_t F>
__global__ __launch_bounds__(kTilePixels) void smooth_combine_kernel(SmoothConst k, const uint32_t *__restrict__ first,
                                                                     const uint32_t *__restrict__ last,
                                                                     const uint32_t *__restrict__ seg_off,
                                                                     const uint32_t *__restrict__ part_off,
                                                                     const uint32_t *__restrict__ seg_tile,
                                                                     uint32_t seg_len, uint32_t part_cap,
                                                                     const double *__restrict__ parts,
                                                                     uint32_t *__restrict__ counts,
                                                                     double *__restrict__ planes) {
    const uint32_t g = blockIdx.x;
    if (g >= seg_off[k.tiles]) return;
    const uint32_t tid = threadIdx.x, tile = seg_tile[g];
    if (tile >= k.tiles || g != seg_off[tile]) return;
    const uint32_t nseg = segments_of(last[tile] - first[tile], seg_len);
    if (nseg < 2 || (size_t)part_off[tile] + nseg > part_cap) return;
    const double *p = parts + (size_t)part_off[tile] * (F + 1) * kTilePixels;
    double sum[F + 1];
    for (uint32_t f = 0; f <= F; ++f) sum[f] = p[f * kTilePixels + tid];
    for (uint32_t sg = 1; sg < nseg; ++sg) {
        p += (F + 1) * kTilePixels;
        for (uint32_t f = 0; f <= F; ++f) sum[f] += p[f * kTilePixels + tid];
    }
    const uint32_t x = (tile % k.tiles_x) * kTile + tid % kTile, y = (tile / k.tiles_x) * kTile + tid / kTile;
    if (x < k.w && y < k.h) {
        const size_t cell = (size_t)y * k.w + x, cells = (size_t)k.w * k.h;
        counts[cell] = (uint32_t)sum[F];  // (exact: below 2^32)
        for (uint32_t f = 0; f < F; ++f) planes[f * cells + cell] = sum[f];
    }
}

// ---- finish ----------------------------------------------------------------------------------------------------
// tally: one slab row of kGlobalFields doubles per block of bodies, from the classes of the count kernel and the
// sum's hit[]
__global__ __launch_bounds__(kThreads) void smooth_tally_kernel(const float4 *__restrict__ posm,
                                                                const uint32_t *__restrict__ cls,
                                                                const uint32_t *__restrict__ hit, uint32_t n,
                                                                double *__restrict__ slabs) {
    __shared__ double part[kThreads / kWave][kGlobalFields];
    double glob[kGlobalFields];
    for (uint32_t f = 0; f < kGlobalFields; ++f) glob[f] = 0.0;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        const uint32_t klass = cls[i];
        if (klass & kClsBad) {
            glob[kGBad] = 1.0;
        } else {
            const double m = posm[i].w;
            glob[kGMass] = m;
            if (klass & kClsBadS) {
                glob[kGBadS] = 1.0;
            } else {
                if (klass & kClsRaised) glob[kGRaised] = 1.0;
                if (klass & kClsLowered) glob[kGLowered] = 1.0;
                if (hit[i]) {
                    glob[kGDeposited] = 1.0;
                    glob[kGDepositedMass] = m;
                } else {
                    glob[kGSkipped] = 1.0;
                }
            }
        }
    }
    block_row<kGlobalFields, kGlobalFields>(glob, part, slabs + (size_t)blockIdx.x * kGlobalFields);
}

// the maximum and the sum of the counts per block (the sum is exact in a double: below 2^53)
__global__ __launch_bounds__(kThreads) void smooth_counts_kernel(const uint32_t *__restrict__ counts, size_t cells,
                                                                 uint32_t *__restrict__ block_max,
                                                                 double *__restrict__ block_sum) {
    __shared__ uint32_t m[kThreads];
    __shared__ unsigned long long t[kThreads];
    uint32_t best = 0;
    unsigned long long sum = 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += (size_t)gridDim.x * kThreads) {
        best = std::max(best, counts[i]);
        sum += counts[i];
    }
    m[threadIdx.x] = best;
    t[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            m[threadIdx.x] = std::max(m[threadIdx.x], m[threadIdx.x + o]);
            t[threadIdx.x] += t[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_max[blockIdx.x] = m[0];
        block_sum[blockIdx.x] = (double)t[0];
    }
}

// res[f] = sum over the tally blocks of slab element f, by sum_over_blocks in 32 groups; res[kGlobalFields] = the
// maximum of block_max, res[kGlobalFields + 1] = the sum of block_sum (integers: exact in any order).
__global__ __launch_bounds__(kThreads) void smooth_finish_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                                 const uint32_t *__restrict__ block_max,
                                                                 const double *__restrict__ block_sum,
                                                                 uint32_t max_blocks, double *__restrict__ res) {
    constexpr uint32_t kGroups = kThreads / kGlobalFields;
    __shared__ double pp[kGroups][kGlobalFields];
    __shared__ uint32_t m[kThreads];
    __shared__ double t[kThreads];
    const uint32_t tid = threadIdx.x;
    uint32_t best = 0;
    double pairs = 0.0;
    for (uint32_t b = tid; b < max_blocks; b += kThreads) {
        best = std::max(best, block_max[b]);
        pairs += block_sum[b];
    }
    m[tid] = best;
    t[tid] = pairs;
    const double sum = sum_over_blocks<kGroups>(slabs, blocks, kGlobalFields, tid % kGlobalFields, pp);
    if (tid < kGlobalFields) res[tid] = sum;
    if (tid == kThreads - 1) {
        uint32_t r = 0;
        double all = 0.0;
        for (uint32_t q = 0; q < kThreads; ++q) {
            r = std::max(r, m[q]);
            all += t[q];
        }
        res[kGlobalFields] = (double)r;
        res[kGlobalFields + 1] = all;
    }
}

uint32_t bits_of(uint32_t x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

}  // namespace

struct SmoothWork : Workspace {  // (all but the last four grow to the largest call so far)
    DeviceBuf<double> s;                     // [n] the caller's smoothing lengths
    DeviceBuf<double> centres;               // [w + h] xc then yc
    DeviceBuf<uint32_t> cls, ntiles, off, hit;  // [n]
    DeviceBuf<uint2> rects;                  // [n]
    DeviceBuf<uint32_t> off_tot;             // [blocks of the offsets scan]
    DeviceBuf<unsigned long long> off_base;  // [those + 1]
    SortBufs<uint32_t> sort;                 // the two sides of (tile key, entry), the histogram: [E]
    DeviceBuf<uint32_t> entry_body;          // [E]
    DeviceBuf<uint32_t> first, last;         // [tiles]
    DeviceBuf<uint32_t> seg_off, part_off;   // [tiles + 1]
    DeviceBuf<uint32_t> seg_tile;            // [segments possible]
    DeviceBuf<uint32_t> block_tot;           // [blocks of the segment scan][2]
    DeviceBuf<double> parts;                 // [partial slots][fields + 1][64]
    DeviceBuf<double> slabs;                 // [tally blocks][kGlobalFields]
    DeviceBuf<uint32_t> counts;              // [cells]
    DeviceBuf<double> planes;                // [fields][cells]
    PinnedBuf<double> h_centres;             // as centres
    DeviceBuf<uint32_t> block_max;           // [kMaxBlocks]
    DeviceBuf<double> block_sum;             // [kMaxBlocks]
    DeviceBuf<double> res;                   // [kResDoubles]
    DeviceBuf<unsigned long long> total;     // [1] E
    PinnedBuf<double> h_res;                 // as res
    PinnedBuf<unsigned long long> h_total;   // as total
};

namespace {

// At least `count` elements behind b.  A failure leaves b empty and the simulator usable: the sticky error
// is cleared.
template <class T, bool P>
int smooth_reserve(Buf<T, P> &b, size_t count) {
    if (b.reserve(count) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("smooth_map: cannot allocate %zu bytes of workspace", sizeof(T) * count);
    return NB_ERR_ALLOC;
}

template <uint32_t F>
int launch_sums(SimBase &sim, SmoothWork &w, const SmoothConst &k, const float4 *posm, const float4 *vel,
                const uint32_t *idx, uint32_t entries, uint32_t seg_len, uint32_t seg_cap, uint32_t part_cap) {
    const uint32_t *first = w.first, *last = w.last, *seg_off = w.seg_off, *part_off = w.part_off;
    const uint32_t *seg_tile = w.seg_tile, *entry_body = w.entry_body;
    const double *s = w.s, *xc = w.centres, *yc = w.centres + k.w;
    hipLaunchKernelGGL(smooth_sum_kernel<F>, dim3(seg_cap), dim3(kThreads), 0, sim.stream, posm, vel, s, k, xc, yc, idx,
                       entry_body, first, last, seg_off, part_off, seg_tile, seg_len, sim.n, entries, part_cap,
                       (const double *)w.res, (uint32_t *)w.hit, (uint32_t *)w.counts, (double *)w.planes,
                       (double *)w.parts);
    NB_HIP_TRY(hipGetLastError());
    if (part_cap > 0) {
        hipLaunchKernelGGL(smooth_combine_kernel<F>, dim3(seg_cap), dim3(kTilePixels), 0, sim.stream, k, first, last,
                           seg_off, part_off, seg_tile, seg_len, part_cap, (const double *)w.parts,
                           (uint32_t *)w.counts, (double *)w.planes);
        NB_HIP_TRY(hipGetLastError());
    }
    return NB_OK;
}

}  // namespace

int sim_smooth_map(SimBase &sim, const nb_smooth_params &params, const SmoothPlan &plan, const double *s,
                   uint32_t *counts, double *planes, nb_smooth_stats *stats) {
    if (int rc = analysis_begin(sim, "smooth_map")) return rc;
    if (!counts && !planes && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    SmoothWork *work = nullptr;
    if (int rc = workspace(sim, kWorkSmooth, &work, [](SmoothWork &f) {
            if (f.block_max.reserve(kMaxBlocks) != hipSuccess || f.block_sum.reserve(kMaxBlocks) != hipSuccess ||
                f.res.reserve(kResDoubles) != hipSuccess || f.h_res.reserve(kResDoubles) != hipSuccess ||
                f.total.reserve(1) != hipSuccess || f.h_total.reserve(1) != hipSuccess) {
                (void)hipGetLastError();
                set_error("smooth_map: cannot allocate the result workspace");
                return NB_ERR_ALLOC;
            }
            return NB_OK;
        }))
        return rc;
    SmoothWork &w = *work;
    const uint32_t n = sim.n, width = params.width, height = params.height;
    const bool com = (params.flags & NB_SMOOTH_CENTER_COM) != 0, velocity = (params.flags & NB_SMOOTH_VELOCITY) != 0;
    const uint32_t fields = velocity ? kMaxFields : 1;
    const size_t cells = (size_t)width * height;

    SmoothConst k{};
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
        k.n[a] = plan.frame.n[a];
        k.e1[a] = plan.frame.e1[a];
        k.e2[a] = plan.frame.e2[a];
    }
    k.xlo = params.x_range[0];
    k.xhi = params.x_range[1];
    k.ylo = params.y_range[0];
    k.yhi = params.y_range[1];
    k.dlo = params.depth_range[0];
    k.dhi = params.depth_range[1];
    k.dx = plan.frame.dx;
    k.dy = plan.frame.dy;
    k.s_min = params.s_min;
    k.s_max = params.s_max;
    k.w = width;
    k.h = height;
    k.tiles_x = (width + kTile - 1) / kTile;
    k.tiles_y = (height + kTile - 1) / kTile;
    k.tiles = k.tiles_x * k.tiles_y;
    k.center_com = com;

    std::memset(w.h_res, 0, sizeof(double) * kResDoubles);
    uint64_t entries64 = 0;
    if (n > 0) {
        const uint32_t seg_len = (uint32_t)sim.smooth_segment_len;
        const uint32_t body_blocks = (n + kThreads - 1) / kThreads;
        const uint32_t off_blocks = (n + kScanThreads - 1) / kScanThreads;
        if (int rc = smooth_reserve(w.s, n)) return rc;
        if (int rc = smooth_reserve(w.centres, (size_t)width + height)) return rc;
        if (int rc = smooth_reserve(w.h_centres, (size_t)width + height)) return rc;
        if (int rc = smooth_reserve(w.cls, n)) return rc;
        if (int rc = smooth_reserve(w.ntiles, n)) return rc;
        if (int rc = smooth_reserve(w.off, n)) return rc;
        if (int rc = smooth_reserve(w.hit, n)) return rc;
        if (int rc = smooth_reserve(w.rects, n)) return rc;
        if (int rc = smooth_reserve(w.off_tot, off_blocks)) return rc;
        if (int rc = smooth_reserve(w.off_base, (size_t)off_blocks + 1)) return rc;

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        std::memcpy(w.h_centres, plan.xc.data(), sizeof(double) * width);
        std::memcpy(w.h_centres + width, plan.yc.data(), sizeof(double) * height);
        NB_HIP_TRY(hipMemcpyAsync(w.centres, w.h_centres, sizeof(double) * ((size_t)width + height),
                                  hipMemcpyHostToDevice, sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(w.s, s, sizeof(double) * n, hipMemcpyHostToDevice, sim.stream));
        hipLaunchKernelGGL(smooth_count_kernel, dim3(body_blocks), dim3(kThreads), 0, sim.stream, posm, vel,
                           (const double *)w.s, n, k, mom, (uint32_t *)w.cls, (uint2 *)w.rects, (uint32_t *)w.ntiles,
                           (double *)w.res);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(smooth_offsets_local_kernel, dim3(off_blocks), dim3(kScanThreads), 0, sim.stream,
                           (const uint32_t *)w.ntiles, n, (uint32_t *)w.off, (uint32_t *)w.off_tot);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(smooth_offsets_blocks_kernel, dim3(1), dim3(kScanThreads), 0, sim.stream,
                           (const uint32_t *)w.off_tot, off_blocks, (unsigned long long *)w.off_base,
                           (unsigned long long *)w.total);
        NB_HIP_TRY(hipGetLastError());
        // the one number read before the end: the entry buffers are sized by it
        NB_HIP_TRY(hipMemcpyAsync(w.h_total, w.total, sizeof(unsigned long long), hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        if (int rc = sim.diag_status()) return rc;
        entries64 = *w.h_total;
        if (entries64 > NB_SMOOTH_MAX_ENTRIES) {
            set_error("smooth_map: %llu tile entries, more than NB_SMOOTH_MAX_ENTRIES = %llu: lower s_max (%g, %.1f x %.1f "
                      "pixels) or coarsen the grid",
                      (unsigned long long)entries64, (unsigned long long)NB_SMOOTH_MAX_ENTRIES, params.s_max,
                      params.s_max / k.dx, params.s_max / k.dy);
            return NB_ERR_UNSUPPORTED;
        }
        const uint32_t entries = (uint32_t)entries64;
        if (int rc = smooth_reserve(w.slabs, (size_t)kGlobalFields * body_blocks)) return rc;
        if (int rc = smooth_reserve(w.counts, cells)) return rc;
        if (int rc = smooth_reserve(w.planes, fields * cells)) return rc;
        NB_HIP_TRY(hipMemsetAsync(w.hit, 0, sizeof(uint32_t) * n, sim.stream));
        NB_HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * cells, sim.stream));
        NB_HIP_TRY(hipMemsetAsync(w.planes, 0, sizeof(double) * fields * cells, sim.stream));
        if (entries > 0) {
            const SortShape shape = sort_shape(entries);
            const uint32_t passes = std::max(1u, (bits_of(k.tiles - 1) + 7) / 8);  // keys run 0 .. tiles - 1
            // segments: a tile with entries has at most 1 + (len - 1) / seg_len; those of longer lists number
            // at most 2 (len / seg_len)
            const uint32_t seg_cap = std::min(k.tiles, entries) + entries / seg_len;
            const uint32_t part_cap = 2 * (entries / seg_len);
            const uint32_t entry_blocks = (entries + kThreads - 1) / kThreads;
            const uint32_t list_blocks = (k.tiles + 1 + kScanThreads - 1) / kScanThreads;
            if (int rc = w.sort.reserve(entries, shape, [](auto &b, size_t count) { return smooth_reserve(b, count); }))
                return rc;
            if (int rc = smooth_reserve(w.entry_body, entries)) return rc;
            if (int rc = smooth_reserve(w.first, k.tiles)) return rc;
            if (int rc = smooth_reserve(w.last, k.tiles)) return rc;
            if (int rc = smooth_reserve(w.seg_off, (size_t)k.tiles + 1)) return rc;
            if (int rc = smooth_reserve(w.part_off, (size_t)k.tiles + 1)) return rc;
            if (int rc = smooth_reserve(w.seg_tile, seg_cap)) return rc;
            if (int rc = smooth_reserve(w.block_tot, (size_t)2 * list_blocks)) return rc;
            if (int rc = smooth_reserve(w.parts, std::max<size_t>(1, part_cap) * (fields + 1) * kTilePixels)) return rc;

            hipLaunchKernelGGL(smooth_emit_kernel, dim3(entry_blocks), dim3(kThreads), 0, sim.stream,
                               (const uint32_t *)w.off, (const unsigned long long *)w.off_base, (const uint2 *)w.rects,
                               n, off_blocks, entries, k.tiles_x, k.tiles, (uint32_t *)w.sort.keys[0],
                               (uint32_t *)w.entry_body);
            NB_HIP_TRY(hipGetLastError());
            if (int rc = enqueue_sort(sim.stream, w.sort, entries, shape, passes, 0, nullptr)) return rc;
            const uint32_t *keys = w.sort.keys[passes & 1], *idx = w.sort.idx[passes & 1];
            NB_HIP_TRY(hipMemsetAsync(w.first, 0, sizeof(uint32_t) * k.tiles, sim.stream));
            NB_HIP_TRY(hipMemsetAsync(w.last, 0, sizeof(uint32_t) * k.tiles, sim.stream));
            hipLaunchKernelGGL(smooth_bounds_kernel, dim3(entry_blocks), dim3(kThreads), 0, sim.stream, keys, entries,
                               k.tiles, (uint32_t *)w.first, (uint32_t *)w.last);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(smooth_segments_local_kernel, dim3(list_blocks), dim3(kScanThreads), 0, sim.stream,
                               (const uint32_t *)w.first, (const uint32_t *)w.last, k.tiles, seg_len,
                               (uint32_t *)w.seg_off, (uint32_t *)w.part_off, (uint32_t *)w.block_tot);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(smooth_segments_final_kernel, dim3(list_blocks), dim3(kScanThreads), 0, sim.stream,
                               (const uint32_t *)w.first, (const uint32_t *)w.last, k.tiles, seg_len,
                               (uint32_t *)w.seg_off, (uint32_t *)w.part_off, (const uint32_t *)w.block_tot,
                               (uint32_t *)w.seg_tile, seg_cap);
            NB_HIP_TRY(hipGetLastError());
            if (int rc = velocity
                             ? launch_sums<kMaxFields>(sim, w, k, posm, vel, idx, entries, seg_len, seg_cap, part_cap)
                             : launch_sums<1>(sim, w, k, posm, vel, idx, entries, seg_len, seg_cap, part_cap))
                return rc;
        }
        hipLaunchKernelGGL(smooth_tally_kernel, dim3(body_blocks), dim3(kThreads), 0, sim.stream, posm,
                           (const uint32_t *)w.cls, (const uint32_t *)w.hit, n, (double *)w.slabs);
        NB_HIP_TRY(hipGetLastError());
        const uint32_t max_blocks = (uint32_t)std::min<size_t>(kMaxBlocks, (cells + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(smooth_counts_kernel, dim3(max_blocks), dim3(kThreads), 0, sim.stream,
                           (const uint32_t *)w.counts, cells, (uint32_t *)w.block_max, (double *)w.block_sum);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(smooth_finish_kernel, dim3(1), dim3(kThreads), 0, sim.stream, (const double *)w.slabs,
                           body_blocks, (const uint32_t *)w.block_max, (const double *)w.block_sum, max_blocks,
                           w.res + kUsed);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(double) * kResDoubles, hipMemcpyDeviceToHost, sim.stream));
        if (counts)
            NB_HIP_TRY(hipMemcpyAsync(counts, w.counts, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, sim.stream));
        if (planes)
            NB_HIP_TRY(hipMemcpyAsync(planes, w.planes, sizeof(double) * fields * cells, hipMemcpyDeviceToHost,
                                      sim.stream));
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    } else {
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        centre_used_empty(w.h_res, com, k.c, k.vc);
        if (counts) std::memset(counts, 0, sizeof(uint32_t) * cells);
        if (planes) std::memset(planes, 0, sizeof(double) * fields * cells);
    }
    if (int rc = sim.diag_status()) return rc;

    if (stats) {
        const double *used = w.h_res, *g = w.h_res + kUsed;
        nb_smooth_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = (uint64_t)g[kGBad];
        o.bad_smoothing = (uint64_t)g[kGBadS];
        o.skipped = (uint64_t)g[kGSkipped];
        o.deposited = (uint64_t)g[kGDeposited];
        o.raised = (uint64_t)g[kGRaised];
        o.lowered = (uint64_t)g[kGLowered];
        o.pairs = (uint64_t)w.h_res[kResPairs];
        o.tile_entries = entries64;
        o.mass = g[kGMass];
        o.deposited_mass = g[kGDepositedMass];
        for (int a = 0; a < 3; ++a) {
            o.center[a] = used[a];
            o.velocity[a] = used[3 + a];
            o.n_hat[a] = plan.frame.n[a];
            o.e1[a] = plan.frame.e1[a];
            o.e2[a] = plan.frame.e2[a];
        }
        o.s_min = params.s_min;
        o.s_max = params.s_max;
        o.width = width;
        o.height = height;
        o.flags = params.flags;
        o.max_count = (uint32_t)w.h_res[kResMax];
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
