// nb_render.hip -- nb_sim_render: the particle state drawn off screen, on the device
// (include/nbody.h "Renderer"; stands for the draw pass of src/runners/online_renderer.rs:224-367 and
// src/draw.wgsl).  The drawing rule is DESIGN.md 6c: one small triangle per body, every fragment the
// same constant, so the image is a function of an integer coverage count per pixel.
//
//   project   -- float4 position -> clip -> three snapped vertices (24.8 fixed point), IEEE binary32
//                with one rounding per operation (no contraction), or a class: clipped / oversize /
//                non-finite.  Every pass that needs a body's triangle recomputes it from the
//                position (16 B) instead of storing it (24 B).
//   coverage  -- integer edge functions (int64) with the top-left rule folded into a bias, stepped
//                over the pixel centres of the bounding box.
// Two designs accumulate the counts of the small triangles (bounding box <= 32 x 32 pixels); each wins
// one of the reference's two workloads, so both are kept, chosen by frame size x bodies:
//   direct    -- one body per lane walks its box, atomicAdd on the uint32 counts in global memory
//                (after a clear);
//   tiled     -- bodies binned by 64 x 32-pixel screen tile (count / scan / scatter, the counts and
//                the reservation per block through an LDS histogram), then one block per tile
//                accumulates its list with LDS atomics and writes the tile once with plain stores.
// A triangle with a larger box (a body near the eye plane, or a large half_size) goes to a list
// and is walked by a whole block, global atomics, after either design.  A resolve pass turns counts
// into RGBA8 and per-block (sum, max) slabs; a one-block finish adds the slabs in a fixed order.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kBodyBlocks = 1024;   // body passes: at most this many blocks, one contiguous chunk each
constexpr uint32_t kPixelBlocks = 1024;  // resolve: grid-stride beyond
constexpr uint32_t kLargeBlocks = 1024;  // blocks striding over the list of large triangles
constexpr int kSmallBox = 32;            // a lane walks boxes up to this many pixels a side
constexpr uint32_t kTileW = 64, kTileH = 32;      // tiled design: 2048 uint32 counts = 8 KB of LDS
constexpr uint32_t kMaxTiles = 8192;              // its per-block LDS histogram: 32 KB
constexpr double kTiledFrom = 1099511627776.0;   // 2^40 body-pixels: 530,000 bodies at 1920 x 1080
constexpr uint32_t kLut = 256;                    // resolve: colours of counts below this, per block

enum Class : int { kDrawn = 0, kClipped = 1, kOversize = 2, kNonfinite = 3 };
// device words: [0] large triangles listed
// result (uint64 x 8): drawn, clipped, oversize, nonfinite, fragments, max_count
enum { kResDrawn = 0, kResClipped, kResOversize, kResNonfinite, kResFragments, kResMax, kResWords = 8 };

struct RenderConst {
    float m[16];  // view_proj, column-major
    float s;      // half_size
    float wf, hf;
    uint32_t w, h;
    uint32_t tiles_x, tiles;
};

struct ColourConst {
    float om[3];  // 1 - clear
    float l2;     // log2(1 - alpha), not below -1e30
    uint32_t srgb;
};

struct Tri {
    int x[3], y[3];
};

// The three snapped vertices of a body, or why it is not drawn.  DESIGN.md 6c, in its order.
__device__ inline int project(float4 p, const RenderConst &c, Tri &t) {
#pragma clang fp contract(off)
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return kNonfinite;
    const float cx = ((c.m[0] * p.x + c.m[4] * p.y) + c.m[8] * p.z) + c.m[12];
    const float cy = ((c.m[1] * p.x + c.m[5] * p.y) + c.m[9] * p.z) + c.m[13];
    const float cz = ((c.m[2] * p.x + c.m[6] * p.y) + c.m[10] * p.z) + c.m[14];
    const float cw = ((c.m[3] * p.x + c.m[7] * p.y) + c.m[11] * p.z) + c.m[15];
    if (!(cw > 0.f && cz >= 0.f && cz <= cw)) return kClipped;
    const float ox[3] = {-c.s, c.s, 0.f}, oy[3] = {-c.s, -c.s, c.s};
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float nx = (cx + ox[k]) / cw;
        const float ny = (cy + oy[k]) / cw;
        const float sx = (nx * 0.5f + 0.5f) * c.wf;
        const float sy = (0.5f - ny * 0.5f) * c.hf;
        // not below 2^22 (a NaN is not): the fixed-point coordinates would leave int32
        const bool ok = fabsf(sx) < 4194304.f && fabsf(sy) < 4194304.f;
        inside = inside && ok;
        t.x[k] = ok ? (int)rintf(sx * 256.f) : 0;
        t.y[k] = ok ? (int)rintf(sy * 256.f) : 0;
    }
    return inside ? kDrawn : kOversize;
}

// Pixels whose centre (256 i + 128, 256 j + 128) lies in the triangle's bounding box, cut to the
// rectangle [rx0, rx1] x [ry0, ry1]
struct Box {
    int i0, i1, j0, j1;
    __device__ bool empty() const { return i1 < i0 || j1 < j0; }
};

__device__ inline Box pixel_box(const Tri &t, int rx0, int ry0, int rx1, int ry1) {
    const int xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
    const int ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
    Box b;
    b.i0 = max(rx0, (xmin + 127) >> 8);  // ceil((xmin - 128) / 256)
    b.i1 = min(rx1, (xmax - 128) >> 8);  // floor
    b.j0 = max(ry0, (ymin + 127) >> 8);
    b.j1 = min(ry1, (ymax - 128) >> 8);
    return b;
}

// Edge functions with the tie rule folded in: pixel covered iff e[0], e[1], e[2] are all >= 0, where
// e[k] = g (ex (py - ay) - ey (px - ax)) - (the edge is top or left ? 0 : 1).  One pixel to the
// right adds dx[k], one down adds dy[k].  valid is false for zero area.
struct Edges {
    long long e[3], dx[3], dy[3];
    bool valid;
};

__device__ inline Edges edge_setup(const Tri &t, int i, int j) {
    Edges r;
    const long long area = (long long)(t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (long long)(t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
    r.valid = area != 0;
    const long long g = area > 0 ? 1 : -1;
    const long long px = 256ll * i + 128, py = 256ll * j + 128;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = k, b = k == 2 ? 0 : k + 1;
        const long long ex = g * ((long long)t.x[b] - t.x[a]), ey = g * ((long long)t.y[b] - t.y[a]);
        const bool topleft = ey < 0 || (ey == 0 && ex > 0);
        r.e[k] = ex * (py - t.y[a]) - ey * (px - t.x[a]) - (topleft ? 0 : 1);
        r.dx[k] = -256 * ey;
        r.dy[k] = 256 * ex;
    }
    return r;
}

// One lane walks a small box; add(i, j) for every covered pixel.
template <class Add>
__device__ inline void walk_box(const Tri &t, const Box &b, Add add) {
    Edges ed = edge_setup(t, b.i0, b.j0);
    if (!ed.valid) return;
    for (int j = b.j0; j <= b.j1; ++j) {
        long long e0 = ed.e[0], e1 = ed.e[1], e2 = ed.e[2];
        for (int i = b.i0; i <= b.i1; ++i) {
            if ((e0 | e1 | e2) >= 0) add(i, j);
            e0 += ed.dx[0];
            e1 += ed.dx[1];
            e2 += ed.dx[2];
        }
        ed.e[0] += ed.dy[0];
        ed.e[1] += ed.dy[1];
        ed.e[2] += ed.dy[2];
    }
}

__device__ inline bool small_box(const Box &b) { return b.i1 - b.i0 < kSmallBox && b.j1 - b.j0 < kSmallBox; }

// Class counts of a block -> its slab (uint32 x 4: -, clipped, oversize, nonfinite).
__device__ inline void write_class_slab(uint32_t n_clip, uint32_t n_over, uint32_t n_bad, uint32_t *slab) {
    __shared__ uint32_t part[3];
    if (threadIdx.x < 3) part[threadIdx.x] = 0;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        n_clip += __shfl_down(n_clip, off);
        n_over += __shfl_down(n_over, off);
        n_bad += __shfl_down(n_bad, off);
    }
    if ((threadIdx.x & 63) == 0) {  // integer adds: the order does not matter
        atomicAdd(&part[0], n_clip);
        atomicAdd(&part[1], n_over);
        atomicAdd(&part[2], n_bad);
    }
    __syncthreads();
    if (threadIdx.x < 3) slab[blockIdx.x * 4 + 1 + threadIdx.x] = part[threadIdx.x];
}

// ---- direct design ------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void render_direct_kernel(const float4 *__restrict__ posm, uint32_t n,
                                                                   uint32_t chunk, RenderConst c,
                                                                   uint32_t *__restrict__ counts,
                                                                   uint32_t *__restrict__ words,
                                                                   uint32_t *__restrict__ large,
                                                                   uint32_t *__restrict__ slab) {
    uint32_t n_clip = 0, n_over = 0, n_bad = 0;
    const uint32_t begin = blockIdx.x * chunk, end = min(n, begin + chunk);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kThreads) {
        Tri t;
        const int cls = project(posm[i], c, t);
        n_clip += cls == kClipped;
        n_over += cls == kOversize;
        n_bad += cls == kNonfinite;
        if (cls != kDrawn) continue;
        const Box b = pixel_box(t, 0, 0, (int)c.w - 1, (int)c.h - 1);
        if (b.empty()) continue;
        if (!small_box(b)) {
            large[atomicAdd(&words[0], 1u)] = i;
            continue;
        }
        walk_box(t, b, [&](int px, int py) { atomicAdd(&counts[(uint32_t)py * c.w + (uint32_t)px], 1u); });
    }
    write_class_slab(n_clip, n_over, n_bad, slab);
}

// ---- tiled design -------------------------------------------------------------------------------
// SCATTER = false: count the small triangles per tile (tile_count += ...), class slabs, large list.
// SCATTER = true:  the same chunk again: count per tile in LDS, reserve each tile's run of the list
//                  with one global atomic per tile and block, then write the body indices.
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void render_bin_kernel(const float4 *__restrict__ posm, uint32_t n,
                                                                uint32_t chunk, RenderConst c,
                                                                uint32_t *__restrict__ tile_count,  // or cursor
                                                                uint32_t *__restrict__ list,
                                                                uint32_t *__restrict__ words,
                                                                uint32_t *__restrict__ large,
                                                                uint32_t *__restrict__ slab) {
    __shared__ uint32_t hist[kMaxTiles];
    for (uint32_t t = threadIdx.x; t < c.tiles; t += kThreads) hist[t] = 0;
    __syncthreads();
    uint32_t n_clip = 0, n_over = 0, n_bad = 0;
    const uint32_t begin = blockIdx.x * chunk, end = min(n, begin + chunk);
    for (int phase = 0; phase < (SCATTER ? 2 : 1); ++phase) {
        for (uint32_t i = begin + threadIdx.x; i < end; i += kThreads) {
            Tri t;
            const int cls = project(posm[i], c, t);
            if (phase == 0) {
                n_clip += cls == kClipped;
                n_over += cls == kOversize;
                n_bad += cls == kNonfinite;
            }
            if (cls != kDrawn) continue;
            const Box b = pixel_box(t, 0, 0, (int)c.w - 1, (int)c.h - 1);
            if (b.empty()) continue;
            if (!small_box(b)) {
                if (!SCATTER) large[atomicAdd(&words[0], 1u)] = i;
                continue;
            }
            // a box of at most 32 x 32 pixels meets at most 2 x 2 tiles
            const uint32_t tx0 = (uint32_t)b.i0 / kTileW, tx1 = (uint32_t)b.i1 / kTileW;
            const uint32_t ty0 = (uint32_t)b.j0 / kTileH, ty1 = (uint32_t)b.j1 / kTileH;
            for (uint32_t ty = ty0; ty <= ty1; ++ty)
                for (uint32_t tx = tx0; tx <= tx1; ++tx) {
                    const uint32_t tile = ty * c.tiles_x + tx;
                    if (SCATTER && phase == 1)
                        list[atomicAdd(&hist[tile], 1u)] = i;
                    else
                        atomicAdd(&hist[tile], 1u);
                }
        }
        __syncthreads();
        if (phase == 0) {
            for (uint32_t t = threadIdx.x; t < c.tiles; t += kThreads) {
                const uint32_t k = hist[t];
                if (!SCATTER) {
                    if (k) atomicAdd(&tile_count[t], k);
                } else {
                    hist[t] = k ? atomicAdd(&tile_count[t], k) : 0u;  // the block's run of tile t starts here
                }
            }
            __syncthreads();
        }
    }
    if (!SCATTER) write_class_slab(n_clip, n_over, n_bad, slab);
}

// exclusive scan of the tile counts (at most kMaxTiles) into offsets[tiles + 1] and the cursors
__global__ __launch_bounds__(1024) void render_scan_kernel(const uint32_t *__restrict__ tile_count, uint32_t tiles,
                                                             uint32_t *__restrict__ offsets,
                                                             uint32_t *__restrict__ cursor) {
    __shared__ uint32_t sums[1024];
    constexpr uint32_t kPer = kMaxTiles / 1024;
    uint32_t v[kPer], total = 0;
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t t = threadIdx.x * kPer + k;
        v[k] = t < tiles ? tile_count[t] : 0u;
        total += v[k];
    }
    sums[threadIdx.x] = total;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t add = threadIdx.x >= off ? sums[threadIdx.x - off] : 0u;
        __syncthreads();
        sums[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = sums[threadIdx.x] - total;
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t t = threadIdx.x * kPer + k;
        if (t < tiles) {
            offsets[t] = run;
            cursor[t] = run;
        }
        run += v[k];
    }
    if (threadIdx.x == 1023) offsets[tiles] = sums[1023];
}

// one block per tile: its list into LDS counts, then the tile's pixels written once
__global__ __launch_bounds__(kThreads) void render_tile_kernel(const float4 *__restrict__ posm, RenderConst c,
                                                                 const uint32_t *__restrict__ offsets,
                                                                 const uint32_t *__restrict__ list,
                                                                 uint32_t *__restrict__ counts) {
    __shared__ uint32_t acc[kTileW * kTileH];
    for (uint32_t p = threadIdx.x; p < kTileW * kTileH; p += kThreads) acc[p] = 0;
    __syncthreads();
    const uint32_t tile = blockIdx.x;
    const int x0 = (int)((tile % c.tiles_x) * kTileW), y0 = (int)((tile / c.tiles_x) * kTileH);
    const int x1 = min(x0 + (int)kTileW, (int)c.w) - 1, y1 = min(y0 + (int)kTileH, (int)c.h) - 1;
    const uint32_t begin = offsets[tile], end = offsets[tile + 1];
    for (uint32_t e = begin + threadIdx.x; e < end; e += kThreads) {
        Tri t;
        if (project(posm[list[e]], c, t) != kDrawn) continue;  // (listed bodies are drawn)
        const Box b = pixel_box(t, x0, y0, x1, y1);
        if (b.empty()) continue;
        walk_box(t, b, [&](int px, int py) { atomicAdd(&acc[(uint32_t)(py - y0) * kTileW + (uint32_t)(px - x0)], 1u); });
    }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < kTileW * kTileH; p += kThreads) {
        const int px = x0 + (int)(p % kTileW), py = y0 + (int)(p / kTileW);
        if (px <= x1 && py <= y1) counts[(uint32_t)py * c.w + (uint32_t)px] = acc[p];
    }
}

// ---- large triangles: a block per triangle, its threads over the box ---------------------------
__global__ __launch_bounds__(kThreads) void render_large_kernel(const float4 *__restrict__ posm, RenderConst c,
                                                                  const uint32_t *__restrict__ words,
                                                                  const uint32_t *__restrict__ large,
                                                                  uint32_t *__restrict__ counts) {
    const uint32_t count = words[0];
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        Tri t;
        if (project(posm[large[e]], c, t) != kDrawn) continue;
        const Box b = pixel_box(t, 0, 0, (int)c.w - 1, (int)c.h - 1);
        if (b.empty()) continue;
        const Edges ed = edge_setup(t, b.i0, b.j0);
        if (!ed.valid) continue;
        const uint32_t bw = (uint32_t)(b.i1 - b.i0 + 1), total = bw * (uint32_t)(b.j1 - b.j0 + 1);
        for (uint32_t p = threadIdx.x; p < total; p += kThreads) {
            const long long di = p % bw, dj = p / bw;
            const long long e0 = ed.e[0] + di * ed.dx[0] + dj * ed.dy[0];
            const long long e1 = ed.e[1] + di * ed.dx[1] + dj * ed.dy[1];
            const long long e2 = ed.e[2] + di * ed.dx[2] + dj * ed.dy[2];
            if ((e0 | e1 | e2) >= 0) atomicAdd(&counts[(uint32_t)(b.j0 + (int)dj) * c.w + (uint32_t)(b.i0 + (int)di)], 1u);
        }
    }
}

// ---- resolve: counts -> RGBA8, and per-block (sum, max) -----------------------------------------
__device__ inline uint32_t shade(uint32_t k, const ColourConst &cc) {
    const float t = exp2f((float)k * cc.l2);  // (1 - alpha)^k
    uint32_t px = 0xff000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float lin = 1.f - cc.om[ch] * t;
        const float v = !cc.srgb ? lin : lin <= 0.0031308f ? 12.92f * lin : 1.055f * powf(lin, 1.f / 2.4f) - 0.055f;
        px |= (uint32_t)fminf(fmaxf(v * 255.f + 0.5f, 0.f), 255.f) << (8 * ch);
    }
    return px;
}

__global__ __launch_bounds__(kThreads) void render_resolve_kernel(const uint32_t *__restrict__ counts, uint32_t pixels,
                                                                    ColourConst cc, uint32_t *__restrict__ rgba,
                                                                    unsigned long long *__restrict__ slab_sum,
                                                                    uint32_t *__restrict__ slab_max) {
    __shared__ uint32_t lut[kLut];
    __shared__ unsigned long long wsum[kThreads / 64];
    __shared__ uint32_t wmax[kThreads / 64];
    lut[threadIdx.x] = shade(threadIdx.x, cc);
    __syncthreads();
    unsigned long long sum = 0;
    uint32_t mx = 0;
    for (uint32_t p = blockIdx.x * kThreads + threadIdx.x; p < pixels; p += gridDim.x * kThreads) {
        const uint32_t k = counts[p];
        rgba[p] = k < kLut ? lut[k] : shade(k, cc);
        sum += k;
        mx = max(mx, k);
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        mx = max(mx, __shfl_down(mx, off));
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = sum;
        wmax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < kThreads / 64; ++k) {
            sum += wsum[k];
            mx = max(mx, wmax[k]);
        }
        slab_sum[blockIdx.x] = sum;
        slab_max[blockIdx.x] = mx;
    }
}

// one block: the slabs in a fixed order -> res[kResWords]
__global__ __launch_bounds__(kThreads) void render_finish_kernel(const uint32_t *__restrict__ class_slab,
                                                                   uint32_t body_blocks, uint32_t n,
                                                                   const unsigned long long *__restrict__ slab_sum,
                                                                   const uint32_t *__restrict__ slab_max,
                                                                   uint32_t pixel_blocks,
                                                                   unsigned long long *__restrict__ res) {
    __shared__ unsigned long long part[5][kThreads];
    unsigned long long v[5] = {0, 0, 0, 0, 0};  // clipped, oversize, nonfinite, fragments, max
    for (uint32_t b = threadIdx.x; b < body_blocks; b += kThreads)
        for (int k = 0; k < 3; ++k) v[k] += class_slab[b * 4 + 1 + k];
    for (uint32_t b = threadIdx.x; b < pixel_blocks; b += kThreads) {
        v[3] += slab_sum[b];
        v[4] = max(v[4], (unsigned long long)slab_max[b]);
    }
    for (int k = 0; k < 5; ++k) part[k][threadIdx.x] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t t = 1; t < kThreads; ++t) {
            for (int k = 0; k < 4; ++k) v[k] += part[k][t];
            v[4] = max(v[4], part[4][t]);
        }
        res[kResClipped] = v[0];
        res[kResOversize] = v[1];
        res[kResNonfinite] = v[2];
        res[kResDrawn] = (unsigned long long)n - v[0] - v[1] - v[2];
        res[kResFragments] = v[3];
        res[kResMax] = v[4];
        res[6] = res[7] = 0;
    }
}

}  // namespace

struct RenderWork : Workspace {
    DeviceBuf<uint32_t> counts, rgba;            // [pixels] of the largest frame so far
    DeviceBuf<uint32_t> large;                   // [n] bodies whose box a lane does not walk
    DeviceBuf<uint32_t> list;                    // tiled: [4 n] body indices by tile
    DeviceBuf<uint32_t> tiles;                   // tiled: count, cursor [kMaxTiles], offsets [kMaxTiles + 1]
    DeviceBuf<uint32_t> words;                   // [8]
    DeviceBuf<uint32_t> class_slab;              // [kBodyBlocks][4]
    DeviceBuf<unsigned long long> slab_sum;      // [kPixelBlocks]
    DeviceBuf<uint32_t> slab_max;                // [kPixelBlocks]
    DeviceBuf<unsigned long long> res;           // [kResWords]
    PinnedBuf<unsigned long long> h_res;         // as res
    int design = 0;                              // "render_design": 0 automatic, 1 direct, 2 tiled
};

static int render_work(SimBase &sim, RenderWork **w) {
    return workspace(sim, kWorkRender, w, [](RenderWork &f) {
        NB_HIP_TRY(f.tiles.reserve(3 * kMaxTiles + 1));
        NB_HIP_TRY(f.words.reserve(8));
        NB_HIP_TRY(f.class_slab.reserve(4 * kBodyBlocks));
        NB_HIP_TRY(f.slab_sum.reserve(kPixelBlocks));
        NB_HIP_TRY(f.slab_max.reserve(kPixelBlocks));
        NB_HIP_TRY(f.res.reserve(kResWords));
        NB_HIP_TRY(f.h_res.reserve(kResWords));
        return NB_OK;
    });
}

int sim_render_set_design(SimBase &sim, int design) {
    if (design < 0 || design > 2) {
        set_error("render_design: 0 (automatic), 1 (direct) or 2 (tiled), not %d", design);
        return NB_ERR_INVALID;
    }
    if (int rc = sim.bind_device()) return rc;
    RenderWork *w = nullptr;
    if (int rc = render_work(sim, &w)) return rc;
    w->design = design;
    return NB_OK;
}

// (the arguments were checked by nb_sim_render)
int sim_render(SimBase &sim, const nb_render_params &rp, uint8_t *rgba, uint32_t *counts, nb_render_stats *stats) {
    if (int rc = analysis_begin(sim, "render")) return rc;
    RenderWork *work = nullptr;
    if (int rc = render_work(sim, &work)) return rc;
    RenderWork &w = *work;
    const uint32_t n = sim.n;
    const size_t pixels = (size_t)rp.width * rp.height;

    RenderConst c{};
    std::memcpy(c.m, rp.view_proj, sizeof c.m);
    c.s = rp.half_size;
    c.wf = (float)rp.width;
    c.hf = (float)rp.height;
    c.w = rp.width;
    c.h = rp.height;
    c.tiles_x = (rp.width + kTileW - 1) / kTileW;
    const size_t tiles = (size_t)c.tiles_x * ((rp.height + kTileH - 1) / kTileH);
    c.tiles = (uint32_t)std::min<size_t>(tiles, kMaxTiles);
    ColourConst cc{};
    for (int k = 0; k < 3; ++k) cc.om[k] = 1.f - rp.clear[k];
    cc.l2 = rp.alpha < 1.f ? (float)std::max(-1e30, std::log2(1.0 - (double)rp.alpha)) : -1e30f;
    cc.srgb = (rp.flags & NB_RENDER_SRGB) != 0;

    // The tiled design needs its per-block histogram of the tiles in LDS; 0 bodies need no binning.
    // Left to itself the renderer bins once the frame is large: the direct design's time grows with the
    // fragments (bodies x pixels a body covers, which grows with W H), the tiled design's with the
    // bodies.  Measured crossings (profiles/render_bench.txt): 2e11 - 7e11 body-pixels for a uniform
    // cloud; a disc, whose few central tiles hold most of the bodies, crosses at 4e11 - 8e11 at
    // 1920 x 1080 and not at all up to 1.6 M bodies at 1280 x 720.
    const bool can_tile = n > 0 && tiles <= kMaxTiles;
    const bool tiled = can_tile && (w.design == 2 || (w.design == 0 && (double)n * (double)pixels >= kTiledFrom));
    if (w.design == 2 && !tiled && n > 0) {
        set_error("render: the tiled design holds at most %u tiles of %u x %u pixels (%zu asked)", kMaxTiles, kTileW,
                  kTileH, tiles);
        return NB_ERR_UNSUPPORTED;
    }
    NB_HIP_TRY(w.counts.reserve(pixels));
    NB_HIP_TRY(w.rgba.reserve(pixels));
    NB_HIP_TRY(w.large.reserve(n));
    if (tiled) NB_HIP_TRY(w.list.reserve(4 * (size_t)n));

    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    const hipStream_t s = sim.stream;
    uint32_t chunk = (n + kBodyBlocks - 1) / kBodyBlocks;
    chunk = std::max(kThreads, (chunk + kThreads - 1) / kThreads * kThreads);
    const uint32_t body_blocks = n ? (n + chunk - 1) / chunk : 0;
    uint32_t *tile_count = w.tiles, *cursor = w.tiles + kMaxTiles, *offsets = w.tiles + 2 * kMaxTiles;

    NB_HIP_TRY(hipMemsetAsync(w.words, 0, sizeof(uint32_t) * 8, s));
    if (!tiled) {
        NB_HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * pixels, s));
        if (n)
            hipLaunchKernelGGL(render_direct_kernel, dim3(body_blocks), dim3(kThreads), 0, s, posm, n, chunk, c,
                               w.counts, w.words, w.large, w.class_slab);
    } else {
        NB_HIP_TRY(hipMemsetAsync(tile_count, 0, sizeof(uint32_t) * c.tiles, s));
        hipLaunchKernelGGL(render_bin_kernel<false>, dim3(body_blocks), dim3(kThreads), 0, s, posm, n, chunk, c,
                           tile_count, w.list, w.words, w.large, w.class_slab);
        hipLaunchKernelGGL(render_scan_kernel, dim3(1), dim3(1024), 0, s, tile_count, c.tiles, offsets, cursor);
        hipLaunchKernelGGL(render_bin_kernel<true>, dim3(body_blocks), dim3(kThreads), 0, s, posm, n, chunk, c, cursor,
                           w.list, w.words, w.large, w.class_slab);
        hipLaunchKernelGGL(render_tile_kernel, dim3(c.tiles), dim3(kThreads), 0, s, posm, c, offsets, w.list,
                           w.counts);
    }
    NB_HIP_TRY(hipGetLastError());
    if (n) hipLaunchKernelGGL(render_large_kernel, dim3(kLargeBlocks), dim3(kThreads), 0, s, posm, c, w.words, w.large, w.counts);
    const uint32_t pixel_blocks = (uint32_t)std::min<size_t>(kPixelBlocks, (pixels + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(pixel_blocks), dim3(kThreads), 0, s, w.counts, (uint32_t)pixels, cc,
                       w.rgba, w.slab_sum, w.slab_max);
    hipLaunchKernelGGL(render_finish_kernel, dim3(1), dim3(kThreads), 0, s, w.class_slab, body_blocks, n, w.slab_sum,
                       w.slab_max, pixel_blocks, w.res);
    NB_HIP_TRY(hipGetLastError());
    NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(unsigned long long) * kResWords, hipMemcpyDeviceToHost, s));
    if (rgba) NB_HIP_TRY(hipMemcpyAsync(rgba, w.rgba, 4 * pixels, hipMemcpyDeviceToHost, s));
    if (counts) NB_HIP_TRY(hipMemcpyAsync(counts, w.counts, sizeof(uint32_t) * pixels, hipMemcpyDeviceToHost, s));
    NB_HIP_TRY(hipStreamSynchronize(s));
    if (int rc = sim.diag_status()) return rc;
    if (stats) {
        nb_render_stats st{};
        st.step_num = sim.step_num;
        st.n = n;
        st.drawn = w.h_res[kResDrawn];
        st.clipped = w.h_res[kResClipped];
        st.oversize = w.h_res[kResOversize];
        st.nonfinite = w.h_res[kResNonfinite];
        st.fragments = w.h_res[kResFragments];
        st.max_count = (uint32_t)w.h_res[kResMax];
        *stats = st;
    }
    return NB_OK;
}

}  // namespace nb
