// nb_tree_cells.hpp -- part of the nb_tree.hip translation unit: included there, inside its
// namespace nb { namespace {, and never compiled on its own.
// stages 4-6: gather and push kernels, cells from key prefixes, node ids, moments, node contents,
// and the AoS conversions of the read-back.

// ---- 4. gather into sorted (DFS) order ----------------------------------------------------------
// positions/masses first (the build needs them), velocities/accelerations separately (only the
// walk needs them): on several GPUs the second pair is still being all-gathered while the build runs
__global__ void gather_va_kernel(const uint32_t *__restrict__ order, uint32_t n,
                                 const float4 *__restrict__ vel_in, const float4 *__restrict__ acc_in,
                                 float4 *__restrict__ vel_out, float4 *__restrict__ acc_out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t s = order[k];
    vel_out[k] = vel_in[s];
    acc_out[k] = acc_in[s];
}

// one-process multi-GPU runner (nb_group.cpp), replicated tree: the rank's new position / velocity /
// acceleration slices stored into every peer's arrays through peer access, one launch
struct PushDst {
    float4 *p[3][kMaxPeers];
    uint32_t n;
};
__global__ __launch_bounds__(256) void push_slices_kernel(const float4 *__restrict__ a, const float4 *__restrict__ b,
                                                          const float4 *__restrict__ c, PushDst dst, uint32_t first,
                                                          uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float4 va = a[first + i], vb = b[first + i], vc = c[first + i];
    for (uint32_t q = 0; q < dst.n; ++q) {
        dst.p[0][q][first + i] = va;
        dst.p[1][q][first + i] = vb;
        dst.p[2][q][first + i] = vc;
    }
}

// ... a few words (the rank's row of an all-gathered LET table) into every peer's copy of the table
struct PushWords {
    uint32_t *p[kMaxPeers];
    uint32_t n;
};
__global__ void push_words_kernel(const uint32_t *__restrict__ src, PushWords dst, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = src[first + i];
    for (uint32_t q = 0; q < dst.n; ++q) dst.p[q][first + i] = v;
}

// ---- 5. cells from key prefixes -----------------------------------------------------------------
// common prefix length in LEVELS of two keys (identical keys are clamped to kLevels-1 so that
// every cell still has a depth <= kLevels; see the header about colliding keys)
__device__ __forceinline__ int cpl_levels(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    if (x == 0) return kLevels - 1;
    const int lead = __clzll((long long)x) - 1;  // the key occupies bits 62..0
    return lead / 3;
}

// exclusive scan of one value per thread over a 256-thread workgroup
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t *s_wave,
                                                             uint32_t *total) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t x = wave_scan_u32(v);
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t w = 0; w < wave; ++w) off += s_wave[w];
    if (total) *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return off + x - v;
}

// depth of the cells body k opens / owns
__device__ __forceinline__ bool starts_node_at(int left, int right, int d) {
    const bool internal = d > left && d <= right;           // first body of a >=2-body cell
    const bool leaf = d == (left > right ? left : right) + 1;  // alone from this depth on
    return internal || leaf;
}

// the record of an internal cell's slot (cells_c_kernel -> fill_kernel): the node id below its depth
constexpr uint32_t kSlotDepthShift = 27, kSlotIdMask = (1u << kSlotDepthShift) - 1u;

// What the walk reads per cell, in one 32-byte scalar load: centre of gravity + mass, and the
// link {first child id, child count} (leaf: {sorted position of its body, 0}).
struct __attribute__((aligned(32))) NodeRec {
    float4 cogm;
    uint32_t first, count;  // children ids first .. first+count-1 (octant order); leaf: count 0
    uint32_t self_pos;      // leaf: sorted position of its body; cell: ~0 (matches no body)
    float mac2;             // cell: its squared ACCEPTANCE RADIUS, size^2 / theta^2 with size^2 = root_width^2 / 4^depth
                            // (tree.wgsl:82; rounded once here, so that every test of the cell -- each body's own,
                            // the group's all-open shortcut, a LET export's box test -- compares the same number
                            // with its r^2: size/dist < theta (tree.wgsl:63-64) as mac2 < r^2);
                            // leaf: -1, which makes the test always true; a cell of mass 0: +inf, never true
};

// ---- 6a. mass moments by prefix sums ------------------------------------------------------------
// A cell's bodies are a contiguous run [k, end) of the sorted order, so its mass and centre of
// gravity follow from exclusive prefix sums of (m x, m y, m z, m) over the sorted bodies:
// sum = P[end] - P[k].  The sums are kept in binary64 -- a difference of fp32 prefix sums would
// lose the small cells at the far end of the array (N eps relative error); in binary64 the
// result is the correctly rounded moment to ~1e-10, where the reference's own sequential fp32
// sum (tree.rs:486-505) is only good to ~1e-6.
struct Moments {
    double x, y, z, m;
};
__device__ __forceinline__ Moments operator+(const Moments &a, const Moments &b) {
    return Moments{a.x + b.x, a.y + b.y, a.z + b.z, a.m + b.m};
}
__device__ __forceinline__ Moments block_scan_moments(Moments v, Moments *s_wave, Moments *total) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Moments x{wave_scan_f64(v.x), wave_scan_f64(v.y), wave_scan_f64(v.z), wave_scan_f64(v.m)};
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    Moments off{0, 0, 0, 0};
    for (uint32_t w = 0; w < wave; ++w) off = off + s_wave[w];
    if (total) *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return Moments{off.x + x.x - v.x, off.y + x.y - v.y, off.z + x.z - v.z, off.m + x.m - v.m};
}

// ---- 5b/6a fused: cells, node ids and moment prefixes in three launches --------------------------
// Round 1 ran this as thirteen small kernels (gather, cpl, three scans of the opened-cell counts,
// depth histogram + scan + bases, ids, two moment passes + scan); it is one prefix computation
// over the sorted bodies with a 28-word state: 1 count of opened cells, 23 per-depth node counts,
// 4 binary64 moments.  A: per tile of 1,024 bodies, gather + cpl + the tile's totals.  B: the
// tiles' totals scanned, a workgroup per table row and per moment component (fixed order:
// deterministic moments).  C: the depth bases and the node count from the rows' totals, then per
// tile the bodies' own prefixes inside the tile + the tile's offsets -> node ids, slots and moment
// prefixes.  Any number of tiles: no size cap.
constexpr uint32_t kCellTile = 1024;                 // bodies per workgroup of A and C: 4 rounds of 256 (1 round
                                                     // = 256 bodies on small problems, which are bound by the
                                                     // chain of barriers inside a workgroup, not by work)
constexpr uint32_t kCellRows = kMaxDepth + 2;        // u32 rows of the tile table: [0] nint, [1 + d] depth d

// GATHER (section 3e: the sort moved high words and indices only): `keys` are the UNSORTED keys, a body's key is
// gathered through `order` like its position, and the sorted key array the later kernels search is written
// here (keys_out); the neighbours' keys come from the neighbouring lanes.
template <bool GATHER>
__global__ __launch_bounds__(256) void cells_a_kernel(
    const uint32_t *__restrict__ order, uint32_t n, const float4 *__restrict__ posm_in,
    float4 *__restrict__ posm_out, const uint64_t *__restrict__ keys, uint64_t *__restrict__ keys_out,
    int8_t *__restrict__ cpl,
    uint32_t *__restrict__ tile_u32, Moments *__restrict__ tile_mom, uint32_t stride, uint32_t rounds,
    uint32_t *__restrict__ status) {
    __shared__ uint32_t s_hist[kCellRows];
    __shared__ Moments s_wave[4];
    if (threadIdx.x < kCellRows) s_hist[threadIdx.x] = 0;
    __syncthreads();
    Moments msum{0, 0, 0, 0};
    uint32_t nint_sum = 0, collide = 0;
    for (uint32_t sub = 0; sub < rounds; ++sub) {
        const uint32_t k = (blockIdx.x * rounds + sub) * 256u + threadIdx.x;
        Moments item{0, 0, 0, 0};
        uint64_t me = 0, me_prev = 0, me_next = 0;
        uint32_t src = 0;
        if (k < n) {
            src = order[k];
            me = GATHER ? keys[src] : keys[k];
        }
        if (GATHER) {  // (outside the bounds check: every lane takes part in the shuffles)
            const uint32_t lane = threadIdx.x & 63u;
            me_prev = ((uint64_t)(uint32_t)__shfl_up((int)(me >> 32), 1) << 32) | (uint32_t)__shfl_up((int)(uint32_t)me, 1);
            me_next = ((uint64_t)(uint32_t)__shfl_down((int)(me >> 32), 1) << 32) | (uint32_t)__shfl_down((int)(uint32_t)me, 1);
            if (lane == 0u && k > 0u && k < n) me_prev = keys[order[k - 1u]];
            if (lane == 63u && k + 1u < n) me_next = keys[order[k + 1u]];
        }
        if (k < n) {
            const float4 p = posm_in[src];  // sort_particles, tree.rs:564-602
            posm_out[k] = p;
            const double m = (double)p.w;
            item = Moments{(double)p.x * m, (double)p.y * m, (double)p.z * m, m};
            if (GATHER) keys_out[k] = me;
            else {
                me_prev = k > 0 ? keys[k - 1] : 0ull;
                me_next = k + 1 < n ? keys[k + 1] : 0ull;
            }
            const int left = k > 0 ? cpl_levels(me_prev, me) : -1;
            // (a lone body: the reference's root is always an internal octant -- the queue starts with the
            // root partition whatever it holds, tree.rs:463-476 -- so the body's leaf sits at depth 1)
            const int right = k + 1 < n ? cpl_levels(me, me_next) : (n == 1u ? 0 : -1);
            if (k == 0) cpl[0] = -1;
            cpl[k + 1] = (int8_t)right;
            nint_sum += right > left ? (uint32_t)(right - left) : 0u;  // internal cells this body opens
            // (LDS atomics, 256 of a round on two or three words: a loop over the wave's depths with ballots, one add
            // per wave and depth, measured SLOWER -- 15.9 -> 19.3 us at 2^20 bodies)
            for (int d = left + 1; d <= right; ++d) atomicAdd(&s_hist[1 + d], 1u);
            atomicAdd(&s_hist[1 + (left > right ? left : right) + 1], 1u);  // its leaf
            if (k + 1 < n && me_next == me) collide += 1u;
        }
        msum = msum + item;  // (per thread over its rounds; the workgroup's total once, below)
    }
    {   // the tile's moments: the threads' sums added in a fixed order (wave scan, then the waves in order)
        Moments total;
        (void)block_scan_moments(msum, s_wave, &total);
        msum = total;
    }
    if (nint_sum) atomicAdd(&s_hist[0], nint_sum);
    if (collide) atomicAdd(&status[2], collide);
    __syncthreads();
    if (threadIdx.x < kCellRows) tile_u32[(size_t)threadIdx.x * stride + blockIdx.x] = s_hist[threadIdx.x];
    if (threadIdx.x == 0) tile_mom[blockIdx.x] = msum;
}

// B: exclusive scan over the tiles of every row.  A workgroup per row (blockIdx.x < kCellRows: the row's
// total goes to row_total[row]; the depth bases that follow from the totals are derived by C itself) and
// four more for the four moment sums -- round 2's first form did all rows in ONE workgroup, 10 us at 2^20 bodies, 31 at
// 4 M, 124 at 16 M; the rows do not depend on each other.
__global__ __launch_bounds__(1024) void cells_scan_kernel(uint32_t *__restrict__ tile_u32,
                                                         Moments *__restrict__ tile_mom, uint32_t ntiles,
                                                         uint32_t stride, uint32_t *__restrict__ row_total,
                                                         uint32_t *__restrict__ bound_slots) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (blockIdx.x < kCellRows) {
        // the row in chunks of 4,096 tiles: a wave 256 of them, every lane 4 consecutive tiles (one 16-byte
        // access; rows are padded to a multiple of 4 words), a wave scan of the lane sums, the waves'
        // totals through LDS, a carry
        __shared__ uint32_t s_w[16];
        uint4 *row = reinterpret_cast<uint4 *>(tile_u32 + (size_t)blockIdx.x * stride);
        uint32_t carry = 0;
        for (uint32_t base = 0; base < stride; base += 4096u) {
            const uint32_t i4 = base / 4u + threadIdx.x;
            uint4 v{0u, 0u, 0u, 0u};
            if (i4 * 4u < stride) v = row[i4];
            if (i4 * 4u + 0u >= ntiles) v.x = 0u;  // (the padding of the row was never written)
            if (i4 * 4u + 1u >= ntiles) v.y = 0u;
            if (i4 * 4u + 2u >= ntiles) v.z = 0u;
            if (i4 * 4u + 3u >= ntiles) v.w = 0u;
            const uint32_t sum = v.x + v.y + v.z + v.w;
            const uint32_t x = wave_scan_u32(sum);
            if (lane == 63u) s_w[wave] = x;
            __syncthreads();
            uint32_t before = 0u, chunk_total = 0u;
            for (uint32_t w = 0; w < 16u; ++w) {
                before += w < wave ? s_w[w] : 0u;
                chunk_total += s_w[w];
            }
            const uint32_t run = carry + before + x - sum;
            if (i4 * 4u < stride) row[i4] = uint4{run, run + v.x, run + v.x + v.y, run + v.x + v.y + v.z};
            carry += chunk_total;
            __syncthreads();  // s_w is reused
        }
        if (threadIdx.x == 0u) row_total[blockIdx.x] = carry;
        return;
    }
    const uint32_t comp = blockIdx.x - kCellRows;  // 0..3: m x, m y, m z, m -- a workgroup per component
    if (comp == 0u)  // this step's walk accumulates the next bound
        for (uint32_t k = threadIdx.x; k < kBoundSlots; k += 1024u) bound_slots[k] = 0u;
    {   // the moments, by the 1,024 threads in a fixed order: thread t sums the tiles [t S, (t+1) S) in
        // order, the threads' sums are scanned by wave (fixed shuffle tree) and the waves' totals
        // added in wave order -- deterministic whatever the launch timing
        __shared__ double s_wtot[16];
        double *vals = reinterpret_cast<double *>(tile_mom) + comp;  // stride 4 doubles
        const uint32_t per = (ntiles + 1023u) / 1024u;
        const uint32_t t_lo = min(threadIdx.x * per, ntiles), t_hi = min(t_lo + per, ntiles);
        double sum = 0.0;
        for (uint32_t i = t_lo; i < t_hi; ++i) sum += vals[4u * (size_t)i];
        const double x = wave_scan_f64(sum);
        if (lane == 63u) s_wtot[wave] = x;
        __syncthreads();
        double run = 0.0;
        for (uint32_t w = 0; w < wave; ++w) run += s_wtot[w];
        run += x - sum;
        for (uint32_t i = t_lo; i < t_hi; ++i) {
            const double v = vals[4u * (size_t)i];
            vals[4u * (size_t)i] = run;
            run += v;
        }
    }
}

// C: node ids (rank of (body k, depth d) among the nodes of depth d in key order = the reference's
// BFS allocation order), slots of the opened cells, moment prefixes
// SCAN_INLINE (up to kCellInlineTiles tiles: the sizes at which a step is a chain of launch latencies): B inside C.
// The tile table comes as cells_a_kernel wrote it and every workgroup sums the tiles before its own itself --
// the u32 rows by a lane per row and eighth of the tiles, the moments by a thread per tile in
// cells_scan_kernel's own order of additions (wave scan, then the waves in order: the same bits) -- one
// dependent launch fewer per step.  Per runner.step(), theta 0.75, B inside C / B launched: 1,024 bodies
// 51.1 / 54.1 us, 4,096: 60.3 / 65.7, 8,192: 70.5 / 75.7, 12,288: 79.5 / 83.0; 16,384 (65 tiles): 84.8 / 85.2,
// 32,768: 98.0 / 98.8, 65,279 (255 tiles): 123.8 / 122.5 -- the code handles up to 256 tiles, the host uses it to 64.
constexpr uint32_t kCellInlineTiles = 64;
template <bool SCAN_INLINE>
__global__ __launch_bounds__(256) void cells_c_kernel(
    const int8_t *__restrict__ cpl, uint32_t n, const uint32_t *__restrict__ tile_u32,
    const Moments *__restrict__ tile_mom, uint32_t stride, uint32_t *__restrict__ row_total,
    uint32_t *__restrict__ depth_base, uint32_t *__restrict__ n_nodes, uint32_t *__restrict__ status,
    const float4 *__restrict__ posm, uint32_t *__restrict__ int_slot, uint32_t *__restrict__ leaf_id,
    uint2 *__restrict__ int_id, uint32_t *__restrict__ node_first, uint8_t *__restrict__ node_depth,
    Moments *__restrict__ prefix, uint32_t cap, uint32_t rounds, const uint32_t *__restrict__ order,
    const float4 *__restrict__ vel_in, const float4 *__restrict__ acc_in, float4 *__restrict__ vel_out,
    float4 *__restrict__ acc_out, NodeRec *__restrict__ rec, uint32_t *__restrict__ bound_slots) {
    __shared__ uint32_t s_cnt[4][kMaxDepth + 1], s_run[kMaxDepth + 1], s_scan[4];
    __shared__ Moments s_wave[4];
    __shared__ uint32_t s_before[8][kCellRows], s_all[8][kCellRows];
    auto sum8 = [](const uint32_t (*a)[kCellRows], uint32_t r) {
        return a[0][r] + a[1][r] + a[2][r] + a[3][r] + a[4][r] + a[5][r] + a[6][r] + a[7][r];
    };
    __shared__ Moments s_mom_run;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    if (SCAN_INLINE) {
        const uint32_t ntiles = gridDim.x;
        if ((lane & 31u) < kCellRows) {  // row `lane & 31`, this half-wave's eighth of the tiles
            const uint32_t r = lane & 31u, part = wave * 2u + (lane >> 5);
            const uint32_t q = (ntiles + 7u) / 8u, t_lo = min(part * q, ntiles), t_hi = min(t_lo + q, ntiles);
            const uint32_t *row = tile_u32 + (size_t)r * stride;
            uint32_t before = 0u, all = 0u;
#pragma unroll 4
            for (uint32_t t = t_lo; t < t_hi; ++t) {
                const uint32_t v = row[t];
                all += v;
                before += t < blockIdx.x ? v : 0u;
            }
            s_before[part][r] = before;
            s_all[part][r] = all;
        }
        Moments v{0, 0, 0, 0};
        if (threadIdx.x < ntiles) v = tile_mom[threadIdx.x];
        const Moments x{wave_scan_f64(v.x), wave_scan_f64(v.y), wave_scan_f64(v.z), wave_scan_f64(v.m)};
        if (lane == 63u) s_wave[wave] = x;
        __syncthreads();
        if (threadIdx.x == blockIdx.x) {
            Moments run{0, 0, 0, 0};
            for (uint32_t w = 0; w < wave; ++w) run = run + s_wave[w];
            s_mom_run = Moments{run.x + (x.x - v.x), run.y + (x.y - v.y), run.z + (x.z - v.z), run.m + (x.m - v.m)};
        }
        if (blockIdx.x == 0u) {
            if (threadIdx.x < kCellRows)
                row_total[threadIdx.x] = sum8(s_all, threadIdx.x);
            for (uint32_t k = threadIdx.x; k < kBoundSlots; k += 256u) bound_slots[k] = 0u;
        }
    }
    if (wave == 0u) {
        // depth_base[d] = nodes of depth < d, from the rows' totals (row 1 + d = depth d); [kMaxDepth + 1] = the
        // node count.  Every workgroup derives them for itself; the first one publishes them for the kernels
        // that follow (fill, LET export, read-out) and checks the 4N capacity.
        uint32_t mine = 0u;
        if (lane <= (uint32_t)kMaxDepth)
            mine = SCAN_INLINE ? sum8(s_all, 1u + lane) : row_total[1u + lane];
        uint32_t x = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if ((int)lane >= o) x += y;
        }
        const uint32_t base_d = x - mine;  // exclusive
        if (lane <= (uint32_t)kMaxDepth)  // where this tile's nodes of depth d start
            s_run[lane] = base_d + (SCAN_INLINE ? sum8(s_before, 1u + lane)
                                                : tile_u32[(size_t)(1u + lane) * stride + blockIdx.x]);
        if (blockIdx.x == 0u) {
            if (lane <= (uint32_t)kMaxDepth) depth_base[lane] = base_d;
            if (lane == (uint32_t)kMaxDepth) {
                depth_base[kMaxDepth + 1] = x;
                *n_nodes = x;
                if (x > cap) atomicAdd(&status[1], 1u);
            }
        }
    }
    uint32_t slot_run = 0u;  // row 0: opened cells before this tile
    Moments mom_run{0, 0, 0, 0};
    if (!SCAN_INLINE) {
        slot_run = tile_u32[blockIdx.x];
        mom_run = tile_mom[blockIdx.x];
    }
    __syncthreads();
    if (SCAN_INLINE) {
        slot_run = sum8(s_before, 0u);
        mom_run = s_mom_run;
        __syncthreads();  // s_wave is reused by the rounds below
    }
    for (uint32_t sub = 0; sub < rounds; ++sub) {
        const uint32_t k = (blockIdx.x * rounds + sub) * 256u + threadIdx.x;
        const bool valid = k < n;
        const int left = valid ? cpl[k] : 0, right = valid ? cpl[k + 1] : 0;
        const int leafd = (left > right ? left : right) + 1;
        // The depths at which the wave's 64 bodies start a node at all (neighbours in tree order sit at similar
        // depths: typically 5 or 6 of the 23).  The counts of the other depths are zero; the ranks inside the wave
        // are not kept but counted again when the ids are written (23 live registers and two unrolled 23-step loops
        // otherwise: 95 VGPRs, 3,800 instructions).
        int d_lo = valid ? (right > left ? left + 1 : leafd) : kMaxDepth + 1, d_hi = valid ? leafd : -1;
        d_lo = __builtin_amdgcn_readlane(wave_min_to_lane63(d_lo), 63);
        d_hi = __builtin_amdgcn_readlane(wave_max_to_lane63(d_hi), 63);
        if (lane <= (uint32_t)kMaxDepth) s_cnt[wave][lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        for (int d = d_lo; d <= d_hi; ++d) {
            const uint64_t bal = __ballot(valid && starts_node_at(left, right, d));
            if (lane == 0) s_cnt[wave][d] = (uint32_t)__popcll(bal);
        }
        const uint32_t ni = valid && right > left ? (uint32_t)(right - left) : 0u;
        Moments item{0, 0, 0, 0};
        float4 p{0.f, 0.f, 0.f, 0.f};
        if (valid) {
            p = posm[k];
            const double m = (double)p.w;
            item = Moments{(double)p.x * m, (double)p.y * m, (double)p.z * m, m};
            if (vel_in) {  // the rest of sort_particles (tree.rs:564-602): velocities and accelerations
                const uint32_t src = order[k];
                vel_out[k] = vel_in[src];
                acc_out[k] = acc_in[src];
            }
        }
        // the opened-cell count and the four moments scanned over the workgroup together: the waves' totals of
        // both meet in LDS behind ONE pair of barriers (two scans, two pairs, before)
        uint32_t ni_total, slot0;
        Moments mom_total, mom0;
        {
            const uint32_t xi = wave_scan_u32(ni);
            const Moments xm{wave_scan_f64(item.x), wave_scan_f64(item.y), wave_scan_f64(item.z), wave_scan_f64(item.m)};
            if (lane == 63u) {
                s_scan[wave] = xi;
                s_wave[wave] = xm;
            }
            __syncthreads();
            uint32_t offi = 0u;
            Moments offm{0, 0, 0, 0};
            for (uint32_t w = 0; w < wave; ++w) {
                offi += s_scan[w];
                offm = offm + s_wave[w];
            }
            ni_total = s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
            mom_total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            __syncthreads();
            slot0 = slot_run + offi + xi - ni;
            mom0 = mom_run + Moments{offm.x + xm.x - item.x, offm.y + xm.y - item.y, offm.z + xm.z - item.z,
                                     offm.m + xm.m - item.m};
        }
        if (k <= n) prefix[k] = mom0;  // includes prefix[n] = the grand total
        if (valid) int_slot[k] = slot0;
        for (int d = d_lo; d <= d_hi; ++d) {
            const bool st = valid && starts_node_at(left, right, d);
            const uint64_t bal = __ballot(st);
            uint32_t before = s_run[d];  // (wave-uniform: where the wave's nodes of depth d start)
            for (uint32_t w = 0; w < wave; ++w) before += s_cnt[w][d];
            if (st) {
                const uint32_t id = before + (uint32_t)__popcll(bal & lt_mask);
                if (d == leafd) {
                    leaf_id[k] = id;
                    // the walk's record of the leaf (tree.rs:521-534: cog = position, mass): written here, where
                    // the body is in registers, so that fill_kernel runs over the internal cells only
                    if (id < cap) rec[id] = NodeRec{p, 0u, 0u, k, -1.0f};
                } else {
                    // (a clustered input can open far more internal cells than the 4N capacity)
                    const uint32_t slot = slot0 + (uint32_t)(d - left - 1);
                    // the slot's record: what fill_kernel needs to start on the cell without looking anything up --
                    // {first body | 'body k opens the next depth too' << 31, id | depth << 27}
                    if (slot < cap) int_id[slot] = uint2{k | (d + 1 <= right ? 0x80000000u : 0u), id | ((uint32_t)d << kSlotDepthShift)};
                }
                if (id < cap) {
                    node_first[id] = k;
                    node_depth[id] = (uint8_t)(d | (d == leafd ? 0x80 : 0));
                }
            }
        }
        __syncthreads();
        if (threadIdx.x <= kMaxDepth)
            s_run[threadIdx.x] += s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] +
                                  s_cnt[3][threadIdx.x];
        slot_run += ni_total;
        mom_run = mom_run + mom_total;
        __syncthreads();
    }
}

// ---- 6. node contents ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound_key(const uint64_t *keys, uint32_t lo, uint32_t hi,
                                                    uint64_t v) {  // first k in [lo,hi) with key >= v
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// AOS = false (every step): only the 32-byte walk records.  AOS = true (nb_sim_read_tree, on
// demand): also the reference's Octant fields -- cog, body count, the 8-entry children table
// indexed by octant -- which cost two more dependent loads per child and 52 B of stores per node.
constexpr uint32_t kFillEagerMax = 262144;  // bodies up to which fill_kernel fetches speculatively
// ... and from which it does again, all but the moment prefix: there the kernel waits out a dozen dependent loads
// per cell with every CU busy, and the probes of the run search and the candidate children sit in the lines the
// cell reads anyway (build 0.625 -> 0.605 ms at 4,000,000 bodies, 2.65 -> 2.63 at 16,777,216; 0.179 -> 0.181 at 2^20)
constexpr uint32_t kFillEagerAgainFrom = 2097152;

// EAGER_MOM: also the first moment prefix ahead of the search (small problems only: see below)
// !AOS: a thread per INTERNAL cell, found through its slot (int_id[slot], slots counted by cells_a/cells_c: row 0 of
// the tile table): two thirds of the nodes are leaves, whose records cells_c_kernel has already written, and a
// wave of 64 internal cells does not wait for the long chain of a few of them while most of its lanes idle.
template <bool AOS, bool EAGER, bool EAGER_MOM = EAGER>
__global__ void fill_kernel(const uint64_t *__restrict__ keys, uint32_t n, uint32_t n_cap,
                            const uint32_t *__restrict__ n_nodes_p,
                            const uint32_t *__restrict__ node_first,
                            const uint8_t *__restrict__ node_depth, const int8_t *__restrict__ cpl,
                            const uint32_t *__restrict__ int_slot,
                            const uint32_t *__restrict__ leaf_id, const uint2 *__restrict__ int_id,
                            const uint32_t *__restrict__ order, const float4 *__restrict__ posm,
                            const Moments *__restrict__ mom, const uint32_t *__restrict__ depth_base,
                            const uint32_t *__restrict__ bound_bits,
                            float4 *__restrict__ cogm, uint32_t *__restrict__ bodies,
                            uint32_t *__restrict__ child, NodeRec *__restrict__ rec, float inv_theta2,
                            const uint32_t *__restrict__ n_internal_p) {
    // (the grid covers ~1.75 N nodes / ~0.75 N internal cells -- a uniform octree has ~1.5 N / 0.5 N, the
    // capacity is 4 N and the counts are only known on the device: the workgroups that would find nothing to do
    // are not launched, a deeper tree takes the loop)
    const uint32_t n_nodes = min(*n_nodes_p, n_cap);
    const uint32_t n_work = AOS ? n_nodes : min(*n_internal_p, n_cap);
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_work; t += gridDim.x * blockDim.x) {
        // !AOS: everything the cell starts from comes in its slot record (written by cells_c_kernel): two dependent
        // look-ups (id -> first body, depth) and the two prefix lengths of the body fewer per cell
        uint2 si{0u, 0u};
        if (!AOS) si = int_id[t];
        const uint32_t id = AOS ? t : si.y & kSlotIdMask;
        if (id >= n_nodes) continue;
        const uint32_t k = AOS ? node_first[id] : si.x & 0x7fffffffu;
        const uint32_t dd = AOS ? node_depth[id] : si.y >> kSlotDepthShift;
        uint32_t ch[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (dd & 0x80) {  // leaf: cog = position, mass, bodies = 1, children[0] = source index
            // (AOS, the read-out after a step: from the record cells_c_kernel wrote -- a walk that gathers velocities
            // has put the NEW positions where the sorted source stood)
            const float4 p = AOS ? rec[id].cogm : posm[k];
            if (AOS) {
                cogm[id] = p;
                bodies[id] = 1;
                ch[0] = order[k];  // tree.rs:532
            }
            rec[id] = NodeRec{p, 0u, 0u, k, -1.0f};  // walk: a leaf knows its body's sorted position
        } else {
            const uint32_t d = dd;
            const uint32_t shift = 3u * (uint32_t)(kLevels - d);  // bits below the depth-d prefix
            // (Small problems are bound by this kernel's chain of dependent loads, not by its work: what
            // depends only on k is fetched together and, EAGER, the first steps of the search and the
            // eight candidate children likewise -- 6 loads deep instead of ~15: 11.6 -> 9.8 us at 16,384
            // bodies.  At 2^20 bodies the kernel is bound by HBM traffic and the speculative loads cost
            // 6 us: not EAGER there.)
            const uint64_t key_k = keys[k];
            int left = 0, right = 0;
            if (AOS) {
                left = cpl[k];
                right = cpl[k + 1];
            }
            // body k also opens the cell one level down: its slot is the next one (a body's cells have consecutive slots)
            const bool opens_next = AOS ? (int)d + 1 <= right : (si.x >> 31) != 0u;
            // (only one of the two is needed: both are fetched ahead only where latency, not traffic, binds)
            const uint32_t slot_k = AOS && opens_next ? int_slot[k] : 0u;
            const uint32_t next_id = !AOS && (EAGER || opens_next) && t + 1u < n_cap ? int_id[t + 1u].y & kSlotIdMask : ~0u;
            const uint32_t leaf_k = (EAGER || !opens_next) ? leaf_id[k] : 0u;
            Moments a{0, 0, 0, 0};
            if (EAGER_MOM) a = mom[k];  // (large problems: beside mom[end] below -- mostly the same cache line, and
                                    // fetched apart it has left the L2 by then: 185 -> 241 MB of HBM reads at 2^20)
            // end of the cell's run: galloping search from k (most cells hold a handful of bodies)
            uint32_t end = n;
            if (d != 0) {
                const uint64_t limit = ((key_k >> shift) + 1ull) << shift;  // first key past the cell
                uint32_t lo_s = k + 1u, off = 1u;
                if (EAGER) {
                    uint64_t probe[4];
    #pragma unroll
                    for (int q = 0; q < 4; ++q) probe[q] = keys[min(k + (1u << q), n - 1u)];  // k+1, k+2, k+4, k+8
    #pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (off == (1u << q) && k + off < n && probe[q] < limit) {
                            lo_s = k + off + 1u;
                            off <<= 1;
                        }
                    }
                }
                if (!EAGER || off == 16u) {
                    while (k + off < n && keys[k + off] < limit) {
                        lo_s = k + off + 1u;
                        off <<= 1;
                    }
                }
                end = lower_bound_key(keys, lo_s, min(k + off, n), limit);
            }
            if (AOS) bodies[id] = end - k;
            // children: the depth-(d+1) nodes whose first body lies in [k, end) -- consecutive ids
            // (nodes of one depth are numbered in key order), starting with body k's own child
            uint32_t f;
            if (opens_next && AOS) {
                const uint32_t slot = slot_k + (d - (uint32_t)(left + 1) + 1u);
                f = slot < n_cap ? int_id[slot].y & kSlotIdMask : ~0u;
            } else if (opens_next) {
                f = next_id;
            } else {
                f = leaf_k;
            }
            const uint32_t lim = min(depth_base[d + 2], n_nodes);  // end of the depth-(d+1) ids
            uint32_t first = 0, cnt = 0;
            if (!EAGER) {
                for (uint32_t j = 0; j < 8u; ++j) {
                    const uint32_t cid = f + j;
                    if (f == ~0u || cid >= lim) break;
                    const uint32_t kc = node_first[cid];
                    if (j > 0 && kc >= end) break;
                    if (AOS) ch[(uint32_t)(keys[kc] >> (shift - 3u)) & 7u] = cid;  // octant = the key digit of level d
                    if (cnt == 0u) first = cid;
                    ++cnt;
                }
            } else if (f != ~0u) {
                uint32_t kc[8];
    #pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) kc[j] = node_first[min(f + j, n_nodes - 1u)];
                bool more = true;
    #pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    const uint32_t cid = f + j;
                    more = more && cid < lim && (j == 0u || kc[j] < end);
                    if (more) {
                        if (AOS) ch[(uint32_t)(keys[kc[j]] >> (shift - 3u)) & 7u] = cid;  // octant = the key digit of level d
                        if (cnt == 0u) first = cid;
                        ++cnt;
                    }
                }
            }
            // mass and centre of gravity of the run [k, end)   (tree.rs:486-505)
            if (!EAGER_MOM) a = mom[k];
            const Moments b2 = mom[end];
            const double m = b2.m - a.m;
            const float4 q = float4{(float)((b2.x - a.x) / m), (float)((b2.y - a.y) / m),
                                    (float)((b2.z - a.z) / m), (float)m};
            if (AOS) cogm[id] = q;
            // A cell whose bodies are all massless (tracers): m = 0 and q = 0 / 0 = NaN, as the reference has it --
            // there the comparison with NaN is false and the cell is merely opened.  The walk with the bodies across
            // the lanes predicates the force by a zero weight, and 0 x NaN is NaN: the RECORD carries a finite centre
            // and an infinite acceptance radius instead -- always opened, never taken, at no cost to the walk.
            const bool massless = m == 0.0;
            const float4 qr = massless ? float4{0.f, 0.f, 0.f, 0.f} : q;
            // children are allocated contiguously in octant order (tree.rs:517-519), so the walk
            // only needs the first child's id and how many there are
            // a tree that outgrew its 4N capacity (status[1]) keeps the walk in bounds: a cell whose
            // children were not all stored is walked as a single body of the cell's mass
            // ... and children always carry larger ids than their parent (breadth-first numbering), which
            // is what lets the walk terminate without a visit budget: enforce it here
            if (cnt == 0u || first + cnt > n_nodes || first <= id) {
                rec[id] = NodeRec{qr, 0u, 0u, ~0u, massless ? __builtin_inff() : -1.0f};
            } else {
                const float root_width = __uint_as_float(*bound_bits) * 2.0f;
                float size2 = root_width * root_width;
                for (uint32_t l = 0; l < d; ++l) size2 *= 0.25f;  // exact: the width halves per level
                rec[id] = NodeRec{qr, first, cnt, ~0u, massless ? __builtin_inff() : size2 * inv_theta2};
            }
        }
        if (AOS) {
    #pragma unroll
            for (int c = 0; c < 8; ++c) child[(size_t)id * 8 + c] = ch[c];
        }
    }
}

// ---- AoS conversion of the device tree (nb_sim_read_tree) ---------------------------------------
__global__ void tree_to_aos_kernel(const float4 *__restrict__ cogm, const uint32_t *__restrict__ bodies,
                                   const uint32_t *__restrict__ child, uint32_t n_nodes,
                                   nb_octant *__restrict__ out) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_nodes) return;
    nb_octant o;
    const float4 q = cogm[id];
    o.cog[0] = q.x; o.cog[1] = q.y; o.cog[2] = q.z;
    o.mass = q.w;
    o.bodies = bodies[id];
    for (int c = 0; c < 8; ++c) o.children[c] = child[(size_t)id * 8 + c];
    out[id] = o;
}

__global__ void tree_aos_to_soa_kernel(const nb_particle *__restrict__ aos, uint32_t n,
                                       float4 *__restrict__ posm, float4 *__restrict__ vel,
                                       float4 *__restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const nb_particle p = aos[i];
    posm[i] = float4{p.position[0], p.position[1], p.position[2], p.mass};
    vel[i] = float4{p.velocity[0], p.velocity[1], p.velocity[2], 0.f};
    acc[i] = float4{p.acceleration[0], p.acceleration[1], p.acceleration[2], 0.f};
}
