// nb_tree_walk.hpp -- part of the nb_tree.hip translation unit: included there, inside its
// namespace nb { namespace {, and never compiled on its own.
// stages 8 and 8b: the per-thread walk and the walk with the cells across the lanes.

// ---- 8. walk + integrate ------------------------------------------------------------------------
// Stack entry: a SIBLING GROUP -- the children first .. first+count-1 of one opened cell (their
// ids are consecutive, octant order) -- and the 64-bit mask of the lanes that opened it.  One
// entry per opened cell instead of one per child: a third of the LDS traffic and of the
// lane-0 read-outs, and the children's records sit back to back in memory.
struct StackEntry {
    uint32_t first, count;
    uint32_t mask_lo, mask_hi;
};
constexpr uint32_t kWalkBatch = 4;  // records fetched together (a group is 1..8 cells)

// The trees a wave walks: its own (record 0) and, on a multi-GPU run, the imported locally
// essential trees of the peers (section 9).
constexpr int kLetMaxWorld = 16;
struct WalkRoots {
    uint32_t count;
    uint32_t id[kLetMaxWorld];
};

struct WalkStats {
    unsigned long long visits = 0, accepts = 0;
    uint32_t wave_cells = 0, wave_leaves = 0, max_sp = 1;
};

// K consecutive cells of one sibling group: their records are fetched together (wave-uniform
// address + immediate offsets: scalar loads), then each is tested and accumulated by every
// lane.  Straight-line per K so that no per-cell loop control or index clamping is needed, and
// light on SCALAR work (the scalar unit is what the loop saturates first): no per-lane
// branches, a leaf and a cell take the same path (a leaf's record makes the acceptance test
// always true and carries the one body position it must skip), the force is predicated
// instead of branched around, and the lane sets are 64-bit masks combined by s_and/s_andn2.
template <uint32_t K, bool COUNT>
__device__ __forceinline__ void walk_cells(const NodeRec *__restrict__ rp, uint64_t gmask, uint32_t i,
                                           float xi, float yi, float zi, float e,
                                           float &ax, float &ay, float &az, StackEntry *stack,
                                           uint32_t &sp, bool lane0, WalkStats &st) {
    NodeRec r[K];
#pragma unroll
    for (uint32_t b = 0; b < K; ++b) r[b] = rp[b];
#pragma unroll
    for (uint32_t b = 0; b < K; ++b) {
        const float4 q = r[b].cogm;
        const float dx = q.x - xi, dy = q.y - yi, dz = q.z - zi;
        const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        // acceptance size/dist < theta (tree.wgsl:63-64) as size^2 / theta^2 < r^2; a leaf's
        // negative radius makes it always true, its self_pos excludes the body itself
        const uint64_t far = __ballot(r[b].mac2 < r2);
        const uint64_t other = __ballot(r[b].self_pos != i);
        const uint64_t take = gmask & far & other;
        const uint64_t open = gmask & ~far;  // never a leaf: its test is always true
        const float dist = __builtin_amdgcn_sqrtf(r2);
        float w = q.w * __builtin_amdgcn_rcpf(__builtin_fmaf(e, dist, r2 * r2));
        w = __builtin_amdgcn_inverse_ballot_w64(take) ? w : 0.0f;  // predicated, not branched
        ax = __builtin_fmaf(w, dx, ax);
        ay = __builtin_fmaf(w, dy, ay);
        az = __builtin_fmaf(w, dz, az);
        if (COUNT) {
            st.visits += __builtin_amdgcn_inverse_ballot_w64(gmask) ? 1ull : 0ull;
            st.accepts += __builtin_amdgcn_inverse_ballot_w64(take) ? 1ull : 0ull;
            if (r[b].count == 0u) st.wave_leaves += 1u;
        }
        if (open) {  // push the cell's children as one group for the opening lanes
            if (lane0)
                stack[sp] = StackEntry{r[b].first, r[b].count, (uint32_t)open, (uint32_t)(open >> 32)};
            sp += 1;
            if (COUNT) st.max_sp = sp > st.max_sp ? sp : st.max_sp;
        }
    }
}

// One wave walks for 64 consecutive sorted bodies, depth-first over sibling groups: a pop
// pushes at most 8 groups one level down, so the stack holds at most 7 x 21 + 1 entries -- it
// cannot overflow.
// PART: 0 = the whole step; 1 = walk the given trees and leave the raw sums in acc_dst (no
// integration); 2 = start from those sums, walk the given trees, integrate.  1 then 2 add the same
// terms in the same order as 0 does over the concatenated roots, so the result is bit-identical --
// a LET host walks the rank's own tree (1) while the imported trees are still on the wire.
template <bool COUNT, int PART = 0>
__global__ __launch_bounds__(256) void walk_kernel(
    const float4 *__restrict__ posm_src, const float4 *__restrict__ vel_src,
    const float4 *__restrict__ acc_src, const NodeRec *__restrict__ rec,
    WalkRoots roots_arg,
    float4 *__restrict__ posm_dst, float4 *__restrict__ vel_dst, float4 *__restrict__ acc_dst,
    uint32_t lo, uint32_t hi, uint32_t bpw_shift, float g, float e, float dt,
    uint32_t *__restrict__ status, unsigned long long *__restrict__ counters,
    uint32_t *__restrict__ bound_slots, const WalkRoots *__restrict__ roots_dev) {
    // (device-made roots: fixed-stride LET imports.  Element-wise, never a copy of the struct: a
    // by-value copy of a kernel argument selected at run time lands in scratch memory)
    const uint32_t n_roots =  // (readfirstlane: see walk_cells_kernel)
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(roots_dev ? roots_dev->count : roots_arg.count));
    __shared__ StackEntry s_stack[4][kWalkStack];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    // this rank walks for the sorted bodies [lo, hi) (single GPU: [0, n)).
    // Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2); remap so that each
    // XCD walks one contiguous eighth of the Morton-ordered bodies and its L2 keeps that region's
    // deep cells instead of everybody's.  Speed only: any placement gives the same result.
    const uint32_t per_xcd = gridDim.x / 8u;
    uint32_t blk = blockIdx.x;
    if (blk < per_xcd * 8u) blk = (blk & 7u) * per_xcd + (blk >> 3);   // bijective on [0, 8*per_xcd)
                                                                       // the last < 8 blocks stay put
    // A wave walks for 2^bpw_shift consecutive bodies (64 on large problems; fewer when there are
    // not enough bodies to fill the chip: a small problem is bound by the LENGTH of one wave's
    // walk, and the union of the cells of 8 bodies is much shorter than that of 64).
    const uint32_t i = lo + ((blk * 4u + wave) << bpw_shift) + lane;
    const bool valid = i < hi && lane < (1u << bpw_shift);
    const uint32_t ic = valid ? i : hi - 1;
    const float4 p = posm_src[ic], v = vel_src[ic], a = acc_src[ic];
    const float vhx = kick(v.x, a.x, dt), vhy = kick(v.y, a.y, dt), vhz = kick(v.z, a.z, dt);
    const float xi = drift(p.x, vhx, dt), yi = drift(p.y, vhy, dt), zi = drift(p.z, vhz, dt);
    if (bound_slots) {  // the next step's root cube: max |coord| of the new positions
        float m = valid ? fmaxf(fabsf(xi), fmaxf(fabsf(yi), fabsf(zi))) : 0.f;
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0u) publish_bound(bound_slots, blockIdx.x * 4u + wave, m);
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (PART == 2 && valid) {
        const float4 part = acc_dst[i];
        ax = part.x;
        ay = part.y;
        az = part.z;
    }
    WalkStats st;
    const bool lane0 = lane == 0u;

    StackEntry *stack = s_stack[wave];
    uint32_t sp = 0;
    const uint64_t all = __ballot(valid);
    if (all) {  // the roots, pushed so that roots.id[0] is walked first
        for (uint32_t k = n_roots; k > 0u; --k) {
            const uint32_t rid =
                (uint32_t)__builtin_amdgcn_readfirstlane((int)(roots_dev ? roots_dev->id[k - 1u] : roots_arg.id[k - 1u]));
            if (lane0) stack[sp] = StackEntry{rid, 1u, (uint32_t)all, (uint32_t)(all >> 32)};
            sp += 1;
        }
    }
    __builtin_amdgcn_wave_barrier();
    // Termination: a group's children have larger ids than their parent (fill_kernel enforces
    // it), so no cell is reached twice; the stack check only guards against a corrupt tree.
    while (sp > 0) {
        if (sp > kWalkStack - 8u) {
            if (lane0) atomicAdd(&status[3], 1u);
            break;
        }
        --sp;
        const StackEntry top = stack[sp];  // every lane reads the same entry (LDS broadcast)
        // (the builtin returns a signed int: go through uint32_t or values sign-extend)
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)top.first);
        const uint32_t gcnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)top.count);
        const uint64_t gmask = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)top.mask_lo) |
                               ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)top.mask_hi) << 32);
        if (COUNT) st.wave_cells += gcnt;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t c0 = 0; c0 < gcnt; c0 += kWalkBatch) {
            const NodeRec *rp = rec + first + c0;
            const uint32_t rem = gcnt - c0;
            if (rem >= 4u)
                walk_cells<4, COUNT>(rp, gmask, i, xi, yi, zi, e, ax, ay, az, stack, sp, lane0, st);
            else if (rem == 3u)
                walk_cells<3, COUNT>(rp, gmask, i, xi, yi, zi, e, ax, ay, az, stack, sp, lane0, st);
            else if (rem == 2u)
                walk_cells<2, COUNT>(rp, gmask, i, xi, yi, zi, e, ax, ay, az, stack, sp, lane0, st);
            else
                walk_cells<1, COUNT>(rp, gmask, i, xi, yi, zi, e, ax, ay, az, stack, sp, lane0, st);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (COUNT && lane0) {  // per-wave statistics: cells fetched, deepest stack
        atomicAdd(&counters[2], (unsigned long long)st.wave_cells);
        atomicMax(&counters[3], (unsigned long long)st.max_sp);
        atomicAdd(&counters[4], (unsigned long long)st.wave_leaves);
        atomicMax(&counters[5], (unsigned long long)st.wave_cells);  // the longest walk of any wave
    }
    if (COUNT && valid) {
        atomicAdd(&counters[0], st.visits);
        atomicAdd(&counters[1], st.accepts);
    }
    if (!valid) return;
    if (PART == 1) {
        acc_dst[i] = float4{ax, ay, az, 0.f};
        return;
    }
    const float gdt = g * dt;
    const float fx = ax * gdt, fy = ay * gdt, fz = az * gdt;
    posm_dst[i] = float4{xi, yi, zi, p.w};
    vel_dst[i] = float4{kick(vhx, fx, dt), kick(vhy, fy, dt), kick(vhz, fz, dt), 0.f};
    acc_dst[i] = float4{fx, fy, fz, 0.f};
}

// ---- 8b. walk with the CELLS across the lanes ---------------------------------------------------
// The kernel above gives every lane a body and feeds the wave one cell at a time, so a cell that
// only a few of the 64 bodies need still costs a full wave instruction: at 2^20 bodies, theta 0.5,
// a wave evaluates 2,417 cells for bodies that need 1,011 each (42 % of the lanes do useful work,
// 17 % at depth 7 -- tools/walk_model.c).  Here the roles are transposed: a wave walks for a GROUP
// of G consecutive bodies (G = 4, 8 or 16) whose drifted positions sit in SGPRs, and its 64 lanes
// hold 64 CELLS of the traversal frontier, each with the G-bit set of bodies that have to test it.
// One batch = pop up to 64 (cell, visit mask) entries from the wave's LDS stack, every lane loads its
// own cell's 32-byte record (all bytes used), then for each of the G bodies one straight-line
// evaluation of acceptance test + force over the 64 cells, with the body's coordinates as scalar
// operands; lanes whose cell was opened by some body push its children (siblings stay adjacent
// in the stack, so the next batch's record loads coalesce).  Every lane accumulates G partial
// sums, added across the lanes once at the end of the walk in a fixed order.
//   * each body still applies ITS OWN acceptance test to exactly the cells the reference's
//     per-thread walk visits (tree.wgsl:57-70): visit and accept counts equal the oracle's;
//   * lane slots are wasted only where a cell concerns a subset of the G bodies: 65 % useful at
//     G = 8 (72 % at G = 4), and the scalar bookkeeping of the per-cell loop is gone;
//   * a walk is a chain of ~25 batches instead of ~2,400 dependent cell visits, which is what
//     bounds the small problems (benches/benchmark.rs sizes).
// A stack entry: a cell and the set of the group's bodies that have to test it -- body b at bit G - 1 - b
// ("low" format; the evaluation shifts it to the top of the word, where the carry of an add takes the
// bodies out one by one).
struct CellEnt {
    uint32_t id, mask;
};
// PACKED: the two in one word -- the mask in the low byte (G <= 8), a cell id below 2^24 above it: half
// the LDS traffic of the stack (walk -2 % at 2^20 bodies, -3 % at 4 M theta 0.75).  The host picks it
// when every id the walk can meet (the tree's capacity, the LET import area) is below 2^24.
constexpr uint32_t kPackedIdBits = 24;
template <bool PACKED>
struct CellStack;
template <>
struct CellStack<false> {
    using Ent = CellEnt;
    static __device__ __forceinline__ Ent make(uint32_t id, uint32_t mask) { return CellEnt{id, mask}; }
    // the entries of the children first, first + 1, ... of a cell: child(base(first, mask), j)
    static __device__ __forceinline__ Ent base(uint32_t first, uint32_t mask) { return CellEnt{first, mask}; }
    static __device__ __forceinline__ Ent child(const Ent &b, uint32_t j) { return CellEnt{b.id + j, b.mask}; }
    static __device__ __forceinline__ uint32_t id(const Ent &e) { return e.id; }
    static __device__ __forceinline__ uint32_t mask(const Ent &e) { return e.mask; }
    // the mask with body b at bit 31 - b
    template <int G>
    static __device__ __forceinline__ uint32_t mask_top(const Ent &e) { return e.mask << (32 - G); }
};
template <>
struct CellStack<true> {
    using Ent = uint32_t;
    static __device__ __forceinline__ Ent make(uint32_t id, uint32_t mask) { return (id << 8) | mask; }
    static __device__ __forceinline__ Ent base(uint32_t first, uint32_t mask) { return (first << 8) | mask; }
    static __device__ __forceinline__ Ent child(const Ent &b, uint32_t j) { return b + (j << 8); }
    static __device__ __forceinline__ uint32_t id(const Ent &e) { return e >> 8; }
    static __device__ __forceinline__ uint32_t mask(const Ent &e) { return e & 0xffu; }
    template <int G>
    static __device__ __forceinline__ uint32_t mask_top(const Ent &e) { return e << (32 - G); }  // (the id falls off the top)
};

// The per-body lane sets come out of the per-lane masks one bit at a time through the carry of an
// add: v <<= 1, the lanes whose top bit was set are returned as a 64-bit lane mask (one VALU
// instruction, where an and + compare would be two) ...
__device__ __forceinline__ uint64_t shl1_carry_out(uint32_t &v) {
    uint32_t o;
    uint64_t c;
    asm("v_add_co_u32_e64 %0, %1, %2, %2" : "=v"(o), "=s"(c) : "v"(v));
    v = o;
    return c;
}
// ... and go back in the same way: (v << 1) | (lane in `bit`), one add-with-carry
__device__ __forceinline__ uint32_t shl1_carry_in(uint32_t v, uint64_t bit) {
    uint32_t o;
    uint64_t unused;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(o), "=s"(unused) : "v"(v), "s"(bit));
    return o;
}
#ifndef NB_CELL_STACK
#define NB_CELL_STACK 896
#endif
#ifndef NB_WALK_WAVES
#define NB_WALK_WAVES 1
#endif
#ifndef NB_WALK_BLOCK_WAVES
#define NB_WALK_BLOCK_WAVES 1
#endif
#ifndef NB_WALK_MIN_WAVES
#define NB_WALK_MIN_WAVES 5  // waves per SIMD the register budget of the cells walk is held to
#endif
constexpr uint32_t kCellBlockWaves = NB_WALK_BLOCK_WAVES;  // waves (= groups) per workgroup
constexpr uint32_t kCellStack = NB_CELL_STACK;  // entries per wave, two-word form (7 KiB: 22 waves per CU; 1,024 entries = 8 KiB = 20 waves: +5 % at 16 M bodies); see the batch-size rule in the loop
#ifndef NB_CELL_STACK_PACKED
#define NB_CELL_STACK_PACKED 1024  // (4 KiB x 32 waves per CU; 896: +1.7 % at 2^20 bodies theta 0.5, larger: no further gain)
#endif
constexpr uint32_t kCellStackPacked = NB_CELL_STACK_PACKED;  // ... one-word form
constexpr uint32_t kCellReserve = 160;
constexpr uint32_t kWalkGatherFrom = 524288;  // bodies from which the walk gathers velocities itself (8c)

// sum over the 64 lanes, in a fixed order; the total lands in lane 63
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    uint32_t x = __float_as_uint(v);
#define NB_STEP(ctrl, row_mask) \
    x = __float_as_uint(__uint_as_float(x) + __uint_as_float(NB_DPP(0, x, ctrl, row_mask)))
    NB_STEP(0x111, 0xf);
    NB_STEP(0x112, 0xf);
    NB_STEP(0x114, 0xf);
    NB_STEP(0x118, 0xf);
    NB_STEP(0x142, 0xa);
    NB_STEP(0x143, 0xc);
#undef NB_STEP
    return __uint_as_float(x);
}

// One batch of the cells walk: the lane's cell (q = centre of gravity + mass, mac2) against the G
// bodies of the group.  vm: the bodies that have to test the cell, body b at bit 31 - b; returns
// the bodies that open it, body b at bit G - 1 - b (the stack's format); a body whose bit is set and
// that accepts the cell takes it.
typedef float v2f __attribute__((ext_vector_type(2)));

// Two bodies of the group per packed-fp32 instruction (v_pk_add/mul/fma_f32: two IEEE binary32
// operations per lane and issue slot, each rounded as the scalar instruction rounds it, so every
// bit is what the one-body-at-a-time form computes): bodies 2k and 2k+1 in the halves of bx[k].
template <int G, bool COUNT>
__device__ __forceinline__ uint32_t cells_batch(const float4 q, const float mac2, uint32_t vm,
                                                const v2f (&bx)[G / 2], const v2f (&by)[G / 2],
                                                const v2f (&bz)[G / 2], const float e,
                                                v2f (&ax)[G / 2], v2f (&ay)[G / 2], v2f (&az)[G / 2],
                                                unsigned long long &n_accepts, uint32_t &n_idle_pairs) {
    uint32_t om = 0u;  // body b ends up at bit G - 1 - b
#pragma unroll
    for (int k = 0; k < G / 2; ++k) {
        const uint64_t visit0 = shl1_carry_out(vm), visit1 = shl1_carry_out(vm);
        if (COUNT && (visit0 | visit1) == 0ull) n_idle_pairs += 1u;  // (statistics: a pair no cell of the batch concerns)
        const v2f dx = v2f{q.x, q.x} - bx[k], dy = v2f{q.y, q.y} - by[k], dz = v2f{q.z, q.z} - bz[k];
        const v2f r2 = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
        // acceptance size/dist < theta (tree.wgsl:63-64) as size^2 / theta^2 < r^2 (NodeRec::mac2); a leaf's
        // negative radius makes it always true.  Lane sets as 64-bit scalar masks.
        const uint64_t far0 = __ballot(mac2 < r2.x), far1 = __ballot(mac2 < r2.y);
        const uint64_t take0 = far0 & visit0, take1 = far1 & visit1;
        const uint64_t open0 = visit0 & ~far0, open1 = visit1 & ~far1;
        v2f dist;
        dist.x = __builtin_amdgcn_sqrtf(r2.x);
        dist.y = __builtin_amdgcn_sqrtf(r2.y);
        const v2f den = __builtin_elementwise_fma(v2f{e, e}, dist, r2 * r2);
        v2f rc;
        rc.x = __builtin_amdgcn_rcpf(den.x);
        rc.y = __builtin_amdgcn_rcpf(den.y);
        v2f w = v2f{q.w, q.w} * rc;
        {   // accumulate under the lanes that take the cell (exec = take), the other lanes' sums untouched:
            // six plain fma instead of two selects and three packed fma
            float a0 = ax[k].x, a1 = ay[k].x, a2 = az[k].x, b0 = ax[k].y, b1 = ay[k].y, b2 = az[k].y;
            uint64_t saved;
            asm("s_mov_b64 %[sv], exec\n\t"
                "s_mov_b64 exec, %[t0]\n\t"
                "v_fmac_f32 %[a0], %[w0], %[dx0]\n\t"
                "v_fmac_f32 %[a1], %[w0], %[dy0]\n\t"
                "v_fmac_f32 %[a2], %[w0], %[dz0]\n\t"
                "s_mov_b64 exec, %[t1]\n\t"
                "v_fmac_f32 %[b0], %[w1], %[dx1]\n\t"
                "v_fmac_f32 %[b1], %[w1], %[dy1]\n\t"
                "v_fmac_f32 %[b2], %[w1], %[dz1]\n\t"
                "s_mov_b64 exec, %[sv]"
                : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [b0] "+v"(b0), [b1] "+v"(b1), [b2] "+v"(b2),
                  [sv] "=&s"(saved)
                : [t0] "s"(take0), [t1] "s"(take1), [w0] "v"(w.x), [w1] "v"(w.y), [dx0] "v"(dx.x), [dy0] "v"(dy.x),
                  [dz0] "v"(dz.x), [dx1] "v"(dx.y), [dy1] "v"(dy.y), [dz1] "v"(dz.y));
            ax[k] = v2f{a0, b0};
            ay[k] = v2f{a1, b1};
            az[k] = v2f{a2, b2};
        }
        om = shl1_carry_in(om, open0);
        om = shl1_carry_in(om, open1);
        if (COUNT)
            n_accepts += (__builtin_amdgcn_inverse_ballot_w64(take0) ? 1ull : 0ull) +
                         (__builtin_amdgcn_inverse_ballot_w64(take1) ? 1ull : 0ull);
#ifdef NB_DIAG_EXTRA_VALU   // sensitivity probe: two more transcendentals and three fma per pair
        for (int h = 0; h < 2; ++h) {
            const float t = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf((h ? r2.y : r2.x) + 1.0f));
            float u = __builtin_fmaf(t, dx.x, dy.x);
            u = __builtin_fmaf(t, u, dz.x);
            u = __builtin_fmaf(t, u, dx.y);
            asm volatile("" ::"v"(u));
        }
#endif
    }
    return om;
}

// roots.id[0 .. split) are walked together and reduced, then roots.id[split .. count): a LET host
// may walk its own tree (PART 1) while the imports are on the wire and add them later (PART 2),
// and gets bit for bit what the one-launch step (PART 0) computes.
template <int G, bool COUNT, int PART, bool PACKED>
// (G <= 8: at most 96 VGPRs, so that five waves fit a SIMD -- the compiler lands on 90..100 by itself)
__global__ __launch_bounds__(64 * NB_WALK_BLOCK_WAVES, (G <= 8 ? NB_WALK_MIN_WAVES : NB_WALK_WAVES)) void walk_cells_kernel(
    const float4 *posm_src, const float4 *__restrict__ vel_src,
    const float4 *__restrict__ acc_src, const NodeRec *__restrict__ rec, WalkRoots roots_arg, uint32_t split,
    float4 *posm_dst, float4 *__restrict__ vel_dst, float4 *__restrict__ acc_dst,
    uint32_t lo, uint32_t hi, float g, float e, float dt,
    uint32_t *__restrict__ status, unsigned long long *__restrict__ counters,
    uint32_t *__restrict__ bound_slots, const WalkRoots *__restrict__ roots_dev,
    const uint32_t *__restrict__ va_order) {
    // va_order (section 8c): velocities and accelerations are still in the step's SOURCE order -- body k's are at
    // va_order[k] -- and the new position goes where the sorted old one was read (posm_dst == posm_src: only the
    // group itself ever reads its bodies' entries, the tree's records carry their own copies)
    // (device-made roots: fixed-stride LET imports.  Element-wise, never a copy of the struct: a
    // by-value copy of a kernel argument selected at run time lands in scratch memory)
    // (readfirstlane: the select between a kernel-argument field and device memory is a load
    // through a flat pointer, which the compiler takes for lane-dependent -- and with it the stack
    // pointer and the whole loop control, which then live in VGPRs under exec masks)
#if defined(NB_DIAG_PHASES) || defined(NB_DIAG_TIMELINE)
    unsigned long long tl_launch;   // the wave's first instruction
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tl_launch)::"memory");
#endif
    const uint32_t n_roots =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(roots_dev ? roots_dev->count : roots_arg.count));
    using Stack = CellStack<PACKED>;
    using Ent = typename Stack::Ent;
    static_assert(!PACKED || G <= 8, "a packed entry has 8 mask bits");
    // (the stack's LDS also carries the G x 64 floats of the final reduction)
    constexpr uint32_t kStack = PACKED ? kCellStackPacked : kCellStack;
    constexpr uint32_t kEntries = kStack * sizeof(Ent) >= (uint32_t)G * 256u ? kStack : (uint32_t)G * 256u / sizeof(Ent);
    __shared__ Ent s_stack[kCellBlockWaves][kEntries];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t per_xcd = gridDim.x / 8u;  // as walk_kernel: an XCD walks one contiguous eighth
    uint32_t blk = blockIdx.x;
    if (blk < per_xcd * 8u) blk = (blk & 7u) * per_xcd + (blk >> 3);
    const uint32_t i0 = lo + (blk * kCellBlockWaves + wave) * (uint32_t)G;  // the group: bodies i0 .. i0+G-1
    if (i0 >= hi) return;                                      // wave-uniform; the kernel has no barrier
    const uint32_t nvalid = min((uint32_t)G, hi - i0);
    const uint32_t ib = i0 + lane;
    const bool owner = lane < nvalid;  // lane b < G owns body b: loads it, integrates it at the end
    const uint32_t ic = owner ? ib : i0;
    float xi, yi, zi;
    {   // kick + drift (tree.wgsl:105-106); redone after the walk instead of kept in registers
        const uint32_t jc = va_order ? va_order[ic] : ic;
        const float4 p = posm_src[ic], v = vel_src[jc], a = acc_src[jc];
        xi = drift(p.x, kick(v.x, a.x, dt), dt);
        yi = drift(p.y, kick(v.y, a.y, dt), dt);
        zi = drift(p.z, kick(v.z, a.z, dt), dt);
    }
    v2f bx[G / 2], by[G / 2], bz[G / 2];  // the group's evaluation points, wave-uniform (SGPR pairs)
#pragma unroll
    for (int b = 0; b < G; ++b) {
        bx[b / 2][b % 2] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(xi), b));
        by[b / 2][b % 2] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(yi), b));
        bz[b / 2][b % 2] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(zi), b));
    }
    // bounding box of the group's evaluation points (for the all-open shortcut below)
    float blx = bx[0].x, bly = by[0].x, blz = bz[0].x, bhx = blx, bhy = bly, bhz = blz;
#pragma unroll
    for (int b = 1; b < G; ++b) {
        if ((uint32_t)b < nvalid) {
            blx = fminf(blx, bx[b / 2][b % 2]); bhx = fmaxf(bhx, bx[b / 2][b % 2]);
            bly = fminf(bly, by[b / 2][b % 2]); bhy = fmaxf(bhy, by[b / 2][b % 2]);
            blz = fminf(blz, bz[b / 2][b % 2]); bhz = fmaxf(bhz, bz[b / 2][b % 2]);
        }
    }
    // (wave-uniform values computed by the vector unit: move them to SGPRs)
#define NB_UNIFORM(x) x = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x)))
    NB_UNIFORM(blx); NB_UNIFORM(bly); NB_UNIFORM(blz); NB_UNIFORM(bhx); NB_UNIFORM(bhy); NB_UNIFORM(bhz);
#undef NB_UNIFORM
    const uint32_t group_mask = ((1u << nvalid) - 1u) << ((uint32_t)G - nvalid);  // body b at bit G - 1 - b
    Ent *stack = s_stack[wave];
    float tx = 0.f, ty = 0.f, tz = 0.f;  // lane b: the finished sums of body b
    if (PART == 2 && owner) {
        const float4 part = acc_dst[ib];
        tx = part.x;
        ty = part.y;
        tz = part.z;
    }
    unsigned long long n_visits = 0, n_accepts = 0;
    uint32_t n_cells = 0, n_leaves = 0, n_batches = 0, max_sp = 0, n_idle_pairs = 0, n_evals = 0;
#ifdef NB_DIAG_PHASES
    unsigned long long ph[4] = {0, 0, 0, 0};  // cycles per phase
#endif
#if defined(NB_DIAG_PHASES) || defined(NB_DIAG_TIMELINE)
    // (three scalars: the probe must not cost the kernel a wave of occupancy)
    const unsigned long long tl_start = __builtin_amdgcn_s_memrealtime();  // the 100 MHz clock
    uint32_t tl_batches = 0;
#endif

    for (uint32_t set = 0; set < 2u; ++set) {
        const uint32_t r_lo = set == 0u ? 0u : split, r_hi = set == 0u ? min(split, n_roots) : n_roots;
        if (r_lo >= r_hi) continue;
        uint32_t sp = r_hi - r_lo;
        if (lane < sp)
            stack[lane] = Stack::make(roots_dev ? roots_dev->id[r_lo + lane] : roots_arg.id[r_lo + lane], group_mask);
        __builtin_amdgcn_wave_barrier();
        v2f ax[G / 2], ay[G / 2], az[G / 2];
#pragma unroll
        for (int k = 0; k < G / 2; ++k) ax[k] = ay[k] = az[k] = v2f{0.f, 0.f};

        bool overflowed = false;
        while (sp > 0u) {
            // Batch size: up to 64 cells, fewer when their children (at most 8 each: 7 net per
            // popped cell) would eat into the reserve.  Popping from the top keeps the walk
            // depth-first, so once batches are down to one cell the stack grows by at most 7 per
            // level below the cell it started from: 7 x 21 = 147 < kCellReserve slots, and a batch of
            // several cells is only taken while it leaves the reserve untouched -- the stack cannot
            // overflow on a consistent tree (the check below guards against a corrupt one).
            const uint32_t free_slots = kStack - sp;
            if (free_slots < 7u) {
                overflowed = true;
                break;
            }
            uint32_t c = sp < 64u ? sp : 64u;
            const uint32_t lim = free_slots >= kCellReserve + 7u ? (free_slots - kCellReserve) / 7u : 1u;
            c = c < lim ? c : lim;
            sp -= c;
#ifdef NB_DIAG_PHASES
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
            // the lanes past the batch (fewer than 64 cells) read its last entry and that cell's record like
            // lane c - 1 -- no divergent load, no second address -- and carry an empty visit set
            const uint64_t batch_lanes = ~0ull >> (64u - c);
            const bool active = __builtin_amdgcn_inverse_ballot_w64(batch_lanes);
            const Ent top = stack[sp + min(lane, c - 1u)];
            // the bodies that test this cell, body b at bit 31 - b, where the carry of an add takes them out
            const uint32_t vm = active ? Stack::template mask_top<G>(top) : 0u;
#ifdef NB_DIAG_PHASES
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(top), "v"(vm));
            const unsigned long long t1 = __builtin_amdgcn_s_memtime();
#endif
            // (a 32-bit byte offset from the uniform base: one shift and a load with a scalar base; the
            // 64-bit form costs a 64-bit shift and a 64-bit add per batch)
            const NodeRec r = *reinterpret_cast<const NodeRec *>(reinterpret_cast<const char *>(rec) +
                                                                 (Stack::id(top) * (uint32_t)sizeof(NodeRec)));
#ifdef NB_DIAG_PHASES
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(r.cogm.x), "v"(r.cogm.w), "v"(r.first), "v"(r.count), "v"(r.self_pos), "v"(r.mac2));
            const unsigned long long t2 = __builtin_amdgcn_s_memtime();
#endif
#ifdef NB_DIAG_EXTRA_LOAD   // sensitivity probe: one more divergent 32-byte record load per lane and batch
            {
                const NodeRec r2 = rec[Stack::id(top) ^ 1u];
                asm volatile("" ::"v"(r2.cogm.x), "v"(r2.cogm.w), "v"(r2.first), "v"(r2.mac2));
            }
#endif
            // The top of the tree: a batch of a few big cells (the root, its children; also the
            // roots of imported trees) that EVERY body of the group opens.  One test per lane against
            // the group's bounding box decides it without touching the bodies: with the largest
            // per-axis distance to the box, r2max >= the r^2 any body computes (fp32 subtract,
            // multiply and fma are monotonic, same operation order), so "not (mac2 < r2max)"
            // implies every body's own test says open -- the same decisions, 1/8 of the work.
            bool all_open = false;
            if (c <= 8u) {
                const float dxm = fmaxf(fabsf(r.cogm.x - blx), fabsf(r.cogm.x - bhx));
                const float dym = fmaxf(fabsf(r.cogm.y - bly), fabsf(r.cogm.y - bhy));
                const float dzm = fmaxf(fabsf(r.cogm.z - blz), fabsf(r.cogm.z - bhz));
                const float r2max = __builtin_fmaf(dzm, dzm, __builtin_fmaf(dym, dym, dxm * dxm));
                all_open = (__ballot(r.mac2 < r2max) & batch_lanes) == 0ull;
            }
            // the bodies that open the lane's cell, body b at bit G - 1 - b.  (Set before the branch and
            // overwritten in it: written as if / else, the merge copies all 24 accumulators every batch.)
            uint32_t om = active ? Stack::mask(top) : 0u;
            if (!all_open) {
                // a leaf is never taken by its own body (cells carry self_pos = ~0, no body of the group):
                // that body's bit leaves the lane's set -- a leaf is never opened, so all the bit could do is
                // take the leaf -- instead of a second evaluation path with "take" masks of its own.
                // (bodies past the group's 8th clear a bit below the mask's)
                const uint32_t sb = min(r.self_pos - i0, (uint32_t)G);
                const uint32_t em = vm & ~(0x80000000u >> sb);
                om = cells_batch<G, COUNT>(r.cogm, r.mac2, em, bx, by, bz, e, ax, ay, az, n_accepts, n_idle_pairs);
                if (COUNT) n_evals += 1u;
            }
            if (COUNT) {
                n_visits += (unsigned long long)__popc(vm);
                n_cells += c;
                n_batches += 1u;
                n_leaves += (uint32_t)__popcll(__ballot(active && r.count == 0u));
            }
#ifdef NB_DIAG_PHASES
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(om), "v"(ax[0].x), "v"(ay[G / 2 - 1].y));
            const unsigned long long t3 = __builtin_amdgcn_s_memtime();
#endif
            // push the children of the opened cells: lane l writes its cnt entries at
            // sp + (children of the lanes below it), so siblings and cousins stay in lane order.
            // (An opened cell has children -- a leaf's test is always true -- so the lanes that push are
            // the lanes with a body in om; a batch that opened nothing, which is most batches of leaves,
            // skips the scan.)
            const uint64_t pushers = __ballot(om != 0u);
            if (pushers != 0ull) {
                const uint32_t cnt = om != 0u ? r.count : 0u;
                const uint32_t incl = wave_scan_u32(cnt);
                const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                Ent *dst = stack + sp + (incl - cnt);
                // Every pushing lane stores all 8 slots, highest first, without looking at its count: a
                // slot past a lane's count lands on a LOWER-numbered slot of a lane above it, which that
                // lane stores later (or beyond the new top, inside the reserve) -- one predicate for
                // the eight stores instead of eight.
                if (om != 0u) {
                    const Ent cb = Stack::base(r.first, om);
#pragma unroll
                    for (int j = 7; j >= 0; --j) {
                        dst[j] = Stack::child(cb, (uint32_t)j);
                        __builtin_amdgcn_wave_barrier();  // keep the stores in this order
                    }
                }
                sp += total;
            }
            if (COUNT) max_sp = max(max_sp, sp);
            __builtin_amdgcn_wave_barrier();
#if defined(NB_DIAG_PHASES) || defined(NB_DIAG_TIMELINE)
            tl_batches += 1u;
#endif
#ifdef NB_DIAG_PHASES
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"s"(sp));
            const unsigned long long t4 = __builtin_amdgcn_s_memtime();
            ph[0] += t1 - t0;
            ph[1] += t2 - t1;
            ph[2] += t3 - t2;
            ph[3] += t4 - t3;
#endif
        }
        if (overflowed && lane == 0u) atomicAdd(&status[3], 1u);  // (reported outside the loop: see sp above)
        // The G sums of this root set, in a fixed order, through the (now empty) stack's LDS: every
        // lane stores its G partial sums of one component; lane l then adds the partial sums of the
        // lanes [p G, p G + G) of body b, with b = l / L, p = l % L, L = 64 / G lanes per body; the L
        // results of a body meet by butterfly; lane b fetches body b's total.
        {
            constexpr uint32_t L = 64u / (uint32_t)G;
            float *red = reinterpret_cast<float *>(stack);  // [G][64] floats <= 4 KiB of the 8 KiB stack
            const uint32_t rb = lane / L, rp = lane % L;
            float sum3[3];
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) {
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int b = 0; b < G; ++b)
                    red[b * 64 + (int)lane] = comp == 0 ? ax[b / 2][b % 2] : comp == 1 ? ay[b / 2][b % 2] : az[b / 2][b % 2];
                __builtin_amdgcn_wave_barrier();
                float sacc = 0.f;
#pragma unroll
                for (int j = 0; j < G; ++j) sacc += red[rb * 64u + rp * (uint32_t)G + (uint32_t)j];
#pragma unroll
                for (uint32_t o = L / 2u; o > 0u; o >>= 1) sacc += __shfl_xor(sacc, (int)o);
                sum3[comp] = __shfl(sacc, (int)((lane % (uint32_t)G) * L));  // lane b < G: body b's total
            }
            __builtin_amdgcn_wave_barrier();
            tx += sum3[0];
            ty += sum3[1];
            tz += sum3[2];
        }
        if (PART == 1) break;  // the own tree only
    }
    if (COUNT) {
        atomicAdd(&counters[0], n_visits);
        atomicAdd(&counters[1], n_accepts);
        if (lane == 0u) {
            atomicAdd(&counters[2], (unsigned long long)n_cells);
            atomicMax(&counters[3], (unsigned long long)max_sp);
            atomicAdd(&counters[4], (unsigned long long)n_leaves);
            atomicMax(&counters[5], (unsigned long long)n_cells);  // the longest walk of any group
            atomicAdd(&counters[6], (unsigned long long)n_batches);
            atomicAdd(&counters[7], (unsigned long long)n_batches * (unsigned long long)(64 * G));
            atomicAdd(&counters[8], (unsigned long long)n_idle_pairs);  // (batch, pair of bodies) with no visit at all
            atomicAdd(&counters[9], (unsigned long long)n_evals);       // batches that ran the pair evaluation
        }
    }
#if defined(NB_DIAG_PHASES) || defined(NB_DIAG_TIMELINE)
    if (lane == 0u && G == 8) {  // per wave, no atomics: counters + 16 + 8 * group index
        unsigned long long *out = counters + 16 + 8 * (size_t)((i0 - lo) / (uint32_t)G);
#ifdef NB_DIAG_PHASES
        for (int k = 0; k < 4; ++k) out[k] = ph[k];
#else
        out[0] = 0ull;
#endif
        out[4] = tl_batches;   // batches, then the wave's first and last batch on the 100 MHz clock
        out[5] = tl_start;
        out[6] = __builtin_amdgcn_s_memrealtime();
        out[7] = tl_launch;
    }
#endif
    if (bound_slots && lane == 0u)  // the next step's root cube: max |coord| of the new positions (nobody waits)
        publish_bound(bound_slots, blockIdx.x, fmaxf(fmaxf(fmaxf(fabsf(blx), fabsf(bhx)), fmaxf(fabsf(bly), fabsf(bhy))),
                                                     fmaxf(fabsf(blz), fabsf(bhz))));
    if (!owner) return;
    if (PART == 1) {
        acc_dst[ib] = float4{tx, ty, tz, 0.f};
        return;
    }
    const float gdt = g * dt;
    const float fx = tx * gdt, fy = ty * gdt, fz = tz * gdt;
    // the same loads and the same operations as before the walk: bit for bit the same half kick
    const uint32_t jb = va_order ? va_order[ib] : ib;
    const float4 p = posm_src[ib], v = vel_src[jb], a = acc_src[jb];
    const float vhx = kick(v.x, a.x, dt), vhy = kick(v.y, a.y, dt), vhz = kick(v.z, a.z, dt);
    posm_dst[ib] = float4{drift(p.x, vhx, dt), drift(p.y, vhy, dt), drift(p.z, vhz, dt), p.w};
    vel_dst[ib] = float4{kick(vhx, fx, dt), kick(vhy, fy, dt), kick(vhz, fz, dt), 0.f};
    acc_dst[ib] = float4{fx, fy, fz, 0.f};
}
