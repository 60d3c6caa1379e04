// nb_tree_let.hpp -- part of the nb_tree.hip translation unit: included there, inside its
// namespace nb { namespace {, and never compiled on its own.
// stage 9: locally essential trees (meta, export, rebase, push) and the migration of bodies.

// ---- 9. locally essential trees (multi-GPU Barnes-Hut) ------------------------
// Every rank owns a Morton range of the bodies and builds the octree of ITS bodies inside the
// GLOBAL root cube.  What a peer needs of that tree to walk it for its own bodies is the
// "locally essential tree" (LET): starting at the root, a cell that EVERY point of the peer's
// bounding box accepts (size^2 < theta^2 * dmin^2, dmin = distance from the cell's centre of
// gravity to the box) is exported as a terminal pseudo-body, any other cell is exported with
// its children.  dmin^2 is evaluated with the walk's own operation order on the per-axis
// clamped distances, and fp32 subtract / multiply / fma are monotonic, so dmin^2 <= the r^2 any
// body inside the box computes: the pruning never changes a decision a body of the peer would
// take -- walking the LET gives bit for bit what walking the whole remote tree would give.
//
// Per-rank meta words exchanged before the build (all-gather): [0] bits of max |coord| of the
// source positions (the global root cube is the max over ranks), [1..3] / [4..6] min / max of the
// DRIFTED positions (the points the walk evaluates at) in an order-preserving u32 encoding.
constexpr int kLetMetaWords = 8;

__device__ __forceinline__ uint32_t let_f2ord(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float let_ord2f(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__global__ __launch_bounds__(256) void let_meta_kernel(const float4 *__restrict__ posm,
                                                       const float4 *__restrict__ vel,
                                                       const float4 *__restrict__ acc, uint32_t n, float dt,
                                                       uint32_t *__restrict__ meta) {
    __shared__ float s_lo[4][3], s_hi[4][3];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = posm[i], v = vel[i], a = acc[i];
        // exactly the walk's evaluation point (kick + drift, tree.wgsl:105-106)
        const float x = drift(p.x, kick(v.x, a.x, dt), dt), y = drift(p.y, kick(v.y, a.y, dt), dt),
                    z = drift(p.z, kick(v.z, a.z, dt), dt);
        lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
        lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
        lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], o));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o));
        }
        if ((threadIdx.x & 63) == 0) {
            s_lo[threadIdx.x >> 6][c] = lo[c];
            s_hi[threadIdx.x >> 6][c] = hi[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const float l = fminf(fminf(s_lo[0][c], s_lo[1][c]), fminf(s_lo[2][c], s_lo[3][c]));
        const float h = fmaxf(fmaxf(s_hi[0][c], s_hi[1][c]), fmaxf(s_hi[2][c], s_hi[3][c]));
        if (l <= h) {  // (a block that saw no body contributes nothing)
            atomicMin(&meta[1 + c], let_f2ord(l));
            atomicMax(&meta[4 + c], let_f2ord(h));
        }
    }
}

// the global root cube: max over ranks of the local bounds (bit patterns of floats >= 1.0)
__global__ void let_global_bound_kernel(const uint32_t *__restrict__ meta_all, int world,
                                        uint32_t *__restrict__ bound_bits, uint32_t *__restrict__ my_counts,
                                        int rank, uint32_t first_free) {
    uint32_t m = __float_as_uint(1.0f);
    for (int r = 0; r < world; ++r) m = max(m, meta_all[r * kLetMetaWords]);
    *bound_bits = m;
    // every peer's export starts with the root in slot 0 (one-launch export: slots 1..72 reserved too)
    if (my_counts)
        for (int r = 0; r < world; ++r) my_counts[r] = r == rank ? 0u : first_free;
}

// One depth of the export, all peers at once (blockIdx.y = peer).  Node ids are breadth-first
// (depth-major), so the nodes of one depth are a contiguous id range and their parents were
// handled by the previous launch: a reached node finds its output slot in out_slot.
__global__ __launch_bounds__(256) void let_export_level_kernel(
    const NodeRec *__restrict__ rec, const uint32_t *__restrict__ depth_base, int depth,
    const uint32_t *__restrict__ n_nodes_p, uint32_t n_cap, const uint32_t *__restrict__ meta_all,
    int rank, bool prune, uint32_t *__restrict__ out_slot, NodeRec *__restrict__ send,
    uint32_t *__restrict__ counts, uint32_t cap, uint32_t *__restrict__ status) {
    const int q = blockIdx.y;
    if (q == rank) return;
    const uint32_t n_nodes = min(*n_nodes_p, n_cap);
    const uint32_t begin = depth_base[depth], end = min(depth_base[depth + 1], n_nodes);
    if (begin >= end) return;
    const uint32_t *mq = meta_all + q * kLetMetaWords;
    const float blo[3] = {let_ord2f(mq[1]), let_ord2f(mq[2]), let_ord2f(mq[3])};
    const float bhi[3] = {let_ord2f(mq[4]), let_ord2f(mq[5]), let_ord2f(mq[6])};
    if (!(blo[0] <= bhi[0])) return;  // the peer has no bodies: nothing to export
    uint32_t *slots = out_slot + (size_t)q * n_cap;
    NodeRec *out = send + (size_t)q * cap;
    // A block takes 256 consecutive nodes at a time and allocates the output slots of all their
    // children with ONE atomic (block-wide scan of the child counts): children of neighbouring
    // cells stay neighbours in the export, which is what the importer's caches want, and the
    // counter sees 1/256 of the traffic.
    __shared__ uint32_t s_wave[4], s_base;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t chunk = begin + blockIdx.x * blockDim.x; chunk < end; chunk += gridDim.x * blockDim.x) {
        const uint32_t id = chunk + threadIdx.x;
        uint32_t slot = ~0u, want = 0u;
        NodeRec r{};
        if (id < end) {
            slot = depth == 0 ? 0u : slots[id];
            if (slot < cap) {  // (~0: not reached for this peer)
                r = rec[id];
                if (r.count != 0u) {
                    // nearest point of the box to the centre of gravity, per axis, then r^2 in the walk's order
                    const float dx = r.cogm.x - fminf(fmaxf(r.cogm.x, blo[0]), bhi[0]);
                    const float dy = r.cogm.y - fminf(fmaxf(r.cogm.y, blo[1]), bhi[1]);
                    const float dz = r.cogm.z - fminf(fmaxf(r.cogm.z, blo[2]), bhi[2]);
                    const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    // some point of the box may open it: export the children too
                    if ((!prune || !(r.mac2 < r2)) && r.first + r.count <= n_nodes) want = r.count;
                }
            }
        }
        uint32_t incl = want;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if ((int)lane >= o) incl += y;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0u;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        if (threadIdx.x == 0) {
            const uint32_t total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            s_base = total ? atomicAdd(&counts[q], total) : 0u;
        }
        __syncthreads();
        if (slot < cap) {
            NodeRec o{r.cogm, 0u, 0u, ~0u, -1.0f};  // terminal: a body / pseudo-body for the peer
            if (want) {
                const uint32_t base = s_base + before + incl - want;
                if (base + want <= cap) {
                    for (uint32_t c = 0; c < want; ++c) slots[r.first + c] = base + c;
                    o = NodeRec{r.cogm, base, want, ~0u, r.mac2};
                } else {
                    atomicAdd(&status[0], 1u);  // capacity exceeded: reported by check_status
                }
            }
            out[slot] = o;
        }
        __syncthreads();  // s_wave / s_base are reused by the next chunk
    }
}

// a peer whose export ran out of room (status[0], an error at the next read-back) still gets a
// count that fits its segment
// The whole export in ONE launch (the level-by-level form above is 23 dependent launches whatever the
// tree's depth: ~115 us of a LET step that takes ~350 at 131,072 bodies per rank).  A workgroup of
// 1,024 threads exports, for one peer q (blockIdx.y), the subtree under one of the 64 grandchildren
// (blockIdx.x) of the root, breadth-first: the level's records sit in the peer's segment already (allocated by their
// parents), each holding -- provisionally, in `first` -- the node it stands for; the workgroup takes
// them 1,024 at a time, decides terminal / exported with children exactly as above, allocates the
// children of a chunk with one atomic on the peer's counter and remembers the (base, length) of every
// allocation in LDS: those ranges are the next level.  Slots 1..72 of a segment are reserved for the
// root's children and grandchildren (unused ones hold terminals nobody references), which is what
// lets the 64 subtrees proceed without meeting (with 8 subtrees a workgroup had up to 1/8 of a big
// export to itself: 400 us instead of 310 for the build + export of 524,288 bodies).  The layout of a segment depends on the order of the atomics; the
// walk does not (siblings stay consecutive and in octant order, and a lane's partial sums are
// added across the wave in a fixed order): bit for bit the level-by-level export's result.
struct LetRange {
    uint32_t base, len;
};
constexpr uint32_t kLetExportThreads = 1024, kLetExportRanges = 3072;  // 2 lists x 24 KiB of LDS
constexpr uint32_t kLetReserved = 73;  // the root, its 8 children, their 64 children: fixed slots
constexpr uint32_t kLetListOverflow = 0x80000000u;  // status[0]: a level outgrew the one-launch export's range list

__device__ __forceinline__ uint32_t let_export_want(const NodeRec &r, const float (&blo)[3], const float (&bhi)[3],
                                                    bool prune, uint32_t n_nodes) {
    if (r.count == 0u) return 0u;
    // nearest point of the box to the centre of gravity, per axis, then r^2 in the walk's order
    const float dx = r.cogm.x - fminf(fmaxf(r.cogm.x, blo[0]), bhi[0]);
    const float dy = r.cogm.y - fminf(fmaxf(r.cogm.y, blo[1]), bhi[1]);
    const float dz = r.cogm.z - fminf(fmaxf(r.cogm.z, blo[2]), bhi[2]);
    const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    // some point of the box may open it: export the children too
    return ((!prune || !(r.mac2 < r2)) && r.first + r.count <= n_nodes) ? r.count : 0u;
}

__global__ __launch_bounds__(kLetExportThreads) void let_export_kernel(
    const NodeRec *__restrict__ rec, const uint32_t *__restrict__ n_nodes_p, uint32_t n_cap,
    const uint32_t *__restrict__ meta_all, int rank, bool prune, NodeRec *send,
    uint32_t *__restrict__ counts, uint32_t cap, uint32_t *__restrict__ status) {
    const int q = blockIdx.y;
    const uint32_t sub = blockIdx.x, tid = threadIdx.x;
    if (q == rank) return;
    const uint32_t n_nodes = min(*n_nodes_p, n_cap);
    const uint32_t *mq = meta_all + q * kLetMetaWords;
    const float blo[3] = {let_ord2f(mq[1]), let_ord2f(mq[2]), let_ord2f(mq[3])};
    const float bhi[3] = {let_ord2f(mq[4]), let_ord2f(mq[5]), let_ord2f(mq[6])};
    if (!(blo[0] <= bhi[0]) || n_nodes == 0u) {  // the peer has no bodies / this rank has none: nothing to export
        if (sub == 0u && tid == 0u) counts[q] = 0u;
        return;
    }
    NodeRec *out = send + (size_t)q * cap;
    const NodeRec root = rec[0];
    const uint32_t want0 = cap >= kLetReserved ? let_export_want(root, blo, bhi, prune, n_nodes) : 0u;
    const NodeRec dummy{float4{0.f, 0.f, 0.f, 0.f}, 0u, 0u, ~0u, -1.0f};
    if (sub == 0u && tid < kLetReserved) {
        // slot 0: the root; 1 + c: child c of the root; 9 + 8 c + j: child j of that child (those that exist
        // and are exported are written by their own workgroups, the rest hold terminals nobody references)
        if (tid == 0u) {
            out[0] = want0 ? NodeRec{root.cogm, 1u, want0, ~0u, root.mac2} : NodeRec{root.cogm, 0u, 0u, ~0u, -1.0f};
            if (!want0) counts[q] = 1u;  // (the counter starts at kLetReserved; nobody else touches it then)
        } else if (want0) {
            const uint32_t c = tid <= 8u ? tid - 1u : (tid - 9u) >> 3, j = (tid - 9u) & 7u;
            NodeRec rc = dummy;
            uint32_t want1 = 0u;
            if (c < want0) {
                rc = rec[root.first + c];
                want1 = let_export_want(rc, blo, bhi, prune, n_nodes);
            }
            if (tid <= 8u) {
                if (c < want0)
                    out[tid] = want1 ? NodeRec{rc.cogm, 9u + 8u * c, want1, ~0u, rc.mac2}
                                     : NodeRec{rc.cogm, 0u, 0u, ~0u, -1.0f};
                else
                    out[tid] = dummy;
            } else if (j >= want1) {
                out[tid] = dummy;
            }
        }
    }
    const uint32_t c = sub >> 3, j = sub & 7u;
    if (c >= want0) return;
    const NodeRec rc = rec[root.first + c];
    if (j >= let_export_want(rc, blo, bhi, prune, n_nodes)) return;
    const uint32_t seed_slot = 9u + 8u * c + j, seed_node = rc.first + j;

    __shared__ LetRange s_list[2][kLetExportRanges];
    __shared__ uint32_t s_n[2], s_wave[kLetExportThreads / 64], s_base;
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    if (tid == 0u) {
        out[seed_slot].first = seed_node;  // provisional: the node this record stands for
        s_list[0][0] = LetRange{seed_slot, 1u};
        s_n[0] = 1u;
        s_n[1] = 0u;
    }
    __threadfence_block();
    __syncthreads();
    for (uint32_t cur = 0;; cur ^= 1u) {
        const uint32_t nr = s_n[cur];
        if (nr == 0u) break;
        for (uint32_t ri = 0; ri < nr; ++ri) {
            const LetRange rg = s_list[cur][ri];
            for (uint32_t off = 0; off < rg.len; off += kLetExportThreads) {
                const uint32_t i = off + tid, slot = rg.base + i;
                const bool valid = i < rg.len;
                NodeRec r{};
                uint32_t want = 0u;
                if (valid) {
                    r = rec[out[slot].first];
                    want = let_export_want(r, blo, bhi, prune, n_nodes);
                }
                uint32_t incl = want;
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(incl, o);
                    if ((int)lane >= o) incl += y;
                }
                if (lane == 63u) s_wave[wave] = incl;
                __syncthreads();
                uint32_t before = 0u;
                for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
                if (tid == 0u) {
                    uint32_t total = 0u;
                    for (uint32_t w = 0; w < kLetExportThreads / 64u; ++w) total += s_wave[w];
                    uint32_t base = 0u;
                    if (total) {
                        base = atomicAdd(&counts[q], total);
                        const uint32_t k = s_n[cur ^ 1u];
                        if (base + total <= cap && k < kLetExportRanges) {
                            s_list[cur ^ 1u][k] = LetRange{base, total};
                            s_n[cur ^ 1u] = k + 1u;
                        } else {
                            // the peer's segment is full (counted), or this level has more ranges than the LDS list
                            // holds (flagged apart: the segment had room, the level-by-level export would succeed);
                            // either way none of this chunk's cells is exported with children.  check_status reports it.
                            if (base + total > cap) atomicAdd(&status[0], 1u);
                            else atomicOr(&status[0], kLetListOverflow);
                            base = ~0u;
                        }
                    }
                    s_base = base;
                }
                __syncthreads();
                if (valid) {
                    NodeRec o{r.cogm, 0u, 0u, ~0u, -1.0f};  // terminal: a body / pseudo-body for the peer
                    if (want && s_base != ~0u) {
                        const uint32_t base = s_base + before + incl - want;
                        for (uint32_t c = 0; c < want; ++c) out[base + c].first = r.first + c;  // provisional
                        o = NodeRec{r.cogm, base, want, ~0u, r.mac2};
                    }
                    out[slot] = o;
                }
                __threadfence_block();
                __syncthreads();  // s_wave / s_base are reused; the provisional records are visible
            }
        }
        if (tid == 0u) s_n[cur] = 0u;
        __syncthreads();
    }
}

__global__ void let_clamp_counts_kernel(uint32_t *__restrict__ counts, int world, uint32_t cap) {
    const int q = threadIdx.x;
    if (q < world) counts[q] = min(counts[q], cap);
}

// ---- migration: a body belongs to the rank whose Morton-key range (in a fixed reference cube)
// holds its position.  Bodies that left are packed per destination, the rest are compacted;
// the order inside the arrays is irrelevant (every step re-sorts).
struct LetOwners {
    uint32_t world;
    float ref_bound;                        // the reference cube is [-ref_bound, ref_bound]^3
    unsigned long long split[kLetMaxWorld]; // rank r owns keys in [split[r-1], split[r]); split[world-1] = inf
};

__device__ __forceinline__ unsigned long long let_spread21(unsigned long long v) {
    v &= 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull;
    v = (v | (v << 16)) & 0x1f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

__device__ __forceinline__ unsigned long long let_ref_key(float4 p, float ref_bound) {
    const double b = (double)ref_bound;
    unsigned long long q[3];
    const float c[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double t = ((double)c[k] + b) / (2.0 * b) * 2097152.0;
        t = t < 0.0 ? 0.0 : (t > 2097151.0 ? 2097151.0 : t);   // NaN falls through to the cast: 0
        q[k] = (unsigned long long)t;
    }
    return let_spread21(q[0]) | (let_spread21(q[1]) << 1) | (let_spread21(q[2]) << 2);
}

// stayers -> dst arrays (compacted), leavers -> send segment of their owner (12 floats per body)
__global__ __launch_bounds__(256) void let_migrate_kernel(
    const float4 *__restrict__ posm, const float4 *__restrict__ vel, const float4 *__restrict__ acc,
    uint32_t n, LetOwners own, int rank, float4 *__restrict__ posm_dst, float4 *__restrict__ vel_dst,
    float4 *__restrict__ acc_dst, float4 *__restrict__ send, uint32_t seg_cap,
    uint32_t *__restrict__ counts, uint32_t *__restrict__ status) {
    __shared__ uint32_t s_cnt[kLetMaxWorld], s_base[kLetMaxWorld];
    if (threadIdx.x < kLetMaxWorld) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t dest = 0, local = 0;
    float4 p{}, v{}, a{};
    if (i < n) {
        p = posm[i];
        v = vel[i];
        a = acc[i];
        const unsigned long long key = let_ref_key(p, own.ref_bound);
        while (dest + 1 < own.world && key >= own.split[dest]) ++dest;
        local = atomicAdd(&s_cnt[dest], 1u);
    }
    __syncthreads();
    if (threadIdx.x < own.world)
        s_base[threadIdx.x] = s_cnt[threadIdx.x] ? atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]) : 0u;
    __syncthreads();
    if (i >= n) return;
    const uint32_t slot = s_base[dest] + local;
    if ((int)dest == rank) {
        posm_dst[slot] = p;   // slot < n: stayers never outnumber the bodies
        vel_dst[slot] = v;
        acc_dst[slot] = a;
    } else if (slot < seg_cap) {
        float4 *o = send + ((size_t)dest * seg_cap + slot) * 3;
        o[0] = p;
        o[1] = v;
        o[2] = a;
    } else {
        atomicAdd(&status[0], 1u);  // more leavers than the segment holds: reported by check_status
    }
}

__global__ void let_append_kernel(const float4 *__restrict__ recv, uint32_t count, uint32_t at,
                                  float4 *__restrict__ posm, float4 *__restrict__ vel,
                                  float4 *__restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    posm[at + i] = recv[3 * (size_t)i + 0];
    vel[at + i] = recv[3 * (size_t)i + 1];
    acc[at + i] = recv[3 * (size_t)i + 2];
}

struct LetSegments {
    uint32_t world;
    uint32_t off[kLetMaxWorld + 1];  // record offsets of the imported segments (exclusive scan)
};

// imported child links are relative to their segment: make them indices into the walk's table,
// and turn any link that does not point forward inside its own segment into a terminal
__global__ void let_rebase_kernel(NodeRec *__restrict__ imp, LetSegments segs, uint32_t import_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= segs.off[segs.world]) return;
    uint32_t s = 0;
    while (s + 1 < segs.world && i >= segs.off[s + 1]) ++s;
    NodeRec r = imp[i];
    const uint32_t local = i - segs.off[s], seg_n = segs.off[s + 1] - segs.off[s];
    r.self_pos = ~0u;
    if (r.count != 0u) {
        if (r.count <= 8u && r.first > local && r.first + r.count <= seg_n) {
            r.first += import_base + segs.off[s];
        } else {
            r.first = 0u;
            r.count = 0u;
            r.mac2 = -1.0f;
        }
    }
    imp[i] = r;
}

// The same for imports that arrive in FIXED-STRIDE segments (nb_sim_let_set_import_stride): segment j
// (the j-th peer in rank order, this rank skipped) starts at record j * stride, and how many of its
// records are real is read HERE, on the device, from the all-gathered counts matrix -- the host
// never sees the counts, so a step needs no host synchronisation.  Also writes the walk's roots.
__global__ void let_rebase_fixed_kernel(NodeRec *__restrict__ imp, const uint32_t *__restrict__ counts_all,
                                        uint32_t me, uint32_t world, uint32_t stride, uint32_t import_base,
                                        uint32_t own_root, WalkRoots *__restrict__ roots_dev,
                                        uint32_t *__restrict__ status) {
    // blockIdx.y = segment (the peers in rank order, this rank left out); the blocks of a segment stride over
    // its LIVE records only -- the launch does not grow with the stride (the one-process runner's is the
    // whole tree_let_cap)
    if (blockIdx.x == 0u && blockIdx.y == 0u && threadIdx.x == 0u) {
        // the trees this rank walks: its own (optional), then the non-empty imports in rank order
        WalkRoots rt{};
        if (own_root) rt.id[rt.count++] = 0u;
        for (uint32_t r = 0; r < world; ++r) {
            if (r == me) continue;
            const uint32_t c = counts_all[r * world + me], j = r < me ? r : r - 1u;
            if (c > stride) atomicAdd(&status[0], 1u);  // the sender had more than the segment holds
            if (c) rt.id[rt.count++] = import_base + j * stride;
        }
        *roots_dev = rt;
    }
    if (world < 2u) return;
    const uint32_t j = blockIdx.y, r = j < me ? j : j + 1u;
    const uint32_t seg_n = min(counts_all[r * world + me], stride);
    NodeRec *seg = imp + (size_t)j * stride;
    for (uint32_t local = blockIdx.x * blockDim.x + threadIdx.x; local < seg_n; local += gridDim.x * blockDim.x) {
        NodeRec rc = seg[local];
        rc.self_pos = ~0u;
        if (rc.count != 0u) {
            if (rc.count <= 8u && rc.first > local && rc.first + rc.count <= seg_n) {
                rc.first += import_base + j * stride;
            } else {
                rc.first = 0u;
                rc.count = 0u;
                rc.mac2 = -1.0f;
            }
        }
        seg[local] = rc;
    }
}

// One-process LET runner (nb_group.cpp): the records exported for peer q go straight into q's import
// area through peer access -- as many as the export counted (this rank's row of the counts table, read
// here on the device), to the segment the fixed-stride layout gives this rank on q.  blockIdx.y = q.
struct LetImportPtrs {
    NodeRec *p[kLetMaxWorld];
};
__global__ __launch_bounds__(256) void let_push_segments_kernel(const NodeRec *__restrict__ send, uint32_t seg_records,
                                                                const uint32_t *__restrict__ my_counts,
                                                                LetImportPtrs imports, uint32_t me, uint32_t stride) {
    const uint32_t q = blockIdx.y;
    if (q == me) return;
    const uint32_t count = min(my_counts[q], stride);  // (more than the segment holds: the receiver reports it)
    const uint32_t j = me < q ? me : me - 1u;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(send + (size_t)q * seg_records);
    uint4 *d4 = reinterpret_cast<uint4 *>(imports.p[q] + (size_t)j * stride);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count * 2u; i += gridDim.x * blockDim.x) d4[i] = s4[i];
}
