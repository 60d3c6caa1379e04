// nb_tree.hip -- Barnes-Hut simulator for gfx950: TreeSim (src/sims/tree.rs) + the tree-walk
// shader (src/sims/shaders/tree.wgsl), rebuilt so that NOTHING leaves the GPU.
//
// The reference's step (TreeSim::encode, tree.rs:262-353) maps the particle buffer to the
// host, builds the octree with a serial BFS over bump-allocated index lists (tree.rs:417-546),
// reorders the particles in DFS order (tree.rs:564-602), uploads particles + tree and only
// then dispatches the walk.  Here the same tree -- same cells, same node numbering, same
// children tables, same body order -- is constructed on the device from Morton keys:
//
//   1 bound               max |coord| (>= 1.0) -> root cube [-b,b]^3              tree.rs:424-446
//   nb_tree_sort.hpp      (bound_kernel; in steady state accumulated by the previous step's walk)
//   2 morton_kernel       63-bit key per body by the reference's own float descent:
//   nb_tree_sort.hpp      digit = (x>cx) | (y>cy)<<1 | (z>cz)<<2 with strict '>',
//                         centre += +-width/4, width /= 2   (21 levels)        tree.rs:549-562
//   3 sort                stable, by (key, index).  Radix passes of 8 bits (per-tile digit histogram in
//   nb_tree_sort.hpp      LDS, per-bin scan over the tiles, stable scatter ranked with wave ballots)
//                         over the HIGH digits only -- 2 or 3 passes on (high word of the key, index)
//                         pairs, 3e -- then a fix-up of the bodies that tie there (runs_rank_kernel:
//                         a thread per body; runs_fix_kernel for the 64-bit form, 3d); the whole sort
//                         in one launch by counting up to 12,288 bodies (3c); 8 passes over the
//                         whole key as the cross-check (tuning key tree_sort_mode 0)
//   4-6a cells_a/scan/c   bodies into sorted order = the reference's DFS order (tree.rs:564-602);
//   nb_tree_cells.hpp     a cell at depth d exists for every key-prefix run: body k opens the
//                         internal cells of depths (cpl[k-1], cpl[k]] and owns one leaf at depth
//                         max(cpl[k-1],cpl[k])+1, where cpl = common prefix length (levels) of
//                         neighbouring keys.  Node id = (#nodes of smaller depth) + rank among
//                         the nodes of its depth in key order -- exactly the reference's BFS
//                         allocation order (tree.rs:461,517-519; slice_alloc.rs:52-59); binary64
//                         prefix sums of (m x, m y, m z, m) over the sorted bodies for the mass /
//                         centre of gravity of every cell (tree.rs:486-505).  Three launches.
//   6 fill_kernel         per node: body range by a galloping search on the keys; children = the
//   nb_tree_cells.hpp     consecutive next-depth ids starting at the first body's own child
//                         (0 = none; a leaf's children[0] = the body's source index, tree.rs:532)
//   8 walk                tree.wgsl:41-111 with the INTENDED semantics: self
//   nb_tree_walk.hpp      excluded by identity, a leaf is a body, no fixed 64-entry stack; every
//                         body applies ITS OWN acceptance test size/dist < theta to exactly the
//                         cells of the reference's per-thread walk (visit counts equal the
//                         oracle's), in a different order of summation (fp32 rounding).
//                         8b walk_cells_kernel (default): a wave walks for 8 (or 16) bodies held in
//                         scalars, its 64 lanes hold 64 cells of the traversal frontier; the test
//                         compares the cell's stored acceptance radius^2 = size^2 / theta^2 with
//                         r^2, the accumulation runs under exec = the lanes that take the cell.
//                         8  walk_kernel: a wave walks for 64 bodies, one cell at a time.
//
//   9 LET                 several GPUs: locally essential trees -- meta words, export, rebase, migration
//   nb_tree_let.hpp
//
// This file is the one translation unit: it includes the stage headers above (and nb_tree_wave.hpp: constants,
// kick / drift, the wave-level scans) and holds the host side, TreeSim.
//
// Deviations, all documented in DESIGN.md: bodies whose 63-bit keys collide (closer than
// root_width/2^21) cannot be separated (the reference would recurse until its 4N-node buffer
// overflows); cog/mass come from binary64 prefix sums instead of a sequential fp32 sum per cell.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "nb_sim.hpp"

namespace nb {
namespace {

// the device code, by pipeline stage (each header builds on the ones before it)
#include "nb_tree_wave.hpp"
#include "nb_tree_sort.hpp"
#include "nb_tree_cells.hpp"
#include "nb_tree_walk.hpp"
#include "nb_tree_let.hpp"

// =================================================================================================
// TreeSim host side
// =================================================================================================
class TreeSim final : public SimBase {
    // ---- the device scalar block `scalars`: word offsets --------------------------------------------
    enum : uint32_t {
        kScBound = 0,       // the root cube: max |coord| (>= 1.0) as float bits
        kScNodes = 1,       // nodes of the last build
                            // (2, 3: unused; words 0..3 are cleared where a build takes its own bound)
        kScStatus = 4,      // kStatusWords sticky error counts, below
        kScRunStat = 8,     // kRunStatWords statistics of the sort's fix-ups, below
        kScDepthBase = 16,  // kMaxDepth + 2 words: the first node id of every depth
        kScRowTotal = 40,   // kCellRows words: the column sums of the tile table
        kScalarWords = 128,
    };
    // the status words, as the kernels count into them and report_status reads them
    enum : uint32_t {
        kStLetExport = 0,     // LET cells (or migrating bodies) that did not fit a segment; kLetListOverflow
        kStNodeOverflow = 1,  // nodes beyond the 4N capacity
        kStKeyTies = 2,       // bodies that share their 63-bit key with a neighbour
        kStWalkStack = 3,     // walks that hit the stack guard
        kStatusWords = 4,
    };
    // the run statistics: each at [.. + parity] of the fix-up launch that wrote it (next_run_stats)
    enum : uint32_t { kRunLongest = 0, kRunProbe = 2, kRunSlow = 4, kRunStatWords = 6 };
    // the pinned mirror h_status (wait()): the status words and the run statistics in one copy, up to the next table
    // (48 bytes, whole 16-byte units: a copy of just the 40 bytes in use made a synchronous 8,192-body step 0.8 us
    // slower)
    static constexpr uint32_t kMirrorWords = kScDepthBase - kScStatus;
    static_assert(kScRunStat == kScStatus + kStatusWords && kStatusWords + kRunStatWords <= kMirrorWords &&
                      kMirrorWords % 4 == 0,
                  "h_status mirrors kMirrorWords contiguous words from kScStatus");
    static_assert(kScDepthBase + kMaxDepth + 2 <= kScRowTotal && kScRowTotal + kCellRows <= kScalarWords,
                  "the scalar block's tables overlap");

   public:
    ~TreeSim() override {
        (void)hipSetDevice(place.device_id);
        drop_graph();
        for (void *p : allocs) (void)hipFree(p);
        for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
        if (h_status) (void)hipHostFree(h_status);
    }

    int init(const nb_particle *host, size_t count) override {
        if (count != n) {
            set_error("particle count %zu does not match sim_params.particle_num %u", count, n);
            return NB_ERR_INVALID;
        }
        theta = add.theta > 0.f ? add.theta : NB_DEFAULT_THETA;
        n_capacity = n;
        const size_t nn = n ? n : 1;
        node_cap = (uint32_t)std::min<size_t>(4 * nn + 8, kSlotIdMask);  // 4N as tree.rs:188-190 (node ids take 27 bits of a slot record: 33 million bodies before the cap is less than 4N)
        sort_items = nn <= kSortSmallMax ? kSortItemsSmall : kSortItems;
        sort_blocks = (uint32_t)((nn + kSortThreads * sort_items - 1) / (kSortThreads * sort_items));
        cell_tiles = (uint32_t)std::max({std::min<size_t>(nn, 131072) / 256, std::min<size_t>(nn, 524288) / 512, nn / kCellTile}) + 4;  // capacity
        const size_t npad = n_pad ? n_pad : 256;  // equal-sized slices for the all-gathers
        for (int b = 0; b < 2; ++b) {
            for (float4 **a : {&posm[b], &vel[b], &acc[b]}) {
                if (int rc = alloc(a, sizeof(float4) * npad)) return rc;
                NB_HIP_TRY(hipMemsetAsync(*a, 0, sizeof(float4) * npad, stream));
            }
            if (int rc = alloc(&keys[b], sizeof(uint64_t) * nn)) return rc;
            if (int rc = alloc(&idx[b], sizeof(uint32_t) * nn)) return rc;
        }
        if (int rc = alloc(&d_aos, sizeof(nb_particle) * nn)) return rc;
        if (int rc = alloc(&hist, sizeof(uint32_t) * kSortMaxBins * (size_t)sort_blocks)) return rc;
        if (int rc = alloc(&totals, sizeof(uint32_t) * kSortMaxBins)) return rc;
        if (int rc = alloc(&cpl, nn + 2)) return rc;
        if (int rc = alloc(&int_slot, sizeof(uint32_t) * nn)) return rc;
        if (int rc = alloc(&tile_u32, sizeof(uint32_t) * kCellRows * ((size_t)cell_tiles + 4))) return rc;
        if (int rc = alloc(&tile_mom, sizeof(Moments) * (size_t)cell_tiles)) return rc;
        if (int rc = alloc(&leaf_id, sizeof(uint32_t) * nn)) return rc;
        if (int rc = alloc(&int_id, sizeof(uint2) * (size_t)node_cap)) return rc;
        if (int rc = alloc(&node_first, sizeof(uint32_t) * (size_t)node_cap)) return rc;
        if (int rc = alloc(&node_depth, (size_t)node_cap)) return rc;
        if (int rc = alloc(&rec, sizeof(NodeRec) * (size_t)node_cap)) return rc;
        if (int rc = alloc(&mom_prefix, sizeof(Moments) * (nn + 1))) return rc;
        // (the reference's Octant fields -- cogm, bodies, child, the AoS staging: 104 B per node -- are
        // only produced for nb_sim_read_tree and allocated on its first call)
        if (int rc = alloc(&scalars, sizeof(uint32_t) * kScalarWords)) return rc;
        #if defined(NB_DIAG_PHASES) || defined(NB_DIAG_TIMELINE)
        if (int rc = alloc(&counters, sizeof(unsigned long long) * (16 + nn + 8))) return rc;
#else
        if (int rc = alloc(&counters, sizeof(unsigned long long) * 16)) return rc;
#endif
        if (int rc = alloc(&bound_buf, sizeof(uint32_t) * kBoundSlots)) return rc;
        NB_HIP_TRY(hipMemsetAsync(scalars, 0, sizeof(uint32_t) * kScalarWords, stream));
        NB_HIP_TRY(hipMemsetAsync(bound_buf, 0, sizeof(uint32_t) * kBoundSlots, stream));
        NB_HIP_TRY(hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 16, stream));
        NB_HIP_TRY(hipHostMalloc((void **)&h_status, sizeof(uint32_t) * kMirrorWords, hipHostMallocDefault));
        return write_particles(host, count);
    }

    int write_particles(const nb_particle *host, size_t count) override {
        if (count != n) {
            set_error("write_particles: count %zu != particle_num %u", count, n);
            return NB_ERR_INVALID;
        }
        if (int rc = bind_device()) return rc;
        if (n == 0) return NB_OK;
        build_done = false;  // a build enqueued for the old state is void
        bound_from_walk = false;
        // a graph captured after an eager step takes the root cube from the slots the previous walk
        // filled and holds no bound_kernel: replayed on the new state it would key the bodies in the
        // OLD state's cube.  Re-capture (the next capture starts from bound_kernel).
        drop_graph();
        NB_HIP_TRY(hipMemcpyAsync(d_aos, host, sizeof(nb_particle) * (size_t)n, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(tree_aos_to_soa_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_aos, n,
                           posm[cur], vel[cur], acc[cur]);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipStreamSynchronize(stream));
        return NB_OK;
    }

    // TreeSim::encode, tree.rs:262-353 -- everything on the device, nothing mapped to the host.
    // One step = 6 to 15 small launches (6 with the counting sort; three radix passes of up to three
    // launches, the fix-up and cells_scan_kernel make it 15; about 30 with the 8-pass sort of tree_sort_mode 0)
    // that never change (same buffers, same arguments every step: the state lands back in buffer `cur`), so the sequence can be captured into a hipGraph once
    // and replayed (tuning key "tree_use_graph").  Off by default: measured, the step is bound by
    // the GPU-side cost of the dependent launches, not by their submission (8,192 bodies: 459 us
    // eager vs 439 us replayed; no difference at 1 M), so the eager path is the one that ships.
    int encode() override {
        if (int rc = bind_device()) return rc;
        if (n == 0) {
            step_num += 1;
            return NB_OK;
        }
        if (!use_graph || time_walk || build_done) {
            if (int rc = enqueue_step()) return rc;
            step_num += 1;
            return NB_OK;
        }
        if (!graph_exec) {
            hipGraph_t graph = nullptr;
            NB_HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue_step();
            const hipError_t ec = hipStreamEndCapture(stream, &graph);
            if (rc) {
                if (graph) (void)hipGraphDestroy(graph);
                return rc;
            }
            NB_HIP_TRY(ec);
            const hipError_t ei = hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            NB_HIP_TRY(ei);
        }
        NB_HIP_TRY(hipGraphLaunch(graph_exec, stream));
        step_num += 1;
        return NB_OK;
    }

    void drop_graph() {
        if (graph_exec) {
            (void)hipGraphExecDestroy(graph_exec);
            graph_exec = nullptr;
        }
    }

    // The step in two halves (nb_sim_encode_phase): the build needs only positions and masses,
    // the walk also velocities and accelerations -- a multi-GPU host starts the build as soon as
    // the position all-gather of the previous step has landed and lets the other two overlap it.
    int encode_phase(int phase) override {
        if (int rc = bind_device()) return rc;
        if (phase == NB_PHASE_LET_MIGRATE) return let_migrate();
        if (phase == NB_PHASE_LET_WALK_OWN) return let_walk_own();
        if (phase >= NB_PHASE_LET_META && phase <= NB_PHASE_LET_WALK) return let_phase(phase);
        if (phase != 0 && phase != 1) {
            set_error("encode_phase: phase must be 0 or 1 (or a NB_PHASE_LET_* value)");
            return NB_ERR_INVALID;
        }
        if (let_world) {
            set_error("encode_phase(%d): this TreeSim runs the LET protocol (phases %d..%d)", phase,
                      NB_PHASE_LET_META, NB_PHASE_LET_WALK);
            return NB_ERR_INVALID;
        }
        if (n == 0) {
            if (phase == 1) step_num += 1;
            return NB_OK;
        }
        if (phase == 0) {
            if (build_done) {
                set_error("encode_phase(0) called twice for one step");
                return NB_ERR_INVALID;
            }
            if (int rc = enqueue_build(false)) return rc;
            build_done = true;
            return NB_OK;
        }
        if (!build_done)
            if (int rc = enqueue_build(false)) return rc;
        build_done = false;
        if (int rc = enqueue_walk(own_root())) return rc;
        step_num += 1;
        return NB_OK;
    }

    WalkRoots own_root() const {
        WalkRoots r{};
        r.count = n >= 2 ? 1u : 0u;  // (the reference's N = 1 tree is ill-formed; a lone body feels nothing)
        return r;
    }

    // ---- locally essential trees: the three phases of a multi-GPU step (see section 9) -----------
    // NB_PHASE_LET_META   local bound + drifted bounding box -> this rank's meta words
    //                     (caller: all-gather exchange region 0)
    // NB_PHASE_LET_BUILD  global root cube, local octree, LET export for every peer
    //                     (caller: all-gather region 1 = export counts, read them on the host,
    //                      all-to-all the segments of region 2 into region 3, nb_sim_let_set_imports)
    // NB_PHASE_LET_WALK   rebase the imported trees, walk own tree + imports, integrate
    int let_phase(int phase) {
        if (!let_world || !let_send) {
            set_error("LET phase %d: set tree_let_world, tree_let_rank and tree_let_cap first", phase);
            return NB_ERR_INVALID;
        }
        if (phase != let_next || let_arrivals_pending) {
            set_error("LET phases must run in order: expected %d, got %d%s", let_next, phase,
                      let_arrivals_pending ? " (a migration awaits nb_sim_let_set_arrivals)" : "");
            return NB_ERR_INVALID;
        }
        return phase == NB_PHASE_LET_META ? let_meta() : phase == NB_PHASE_LET_BUILD ? let_build() : let_walk();
    }

    int let_meta() {
        const int s = cur;
        uint32_t *my_meta = let_metas + (size_t)let_rank * kLetMetaWords;
        const uint32_t init_meta[kLetMetaWords] = {0u, ~0u, ~0u, ~0u, 0u, 0u, 0u, 0u};
        NB_HIP_TRY(hipMemcpyAsync(my_meta, init_meta, sizeof init_meta, hipMemcpyHostToDevice, stream));
        if (n) {
            const uint32_t g = std::min<uint32_t>((n + 255) / 256, 512);
            hipLaunchKernelGGL(bound_kernel, dim3(g), dim3(256), 0, stream, posm[s], n, my_meta);
            hipLaunchKernelGGL(let_meta_kernel, dim3(g), dim3(256), 0, stream, posm[s], vel[s], acc[s], n,
                               params.dt, my_meta);
        }
        NB_HIP_TRY(hipGetLastError());
        let_next = NB_PHASE_LET_BUILD;
        return NB_OK;
    }

    int let_build() {
        uint32_t *n_nodes = scalars + kScNodes, *status = scalars + kScStatus;
        uint32_t *my_counts = let_counts + (size_t)let_rank * let_world;
        NB_HIP_TRY(hipMemsetAsync(my_counts, 0, sizeof(uint32_t) * let_world, stream));
        if (n) {
            NB_HIP_TRY(hipMemsetAsync(scalars, 0, sizeof(uint32_t) * kScStatus, stream));
            // (segments too small for the one-launch export's reserved slots take the level-by-level form)
            const bool one_launch = let_export_mode == 1 && let_cap >= kLetReserved;
            hipLaunchKernelGGL(let_global_bound_kernel, dim3(1), dim3(1), 0, stream, let_metas, let_world,
                               scalars + kScBound, my_counts, let_rank, one_launch ? kLetReserved : 1u);
            if (int rc = enqueue_build(true, true)) return rc;  // (a LET rank's velocities never travel)
            if (one_launch) {
                hipLaunchKernelGGL(let_export_kernel, dim3(64, let_world), dim3(kLetExportThreads), 0, stream, rec,
                                   n_nodes, node_cap, let_metas, let_rank, let_prune, let_send,
                                   my_counts, let_cap, status);
            } else {
                NB_HIP_TRY(hipMemsetAsync(let_out_slot, 0xff, sizeof(uint32_t) * (size_t)let_world * node_cap,
                                          stream));
                for (int d = 0; d <= kMaxDepth; ++d)
                    hipLaunchKernelGGL(let_export_level_kernel, dim3(128, let_world), dim3(256), 0, stream, rec,
                                       scalars + kScDepthBase, d, n_nodes, node_cap, let_metas, let_rank,
                                       let_prune, let_out_slot, let_send, my_counts, let_cap, status);
            }
            hipLaunchKernelGGL(let_clamp_counts_kernel, dim3(1), dim3(64), 0, stream, my_counts, let_world,
                               let_cap);
            NB_HIP_TRY(hipGetLastError());
        }
        let_next = NB_PHASE_LET_WALK;
        let_imports_set = false;
        return NB_OK;
    }

    int let_walk() {
        if (!let_imports_set) {
            set_error("LET walk: call nb_sim_let_set_imports with this step's import counts first");
            return NB_ERR_INVALID;
        }
        // set 0 = the own tree (already walked by NB_PHASE_LET_WALK_OWN if let_own_walked), set 1 = the imports
        const int part = let_own_walked ? 2 : 0;
        const uint32_t split = let_own_walked ? 0u : 1u;
        WalkRoots roots{};
        if (let_import_stride) {
            // imports in fixed-stride segments, their counts read on the device (no host round trip)
            hipLaunchKernelGGL(let_rebase_fixed_kernel, dim3(64, std::max(1, let_world - 1)), dim3(256), 0, stream,
                               rec + node_cap, let_counts, (uint32_t)let_rank, (uint32_t)let_world,
                               let_import_stride, node_cap, (n && !let_own_walked) ? 1u : 0u, let_roots_dev,
                               scalars + kScStatus);
            if (n)
                if (int rc = enqueue_walk(roots, part, split, let_roots_dev)) return rc;
        } else {
            if (n && !let_own_walked) roots.id[roots.count++] = 0u;
            const uint32_t total = let_segs.off[let_segs.world];
            if (total) {
                hipLaunchKernelGGL(let_rebase_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, rec + node_cap,
                                   let_segs, node_cap);
                for (uint32_t r = 0; r < let_segs.world; ++r)
                    if (let_segs.off[r + 1] > let_segs.off[r]) roots.id[roots.count++] = node_cap + let_segs.off[r];
            }
            if (n)
                if (int rc = enqueue_walk(roots, part, split)) return rc;
        }
        let_own_walked = false;
        step_num += 1;
        let_next = NB_PHASE_LET_META;
        return NB_OK;
    }

    // NB_PHASE_LET_WALK_OWN (optional, between BUILD and WALK): the rank's own tree needs nothing
    // from the peers, so its part of the walk can run while the exported trees are exchanged;
    // NB_PHASE_LET_WALK then adds the imported trees and integrates (same sums, same order).
    int let_walk_own() {
        if (!let_world || let_next != NB_PHASE_LET_WALK || let_own_walked) {
            set_error("LET own-tree walk: only once, between NB_PHASE_LET_BUILD and NB_PHASE_LET_WALK");
            return NB_ERR_INVALID;
        }
        if (n) {
            WalkRoots roots{};
            roots.id[roots.count++] = 0u;
            if (int rc = enqueue_walk(roots, 1)) return rc;
        }
        let_own_walked = true;
        return NB_OK;
    }

    // NB_PHASE_LET_MIGRATE (optional, before NB_PHASE_LET_META): re-home the bodies whose position
    // left the rank's Morton-key range.  Stayers are compacted, leavers packed per owner into
    // region 5, counts (stayers at [rank]) into region 4; the caller all-gathers region 4, moves
    // the segments into region 6 and calls nb_sim_let_set_arrivals.
    int let_migrate() {
        if (!let_world || !let_send || !let_mig_send) {
            set_error("LET migrate: set tree_let_world / rank / cap and the owners (nb_sim_let_set_owners) first");
            return NB_ERR_INVALID;
        }
        if (let_next != NB_PHASE_LET_META) {
            set_error("LET migrate: only between steps");
            return NB_ERR_INVALID;
        }
        const int s = cur, d = cur ^ 1;
        uint32_t *my_counts = let_mig_counts + (size_t)let_rank * let_world;
        NB_HIP_TRY(hipMemsetAsync(my_counts, 0, sizeof(uint32_t) * let_world, stream));
        if (n)
            hipLaunchKernelGGL(let_migrate_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, posm[s], vel[s],
                               acc[s], n, let_owners, let_rank, posm[d], vel[d], acc[d], let_mig_send,
                               let_mig_cap, my_counts, scalars + kScStatus);
        NB_HIP_TRY(hipGetLastError());
        cur = d;  // the compacted stayers are the state now (their number: counts[rank])
        let_arrivals_pending = true;
        return NB_OK;
    }

    int let_set_owners(const unsigned long long *splits, int world, float ref_bound, uint32_t seg_cap) override {
        if (!let_world || world != let_world || !splits || !(ref_bound > 0.f) || seg_cap == 0) {
            set_error("let_set_owners: bad arguments (world %d, tree_let_world %d)", world, let_world);
            return NB_ERR_INVALID;
        }
        if (int rc = bind_device()) return rc;
        let_owners.world = (uint32_t)world;
        let_owners.ref_bound = ref_bound;
        for (int r = 0; r < world; ++r) let_owners.split[r] = r + 1 < world ? splits[r] : ~0ull;
        if (!let_mig_send) {
            const size_t w = (size_t)world;
            let_mig_cap = seg_cap;
            if (int rc = alloc(&let_mig_counts, sizeof(uint32_t) * w * w)) return rc;
            if (int rc = alloc(&let_mig_send, kMigratedBodyBytes * w * (size_t)seg_cap)) return rc;
            if (int rc = alloc(&let_mig_recv, kMigratedBodyBytes * w * (size_t)seg_cap)) return rc;
            NB_HIP_TRY(hipMemsetAsync(let_mig_counts, 0, sizeof(uint32_t) * w * w, stream));
            NB_HIP_TRY(hipStreamSynchronize(stream));
        }
        return NB_OK;
    }

    // after the exchange: `stay` bodies were kept, counts[r] arrived from rank r (packed in rank
    // order in region 6); the simulator's body count becomes stay + sum(counts)
    int let_set_arrivals(uint32_t stay, const uint32_t *counts, int world) override {
        if (!let_arrivals_pending || world != let_world || !counts) {
            set_error("let_set_arrivals: no migration in flight (or world mismatch)");
            return NB_ERR_INVALID;
        }
        if (int rc = bind_device()) return rc;
        uint64_t total = 0;
        for (int r = 0; r < world; ++r) total += (r == let_rank) ? 0u : counts[r];
        if (stay > n || stay + total > n_capacity || total > (uint64_t)let_mig_cap * world) {
            set_error("let_set_arrivals: %u kept + %llu arrived exceed the capacity of %u bodies", stay,
                      (unsigned long long)total, n_capacity);
            return NB_ERR_UNSUPPORTED;
        }
        if (total)
            hipLaunchKernelGGL(let_append_kernel, dim3(((uint32_t)total + 255) / 256), dim3(256), 0, stream,
                               let_mig_recv, (uint32_t)total, stay, posm[cur], vel[cur], acc[cur]);
        NB_HIP_TRY(hipGetLastError());
        set_active(stay + (uint32_t)total);
        let_arrivals_pending = false;
        return NB_OK;
    }

    // the number of bodies this simulator currently holds (<= the capacity it was created with)
    void set_active(uint32_t count) {
        n = count;
        hi = count;
        lo = 0;
        params.particle_num = count;
        const size_t nn = n ? n : 1;  // (the tile size stays the one the buffers were sized for)
        sort_blocks = (uint32_t)((nn + kSortThreads * sort_items - 1) / (kSortThreads * sort_items));
    }

    // Imports of this step arrive in region 3 as (world - 1) segments of `stride` records, in rank
    // order with this rank skipped; how many records of a segment are real is taken on the device
    // from the all-gathered counts (region 1).  Replaces nb_sim_let_set_imports for this step.
    int let_set_import_stride(uint32_t stride) override {
        if (!let_world || !let_send || stride == 0 || stride > let_cap) {
            set_error("let_set_import_stride: needs the LET buffers and 0 < stride <= tree_let_cap (%u)", let_cap);
            return NB_ERR_INVALID;
        }
        let_import_stride = stride;
        let_imports_set = true;
        return NB_OK;
    }

    int let_set_imports(const uint32_t *counts, int world) override {
        if (!let_world || world != let_world || !counts) {
            set_error("let_set_imports: world %d does not match tree_let_world %d", world, let_world);
            return NB_ERR_INVALID;
        }
        uint64_t run = 0;
        let_segs.world = (uint32_t)world;
        for (int r = 0; r < world; ++r) {
            let_segs.off[r] = (uint32_t)run;
            run += (r == let_rank) ? 0u : counts[r];
            if (counts[r] > let_cap) {
                set_error("let_set_imports: %u records from rank %d exceed the capacity %u", counts[r], r, let_cap);
                return NB_ERR_INVALID;
            }
        }
        let_segs.off[world] = (uint32_t)run;
        let_import_stride = 0;
        let_imports_set = true;
        return NB_OK;
    }

    int let_setup(uint32_t cap) {
        if (let_world < 1 || let_world > kLetMaxWorld || let_rank < 0 || let_rank >= let_world) {
            set_error("LET: world %d / rank %d out of range (at most %d ranks)", let_world, let_rank, kLetMaxWorld);
            return NB_ERR_INVALID;
        }
        if (place.world != 1) {
            set_error("LET: create the TreeSim over the rank's own bodies (placement world 1)");
            return NB_ERR_INVALID;
        }
        if (let_send) {
            set_error("LET buffers are already allocated");
            return NB_ERR_INVALID;
        }
        if (int rc = bind_device()) return rc;
        let_cap = cap;
        const size_t w = (size_t)let_world;
        if (int rc = alloc(&let_metas, sizeof(uint32_t) * kLetMetaWords * w)) return rc;
        if (int rc = alloc(&let_counts, sizeof(uint32_t) * w * w)) return rc;
        if (int rc = alloc(&let_out_slot, sizeof(uint32_t) * w * (size_t)node_cap)) return rc;
        if (int rc = alloc(&let_roots_dev, sizeof(WalkRoots))) return rc;
        if (int rc = alloc(&let_send, sizeof(NodeRec) * w * (size_t)cap)) return rc;
        // the walk addresses own and imported records through one table: own tree first, imports after
        NodeRec *table = nullptr;
        if (int rc = alloc(&table, sizeof(NodeRec) * ((size_t)node_cap + w * (size_t)cap + 4))) return rc;
        rec = table;
        NB_HIP_TRY(hipMemsetAsync(let_metas, 0, sizeof(uint32_t) * kLetMetaWords * w, stream));
        NB_HIP_TRY(hipMemsetAsync(let_counts, 0, sizeof(uint32_t) * w * w, stream));
        NB_HIP_TRY(hipStreamSynchronize(stream));
        let_next = NB_PHASE_LET_META;
        return NB_OK;
    }

    int enqueue_step() {
        if (let_world) {
            set_error("this TreeSim runs the LET protocol: use nb_sim_encode_phase(NB_PHASE_LET_*)");
            return NB_ERR_INVALID;
        }
        // 8c: from kWalkGatherFrom bodies the walk fetches a body's velocity and acceleration through the order
        // itself instead of having cells_c_kernel copy all of them into sorted arrays first (64 B read + 64 B
        // written per body by a kernel that runs at the HBM limit); the new state then lands in the OTHER buffer set
        // (positions in place over the sorted source) and `cur` flips.  Whole one-GPU steps only; not under a captured
        // graph (its arguments would alternate).
        const bool gather = !build_done && place.world == 1 && !use_graph && walk_mode != 0 && walk_gathers != 0 &&
                            (walk_gathers > 1 || n >= kWalkGatherFrom);
        if (!build_done)
            if (int rc = enqueue_build(false, place.world == 1 && !gather)) return rc;
        build_done = false;
        return enqueue_walk(own_root(), 0, 1, nullptr, gather);
    }

    // What the sort of a build does: the counting sort, or `passes` radix passes of W-bit digits over the top `bits`
    // key bits -- on the whole keys or (hi_mode) on their high words -- and a fix-up of the ties.  adapt_sort, the
    // graph drop and both fix-up launches depend on it.
    struct SortPlan {
        bool rank_sort;    // 3c: the whole sort in one launch, by counting
        uint32_t bits;     // high key bits the radix passes sort (63: all)
        uint32_t W;        // digit width
        uint32_t passes;
        uint32_t shift0;   // the passes cover key bits shift0 .. 62
        bool hi_mode;      // 3e: the passes move (high word, index)
        uint32_t hs0;      // ... and where the first digit sits inside the high word
    };
    SortPlan sort_plan() const {
        SortPlan p{};
        p.rank_sort = n <= (uint32_t)rank_sort_max && sort_mode == 1;
        // 3 / 3d: stable radix passes of kSortBits bits -- over all 63 key bits, or (sort_mode 1) only
        // over the top `bits` bits, such that a cell of that level holds 1/64 body on average
        // (2^bits >= 64 N), followed by the fix-up of the runs that tie there.
        // Digits of 8 bits.  (9 where that saves a pass -- 25..27 bits: 262,145 .. 2,097,152 bodies -- is tuning
        // key "tree_sort_wide": measured twice and not faster, a 9-bit scatter costs 17 instead of 13 us at
        // 2^20 bodies and the fix-up sees 30x the runs, which eats the pass saved:
        // profiles/r02_sort_experiments.txt.)
        // How many: with the thread-per-body fix-up of the high-word sort (3e) ties are cheap, so only as many
        // bits as leave about two bodies per cell of the resolved level (2^bits >= N / 2: 16 bits up to 131,072
        // bodies, 24 up to 33 million -- a pass less than the 64-bit form needs, whose wave-per-run fix-up wants
        // 1/64 body per cell: 2^bits >= 64 N).  tree_sort_spare_hi / tree_sort_spare: log2 of cells per body.
        p.bits = 63;
        bool hi_fit = false;
        if (sort_mode == 1) {
            auto bits_for = [&](int spare) {
                uint32_t b = 8u;
                while (b < 63u && std::ldexp(1.0, (int)b) < std::ldexp((double)n, spare)) ++b;
                return b;
            };
            // a step whose fix-up met a long run (a dense core in a cube stretched by escapers) makes the next
            // steps sort more high digits (wait(): sort_boost), until the probe says they can go again
            const uint32_t boost = p.rank_sort ? 0u : kSortBits * sort_boost;
            const uint32_t fixed = (uint32_t)sort_bits;  // tree_sort_bits, 0: by the spare keys
            const uint32_t bits_hi = (fixed ? fixed : std::max(16u, bits_for(sort_spare_hi))) + boost;
            hi_fit = sort_hi && !p.rank_sort && !sort_wide && bits_hi <= 31u;
            p.bits = hi_fit ? bits_hi : std::min(63u, (fixed ? fixed : std::max(21u, bits_for(sort_spare))) + boost);
        }
        p.W = (p.bits + kSortWideBits - 1u) / kSortWideBits < (p.bits + kSortBits - 1u) / kSortBits && sort_wide
                  ? kSortWideBits : kSortBits;
        p.passes = (p.bits + p.W - 1u) / p.W;
        p.shift0 = 63u > p.passes * p.W ? 63u - p.passes * p.W : 0u;
        // 3e: up to 31 sorted bits all lie in the keys' HIGH WORDS, so the passes move (high word, index) --
        // 8-byte instead of 12-byte elements, and no identity index array to begin with -- the fix-up looks a
        // tied body's full key up through its index, and the sorted 64-bit keys are gathered once, by
        // cells_a_kernel beside the positions.  hs0: where the first digit sits inside the high word (three
        // passes: bits 7..30, the same 24 key bits as without; four: the whole word, key bits 32..62).
        p.hi_mode = hi_fit && p.W == kSortBits && p.passes <= 4u;
        p.hs0 = 31u > kSortBits * p.passes ? 31u - kSortBits * p.passes : 0u;
        return p;
    }

    // one stable radix pass on digit `shift` of W bits: (kin, vin) -> (kout, vout).  The first pass finds its tile
    // histograms written by morton_kernel; vin == nullptr: the values are the bodies' own indices.
    template <uint32_t W, uint32_t ITEMS, typename KeyT>
    void launch_radix_pass(bool first, const KeyT *kin, const uint32_t *vin, KeyT *kout, uint32_t *vout,
                           uint32_t shift) {
        constexpr uint32_t TH = 2u * kSortThreads;          // scatter's threads
        constexpr uint32_t IT = kSortThreads * ITEMS / TH;  // ... and items
        const dim3 grid(sort_blocks), block(TH);
        if (!first)
            hipLaunchKernelGGL((radix_hist_kernel<IT, KeyT>), grid, block, 0, stream, kin, n, shift, 1u << W, hist,
                               sort_blocks);
        if (sort_blocks <= kSortInlineScanBlocks) {
            hipLaunchKernelGGL((radix_scatter_kernel<(int)W, TH, IT, true, KeyT>), grid, block, 0, stream, kin, vin, kout,
                               vout, n, shift, hist, totals, sort_blocks);
        } else {
            hipLaunchKernelGGL(bin_scan_kernel, dim3(1u << W), dim3(256), 0, stream, hist, sort_blocks, totals);
            hipLaunchKernelGGL((radix_scatter_kernel<(int)W, TH, IT, false, KeyT>), grid, block, 0, stream, kin, vin, kout,
                               vout, n, shift, hist, totals, sort_blocks);
        }
    }
    // ... for a digit width chosen at run time and this simulator's tile size
    template <typename KeyT>
    void radix_pass(uint32_t W, bool first, const KeyT *kin, const uint32_t *vin, KeyT *kout, uint32_t *vout,
                    uint32_t shift) {
        const bool small = sort_items == kSortItemsSmall;
        if constexpr (sizeof(KeyT) == 8) {  // (9-bit digits: whole keys only)
            if (W == kSortWideBits) {
                if (small) launch_radix_pass<kSortWideBits, kSortItemsSmall, KeyT>(first, kin, vin, kout, vout, shift);
                else launch_radix_pass<kSortWideBits, kSortItems, KeyT>(first, kin, vin, kout, vout, shift);
                return;
            }
        }
        if (small) launch_radix_pass<kSortBits, kSortItemsSmall, KeyT>(first, kin, vin, kout, vout, shift);
        else launch_radix_pass<kSortBits, kSortItems, KeyT>(first, kin, vin, kout, vout, shift);
    }

    // the fix-up launch that is about to be enqueued: where its run statistics go, and what adapt_sort reads them as
    // (its parity: the launch fills the words of that parity and clears the other's)
    uint32_t next_run_stats(bool hi_mode) {
        run_stat_seq = build_seq;
        run_stat_boost = sort_boost;
        run_stat_hi = hi_mode;
        return build_seq++ & 1u;
    }

    // fill_kernel in one of its forms: for the walk (rec), or (AOS) the reference's Octant fields, from the arrays of
    // the last build
    template <typename Kernel>
    void launch_fill(Kernel kernel, uint32_t grid, const float4 *sorted_posm) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, sorted_keys, n, node_cap, scalars + kScNodes,
                           node_first, node_depth, cpl, int_slot, leaf_id, int_id, order, sorted_posm, mom_prefix,
                           scalars + kScDepthBase, scalars + kScBound, cogm, bodies, child, rec, inv_theta2(),
                           scalars + kScRowTotal);
    }

    // external_bound: the root cube is already in scalars[kScBound] (LET: the max over all ranks)
    // with_va: also reorder velocities and accelerations (they are complete: not a sharded host
    // that still gathers them while the tree is built)
    int enqueue_build(bool external_bound, bool with_va = false) {
        const int s = cur, d = cur ^ 1;
        uint32_t *bound_bits = scalars + kScBound, *n_nodes = scalars + kScNodes, *status = scalars + kScStatus;
        uint32_t *depth_base = scalars + kScDepthBase, *row_total = scalars + kScRowTotal;
        uint32_t *bound_slots = bound_buf;    // kBoundSlots words: the next bound, from the walk
        const dim3 b256(256);
        const uint32_t g256 = (n + 255) / 256;
        // 1-2: bound + keys from the step's source positions (old positions, tree.rs:290-295)
        const uint32_t *bound_src = bound_bits;
        uint32_t n_src = 1;
        if (!external_bound) {
            if (bound_from_walk) {  // the previous step's walk has already taken max |coord| of this state
                bound_src = bound_slots;
                n_src = kBoundSlots;
            } else {
                NB_HIP_TRY(hipMemsetAsync(scalars, 0, sizeof(uint32_t) * kScStatus, stream));  // status words are sticky
                hipLaunchKernelGGL(bound_kernel, dim3(std::min<uint32_t>(g256, 512)), b256, 0, stream, posm[s], n,
                                   bound_bits);
            }
        }
        bound_from_walk = false;
        const SortPlan sp = sort_plan();
        uint32_t *khi[2] = {reinterpret_cast<uint32_t *>(keys[1]), reinterpret_cast<uint32_t *>(keys[1]) + n};
        if (sp.rank_sort)
            hipLaunchKernelGGL(morton_kernel, dim3((n + kSortThreads - 1) / kSortThreads), dim3(kSortThreads), 0, stream,
                               posm[s], n, bound_src, n_src, bound_bits, keys[0], idx[0], (uint32_t *)nullptr, 0u, 1u,
                               0u, 1u, (uint32_t *)nullptr, key_descent);
        else  // (with the tile histograms of the first pass's digit)
            // (512 threads x half the sort's items per thread: the same tile, twice the waves per SIMD for the
            // 21 dependent levels of the key descent)
            hipLaunchKernelGGL(morton_kernel, dim3(sort_blocks), dim3(2 * kSortThreads), 0, stream, posm[s], n, bound_src,
                               n_src, bound_bits, keys[0], idx[0], hist, sort_blocks, sort_items / 2u,
                               sp.hi_mode ? 32u + sp.hs0 : sp.shift0, 1u << sp.W,
                               sp.hi_mode ? khi[0] : (uint32_t *)nullptr, key_descent);
        int kb = 0;
        if (sp.rank_sort) {
            // 3c: the sorted position of every body counted in one launch
            hipLaunchKernelGGL(rank_sort_kernel, dim3((n + 63u) / 64u), dim3(64 * kRankWaves), 0, stream, keys[0], n,
                               keys[1], idx[1]);
            kb = 1;
        } else if (sp.hi_mode) {
            for (uint32_t ps = 0; ps < sp.passes; ++ps, kb ^= 1)
                radix_pass<uint32_t>(kSortBits, ps == 0u, khi[kb], ps == 0u ? nullptr : idx[kb], khi[kb ^ 1], idx[kb ^ 1],
                                     sp.hs0 + ps * kSortBits);
            // the ties: on the sorted high words, full keys through the indices; every body finds its place
            // and the order comes out in the other index array
            // (scratch for a long run's keys: the moment prefixes, which cells_c_kernel writes later)
            uint64_t *scratch = reinterpret_cast<uint64_t *>(mom_prefix);
            const uint32_t par = next_run_stats(true);
            hipLaunchKernelGGL(runs_rank_kernel, dim3((n + 256u * kRankItems - 1u) / (256u * kRankItems)), b256, 0, stream,
                               khi[kb], keys[0], idx[kb], idx[kb ^ 1], scratch, scratch + n, n, 32u + sp.hs0,
                               sort_boost ? std::min(62u, 32u + sp.hs0 + kSortBits) : 0u, scalars + kScRunStat + par,
                               scalars + kScRunStat + (par ^ 1u));
            kb ^= 1;
        } else {
            for (uint32_t ps = 0; ps < sp.passes; ++ps, kb ^= 1)
                radix_pass<uint64_t>(sp.W, ps == 0u, keys[kb], idx[kb], keys[kb ^ 1], idx[kb ^ 1], sp.shift0 + ps * sp.W);
            if (sp.shift0 || sort_boost) {  // (all 63 bits sorted: nothing to fix, but the probe still has to run)
                const uint32_t par = next_run_stats(false);
                hipLaunchKernelGGL(runs_fix_kernel, dim3((n + 256u * kRunItems - 1u) / (256u * kRunItems)), b256,
                                   0, stream, keys[kb], idx[kb], keys[kb ^ 1], idx[kb ^ 1], n, sp.shift0,
                                   sort_boost ? std::min(62u, sp.shift0 + sp.W) : 0u, scalars + kScRunStat + par,
                               scalars + kScRunStat + (par ^ 1u));
            }
        }
        // (hi_mode: cells_a_kernel gathers the sorted keys into the buffer the high words lived in)
        uint64_t *skeys = sp.hi_mode ? keys[1] : keys[kb];
        order = idx[kb];
        sorted_keys = skeys;
        // 4-6a: the step's source permuted into DFS/Morton order (tree.rs:297,315-325), cells from
        // key prefixes, node ids, moment prefixes: A, B, C of section 5b
        // 256-body rounds per workgroup: small problems are bound by the chain of barriers inside a
        // workgroup (1 round), large ones by the length of the one-workgroup scan over the tiles (4)
        uint32_t rounds = n <= 131072u ? 1u : n <= 524288u ? 2u : kCellTile / 256u;
        if (cell_rounds && ((size_t)n + 256 * cell_rounds) / (256 * cell_rounds) + 1 <= cell_tiles) rounds = cell_rounds;
        const uint32_t ct = (uint32_t)(((size_t)n + 1 + 256 * rounds - 1) / (256 * rounds));  // covers prefix[n] too
        const uint32_t cstride = (ct + 3u) & ~3u;  // rows of the tile table, padded to 16 bytes
        hipLaunchKernelGGL(sp.hi_mode ? cells_a_kernel<true> : cells_a_kernel<false>, dim3(ct), b256, 0, stream, order, n,
                           posm[s], posm[d], sp.hi_mode ? keys[0] : skeys, sp.hi_mode ? skeys : (uint64_t *)nullptr, cpl,
                           tile_u32, tile_mom, cstride, rounds, status);
        const bool scan_inline = ct <= (cell_scan_inline > 1 ? 256u : kCellInlineTiles) && cell_scan_inline;
        if (!scan_inline)
            hipLaunchKernelGGL(cells_scan_kernel, dim3(kCellRows + 4), dim3(1024), 0, stream, tile_u32, tile_mom, ct, cstride,
                               row_total, bound_slots);
        const auto cells_c = scan_inline ? cells_c_kernel<true> : cells_c_kernel<false>;
        hipLaunchKernelGGL(cells_c, dim3(ct), b256, 0, stream, cpl, n, tile_u32, tile_mom, cstride, row_total, depth_base,
                           n_nodes, status, posm[d], int_slot, leaf_id, int_id, node_first, node_depth, mom_prefix, node_cap,
                           rounds, order, with_va ? vel[s] : (const float4 *)nullptr, acc[s], vel[d], acc[d], rec,
                           bound_slots);
        va_gathered = with_va;
        // 6: node contents
        const uint32_t gnodes = (std::min<uint64_t>(node_cap, 3ull * (n / 4u) + 256ull) + 255) / 256;  // internal cells
        launch_fill(n <= kFillEagerMax         ? fill_kernel<false, true>
                    : n >= kFillEagerAgainFrom ? fill_kernel<false, true, false>
                                               : fill_kernel<false, false>,
                    gnodes, posm[d]);
        NB_HIP_TRY(hipGetLastError());
        return NB_OK;
    }

    // the instantiation of a walk kernel for a run-time choice; exactly these are compiled: the per-thread walk
    // for COUNT x PART in {0, 1, 2} ...
    template <bool COUNT>
    static auto walk_for(int part) {
        return part == 0 ? walk_kernel<COUNT, 0> : part == 1 ? walk_kernel<COUNT, 1> : walk_kernel<COUNT, 2>;
    }
    // ... and the cells walk for G in {4, 8, 16} x COUNT x PART, PACKED only for G <= 8
    template <int G, bool COUNT, bool PACKED>
    static auto walk_cells_for(int part) {
        return part == 0   ? walk_cells_kernel<G, COUNT, 0, PACKED>
               : part == 1 ? walk_cells_kernel<G, COUNT, 1, PACKED>
                           : walk_cells_kernel<G, COUNT, 2, PACKED>;
    }
    template <bool COUNT>
    static auto walk_cells_for(uint32_t gsize, int part, bool packed) {
        if (gsize == 16u) return walk_cells_for<16, COUNT, false>(part);
        if (gsize == 4u) return packed ? walk_cells_for<4, COUNT, true>(part) : walk_cells_for<4, COUNT, false>(part);
        return packed ? walk_cells_for<8, COUNT, true>(part) : walk_cells_for<8, COUNT, false>(part);
    }

    // part: 0 whole step, 1 own-tree sums only, 2 continue from those sums and integrate
    int enqueue_walk(const WalkRoots &roots, int part = 0, uint32_t split = 1,
                     const WalkRoots *roots_dev = nullptr, bool gather = false) {
        const int s = cur, d = cur ^ 1;
        uint32_t *status = scalars + kScStatus;
        const dim3 b256(256);
        if (part != 2 && !va_gathered && !gather)
            hipLaunchKernelGGL(gather_va_kernel, dim3((n + 255) / 256), b256, 0, stream, order, n, vel[s], acc[s],
                               vel[d], acc[d]);
        va_gathered = false;
        // 8: walk + integrate: sorted source (now in buffer d) -> buffer s.  A walk over the whole state in
        // one launch also leaves max |coord| of the new positions for the next step's root cube.
        const bool whole = part == 0 && !let_world && place.world == 1 && lo == 0 && hi == n;
        uint32_t *bslots = whole ? bound_buf : nullptr;
        if (time_walk) NB_HIP_TRY(hipEventRecord(time_walk[0], stream));
        if (hi > lo && walk_mode == 0) {
            // bodies per wave: 64 when that still gives >= 4096 waves (4 per SIMD), else halve down to 8
            uint32_t shift = 6;
            if (walk_bpw) {
                shift = walk_bpw >= 64 ? 6 : walk_bpw >= 32 ? 5 : walk_bpw >= 16 ? 4 : 3;
            } else {
                while (shift > 3 && ((hi - lo) >> shift) < 4096u) --shift;
            }
            const uint32_t per_block = 4u << shift;
            const dim3 gwalk((hi - lo + per_block - 1) / per_block);
            const auto walk = count_visits ? walk_for<true>(part) : walk_for<false>(part);
            hipLaunchKernelGGL(walk, gwalk, b256, 0, stream, posm[d], vel[d], acc[d], rec, roots, posm[s], vel[s], acc[s],
                               lo, hi, shift, params.g, params.e, params.dt, status, counters, bslots, roots_dev);
        } else if (hi > lo) {
            // cells across the lanes (section 8b): a wave walks for a group of G bodies
            // bodies per wave: 8; 4 on small problems (below 24,576 bodies: twice the waves for the SIMDs a small
            // walk leaves idle, -5 .. -17 % of the walk at 8,192 and 16,384 bodies); 16 where a wide acceptance test
            // (theta >= 0.9) meets many bodies (from 393,216: -2 .. -3 %).  Measured after the walk stopped reading
            // the bound slots in its prologue -- until then a wave's start cost a trip to one hot cache line, and 16
            // bodies per wave, half the trips, "won" the middle sizes by up to 25 %:
            // profiles/r03_walk_experiments.txt section 4.
            // (by the tree's size, not by the range walked: the ranks of a replicated build add the same terms in
            // the same order as the one-GPU step -- bit for bit its result)
            const uint32_t gauto = n < 24576u ? 4u : (theta >= 0.9f && n >= 393216u) ? 16u : 8u;
            const uint32_t gsize = walk_group ? walk_group : gauto;
            const uint32_t per_block = kCellBlockWaves * gsize;
            const dim3 gwalk((hi - lo + per_block - 1) / per_block), bwalk(64 * kCellBlockWaves);
            // one-word stack entries when the group has 8 mask bits and every id is below 2^24
            const uint64_t id_limit = (uint64_t)node_cap + (let_world ? (uint64_t)let_world * let_cap : 0ull);
            const bool packed = walk_packed != 0 && gsize <= 8u && id_limit <= (1ull << kPackedIdBits);
            // (gather: sorted positions in buffer d, velocities / accelerations in source order in buffer s; the new
            // state -> buffer d)
            const float4 *w_vel = gather ? vel[s] : vel[d], *w_acc = gather ? acc[s] : acc[d];
            float4 *w_posm_dst = gather ? posm[d] : posm[s], *w_vel_dst = gather ? vel[d] : vel[s],
                   *w_acc_dst = gather ? acc[d] : acc[s];
            const uint32_t *w_order = gather ? order : nullptr;
            const auto walk = count_visits ? walk_cells_for<true>(gsize, part, packed)
                                           : walk_cells_for<false>(gsize, part, packed);
            hipLaunchKernelGGL(walk, gwalk, bwalk, 0, stream, posm[d], w_vel, w_acc, rec, roots, split, w_posm_dst, w_vel_dst,
                               w_acc_dst, lo, hi, params.g, params.e, params.dt, status, counters, bslots, roots_dev,
                               w_order);
        }
        if (time_walk) NB_HIP_TRY(hipEventRecord(time_walk[1], stream));
        NB_HIP_TRY(hipGetLastError());
        bound_from_walk = whole && hi > lo;
        // the post-step state is in buffer s (= cur); buffer d holds the sorted source
        // (gather: the post-step state is in buffer d, which becomes cur; s keeps the unsorted source)
        if (gather && hi > lo && walk_mode != 0) cur = d;
        return NB_OK;
    }

    int read_particles(nb_particle *dst, size_t count) override {
        if (count > n) {
            set_error("read_particles: asked for %zu of %u particles", count, n);
            return NB_ERR_INVALID;
        }
        if (int rc = bind_device()) return rc;
        if (count == 0) return wait();
        NB_HIP_TRY(launch_soa_to_aos(posm[cur], vel[cur], acc[cur], d_aos, n, 0, n, stream));
        NB_HIP_TRY(hipMemcpyAsync(dst, d_aos, sizeof(nb_particle) * count, hipMemcpyDeviceToHost, stream));
        NB_HIP_TRY(hipStreamSynchronize(stream));
        return check_status();
    }

    // the state read_particles converts: buffer set `cur` (which flips when the walk gathers)
    void diag_state(const float4 **posm_out, const float4 **vel_out) const override {
        *posm_out = posm[cur];
        *vel_out = vel[cur];
    }
    int diag_status() override { return check_status(); }

    // device.poll(Wait) (offline_headless.rs:43) + the device status words: a step that overflowed
    // the 4N node buffer, cut a LET export short, met inseparable bodies or tripped the walk's
    // stack guard must not look like a good step to a caller that never reads particles back
    // (nb_runner_step, the headless CLI, timing loops).  The words ride the same stream: one
    // 48-byte copy into pinned memory ahead of the one synchronisation -- the four status words and the
    // fix-ups' run statistics (runs_fix_kernel, runs_rank_kernel), which steer how many high digits the next
    // builds sort.
    int wait() override {
        if (int rc = bind_device()) return rc;
        if (!h_status || !scalars) return SimBase::wait();
        NB_HIP_TRY(hipMemcpyAsync(h_status, scalars + kScStatus, sizeof(uint32_t) * kMirrorWords, hipMemcpyDeviceToHost,
                                  stream));
        NB_HIP_TRY(hipStreamSynchronize(stream));
        adapt_sort(h_status + (kScRunStat - kScStatus));
        return report_status(h_status);
    }

    // st: {longest run; probe; bodies in long runs} x {parity 0, parity 1} of the last two fix-ups.
    // Speed only -- the sort's result does not depend on it -- so it does not matter which step's
    // statistics a given wait() happens to see.
    void adapt_sort(const uint32_t *st) {
        if (run_stat_seq == ~0u || run_stat_seq == run_stat_seen) return;  // no fix-up since the last look
        run_stat_seen = run_stat_seq;
        const uint32_t par = run_stat_seq & 1u, longest = st[kRunLongest + par], probe = st[kRunProbe + par],
                       slow = st[kRunSlow + par];
        const uint32_t before = sort_boost;
        // one more digit: a run that is radix-sorted by one workgroup, or (high-word sort: every run of 64 or
        // more takes a workgroup's turn) more than 1/64 of the bodies in such runs -- a disc, a dense core
        if (longest > kRunBoostAbove || slow > n / 64u) {
            sort_boost = std::min(kSortBoostMax, run_stat_boost + (longest > 256u * kRunBoostAbove ? 2u : 1u));
        } else if (run_stat_boost != 0u && sort_boost == run_stat_boost &&
                   (run_stat_hi ? probe <= n / 256u : probe == 0u)) {
            sort_boost = run_stat_boost - 1u;  // with one digit less the runs would still be short
        }
        if (sort_boost != before) drop_graph();  // the captured launch sequence has the old number of passes
    }

    int check_status() {
        uint32_t st[kStatusWords] = {};
        NB_HIP_TRY(hipMemcpy(st, scalars + kScStatus, sizeof st, hipMemcpyDeviceToHost));
        return report_status(st);
    }

    int report_status(const uint32_t *st) {
        if (st[kStLetExport] & kLetListOverflow) {
            set_error("LET export: a tree level inside one grandchild of the root is wider than the one-launch export's "
                      "list (%u ranges of up to %u cells: a heavily clustered rank); the segments had room -- set "
                      "tree_let_export_mode 0 (one launch per tree level) for this simulator",
                      kLetExportRanges, kLetExportThreads);
            return NB_ERR_UNSUPPORTED;
        }
        if (st[kStLetExport]) {
            set_error("LET export needs more than tree_let_cap = %u records for a peer (%u cells cut short)",
                      let_cap, st[kStLetExport]);
            return NB_ERR_UNSUPPORTED;
        }
        if (st[kStWalkStack]) {
            set_error("tree walk hit its stack guard %u times (more than %u pending groups per wave: "
                      "inconsistent tree)", st[kStWalkStack], kWalkStack - 8);
            return NB_ERR_UNSUPPORTED;
        }
        if (st[kStNodeOverflow]) {
            set_error("octree needs more than %u nodes (4N, the reference's capacity, tree.rs:188-190)",
                      node_cap);
            return NB_ERR_UNSUPPORTED;
        }
        if (st[kStKeyTies]) {
            set_error("%u bodies share their 63-bit Morton key with a neighbour (closer than root_width / 2^21): "
                      "the octree cannot separate them (the reference's build_tree, tree.rs:473-544, never "
                      "terminates on such input)", st[kStKeyTies]);
            return NB_ERR_UNSUPPORTED;
        }
        return NB_OK;
    }

    int read_tree(nb_octant *dst, size_t cap, size_t *n_nodes_out, float *root_width) override {
        if (int rc = bind_device()) return rc;
        NB_HIP_TRY(hipStreamSynchronize(stream));
        uint32_t sc[kScNodes + 1] = {};
        NB_HIP_TRY(hipMemcpy(sc, scalars, sizeof sc, hipMemcpyDeviceToHost));
        if (step_num == 0 || n == 0) {
            if (n_nodes_out) *n_nodes_out = 0;
            if (root_width) *root_width = 2.0f;  // TreeSimParams initial root_width, tree.rs:50
            return NB_OK;
        }
        const uint32_t nodes = std::min(sc[kScNodes], node_cap);
        float b;
        std::memcpy(&b, &sc[kScBound], 4);
        if (root_width) *root_width = b * 2.0f;
        if (n_nodes_out) *n_nodes_out = nodes;
        const size_t m = std::min<size_t>(nodes, cap);
        if (m && dst) {
            if (!d_tree_aos) {  // first read-back: the reference's Octant fields, 104 B per node
                if (int rc = alloc(&cogm, sizeof(float4) * (size_t)node_cap)) return rc;
                if (int rc = alloc(&bodies, sizeof(uint32_t) * (size_t)node_cap)) return rc;
                if (int rc = alloc(&child, sizeof(uint32_t) * 8 * (size_t)node_cap)) return rc;
                if (int rc = alloc(&d_tree_aos, sizeof(nb_octant) * (size_t)node_cap)) return rc;
            }
            // the Octant fields are produced on demand from the step's build arrays, which stay
            // intact until the next step (buffer cur^1 holds the sorted source the tree was built on)
            launch_fill(fill_kernel<true, false>, (node_cap + 255) / 256, posm[cur ^ 1]);
            hipLaunchKernelGGL(tree_to_aos_kernel, dim3((nodes + 255) / 256), dim3(256), 0, stream, cogm,
                               bodies, child, nodes, d_tree_aos);
            NB_HIP_TRY(hipMemcpyAsync(dst, d_tree_aos, sizeof(nb_octant) * m, hipMemcpyDeviceToHost, stream));
            NB_HIP_TRY(hipStreamSynchronize(stream));
        }
        return check_status();
    }

    int encode_n_timed(int count, float *ms_total, float *ms_kernel) override {
        if (count <= 0) {
            set_error("encode_n_timed: n must be positive");
            return NB_ERR_INVALID;
        }
        if (int rc = bind_device()) return rc;
        while (events.size() < (size_t)(2 * count + 2)) {
            hipEvent_t ev;
            NB_HIP_TRY(hipEventCreate(&ev));
            events.push_back(ev);
        }
        NB_HIP_TRY(hipEventRecord(events[0], stream));
        for (int k = 0; k < count; ++k) {
            time_walk = &events[2 + 2 * k];  // brackets the walk kernel inside encode()
            const int rc = encode();
            time_walk = nullptr;
            if (rc) return rc;
        }
        NB_HIP_TRY(hipEventRecord(events[1], stream));
        NB_HIP_TRY(hipStreamSynchronize(stream));
        float total = 0.f, walk_sum = 0.f;
        NB_HIP_TRY(hipEventElapsedTime(&total, events[0], events[1]));
        for (int k = 0; k < count; ++k) {
            float ms = 0.f;
            NB_HIP_TRY(hipEventElapsedTime(&ms, events[2 + 2 * k], events[3 + 2 * k]));
            walk_sum += ms;
        }
        if (ms_total) *ms_total = total;
        if (ms_kernel) *ms_kernel = walk_sum / (float)count;  // the dominant kernel: the walk
        return check_status();  // a degraded step must not be reported as a timing
    }

    // Sharded TreeSim = replicated tree, partitioned walk: after encode the
    // rank's range of the three state arrays is new; the caller all-gathers each in place.
    // In LET mode the regions are the protocol's four buffers: 0 meta words (all-gather, 32 B per
    // rank), 1 export counts (all-gather, one row of `world` u32 per rank), 2 the export segments
    // (segment q = records for peer q, stride = slice_bytes), 3 the import area (packed by the
    // caller in rank order, skipping itself).
    int exchange_count() override {
        return let_world ? (let_mig_send ? kLetRegionsWithMigration : kLetRegions) : kReplicatedRegions;
    }
    int exchange_region(int index, void **dev_ptr, size_t *off, size_t *len, size_t *total) override {
        if (let_world) {
            if (index < 0 || index >= exchange_count() || !let_send) {
                set_error("LET exchange region %d out of range (4 regions after tree_let_cap is set, 7 with "
                          "nb_sim_let_set_owners)", index);
                return NB_ERR_INVALID;
            }
            const size_t w = (size_t)let_world;
            void *base = nullptr;
            size_t o = 0, l = 0, t = 0;
            switch (index) {
            case kLetMeta: base = let_metas; l = sizeof(uint32_t) * kLetMetaWords; o = l * let_rank; t = l * w; break;
            case kLetExportCounts: base = let_counts; l = sizeof(uint32_t) * w; o = l * let_rank; t = l * w; break;
            case kLetExportSegments: base = let_send; l = sizeof(NodeRec) * (size_t)let_cap; t = l * w; break;
            case kLetImportArea: base = rec + node_cap; l = sizeof(NodeRec) * (size_t)let_cap; t = l * w; break;
            // migration: 4 counts (all-gather, `world` u32 per rank, stayers at [rank]), 5 leavers per
            // owner (48 B per body, segment stride = slice_bytes), 6 arrivals (packed in rank order)
            case kLetMigrationCounts: base = let_mig_counts; l = sizeof(uint32_t) * w; o = l * let_rank; t = l * w; break;
            case kLetLeavers: base = let_mig_send; l = kMigratedBodyBytes * (size_t)let_mig_cap; t = l * w; break;
            default: base = let_mig_recv; l = kMigratedBodyBytes * (size_t)let_mig_cap; t = l * w; break;  // kLetArrivals
            }
            if (dev_ptr) *dev_ptr = base;
            if (off) *off = o;
            if (len) *len = l;
            if (total) *total = t;
            return NB_OK;
        }
        if (index < 0 || index >= kReplicatedRegions) {
            set_error("exchange region %d out of range (TreeSim has 3)", index);
            return NB_ERR_INVALID;
        }
        float4 *base = index == kRegionPositions ? posm[cur] : index == kRegionVelocities ? vel[cur] : acc[cur];
        if (dev_ptr) *dev_ptr = base;
        if (off) *off = sizeof(float4) * (size_t)per_rank * (size_t)place.rank;
        if (len) *len = sizeof(float4) * (size_t)per_rank;
        if (total) *total = sizeof(float4) * (size_t)n_pad;
        return NB_OK;
    }

    int push_exchange(void *const *peer_bases, int npeers) override {
        if (let_world || npeers < 0 || npeers > kMaxPeers) {
            set_error("push_exchange: replicated-tree placements only, at most %d peers", kMaxPeers);
            return NB_ERR_INVALID;
        }
        const uint32_t first = per_rank * (uint32_t)place.rank;
        const uint32_t count = first < n ? std::min(per_rank, n - first) : 0u;
        if (npeers == 0 || count == 0u) return NB_OK;
        if (int rc = bind_device()) return rc;
        PushDst dst;
        dst.n = (uint32_t)npeers;
        for (int q = 0; q < npeers; ++q)
            for (int k = 0; k < 3; ++k) dst.p[k][q] = static_cast<float4 *>(peer_bases[q * 3 + k]);
        hipLaunchKernelGGL(push_slices_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, posm[cur], vel[cur],
                           acc[cur], dst, first, count);
        NB_HIP_TRY(hipGetLastError());
        return NB_OK;
    }

    int push_region(int k, void *const *peer_bases, int npeers) override {
        void *base = nullptr;
        size_t off = 0, len = 0, total = 0;
        if (int rc = exchange_region(k, &base, &off, &len, &total)) return rc;
        if (npeers < 0 || npeers > kMaxPeers || (off & 3u) || (len & 3u) || len > (1u << 20)) {
            set_error("push_region: a small table of 4-byte words and at most %d peers", kMaxPeers);
            return NB_ERR_INVALID;
        }
        if (npeers == 0 || len == 0) return NB_OK;
        if (int rc = bind_device()) return rc;
        PushWords dst;
        dst.n = (uint32_t)npeers;
        for (int q = 0; q < npeers; ++q) dst.p[q] = static_cast<uint32_t *>(peer_bases[q]);
        const uint32_t count = (uint32_t)(len / 4u);
        hipLaunchKernelGGL(push_words_kernel, dim3((count + 63u) / 64u), dim3(64), 0, stream,
                           static_cast<const uint32_t *>(base), dst, (uint32_t)(off / 4u), count);
        NB_HIP_TRY(hipGetLastError());
        return NB_OK;
    }

    int let_push_segments(void *const *import_bases, int world, uint32_t stride) override {
        if (!let_world || world != let_world || !let_send || stride == 0 || stride > let_cap) {
            set_error("let_push_segments: needs the LET buffers, tree_let_world ranks and 0 < stride <= tree_let_cap");
            return NB_ERR_INVALID;
        }
        if (world < 2) return NB_OK;
        if (int rc = bind_device()) return rc;
        LetImportPtrs imp{};
        for (int q = 0; q < world; ++q) imp.p[q] = static_cast<NodeRec *>(import_bases[q]);
        hipLaunchKernelGGL(let_push_segments_kernel, dim3(64, (uint32_t)world), dim3(256), 0, stream, let_send, let_cap,
                           let_counts + (size_t)let_rank * (size_t)let_world, imp, (uint32_t)let_rank, stride);
        NB_HIP_TRY(hipGetLastError());
        return NB_OK;
    }

    // ---- tuning keys (nb_sim_set_tuning) ---------------------------------------------------------------
    // One row per key: the member it sets (whose initialiser, among the data members below, is the default), how
    // the value is normalised, whether a captured graph holds launches that depend on it, and the values accepted.
    enum Norm { kFlag, kFloor0, kRaw };  // != 0 -> 1; negative -> 0; as given
    struct Tunable {
        const char *key;
        int TreeSim::*member;
        Norm norm;
        bool drops_graph = true;
        bool (*accepts)(int) = nullptr;  // nullptr: every value
        const char *accepted = nullptr;  // ... in the error message's words
    };
    int set_tuning(const char *key, int value) override {
        using T = TreeSim;
        static const Tunable rows[] = {
            {"tree_count_visits", &T::count_visits, kFlag},  // a different walk kernel: re-capture
            {"tree_walk_bpw", &T::walk_bpw, kFloor0},        // bodies per wave: 0 = automatic, else 8/16/32/64
            {"tree_walk_mode", &T::walk_mode, kFlag},        // 0: bodies across the lanes, 1: cells across the lanes
            // 1: one-word stack entries where the ids allow it (default), 0: never
            {"tree_walk_packed", &T::walk_packed, kFlag},
            // bodies per wave of mode 1: 0 = automatic, else 4/8/16
            {"tree_walk_group", &T::walk_group, kRaw, true, [](int v) { return v == 0 || v == 4 || v == 8 || v == 16; },
             "0, 4, 8 or 16"},
            // 256-body rounds per workgroup of cells_a / cells_c; 0 = automatic
            {"tree_cell_rounds", &T::cell_rounds, kRaw, true, [](int v) { return v >= 0 && v <= 4; }, "0 .. 4"},
            // 1: radix passes on (high word, index) where <= 31 bits are sorted (default)
            {"tree_sort_hi", &T::sort_hi, kFlag},
            // the high key bits the radix passes sort (0: by tree_sort_spare)
            {"tree_sort_bits", &T::sort_bits, kRaw, true, [](int v) { return v == 0 || (v >= 8 && v <= 63); }, "0 or 8..63"},
            // ... for the high-word sort (default -1: two bodies per cell)
            {"tree_sort_spare_hi", &T::sort_spare_hi, kRaw, true, [](int v) { return v >= -8 && v <= 12; }, "-8..12"},
            // log2 of the cells per body at the level the radix passes resolve
            {"tree_sort_spare", &T::sort_spare, kRaw, true, [](int v) { return v >= 0 && v <= 12; }, "0..12"},
            {"tree_sort_wide", &T::sort_wide, kFlag},  // 1: 9-bit digits where they save a pass, 0: always 8 (default)
            // 1: counting sort (<= 12,288 bodies) / high digits + fix-up; 0: always the full 8-pass radix sort
            {"tree_sort_mode", &T::sort_mode, kFlag},
            // 1: the walk gathers velocities from kWalkGatherFrom bodies (default), 0: cells_c sorts them first at
            // every size, 2: gathers at every size
            {"tree_walk_gathers", &T::walk_gathers, kRaw, false},
            {"tree_key_descent", &T::key_descent, kFlag},  // 1: the keys by the 21-level descent even in a power-of-two cube
            // 1: cells_c sums the tile table itself up to 64 tiles (default) (2: up to the 256 tiles the kernel can do)
            {"tree_cell_scan_inline", &T::cell_scan_inline, kRaw},
            {"tree_rank_sort_max", &T::rank_sort_max, kFloor0},  // the counting sort up to this many bodies (default 12,288)
            {"tree_use_graph", &T::use_graph, kFlag},
            {"tree_let_world", &T::let_world, kRaw, false},
            {"tree_let_rank", &T::let_rank, kRaw, false},
            {"tree_let_export_mode", &T::let_export_mode, kFlag, false},  // 1: the export in one launch, 0: a launch per tree level
            {"tree_let_prune", &T::let_prune, kFlag, false},              // 0: export whole trees (testing: same result)
        };
        for (const Tunable &t : rows) {
            if (std::strcmp(key, t.key) != 0) continue;
            if (t.accepts && !t.accepts(value)) {
                set_error("%s must be %s", t.key, t.accepted);
                return NB_ERR_INVALID;
            }
            this->*t.member = t.norm == kFlag ? (value != 0 ? 1 : 0) : t.norm == kFloor0 ? std::max(value, 0) : value;
            if (t.drops_graph) drop_graph();
            return NB_OK;
        }
        // the keys with side effects
        if (std::strcmp(key, "tree_let_active") == 0) {  // bodies in use; the rest of the capacity is headroom
            if (value < 0 || (uint32_t)value > n_capacity || !let_world) {
                set_error("tree_let_active: %d out of range (capacity %u; LET mode only)", value, n_capacity);
                return NB_ERR_INVALID;
            }
            set_active((uint32_t)value);
            return NB_OK;
        }
        if (std::strcmp(key, "tree_let_cap") == 0) {  // records per peer; allocates the LET buffers
            if (value <= 0) {
                set_error("tree_let_cap must be positive");
                return NB_ERR_INVALID;
            }
            return let_setup((uint32_t)value);
        }
        return SimBase::set_tuning(key, value);
    }

    int debug_buffer(const char *name, void *dst, size_t cap, size_t *bytes) override {
        if (int rc = bind_device()) return rc;
        NB_HIP_TRY(hipStreamSynchronize(stream));
        const void *src = nullptr;
        size_t len = 0;
        const std::string nm(name);
        if (nm == "order") { src = order; len = sizeof(uint32_t) * n; }
        else if (nm == "counters") { src = counters; len = sizeof(unsigned long long) * 16; }
#if defined(NB_DIAG_PHASES) || defined(NB_DIAG_TIMELINE)
        else if (nm == "phases") { src = counters + 16; len = sizeof(unsigned long long) * 4 * ((n + 3) / 4); }  // (8 words per group of 8)
#endif
        else if (nm == "status") { src = scalars + kScStatus; len = sizeof(uint32_t) * kStatusWords; }
        else if (nm == "depth_base") { src = scalars + kScDepthBase; len = sizeof(uint32_t) * (kMaxDepth + 2); }
        else {
            set_error("unknown debug buffer '%s'", name);
            return NB_ERR_INVALID;
        }
        if (bytes) *bytes = len;
        if (!src || !dst) return NB_OK;
        NB_HIP_TRY(hipMemcpy(dst, src, std::min(len, cap), hipMemcpyDeviceToHost));
        return NB_OK;
    }

   private:
    template <typename T>
    int alloc(T **p, size_t bytes) {
        void *q = nullptr;
        NB_HIP_TRY(hipMalloc(&q, bytes ? bytes : 16));
        allocs.push_back(q);
        *p = static_cast<T *>(q);
        return NB_OK;
    }

    float theta = NB_DEFAULT_THETA;
    // what fill_kernel scales a cell's size^2 by (NodeRec::mac2); theta = 0 gives +inf: every cell is opened
    float inv_theta2() const { return 1.0f / (theta * theta); }
    int cur = 0;  // posm/vel/acc[cur] hold the current state
    float4 *posm[2] = {nullptr, nullptr}, *vel[2] = {nullptr, nullptr}, *acc[2] = {nullptr, nullptr};
    uint64_t *keys[2] = {nullptr, nullptr};
    uint32_t *idx[2] = {nullptr, nullptr}, *order = nullptr;
    uint64_t *sorted_keys = nullptr;  // of the last build
    nb_particle *d_aos = nullptr;
    nb_octant *d_tree_aos = nullptr;
    uint32_t *hist = nullptr, *totals = nullptr, *int_slot = nullptr;
    uint32_t *leaf_id = nullptr;
    uint2 *int_id = nullptr;  // per internal-cell slot: {first body | opens-next flag, id | depth << 27}
    uint32_t *node_first = nullptr, *bodies = nullptr, *child = nullptr, *scalars = nullptr;
    uint8_t *node_depth = nullptr;
    int8_t *cpl = nullptr;
    float4 *cogm = nullptr;
    NodeRec *rec = nullptr;  // per node: cogm + {first child id, child count} / leaf {sorted position, 0}
    Moments *mom_prefix = nullptr;
    unsigned long long *counters = nullptr;
    uint32_t node_cap = 0, sort_blocks = 0, sort_items = kSortItems;
    // the tuning keys' members (the rows of set_tuning say what the values mean), with their defaults
    int count_visits = 0, use_graph = 0;
    int walk_mode = 1, walk_bpw = 0, walk_group = 0, walk_packed = 1, walk_gathers = 1;
    int sort_mode = 1, sort_hi = 1, sort_wide = 0, sort_bits = 0, sort_spare = 6, sort_spare_hi = -1;
    int rank_sort_max = kRankSortMax, key_descent = 0;
    int cell_rounds = 0, cell_scan_inline = 1;
    int let_export_mode = 1, let_prune = 1;
    uint32_t *tile_u32 = nullptr;
    bool bound_from_walk = false;  // bound_buf holds max |coord| of the current state
    uint32_t *bound_buf = nullptr;  // kBoundSlots words
    bool va_gathered = false;      // the build has already reordered velocities and accelerations
    Moments *tile_mom = nullptr;
    uint32_t cell_tiles = 0;
    bool build_done = false;  // phase 0 of the next step already enqueued
    // locally essential trees (section 9); let_world == 0: not in use
    int let_world = 0, let_rank = 0, let_next = 0;  // (world and rank: tuning keys too)
    uint32_t let_cap = 0;
    uint32_t *let_metas = nullptr, *let_counts = nullptr, *let_out_slot = nullptr;
    NodeRec *let_send = nullptr;
    LetSegments let_segs{};
    uint32_t let_import_stride = 0;       // != 0: this step's imports are fixed-stride segments
    WalkRoots *let_roots_dev = nullptr;
    bool let_imports_set = false, let_arrivals_pending = false, let_own_walked = false;
    uint32_t n_capacity = 0, let_mig_cap = 0;
    uint32_t *let_mig_counts = nullptr;
    float4 *let_mig_send = nullptr, *let_mig_recv = nullptr;
    LetOwners let_owners{};
    hipGraphExec_t graph_exec = nullptr;
    uint32_t *h_status = nullptr;  // pinned mirror of scalars[kScStatus ..]: kMirrorWords words (wait())
    // extra high digits the radix passes cover (adapt_sort), and the fix-up launch its statistics belong to
    static constexpr uint32_t kSortBoostMax = 6;
    uint32_t sort_boost = 0, build_seq = 0, run_stat_seq = ~0u, run_stat_seen = ~0u, run_stat_boost = 0;
    bool run_stat_hi = false;
    hipEvent_t *time_walk = nullptr;
    std::vector<void *> allocs;
    std::vector<hipEvent_t> events;
};

}  // namespace

SimBase *make_tree_sim() { return new (std::nothrow) TreeSim(); }

}  // namespace nb
