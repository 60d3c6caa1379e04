// nb_simbase.cpp -- the simulator objects behind the nb_sim handle: SimBase and the host side of NaiveSim (the
// reference's `trait Simulator` and its all-pairs implementor; TreeSim's host side is in nb_tree.hip).
//
// Host side only; the kernels live in nb_naive.hip.  Everything the reference does through wgpu (buffers, bind
// groups, command encoders, queue.submit, device.poll) maps to hipMalloc'd SoA buffers, a ping-pong index and
// one hipStream_t.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

static size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// nb_shard_bodies_per_rank / nb_shard_padded_bodies behind the ABI boundary
size_t shard_bodies_per_rank(size_t particle_num, int world) {
    if (world < 1) world = 1;
    const size_t per = (particle_num + (size_t)world - 1) / (size_t)world;
    return round_up(per ? per : 1, kPadTo);
}

size_t shard_padded_bodies(size_t particle_num, int world) {
    if (world < 1) world = 1;
    return shard_bodies_per_rank(particle_num, world) * (size_t)world;
}

// ------------------------------------------------------------------------------------------
// SimBase
// ------------------------------------------------------------------------------------------
SimBase::~SimBase() {
    for (auto &w : work) w.reset();  // in slot order, before the stream (the derived destructor has bound the device)
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

int SimBase::setup_common(const nb_sim_params &p, const nb_add_params &ap, const nb_placement *pl) {
    params = p;
    add = ap;
    nb_placement d{};
    d.device_id = 0;
    d.rank = 0;
    d.world = 1;
    place = pl ? *pl : d;
    if (place.world < 1 || place.rank < 0 || place.rank >= place.world) {
        set_error("invalid placement: rank %d of world %d", place.rank, place.world);
        return NB_ERR_INVALID;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device is visible (hipGetDeviceCount); there is no CPU fallback");
        return NB_ERR_NO_DEVICE;
    }
    if (place.device_id < 0) place.device_id = 0;
    if (place.device_id >= count) {
        set_error("device_id %d out of range (%d devices)", place.device_id, count);
        return NB_ERR_INVALID;
    }
    NB_HIP_TRY(hipSetDevice(place.device_id));
    if (place.stream) {
        stream = static_cast<hipStream_t>(place.stream);
        own_stream = false;
    } else {
        NB_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        own_stream = true;
    }
    n = p.particle_num;
    per_rank = (uint32_t)shard_bodies_per_rank(n, place.world);
    n_pad = (uint32_t)shard_padded_bodies(n, place.world);
    const uint64_t lo64 = (uint64_t)per_rank * (uint64_t)place.rank;
    lo = (uint32_t)(lo64 < n ? lo64 : n);
    const uint64_t hi64 = lo64 + per_rank;
    hi = (uint32_t)(hi64 < n ? hi64 : n);
    return NB_OK;
}

int SimBase::bind_device() const {
    NB_HIP_TRY(hipSetDevice(place.device_id));
    return NB_OK;
}

int SimBase::wait() {
    if (int rc = bind_device()) return rc;
    NB_HIP_TRY(hipStreamSynchronize(stream));
    return NB_OK;
}

// ------------------------------------------------------------------------------------------
// NaiveSim -- src/sims/naive.rs
// ------------------------------------------------------------------------------------------
NaiveSim::~NaiveSim() {
    (void)hipSetDevice(place.device_id);
    if (own_posm) {
        if (posm[0]) (void)hipFree(posm[0]);
        if (posm[1]) (void)hipFree(posm[1]);
    }
    if (vel) (void)hipFree(vel);
    if (acc) (void)hipFree(acc);
    if (d_aos) (void)hipFree(d_aos);
    if (partial) (void)hipFree(partial);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
}

// NaiveSim::new, src/sims/naive.rs:20-145: two particle buffers, both initialised with the
// same particles (:99-111); here: two position/mass buffers + one velocity + one
// acceleration array (a body's v and a are only ever touched by its own thread, so they
// need no ping-pong).
int NaiveSim::init(const nb_particle *host, size_t count) {
    if (count != n) {
        set_error("particle count %zu does not match sim_params.particle_num %u", count, n);
        return NB_ERR_INVALID;
    }
    const size_t posm_bytes = sizeof(float4) * (size_t)n_pad;
    if (place.posm[0] || place.posm[1]) {
        if (!place.posm[0] || !place.posm[1] || place.posm[0] == place.posm[1]) {
            set_error("placement.posm needs two distinct device buffers (or none)");
            return NB_ERR_INVALID;
        }
        posm[0] = static_cast<float4 *>(place.posm[0]);
        posm[1] = static_cast<float4 *>(place.posm[1]);
        own_posm = false;
    } else {
        NB_HIP_TRY(hipMalloc(&posm[0], posm_bytes));
        NB_HIP_TRY(hipMalloc(&posm[1], posm_bytes));
        own_posm = true;
    }
    const size_t local_bytes = sizeof(float4) * (size_t)(per_rank ? per_rank : kPadTo);
    NB_HIP_TRY(hipMalloc(&vel, local_bytes));
    NB_HIP_TRY(hipMalloc(&acc, local_bytes));
    NB_HIP_TRY(hipMalloc(&d_aos, sizeof(nb_particle) * (size_t)(n ? n : 1)));
    NB_HIP_TRY(hipMemsetAsync(posm[0], 0, posm_bytes, stream));
    NB_HIP_TRY(hipMemsetAsync(posm[1], 0, posm_bytes, stream));
    NB_HIP_TRY(hipMemsetAsync(vel, 0, local_bytes, stream));
    NB_HIP_TRY(hipMemsetAsync(acc, 0, local_bytes, stream));
    if (const char *v = getenv("NB_NAIVE_VARIANT")) variant = atoi(v);
    if (const char *v = getenv("NB_NAIVE_JSPLIT")) jsplit = atoi(v);
    if (int rc = ensure_workspace()) return rc;
    return write_particles(host, count);
}

// The j-split path needs room for its partial sums; (re)allocated whenever the plan changes.
int NaiveSim::ensure_workspace() {
    // room for whichever shape needs more slices: the single-launch or the two-phase step
    const NaivePlan p1 = plan_naive(n, lo, hi, variant, jsplit, false);
    const NaivePlan p2 = plan_naive(n, lo, hi, variant, jsplit, place.world > 1);
    NaivePlan p = p1;
    if (p2.two_phase && p2.jsplit > p.jsplit) p.jsplit = p2.jsplit;
    if ((p.jsplit > 1 || p2.two_phase) && p.jsplit > partial_slices) {
        if (int rc = bind_device()) return rc;
        NB_HIP_TRY(hipStreamSynchronize(stream));
        if (partial) NB_HIP_TRY(hipFree(partial));
        partial = nullptr;
        partial_slices = 0;
        NB_HIP_TRY(hipMalloc(&partial, sizeof(float4) * (size_t)p.jsplit * (size_t)per_rank));
        partial_slices = p.jsplit;
    }
    return NB_OK;
}

int NaiveSim::write_particles(const nb_particle *host, size_t count) {
    if (count != n) {
        set_error("write_particles: count %zu != particle_num %u", count, n);
        return NB_ERR_INVALID;
    }
    if (int rc = bind_device()) return rc;
    if (n == 0) return NB_OK;
    local_done = false;  // a first half enqueued for the old state is void
    NB_HIP_TRY(hipMemcpyAsync(d_aos, host, sizeof(nb_particle) * (size_t)n, hipMemcpyHostToDevice,
                              stream));
    NB_HIP_TRY(launch_aos_to_soa(d_aos, posm[cur], vel, acc, n, lo, hi, stream));
    // both buffers start equal, as in naive.rs:99-111
    NB_HIP_TRY(hipMemcpyAsync(posm[cur ^ 1], posm[cur], sizeof(float4) * (size_t)n_pad,
                              hipMemcpyDeviceToDevice, stream));
    NB_HIP_TRY(hipStreamSynchronize(stream));  // `host` may be freed by the caller on return
    return NB_OK;
}

int NaiveSim::launch(int phase) {
    NaiveLaunch a{};
    a.posm_src = posm[cur];
    a.posm_dst = posm[cur ^ 1];
    a.vel = vel;
    a.acc = acc;
    a.n = n;
    a.n_pad = n_pad;
    a.lo = lo;
    a.hi = hi;
    a.g = params.g;
    a.e = params.e;
    a.dt = params.dt;
    a.variant = variant;
    a.jsplit = jsplit;
    a.mass_runs = mass_runs;
    a.partial = partial;
    a.partial_stride = per_rank;
    a.partial_slices = partial_slices;
    a.phase = phase;
    a.peers = peers[cur ^ 1];  // the finish kernel writes the new slice there too
    if (a.peers.n && hi > lo && !(lo == 0 && hi == n)) {  // (a rank that owns no body, or all of them,
                                                           // has nothing its peers wait for)
        const NaivePlan p = plan_naive(n, lo, hi, variant, jsplit, phase != kPhaseAll);
        if (phase == kPhaseAll && p.jsplit <= 1) {
            set_error("a NaiveSim with peers steps in two phases (nb_sim_encode_phase)");
            return NB_ERR_INVALID;
        }
    }
    NB_HIP_TRY(launch_naive_step(a, stream));
    return NB_OK;
}

// NaiveSim::encode, src/sims/naive.rs:147-162: one dispatch, then flip the ping-pong.
int NaiveSim::encode() {
    if (int rc = bind_device()) return rc;
    if (local_done) return encode_phase(1);  // the step's first half is already enqueued
    if (int rc = launch(kPhaseAll)) return rc;
    cur ^= 1;
    step_num += 1;
    return NB_OK;
}

// The step in two halves, for overlapping the multi-GPU exchange with compute:
//   phase 0: partial sums over the rank's OWN j tiles.  They only need this rank's slice of the
//            current positions, so the caller may enqueue phase 0 of step k+1 right after step
//            k, while the all-gather of step k's other slices is still in flight;
//   phase 1: partial sums over all other j tiles (after the all-gather), then the finish
//            kernel (fixed-order sum + integrator) and the ping-pong flip.
int NaiveSim::encode_phase(int phase) {
    if (int rc = bind_device()) return rc;
    const NaivePlan p = plan_naive(n, lo, hi, variant, jsplit, true);
    if (!p.two_phase) {  // nothing to split (single rank, or a rank without bodies)
        if (phase == 0) return NB_OK;
        if (int rc = launch(kPhaseAll)) return rc;
        cur ^= 1;
        step_num += 1;
        return NB_OK;
    }
    if (phase == 0) {
        if (local_done) {
            set_error("encode_phase(0) called twice for one step");
            return NB_ERR_INVALID;
        }
        if (int rc = launch(kPhaseLocal)) return rc;
        local_done = true;
        return NB_OK;
    }
    if (phase != 1) {
        set_error("encode_phase: phase must be 0 or 1");
        return NB_ERR_INVALID;
    }
    if (!local_done)
        if (int rc = launch(kPhaseLocal)) return rc;
    if (int rc = launch(kPhaseRemote)) return rc;
    local_done = false;
    cur ^= 1;
    step_num += 1;
    return NB_OK;
}

int NaiveSim::encode_n_timed(int count, float *ms_total, float *ms_kernel) {
    if (count <= 0) {
        set_error("encode_n_timed: n must be positive");
        return NB_ERR_INVALID;
    }
    if (int rc = bind_device()) return rc;
    while (events.size() < (size_t)(2 * count + 2)) {
        hipEvent_t e;
        NB_HIP_TRY(hipEventCreate(&e));
        events.push_back(e);
    }
    NB_HIP_TRY(hipEventRecord(events[0], stream));
    for (int k = 0; k < count; ++k) {
        NB_HIP_TRY(hipEventRecord(events[2 + 2 * k], stream));
        if (int rc = encode()) return rc;
        NB_HIP_TRY(hipEventRecord(events[3 + 2 * k], stream));
    }
    NB_HIP_TRY(hipEventRecord(events[1], stream));
    NB_HIP_TRY(hipStreamSynchronize(stream));
    float total = 0.f, ksum = 0.f;
    NB_HIP_TRY(hipEventElapsedTime(&total, events[0], events[1]));
    for (int k = 0; k < count; ++k) {
        float ms = 0.f;
        NB_HIP_TRY(hipEventElapsedTime(&ms, events[2 + 2 * k], events[3 + 2 * k]));
        ksum += ms;
    }
    if (ms_total) *ms_total = total;
    if (ms_kernel) *ms_kernel = ksum / (float)count;
    return NB_OK;
}

int NaiveSim::read_particles(nb_particle *dst, size_t count) {
    if (count > n) {
        set_error("read_particles: asked for %zu of %u particles", count, n);
        return NB_ERR_INVALID;
    }
    if (int rc = bind_device()) return rc;
    if (count == 0) return wait();
    NB_HIP_TRY(launch_soa_to_aos(posm[cur], vel, acc, d_aos, n, lo, hi, stream));
    NB_HIP_TRY(hipMemcpyAsync(dst, d_aos, sizeof(nb_particle) * count, hipMemcpyDeviceToHost,
                              stream));
    NB_HIP_TRY(hipStreamSynchronize(stream));
    return NB_OK;
}

int NaiveSim::exchange_region(int index, void **dev_ptr, size_t *off, size_t *len, size_t *total) {
    if (index != 0) {
        set_error("exchange region %d out of range (NaiveSim has 1)", index);
        return NB_ERR_INVALID;
    }
    if (dev_ptr) *dev_ptr = posm[cur];
    if (off) *off = sizeof(float4) * (size_t)per_rank * (size_t)place.rank;
    if (len) *len = sizeof(float4) * (size_t)per_rank;
    if (total) *total = sizeof(float4) * (size_t)n_pad;
    return NB_OK;
}

int NaiveSim::set_peers(float4 *const *peer_buf0, float4 *const *peer_buf1, int count) {
    if (count < 0 || count > kMaxPeers) {
        set_error("at most %d peers", kMaxPeers);
        return NB_ERR_INVALID;
    }
    for (int k = 0; k < count; ++k) {
        peers[0].p[k] = peer_buf0[k];
        peers[1].p[k] = peer_buf1[k];
    }
    peers[0].n = peers[1].n = (uint32_t)count;
    return NB_OK;
}

int NaiveSim::set_tuning(const char *key, int value) {
    if (strcmp(key, "naive_variant") == 0) {
        if (value >= naive_variant_count()) {
            set_error("naive_variant %d out of range (%d variants)", value, naive_variant_count());
            return NB_ERR_INVALID;
        }
        variant = value;
        return ensure_workspace();
    }
    if (strcmp(key, "naive_jsplit") == 0) {
        if (value < 0 || value > 32) {
            set_error("naive_jsplit %d out of range [0, 32]", value);
            return NB_ERR_INVALID;
        }
        jsplit = value;
        return ensure_workspace();
    }
    if (strcmp(key, "naive_mass_runs") == 0) {
        if (value != 0 && value != 1) {
            set_error("naive_mass_runs %d is neither 0 nor 1", value);
            return NB_ERR_INVALID;
        }
        mass_runs = value;
        return NB_OK;
    }
    set_error("unknown tuning key '%s'", key);
    return NB_ERR_INVALID;
}

// add_params == NULL: the all-pairs simulator
nb_add_params add_params_or_default(const nb_add_params *ap) {
    return ap ? *ap : nb_add_params{NB_NAIVE_SIM_PARAMS, 0.f};
}

int make_sim_impl(std::unique_ptr<SimBase> &out, const nb_sim_params *sp, const nb_add_params *ap,
                  const nb_placement *pl, const nb_particle *particles, size_t count) {
    nb_add_params add = add_params_or_default(ap);
    std::unique_ptr<SimBase> impl;
    if (add.kind == NB_NAIVE_SIM_PARAMS) {
        impl.reset(new (std::nothrow) NaiveSim());
    } else if (add.kind == NB_TREE_SIM_PARAMS) {
        impl.reset(make_tree_sim());
        if (!impl) {
            set_error("TreeSim (Barnes-Hut) is not available in this build");
            return NB_ERR_UNSUPPORTED;
        }
        if (!(add.theta > 0.f)) add.theta = NB_DEFAULT_THETA;  // tree.rs:42-51
        if (pl && (pl->posm[0] || pl->posm[1])) {
            set_error("TreeSim owns its buffers (placement.posm must be NULL)");
            return NB_ERR_INVALID;
        }
    } else {
        set_error("unknown add_params.kind %d", add.kind);
        return NB_ERR_INVALID;
    }
    if (!impl) {
        set_error("out of host memory");
        return NB_ERR_ALLOC;
    }
    if (int rc = impl->setup_common(*sp, add, pl)) return rc;
    if (int rc = impl->init(particles, count)) return rc;
    out = std::move(impl);
    return NB_OK;
}

}  // namespace nb
