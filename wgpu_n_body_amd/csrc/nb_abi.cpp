// nb_abi.cpp -- the C ABI of include/nbody.h: simulator objects (the reference's
// `trait Simulator` implementors NaiveSim / TreeSim) and the OfflineHeadless-shaped runner.
//
// Host side only; the kernels live in nb_naive.hip / nb_tree.hip (nb_tree_*.hpp).  Everything the
// reference does through wgpu (buffers, bind groups, command encoders, queue.submit,
// device.poll) maps to hipMalloc'd SoA buffers, a ping-pong index and one hipStream_t.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "nb_common.hpp"
#include "nb_group.hpp"
#include "nb_sim.hpp"

namespace nb {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

static size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// The frame nb_field_rings and the maps share (include/nbody.h): n the unit axis, e1 the coordinate axis
// of the smallest |n_k| made orthogonal to n, e2 = n x e1.
bool axis_frame(const double axis[3], double n[3], double e1[3], double e2[3]) {
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(axis[a])) return false;
    // (an axis whose length over- or underflows has no finite unit vector either)
    const double len = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    for (int a = 0; a < 3; ++a) n[a] = axis[a] / len;
    int s = 0;  // the coordinate axis of the smallest |n_k|, the lowest index on ties
    for (int a = 1; a < 3; ++a)
        if (std::fabs(n[a]) < std::fabs(n[s])) s = a;
    double el = 0.0;
    for (int a = 0; a < 3; ++a) {
        e1[a] = (a == s ? 1.0 : 0.0) - n[s] * n[a];
        el += e1[a] * e1[a];
    }
    el = std::sqrt(el);  // >= sqrt(2/3): |n_s| <= 1/sqrt(3)
    for (int a = 0; a < 3; ++a) e1[a] /= el;
    e2[0] = n[1] * e1[2] - n[2] * e1[1];
    e2[1] = n[2] * e1[0] - n[0] * e1[2];
    e2[2] = n[0] * e1[1] - n[1] * e1[0];
    return true;
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
    per_rank = (uint32_t)nb_shard_bodies_per_rank(n, place.world);
    n_pad = (uint32_t)nb_shard_padded_bodies(n, place.world);
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
static nb_add_params add_params_or_default(const nb_add_params *ap) {
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

static int make_sim(nb_sim **out, const nb_sim_params *sp, const nb_add_params *ap,
                    const nb_placement *pl, const nb_particle *particles, size_t count) {
    if (!out || !sp) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<SimBase> impl;
    if (int rc = make_sim_impl(impl, sp, ap, pl, particles, count)) return rc;
    nb_sim *s = new (std::nothrow) nb_sim();
    if (!s) {
        set_error("out of host memory");
        return NB_ERR_ALLOC;
    }
    s->impl = std::move(impl);
    *out = s;
    return NB_OK;
}

}  // namespace nb

// ==========================================================================================
// extern "C"
// ==========================================================================================
using namespace nb;

// nb_sim_radial_profile: everything that can be refused without a device
static int radial_check_params(const nb_radial_params *p, const nb_radial_profile *out, const nb_radial_bin *bins) {
    if (!p || !out || !bins || !p->edges) {
        set_error("radial_profile: null %s", !p ? "params" : !out ? "out" : !bins ? "bins" : "edges");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_RADIAL_MAX_BINS) {
        set_error("radial_profile: nbins must be 1..%u (got %u)", NB_RADIAL_MAX_BINS, p->nbins);
        return NB_ERR_INVALID;
    }
    if (p->flags & ~(NB_RADIAL_CYLINDRICAL | NB_RADIAL_CENTER_COM)) {
        set_error("radial_profile: unknown flag bits 0x%x", p->flags & ~(NB_RADIAL_CYLINDRICAL | NB_RADIAL_CENTER_COM));
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k) {
        const double e = p->edges[k];
        if (!std::isfinite(e) || e < 0.0 || (k > 0 && !(e > p->edges[k - 1]))) {
            set_error("radial_profile: edges must be finite, >= 0 and strictly ascending (edges[%u] = %g)", k, e);
            return NB_ERR_INVALID;
        }
    }
    if (!(p->flags & NB_RADIAL_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("radial_profile: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    const double *a = p->axis;
    if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) {
        set_error("radial_profile: axis must be finite");
        return NB_ERR_INVALID;
    }
    if (p->flags & NB_RADIAL_CYLINDRICAL) {
        // (an axis whose length over- or underflows has no finite unit vector either)
        const double len = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        if (!(len > 0.0) || !std::isfinite(len)) {
            set_error("radial_profile: a cylindrical profile needs a non-zero axis");
            return NB_ERR_INVALID;
        }
    }
    return NB_OK;
}

static int radial_edges(const char *what, bool log, double rmin, double rmax, uint32_t nbins, double *edges) {
    if (!edges) {
        set_error("%s: edges is null", what);
        return NB_ERR_INVALID;
    }
    if (nbins < 1 || nbins > NB_RADIAL_MAX_BINS) {
        set_error("%s: nbins must be 1..%u (got %u)", what, NB_RADIAL_MAX_BINS, nbins);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(rmin) || !std::isfinite(rmax) || !(rmax > rmin) || !(log ? rmin > 0.0 : rmin >= 0.0)) {
        set_error("%s: needs finite %s rmin < rmax (got %g, %g)", what, log ? "0 <" : "0 <=", rmin, rmax);
        return NB_ERR_INVALID;
    }
    double prev = rmin;
    for (uint32_t k = 1; k < nbins; ++k) {  // checked before anything is written
        const double t = (double)k / (double)nbins;
        const double e = log ? rmin * std::pow(rmax / rmin, t) : rmin + (rmax - rmin) * t;
        if (!(e > prev) || !(e < rmax)) {
            set_error("%s: %u bins between %g and %g are not strictly ascending in fp64", what, nbins, rmin, rmax);
            return NB_ERR_INVALID;
        }
        prev = e;
    }
    edges[0] = rmin;
    for (uint32_t k = 1; k < nbins; ++k) {
        const double t = (double)k / (double)nbins;
        edges[k] = log ? rmin * std::pow(rmax / rmin, t) : rmin + (rmax - rmin) * t;
    }
    edges[nbins] = rmax;
    return NB_OK;
}

// nb_sim_field: everything about the arguments that can be refused without a device
static int field_check_args(const float *points, size_t m, uint32_t flags, const nb_field_sample *out) {
    if (m > 0 && (!points || !out)) {
        set_error("field: null %s", !points ? "points" : "out");
        return NB_ERR_INVALID;
    }
    if (!flags || (flags & ~(NB_FIELD_ACCEL | NB_FIELD_POTENTIAL))) {
        set_error("field: flags must be NB_FIELD_ACCEL, NB_FIELD_POTENTIAL or both (got 0x%x)", flags);
        return NB_ERR_INVALID;
    }
    if (m > NB_FIELD_MAX_POINTS) {
        set_error("field: at most %u points (got %zu)", NB_FIELD_MAX_POINTS, m);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_field_rings / nb_field_ring_means: the unit axis n and the ring basis e1, e2 = n x e1
static int ring_basis(const char *what, const double *center, const double *axis, const double *radii, uint32_t k,
                      uint32_t n_phi, double n[3], double e1[3], double e2[3]) {
    if (!center || !axis || (k && !radii)) {
        set_error("%s: null %s", what, !center ? "center" : !axis ? "axis" : "radii");
        return NB_ERR_INVALID;
    }
    if (n_phi == 0) {
        set_error("%s: n_phi must be at least 1", what);
        return NB_ERR_INVALID;
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(center[a]) || !std::isfinite(axis[a])) {
            set_error("%s: center and axis must be finite", what);
            return NB_ERR_INVALID;
        }
    double fn[3], f1[3], f2[3];  // (nothing is written on a refusal)
    if (!axis_frame(axis, fn, f1, f2)) {
        set_error("%s: needs a non-zero axis", what);
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i)
        if (!std::isfinite(radii[i]) || radii[i] < 0.0) {
            set_error("%s: radii must be finite and >= 0 (radii[%u] = %g)", what, i, radii[i]);
            return NB_ERR_INVALID;
        }
    for (int a = 0; a < 3; ++a) {
        n[a] = fn[a];
        e1[a] = f1[a];
        e2[a] = f2[a];
    }
    return NB_OK;
}

// nb_sim_fof: everything that can be refused without a device
static int fof_check_params(const nb_fof_params *p) {
    if (!p) {
        set_error("fof: null params");
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->link) || !(p->link > 0.0)) {
        set_error("fof: link must be finite and > 0 (got %g)", p->link);
        return NB_ERR_INVALID;
    }
    const double b2 = p->link * p->link;  // what the rule compares with
    if (!(b2 > 0.0) || !std::isfinite(b2)) {
        set_error("fof: link %g squared is not a positive finite double", p->link);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("fof: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved) {
        set_error("fof: unknown flag bits 0x%x or reserved %llu != 0", p->flags, (unsigned long long)p->reserved);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_sim_bound: everything that can be refused without a device (the softening is the simulator's: bound_check_e)
static int bound_check_params(const nb_bound_params *p) {
    if (!p) {
        set_error("bound: null params");
        return NB_ERR_INVALID;
    }
    nb_fof_params fp{};
    fp.link = p->link;
    fp.min_members = p->min_members;
    if (int rc = fof_check_params(&fp)) return rc;
    if (p->max_iter < 1 || p->max_iter > NB_BOUND_MAX_ITER) {
        set_error("bound: max_iter must be 1..%u (got %u)", NB_BOUND_MAX_ITER, p->max_iter);
        return NB_ERR_INVALID;
    }
    if (p->min_bound < 1) {
        set_error("bound: min_bound must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved32 || p->reserved) {
        set_error("bound: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}
static int bound_check_e(const nb_sim *sim) {
    if (!sim || !sim->impl) {
        set_error("null simulator");
        return NB_ERR_INVALID;
    }
    if (!(sim->impl->params.e >= 0.f)) {
        set_error("bound: the pair potential needs e >= 0 (e = %g)", (double)sim->impl->params.e);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_sim_group_shapes: everything that can be refused without a device -- the parameters alone, then (a handle in
// hand) what needs the simulator's n and step number
static int shape_check_params(const nb_shape_params *p) {
    if (!p) {
        set_error("group_shapes: null params");
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~NB_SHAPE_REDUCED) || p->reserved32 || p->reserved) {
        set_error("group_shapes: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("group_shapes: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->max_iter < 1 || p->max_iter > NB_SHAPE_MAX_ITER) {
        set_error("group_shapes: max_iter must be 1..%u (got %u)", NB_SHAPE_MAX_ITER, p->max_iter);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->tol) || !(p->tol > 0.0)) {
        set_error("group_shapes: tol must be finite and > 0 (got %g)", p->tol);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}
static int shape_check_args(const nb_sim *sim, const nb_shape_params *p, const uint32_t *group_of, size_t m,
                            const double *centers, const double *velocities, const double *radius) {
    if (!sim || !sim->impl) {
        set_error("null simulator");
        return NB_ERR_INVALID;
    }
    const SimBase &s = *sim->impl;
    if (s.n > 0 && !group_of) {
        set_error("group_shapes: null group_of");
        return NB_ERR_INVALID;
    }
    if (m > std::max<size_t>(s.n, 1)) {
        set_error("group_shapes: %zu rows are more than %u bodies can fill", m, s.n);
        return NB_ERR_INVALID;
    }
    for (size_t k = 0; k < 3 * m; ++k)
        if ((centers && !std::isfinite(centers[k])) || (velocities && !std::isfinite(velocities[k]))) {
            set_error("group_shapes: the centre or the velocity of row %zu is not finite", k / 3);
            return NB_ERR_INVALID;
        }
    const bool reduced = (p->flags & NB_SHAPE_REDUCED) != 0;
    if (reduced && !radius && m > 0) {
        set_error("group_shapes: NB_SHAPE_REDUCED needs a finite radius for every row (radius is null)");
        return NB_ERR_INVALID;
    }
    for (size_t r = 0; radius && r < m; ++r) {
        if (!(radius[r] > 0.0)) {  // (a NaN too)
            set_error("group_shapes: radius[%zu] = %g is neither finite and > 0 nor +inf", r, radius[r]);
            return NB_ERR_INVALID;
        }
        if (reduced && std::isinf(radius[r])) {
            set_error("group_shapes: NB_SHAPE_REDUCED needs a finite radius (radius[%zu] is +inf)", r);
            return NB_ERR_INVALID;
        }
    }
    if (p->step_num != NB_SHAPE_ANY_STEP && p->step_num != s.step_num) {
        set_error("group_shapes: the assignment was made at step %llu, the simulator is at step %llu",
                  (unsigned long long)p->step_num, (unsigned long long)s.step_num);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_sim_knn: everything that can be refused without a device
static int knn_check_params(const nb_knn_params *p) {
    if (!p) {
        set_error("knn: null params");
        return NB_ERR_INVALID;
    }
    if (p->k < 1 || p->k > NB_KNN_MAX_K) {
        set_error("knn: k must be 1..%u (got %u)", NB_KNN_MAX_K, p->k);
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved) {
        set_error("knn: unknown flag bits 0x%x or reserved %llu != 0", p->flags, (unsigned long long)p->reserved);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_sim_hop: everything that can be refused without a device
static int hop_check_params(const nb_hop_params *p) {
    if (!p) {
        set_error("hop: null params");
        return NB_ERR_INVALID;
    }
    if (p->k_density < 2 || p->k_density > NB_KNN_MAX_K) {
        set_error("hop: k_density must be 2..%u (got %u)", NB_KNN_MAX_K, p->k_density);
        return NB_ERR_INVALID;
    }
    if (p->k_hop < 1 || p->k_hop > NB_KNN_MAX_K || p->k_merge < 1 || p->k_merge > NB_KNN_MAX_K) {
        set_error("hop: k_hop and k_merge must be 1..%u (got %u, %u)", NB_KNN_MAX_K, p->k_hop, p->k_merge);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("hop: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (std::isnan(p->density_min)) {
        set_error("hop: density_min must not be NaN (-inf: no cut)");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved32 || p->reserved) {
        set_error("hop: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_hop_regroup behind the ABI boundary (include/nbody.h: the rule, step by step)
// the ordering key of a density, and the "denser" order of include/nbody.h
static double hop_rho_key(double d) { return std::isnan(d) ? -INFINITY : d; }
static bool hop_denser(double ra, uint32_t a, double rb, uint32_t b) { return ra > rb || (ra == rb && a < b); }

static int hop_regroup(const nb_fof_group *rows, const double *peak_density, size_t m, const nb_hop_boundary *bnd,
                       size_t b, const nb_hop_regroup_params *params, uint32_t *merged_of_row, nb_fof_group *out_rows,
                       double *out_peak, size_t out_capacity, size_t *out_count) {
    {
        if (!params || !out_count || (m && (!rows || !peak_density)) || (b && !bnd)) {
            set_error("hop_regroup: null argument");
            return NB_ERR_INVALID;
        }
        if (std::isnan(params->saddle) || std::isnan(params->peak) || params->saddle > params->peak) {
            set_error("hop_regroup: saddle and peak must not be NaN, with saddle <= peak (got %g, %g)", params->saddle,
                      params->peak);
            return NB_ERR_INVALID;
        }
        if (params->flags || params->reserved) {
            set_error("hop_regroup: unknown flag bits 0x%x or reserved != 0", params->flags);
            return NB_ERR_INVALID;
        }
        for (size_t r = 1; r < m; ++r)
            if (!(rows[r - 1].label < rows[r].label)) {
                set_error("hop_regroup: rows must be in strictly ascending label order (row %zu)", r);
                return NB_ERR_INVALID;
            }
        for (size_t e = 0; e < b; ++e) {
            const bool ordered = e == 0 || bnd[e - 1].a < bnd[e].a || (bnd[e - 1].a == bnd[e].a && bnd[e - 1].b < bnd[e].b);
            if (!ordered || !(bnd[e].a < bnd[e].b)) {
                set_error("hop_regroup: boundaries must be in strictly ascending (a, b) with a < b (boundary %zu)", e);
                return NB_ERR_INVALID;
            }
        }
        // the row of a label: a binary search in the ascending labels
        auto row_of = [&](uint32_t label) -> size_t {
            size_t lo = 0, hi = m;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (rows[mid].label < label) lo = mid + 1;
                else hi = mid;
            }
            return lo < m && rows[lo].label == label ? lo : m;
        };
        struct Edge {
            double density;
            size_t ra, rb, at;
        };
        std::vector<Edge> edges;
        for (size_t e = 0; e < b; ++e) {
            const size_t ra = row_of(bnd[e].a), rb = row_of(bnd[e].b);
            if (ra < m && rb < m) edges.push_back({bnd[e].density, ra, rb, e});
        }
        // descending density (a NaN as -inf, like a peak's), ties in ascending (a, b) -- the table's own order
        std::stable_sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) {
            return hop_rho_key(x.density) > hop_rho_key(y.density);
        });
        std::vector<size_t> parent(m);
        std::vector<char> viable(m);  // of a root: its set's
        for (size_t r = 0; r < m; ++r) {
            parent[r] = r;
            viable[r] = hop_rho_key(peak_density[r]) >= params->peak;
        }
        auto find = [&](size_t x) {
            while (parent[x] != x) {
                parent[x] = parent[parent[x]];
                x = parent[x];
            }
            return x;
        };
        for (const Edge &e : edges) {
            const size_t x = find(e.ra), y = find(e.rb);
            if (x == y) continue;
            if (viable[x] && viable[y] && e.density < params->saddle) continue;
            parent[y] = x;
            viable[x] = viable[x] || viable[y];
        }
        // the representative of every set: its densest peak
        std::vector<size_t> rep(m);
        for (size_t r = 0; r < m; ++r) rep[r] = m;
        for (size_t r = 0; r < m; ++r) {
            const size_t x = find(r);
            if (rep[x] == m || hop_denser(hop_rho_key(peak_density[r]), rows[r].label, hop_rho_key(peak_density[rep[x]]),
                                          rows[rep[x]].label))
                rep[x] = r;
        }
        // the viable sets in ascending representative label: a set is listed at its representative's row
        std::vector<size_t> out_of(m, m);
        size_t count = 0;
        for (size_t r = 0; r < m; ++r) {
            const size_t x = find(r);
            if (viable[x] && rep[x] == r) out_of[r] = count++;
        }
        for (size_t r = 0; r < m; ++r) {
            const size_t x = find(r);
            if (merged_of_row) merged_of_row[r] = viable[x] ? rows[rep[x]].label : NB_HOP_NONE;
            if (!viable[x] || out_of[rep[x]] >= out_capacity) continue;
            const size_t o = out_of[rep[x]];
            if (out_peak && rep[x] == r) out_peak[o] = peak_density[r];
        }
        if (out_rows) {
            const size_t listed = std::min(count, out_capacity);
            for (size_t o = 0; o < listed; ++o) out_rows[o] = nb_fof_group{};
            for (size_t r = 0; r < m; ++r) {  // the member rows in ascending row order
                const size_t x = find(r);
                if (!viable[x] || out_of[rep[x]] >= out_capacity) continue;
                nb_fof_group &g = out_rows[out_of[rep[x]]];
                g.label = rows[rep[x]].label;
                g.count += rows[r].count;
                g.mass += rows[r].mass;
                for (int a = 0; a < 3; ++a) {
                    g.mx[a] += rows[r].mx[a];
                    g.mv[a] += rows[r].mv[a];
                }
                g.mr2 += rows[r].mr2;
                g.mv2 += rows[r].mv2;
            }
        }
        *out_count = count;
        return NB_OK;
    }
}

// nb_sim_halo_profiles: everything that can be refused without a device (a body index needs n: sim_halo_profiles)
static int halo_check_params(const nb_halo_params *p) {
    if (!p || !p->edges) {
        set_error("halo_profiles: null %s", !p ? "params" : "edges");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_HALO_MAX_BINS) {
        set_error("halo_profiles: nbins must be 1..%u (got %u)", NB_HALO_MAX_BINS, p->nbins);
        return NB_ERR_INVALID;
    }
    if (p->flags) {
        set_error("halo_profiles: unknown flag bits 0x%x", p->flags);
        return NB_ERR_INVALID;
    }
    if (p->m > NB_HALO_MAX_CENTERS || p->m * p->nbins > NB_HALO_MAX_ROWS) {
        set_error("halo_profiles: %llu centres of %u bins are more than one call takes (%u centres, %u rows)",
                  (unsigned long long)p->m, p->nbins, NB_HALO_MAX_CENTERS, NB_HALO_MAX_ROWS);
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k) {
        const double e = p->edges[k];
        if (!std::isfinite(e) || e < 0.0 || (k > 0 && !(e > p->edges[k - 1]))) {
            set_error("halo_profiles: edges must be finite, >= 0 and strictly ascending (edges[%u] = %g)", k, e);
            return NB_ERR_INVALID;
        }
    }
    if (p->m == 0) return NB_OK;
    if (!p->centers == !p->bodies) {
        set_error("halo_profiles: exactly one of centers and bodies must be given (%s)",
                  p->centers ? "got both" : "got neither");
        return NB_ERR_INVALID;
    }
    for (uint64_t j = 0; j < 3 * p->m; ++j)
        if ((p->centers && !std::isfinite(p->centers[j])) || (p->velocities && !std::isfinite(p->velocities[j]))) {
            set_error("halo_profiles: centre %llu has a non-finite %s", (unsigned long long)(j / 3),
                      p->centers && !std::isfinite(p->centers[j]) ? "position" : "velocity");
            return NB_ERR_INVALID;
        }
    return NB_OK;
}

// nb_map_edges / nb_sim_map: the cell size of `cells` cells in [lo, hi), refused unless the edges
// lo + i * size (i < cells), hi come out strictly ascending
static int map_cell_size(const char *what, double lo, double hi, uint32_t cells, double *size) {
    if (cells < 1 || cells > NB_MAP_MAX_SIDE) {
        set_error("%s: a side must be 1..%u cells (got %u)", what, NB_MAP_MAX_SIDE, cells);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) {
        set_error("%s: a window needs finite lo < hi (got %g, %g)", what, lo, hi);
        return NB_ERR_INVALID;
    }
    const double d = (hi - lo) / (double)cells;
    double prev = lo;
    for (uint32_t i = 1; i <= cells; ++i) {
        const double e = i < cells ? lo + (double)i * d : hi;
        if (!(e > prev) || !std::isfinite(e)) {
            set_error("%s: %u cells between %g and %g are not strictly ascending in fp64", what, cells, lo, hi);
            return NB_ERR_INVALID;
        }
        prev = e;
    }
    *size = d;
    return NB_OK;
}

// nb_sim_map: everything that can be refused without a device; the frame and the cell sizes on the way
static int map_check_params(const nb_map_params *p, MapPlan *plan) {
    if (!p) {
        set_error("map: null params");
        return NB_ERR_INVALID;
    }
    if (p->width < 1 || p->width > NB_MAP_MAX_SIDE || p->height < 1 || p->height > NB_MAP_MAX_SIDE) {
        set_error("map: a side must be 1..%u cells (got %u x %u)", NB_MAP_MAX_SIDE, p->width, p->height);
        return NB_ERR_INVALID;
    }
    if ((uint64_t)p->width * p->height > NB_MAP_MAX_CELLS) {
        set_error("map: at most %u cells (got %u x %u)", NB_MAP_MAX_CELLS, p->width, p->height);
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~(NB_MAP_CENTER_COM | NB_MAP_VELOCITY)) || p->reserved) {
        set_error("map: unknown flag bits 0x%x or reserved %u != 0", p->flags & ~(NB_MAP_CENTER_COM | NB_MAP_VELOCITY),
                  p->reserved);
        return NB_ERR_INVALID;
    }
    if (!axis_frame(p->axis, plan->n, plan->e1, plan->e2)) {
        set_error("map: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    if (!(p->flags & NB_MAP_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("map: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    if (int rc = map_cell_size("map: x_range", p->x_range[0], p->x_range[1], p->width, &plan->dx)) return rc;
    if (int rc = map_cell_size("map: y_range", p->y_range[0], p->y_range[1], p->height, &plan->dy)) return rc;
    // (either bound may be infinite; a NaN fails the comparison)
    if (!(p->depth_range[1] > p->depth_range[0])) {
        set_error("map: depth_range needs lo < hi without NaN (got %g, %g)", p->depth_range[0], p->depth_range[1]);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_smooth_centres / nb_sim_smooth_map: the `cells` pixel centres of a window, from the edges of nb_map_edges
static void smooth_centres(double lo, double hi, uint32_t cells, double size, double *out) {
    double prev = lo;  // xe[i]
    for (uint32_t i = 0; i < cells; ++i) {
        const double next = i + 1 < cells ? lo + (double)(i + 1) * size : hi;
        out[i] = 0.5 * (prev + next);
        prev = next;
    }
}

// nb_sim_smooth_map: everything that can be refused without a device, in the words of the pass; the frame, the
// pixel sizes and the pixel centres on the way.  The fields the two share are checked by map_check_params.
static int smooth_check_params(const nb_smooth_params *p, SmoothPlan *plan) {
    if (!p) {
        set_error("smooth_map: null params");
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~(NB_SMOOTH_CENTER_COM | NB_SMOOTH_VELOCITY)) || p->reserved) {
        set_error("smooth_map: unknown flag bits 0x%x or reserved %u != 0",
                  p->flags & ~(NB_SMOOTH_CENTER_COM | NB_SMOOTH_VELOCITY), p->reserved);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->s_min) || !std::isfinite(p->s_max) || !(p->s_min > 0.0) || !(p->s_max >= p->s_min)) {
        set_error("smooth_map: needs finite 0 < s_min <= s_max (got %g, %g)", p->s_min, p->s_max);
        return NB_ERR_INVALID;
    }
    static_assert(NB_SMOOTH_CENTER_COM == NB_MAP_CENTER_COM && NB_SMOOTH_VELOCITY == NB_MAP_VELOCITY, "shared flag bits");
    nb_map_params m{};
    m.width = p->width;
    m.height = p->height;
    m.flags = p->flags;
    for (int k = 0; k < 3; ++k) {
        m.center[k] = p->center[k];
        m.velocity[k] = p->velocity[k];
        m.axis[k] = p->axis[k];
    }
    for (int k = 0; k < 2; ++k) {
        m.x_range[k] = p->x_range[k];
        m.y_range[k] = p->y_range[k];
        m.depth_range[k] = p->depth_range[k];
    }
    if (int rc = map_check_params(&m, &plan->frame)) {
        const std::string why = g_last_error;  // "map: ..."
        set_error("smooth_%s", why.c_str());
        return rc;
    }
    plan->xc.resize(p->width);
    plan->yc.resize(p->height);
    smooth_centres(p->x_range[0], p->x_range[1], p->width, plan->frame.dx, plan->xc.data());
    smooth_centres(p->y_range[0], p->y_range[1], p->height, plan->frame.dy, plan->yc.data());
    return NB_OK;
}

#define NB_GUARD(body)                                            \
    try {                                                         \
        body                                                      \
    } catch (const std::bad_alloc &) {                            \
        set_error("out of host memory");                          \
        return NB_ERR_ALLOC;                                      \
    } catch (...) {                                               \
        set_error("unexpected C++ exception at the ABI boundary"); \
        return NB_ERR_INVALID;                                    \
    }

extern "C" {

const char *nb_last_error(void) { return g_last_error.c_str(); }
#ifndef NB_SOURCE_HASH
#define NB_SOURCE_HASH "unknown"
#endif
// "... src:<hash>": sha256 prefix of the sources this binary was built from (build.py), so that a
// stale library next to newer sources is detectable (tests/test_abi.py)
const char *nb_version(void) { return "nbody_hip 0.2.0 gfx950 src:" NB_SOURCE_HASH; }

int nb_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

size_t nb_shard_bodies_per_rank(size_t particle_num, int world) {
    if (world < 1) world = 1;
    const size_t per = (particle_num + (size_t)world - 1) / (size_t)world;
    return round_up(per ? per : 1, kPadTo);
}

size_t nb_shard_padded_bodies(size_t particle_num, int world) {
    if (world < 1) world = 1;
    return nb_shard_bodies_per_rank(particle_num, world) * (size_t)world;
}

int nb_sim_create(nb_sim **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                  const nb_placement *placement, nb_init_fn init, void *user) {
    NB_GUARD({
        if (!sim_params || !init) {
            set_error("nb_sim_create: sim_params and init must be non-null");
            return NB_ERR_INVALID;
        }
        // init_fn(&sim_params) -> Vec<Particle>, naive.rs:97 / tree.rs:149
        std::vector<nb_particle> host(sim_params->particle_num);
        init(sim_params, host.data(), user);
        return make_sim(out, sim_params, add_params, placement, host.data(), host.size());
    })
}

int nb_sim_create_from_particles(nb_sim **out, const nb_sim_params *sim_params,
                                 const nb_add_params *add_params, const nb_placement *placement,
                                 const nb_particle *particles, size_t n) {
    NB_GUARD({
        if (!particles && n) {
            set_error("nb_sim_create_from_particles: particles is null");
            return NB_ERR_INVALID;
        }
        return make_sim(out, sim_params, add_params, placement, particles, n);
    })
}

#define NB_SIM_CALL(sim, expr)                \
    NB_GUARD({                                \
        if (!(sim) || !(sim)->impl) {         \
            set_error("null simulator");      \
            return NB_ERR_INVALID;            \
        }                                     \
        return (sim)->impl->expr;             \
    })
// ... and a free function over the object behind the handle: the analysis passes
#define NB_SIM_PASS(sim, fn, ...)                 \
    NB_GUARD({                                    \
        if (!(sim) || !(sim)->impl) {             \
            set_error("null simulator");          \
            return NB_ERR_INVALID;                \
        }                                         \
        return fn(*(sim)->impl, __VA_ARGS__);     \
    })

int nb_sim_encode(nb_sim *sim) { NB_SIM_CALL(sim, encode()) }
int nb_sim_encode_phase(nb_sim *sim, int phase) { NB_SIM_CALL(sim, encode_phase(phase)) }
int nb_sim_let_set_imports(nb_sim *sim, const uint32_t *counts, int world) {
    NB_SIM_CALL(sim, let_set_imports(counts, world))
}
int nb_sim_let_set_import_stride(nb_sim *sim, uint32_t stride) {
    NB_SIM_CALL(sim, let_set_import_stride(stride))
}
int nb_sim_let_set_owners(nb_sim *sim, const unsigned long long *splits, int world, float ref_bound,
                          uint32_t seg_cap) {
    NB_SIM_CALL(sim, let_set_owners(splits, world, ref_bound, seg_cap))
}
int nb_sim_let_set_arrivals(nb_sim *sim, uint32_t stay, const uint32_t *counts, int world) {
    NB_SIM_CALL(sim, let_set_arrivals(stay, counts, world))
}
int nb_sim_cleanup(nb_sim *sim) { NB_SIM_CALL(sim, cleanup()) }
int nb_sim_wait(nb_sim *sim) { NB_SIM_CALL(sim, wait()) }

int nb_sim_sim_params(const nb_sim *sim, nb_sim_params *out) {
    if (!sim || !sim->impl || !out) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *out = sim->impl->params;
    return NB_OK;
}

int nb_sim_read_particles(nb_sim *sim, nb_particle *dst, size_t n) {
    if (!dst && n) {
        set_error("read_particles: dst is null");
        return NB_ERR_INVALID;
    }
    NB_SIM_CALL(sim, read_particles(dst, n))
}

int nb_sim_write_particles(nb_sim *sim, const nb_particle *src, size_t n) {
    if (!src && n) {
        set_error("write_particles: src is null");
        return NB_ERR_INVALID;
    }
    NB_SIM_CALL(sim, write_particles(src, n))
}

int nb_sim_read_tree(nb_sim *sim, nb_octant *dst, size_t cap, size_t *n_nodes, float *root_width) {
    NB_SIM_CALL(sim, read_tree(dst, cap, n_nodes, root_width))
}

int nb_sim_exchange_region(nb_sim *sim, void **dev_ptr, size_t *offset_bytes, size_t *slice_bytes,
                           size_t *total_bytes) {
    NB_SIM_CALL(sim, exchange_region(0, dev_ptr, offset_bytes, slice_bytes, total_bytes))
}

int nb_sim_exchange_count(nb_sim *sim, int *count) {
    if (!sim || !sim->impl || !count) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *count = sim->impl->exchange_count();
    return NB_OK;
}

int nb_sim_exchange_region_i(nb_sim *sim, int index, void **dev_ptr, size_t *offset_bytes,
                             size_t *slice_bytes, size_t *total_bytes) {
    NB_SIM_CALL(sim, exchange_region(index, dev_ptr, offset_bytes, slice_bytes, total_bytes))
}

int nb_sim_step_num(const nb_sim *sim, uint64_t *out) {
    if (!sim || !sim->impl || !out) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *out = sim->impl->step_num;
    return NB_OK;
}

int nb_sim_encode_n_timed(nb_sim *sim, int n, float *ms_total, float *ms_kernel) {
    NB_SIM_CALL(sim, encode_n_timed(n, ms_total, ms_kernel))
}

int nb_sim_set_tuning(nb_sim *sim, const char *key, int value) {
    if (!key) {
        set_error("null key");
        return NB_ERR_INVALID;
    }
    if (!std::strcmp(key, "render_design")) {  // the renderer's, whichever simulator holds the state
        NB_SIM_PASS(sim, sim_render_set_design, value)
    }
    if (!std::strcmp(key, "field_launch_pairs_log2")) {  // the field probes', whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 16 || value > 40) {
            set_error("field_launch_pairs_log2: 16..40, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->field_pairs_log2 = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "map_segment_len")) {  // the maps', whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 256 || value > 65536 || value % 256) {
            set_error("map_segment_len: a multiple of 256 in 256..65536, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->map_segment_len = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "smooth_segment_len")) {  // the smoothed maps', whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 256 || value > 65536 || value % 256) {
            set_error("smooth_segment_len: a multiple of 256 in 256..65536, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->smooth_segment_len = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "fof_chunk_len")) {  // the group finder's, whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 64 || value > 65536 || value % 64) {
            set_error("fof_chunk_len: a multiple of 64 in 64..65536, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->fof_chunk_len = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "fof_cell_boxes")) {
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value != 0 && value != 1) {
            set_error("fof_cell_boxes: 0 or 1, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->fof_cell_boxes = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "bound_chunk_len")) {  // the unbinding's, whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 64 || value > 1048576 || value % 64) {
            set_error("bound_chunk_len: a multiple of 64 in 64..1048576, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->bound_chunk_len = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "shape_chunk_len")) {  // the group shapes', whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 64 || value > 65536 || value % 64) {
            set_error("shape_chunk_len: a multiple of 64 in 64..65536, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->shape_chunk_len = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "bound_tile")) {
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value != 0 && value != 64 && value != 256) {
            set_error("bound_tile: 0, 64 or 256, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->bound_tile = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "knn_span_cells")) {  // the neighbour search's, whichever simulator holds the state
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value < 1 || value > 8) {
            set_error("knn_span_cells: 1..8, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->knn_span_cells = value;
        return NB_OK;
    }
    if (!std::strcmp(key, "knn_block_queries")) {
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (value != 1 && value != 2 && value != 4) {
            set_error("knn_block_queries: 1, 2 or 4, not %d", value);
            return NB_ERR_INVALID;
        }
        sim->impl->knn_block_queries = value;
        return NB_OK;
    }
    NB_SIM_CALL(sim, set_tuning(key, value))
}

int nb_sim_debug_buffer(nb_sim *sim, const char *name, void *dst, size_t cap, size_t *bytes) {
    if (!name) {
        set_error("null name");
        return NB_ERR_INVALID;
    }
    NB_SIM_CALL(sim, debug_buffer(name, dst, cap, bytes))
}

int nb_sim_diagnostics(nb_sim *sim, uint32_t flags, nb_diagnostics *out) {
    if (!out) {
        set_error("diagnostics: out is null");
        return NB_ERR_INVALID;
    }
    if (flags & ~(NB_DIAG_MOMENTS | NB_DIAG_POTENTIAL)) {
        set_error("diagnostics: unknown flag bits 0x%x", flags & ~(NB_DIAG_MOMENTS | NB_DIAG_POTENTIAL));
        return NB_ERR_INVALID;
    }
    NB_SIM_PASS(sim, sim_diagnostics, flags, out)
}

int nb_sim_radial_profile(nb_sim *sim, const nb_radial_params *params, nb_radial_profile *out,
                          nb_radial_bin *bins) {
    if (int rc = radial_check_params(params, out, bins)) return rc;
    NB_SIM_PASS(sim, sim_radial_profile, *params, out, bins)
}

int nb_radial_edges_log(double rmin, double rmax, uint32_t nbins, double *edges) {
    return radial_edges("radial_edges_log", true, rmin, rmax, nbins, edges);
}
int nb_radial_edges_linear(double rmin, double rmax, uint32_t nbins, double *edges) {
    return radial_edges("radial_edges_linear", false, rmin, rmax, nbins, edges);
}

int nb_radial_lagrangian(const nb_radial_profile *p, const nb_radial_bin *bins, const double *edges,
                         const double *fractions, uint32_t k, double *radii) {
    if (!p || !bins || !edges || (k && (!fractions || !radii))) {
        set_error("radial_lagrangian: null argument");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_RADIAL_MAX_BINS) {
        set_error("radial_lagrangian: profile with %u bins", p->nbins);
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i) {
        const double f = fractions[i], target = f * p->mass;
        radii[i] = std::nan("");
        if (!(f > 0.0 && f < 1.0) || !(target >= p->inside_mass)) continue;  // ... or the crossing lies in `inside`
        double cum = p->inside_mass;
        for (uint32_t b = 0; b < p->nbins; ++b) {
            const double m = bins[b].mass, next = cum + m;
            if (target <= next) {  // linear in r inside the bin that crosses
                radii[i] = m > 0.0 ? edges[b] + (target - cum) / m * (edges[b + 1] - edges[b]) : edges[b];
                break;
            }
            cum = next;
        }
    }
    return NB_OK;
}

int nb_sim_field(nb_sim *sim, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                 nb_field_stats *stats) {
    if (int rc = field_check_args(points, m, flags, out)) return rc;
    NB_SIM_PASS(sim, sim_field, points, m, flags, out, stats)
}

int nb_field_rings(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                   float *points) {
    double n[3], e1[3], e2[3];
    if (int rc = ring_basis("field_rings", center, axis, radii, k, n_phi, n, e1, e2)) return rc;
    if (k && !points) {
        set_error("field_rings: null points");
        return NB_ERR_INVALID;
    }
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t q = 0; q < n_phi; ++q) {
            const double phi = two_pi * (double)q / (double)n_phi, c = std::cos(phi), s = std::sin(phi);
            float *p = points + 3 * ((size_t)i * n_phi + q);
            for (int a = 0; a < 3; ++a) p[a] = (float)(center[a] + radii[i] * (c * e1[a] + s * e2[a]));
        }
    return NB_OK;
}

int nb_field_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k,
                        uint32_t n_phi, const float *points, const nb_field_sample *samples, nb_field_ring *out) {
    double n[3], e1[3], e2[3];
    if (int rc = ring_basis("field_ring_means", center, axis, radii, k, n_phi, n, e1, e2)) return rc;
    if (k && (!points || !samples || !out)) {
        set_error("field_ring_means: null %s", !points ? "points" : !samples ? "samples" : "out");
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i) {
        double a_r = 0.0, a_n = 0.0, pot = 0.0;
        for (uint32_t q = 0; q < n_phi; ++q) {
            const size_t j = (size_t)i * n_phi + q;
            const nb_field_sample &f = samples[j];
            double d[3], h = 0.0;  // the fp32 point actually used, from the centre; its height along n
            for (int a = 0; a < 3; ++a) {
                d[a] = (double)points[3 * j + a] - center[a];
                h += d[a] * n[a];
            }
            double len = 0.0, dot = 0.0;
            for (int a = 0; a < 3; ++a) {
                d[a] -= h * n[a];
                len += d[a] * d[a];
                dot += f.acc[a] * d[a];
            }
            len = std::sqrt(len);
            if (len > 0.0) a_r += dot / len;
            a_n += f.acc[0] * n[0] + f.acc[1] * n[1] + f.acc[2] * n[2];
            pot += f.potential;
        }
        nb_field_ring r{};
        r.a_R = a_r / (double)n_phi;
        r.a_n = a_n / (double)n_phi;
        r.potential = pot / (double)n_phi;
        r.v_c = std::sqrt(std::fmax(0.0, -radii[i] * r.a_R));
        out[i] = r;
    }
    return NB_OK;
}

int nb_sim_map(nb_sim *sim, const nb_map_params *params, uint32_t *counts, double *planes, nb_map_stats *stats) {
    MapPlan plan{};
    if (int rc = map_check_params(params, &plan)) return rc;
    NB_SIM_PASS(sim, sim_map, *params, plan, counts, planes, stats)
}

int nb_sim_fof(nb_sim *sim, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
               size_t group_capacity, nb_fof_stats *stats) {
    if (int rc = fof_check_params(params)) return rc;
    NB_SIM_PASS(sim, sim_fof, *params, labels, group_of, groups, group_capacity, stats)
}

int nb_sim_bound(nb_sim *sim, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of, double *energy,
                 nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats) {
    if (int rc = bound_check_params(params)) return rc;
    if (int rc = bound_check_e(sim)) return rc;
    NB_SIM_PASS(sim, sim_bound, *params, group_of, bound_of, energy, groups, group_capacity, stats)
}

int nb_sim_knn(nb_sim *sim, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in, double *density,
               nb_knn_stats *stats) {
    if (int rc = knn_check_params(params)) return rc;
    NB_SIM_PASS(sim, sim_knn, *params, r2, kth, mass_in, density, stats)
}

int nb_sim_hop(nb_sim *sim, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of, double *density,
               nb_fof_group *groups, double *peak_density, size_t group_capacity, nb_hop_boundary *boundaries,
               size_t boundary_capacity, nb_hop_stats *stats) {
    if (int rc = hop_check_params(params)) return rc;
    NB_SIM_PASS(sim, sim_hop, *params, labels, group_of, density, groups, peak_density, group_capacity, boundaries,
                boundary_capacity, stats)
}

int nb_hop_regroup(const nb_fof_group *rows, const double *peak_density, size_t m, const nb_hop_boundary *bnd,
                   size_t b, const nb_hop_regroup_params *params, uint32_t *merged_of_row, nb_fof_group *out_rows,
                   double *out_peak, size_t out_capacity, size_t *out_count) {
    NB_GUARD({
        return hop_regroup(rows, peak_density, m, bnd, b, params, merged_of_row, out_rows, out_peak, out_capacity,
                           out_count);
    })
}

int nb_sim_halo_profiles(nb_sim *sim, const nb_halo_params *params, nb_halo_head *heads, nb_radial_bin *bins,
                         nb_halo_stats *stats) {
    if (int rc = halo_check_params(params)) return rc;
    NB_SIM_PASS(sim, sim_halo_profiles, *params, heads, bins, stats)
}

int nb_sim_group_shapes(nb_sim *sim, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                        const double *centers, const double *velocities, const double *radius,
                        nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats) {
    if (int rc = shape_check_params(params)) return rc;
    if (int rc = shape_check_args(sim, params, group_of, m, centers, velocities, radius)) return rc;
    NB_SIM_PASS(sim, sim_group_shapes, *params, group_of, m, centers, velocities, radius, rows_out, selected_of, stats)
}

int nb_shape_eigen(const double t[6], double lambda[3], double axes[9]) {
    if (!t || !lambda || !axes) {
        set_error("shape_eigen: null argument");
        return NB_ERR_INVALID;
    }
    shape_eigen_host(t, lambda, axes);
    return NB_OK;
}

int nb_halo_enclosed(const nb_halo_head *head, const nb_radial_bin *bins, uint32_t nbins, double *out) {
    if (!head || !bins || !out) {
        set_error("halo_enclosed: null argument");
        return NB_ERR_INVALID;
    }
    if (nbins < 1 || nbins > NB_HALO_MAX_BINS) {
        set_error("halo_enclosed: nbins must be 1..%u (got %u)", NB_HALO_MAX_BINS, nbins);
        return NB_ERR_INVALID;
    }
    out[0] = head->inside_mass;
    for (uint32_t k = 0; k < nbins; ++k) out[k + 1] = out[k] + bins[k].mass;
    return NB_OK;
}

int nb_halo_overdensity(const nb_halo_head *head, const nb_radial_bin *bins, const double *edges, uint32_t nbins,
                        double rho, double *r, double *mass) {
    if (!edges || !r || !mass) {
        set_error("halo_overdensity: null argument");
        return NB_ERR_INVALID;
    }
    double enclosed[NB_HALO_MAX_BINS + 1];
    if (int rc = nb_halo_enclosed(head, bins, nbins, enclosed)) return rc;
    if (!std::isfinite(rho) || !(rho > 0.0)) {
        set_error("halo_overdensity: rho must be finite and > 0 (got %g)", rho);
        return NB_ERR_INVALID;
    }
    *r = *mass = std::nan("");
    for (uint32_t k = 1; k <= nbins; ++k) {
        const double e0 = edges[k - 1], e1 = edges[k];
        if (!(e0 > 0.0)) continue;
        const double rho0 = enclosed[k - 1] / (NB_KNN_SPHERE * ((e0 * e0) * e0));
        const double rho1 = enclosed[k] / (NB_KNN_SPHERE * ((e1 * e1) * e1));
        if (rho0 >= rho && rho > rho1) {
            const double t = (std::log(rho0) - std::log(rho)) / (std::log(rho0) - std::log(rho1));
            const double x = std::exp(std::log(e0) + t * (std::log(e1) - std::log(e0)));
            *r = x;
            *mass = rho * NB_KNN_SPHERE * ((x * x) * x);
            break;
        }
    }
    return NB_OK;
}

int nb_sim_smooth_map(nb_sim *sim, const nb_smooth_params *params, const double *s, uint32_t *counts, double *planes,
                      nb_smooth_stats *stats) {
    NB_GUARD({
        SmoothPlan plan{};
        if (int rc = smooth_check_params(params, &plan)) return rc;
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (!s && sim->impl->n > 0) {
            set_error("smooth_map: null s for %u bodies", sim->impl->n);
            return NB_ERR_INVALID;
        }
        return sim_smooth_map(*sim->impl, *params, plan, s, counts, planes, stats);
    })
}

int nb_smooth_centres(double lo, double hi, uint32_t cells, double *out) {
    if (!out) {
        set_error("smooth_centres: out is null");
        return NB_ERR_INVALID;
    }
    double d = 0.0;
    if (int rc = map_cell_size("smooth_centres", lo, hi, cells, &d)) return rc;
    smooth_centres(lo, hi, cells, d, out);
    return NB_OK;
}

int nb_map_frame(const double axis[3], double n_hat[3], double e1[3], double e2[3]) {
    if (!axis || !n_hat || !e1 || !e2) {
        set_error("map_frame: null argument");
        return NB_ERR_INVALID;
    }
    double n[3], f1[3], f2[3];
    if (!axis_frame(axis, n, f1, f2)) {
        set_error("map_frame: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    for (int a = 0; a < 3; ++a) {
        n_hat[a] = n[a];
        e1[a] = f1[a];
        e2[a] = f2[a];
    }
    return NB_OK;
}

int nb_map_edges(double lo, double hi, uint32_t cells, double *edges) {
    if (!edges) {
        set_error("map_edges: edges is null");
        return NB_ERR_INVALID;
    }
    double d = 0.0;
    if (int rc = map_cell_size("map_edges", lo, hi, cells, &d)) return rc;
    for (uint32_t i = 0; i < cells; ++i) edges[i] = lo + (double)i * d;
    edges[cells] = hi;
    return NB_OK;
}

int nb_sim_render(nb_sim *sim, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                  nb_render_stats *stats) {
    if (int rc = render_check_params(params)) return rc;
    NB_SIM_PASS(sim, sim_render, *params, rgba, counts, stats)
}

int nb_naive_variant_count(void) { return naive_variant_count(); }
const char *nb_naive_variant_name(int v) { return naive_variant_name(v); }

int nb_sim_destroy(nb_sim *sim) {
    if (!sim) return NB_OK;
    if (sim->impl) (void)sim->impl->wait();
    delete sim;
    return NB_OK;
}

// ---- runner: OfflineHeadless<T>, src/runners/offline_headless.rs ---------------------------
struct nb_runner {
    nb_sim *sim = nullptr;                  // one device
    std::unique_ptr<DeviceGroup> group;      // several devices of this process (nb_runner_create_multi)
    bool profiling = false;                  // nb_runner_set_profiling, one device: events around step_n
    float kernel_ms = 0.f;
};

int nb_runner_create(nb_runner **out, const nb_sim_params *sim_params,
                     const nb_add_params *add_params, nb_init_fn init, void *user, int device_id) {
    NB_GUARD({
        if (!out) {
            set_error("null argument");
            return NB_ERR_INVALID;
        }
        *out = nullptr;
        nb_placement pl{};
        pl.device_id = device_id < 0 ? 0 : device_id;  // HighPerformance adapter, :23-30
        pl.rank = 0;
        pl.world = 1;
        nb_sim *sim = nullptr;
        if (int rc = nb_sim_create(&sim, sim_params, add_params, &pl, init, user)) return rc;
        nb_runner *r = new nb_runner();
        r->sim = sim;
        *out = r;
        return NB_OK;
    })
}

static int runner_create_group(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                               nb_init_fn init, void *user, const int *device_ids, int n_devices, int let_migrate_every);

static int check_runner(const nb_runner *runner) {  // a runner that owns a simulator or a group
    if (!runner || (!runner->sim && !runner->group)) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

int nb_runner_create_multi(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                           nb_init_fn init, void *user, const int *device_ids, int n_devices) {
    return runner_create_group(out, sim_params, add_params, init, user, device_ids, n_devices, -1);
}

int nb_runner_create_multi_let(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                               nb_init_fn init, void *user, const int *device_ids, int n_devices, int migrate_every) {
    if (!add_params || add_params->kind != NB_TREE_SIM_PARAMS || migrate_every < 0) {
        set_error("nb_runner_create_multi_let: TreeSimParams and migrate_every >= 0");
        return NB_ERR_INVALID;
    }
    return runner_create_group(out, sim_params, add_params, init, user, device_ids, n_devices, migrate_every);
}

static int runner_create_group(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                               nb_init_fn init, void *user, const int *device_ids, int n_devices, int let_migrate_every) {
    NB_GUARD({
        if (!out || !sim_params || !init || !device_ids || n_devices < 1) {
            set_error("nb_runner_create_multi: null argument or no device");
            return NB_ERR_INVALID;
        }
        *out = nullptr;
        if (n_devices == 1 && let_migrate_every < 0)
            return nb_runner_create(out, sim_params, add_params, init, user, device_ids[0]);
        const nb_add_params add = add_params_or_default(add_params);
        if (add.kind != NB_NAIVE_SIM_PARAMS && add.kind != NB_TREE_SIM_PARAMS) {
            set_error("unknown add_params.kind %d", add.kind);
            return NB_ERR_INVALID;
        }
        std::vector<nb_particle> host(sim_params->particle_num);
        init(sim_params, host.data(), user);  // init_fn(&sim_params) -> Vec<Particle>, once, on the host
        std::unique_ptr<DeviceGroup> g;
        if (int rc = DeviceGroup::create(g, *sim_params, add, host.data(), device_ids, n_devices, let_migrate_every))
            return rc;
        nb_runner *r = new nb_runner();
        r->group = std::move(g);
        *out = r;
        return NB_OK;
    })
}

// offline_headless.rs:38-44: encode -> submit -> cleanup -> poll(Wait)
int nb_runner_step(nb_runner *runner) {
    if (int rc = check_runner(runner)) return rc;
    if (runner->group) NB_GUARD({ return runner->group->step_n(1); })
    if (int rc = nb_sim_encode(runner->sim)) return rc;
    if (int rc = nb_sim_cleanup(runner->sim)) return rc;
    return nb_sim_wait(runner->sim);
}

int nb_runner_step_n(nb_runner *runner, int n) {
    if (int rc = check_runner(runner)) return rc;
    if (runner->group) NB_GUARD({ return runner->group->step_n(n); })
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool prof = runner->profiling && runner->sim->impl && runner->sim->impl->bind_device() == NB_OK &&
                      hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    if (prof) (void)hipEventRecord(ev[0], runner->sim->impl->stream);
    int rc = NB_OK;
    for (int k = 0; k < n && rc == NB_OK; ++k) {
        rc = nb_sim_encode(runner->sim);
        if (rc == NB_OK) rc = nb_sim_cleanup(runner->sim);
    }
    if (prof) (void)hipEventRecord(ev[1], runner->sim->impl->stream);
    const int rw = nb_sim_wait(runner->sim);
    if (prof && hipEventElapsedTime(&runner->kernel_ms, ev[0], ev[1]) != hipSuccess) runner->kernel_ms = 0.f;
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc != NB_OK ? rc : rw;
}

int nb_runner_set_profiling(nb_runner *runner, int on) {
    if (int rc = check_runner(runner)) return rc;
    runner->profiling = on != 0;
    if (runner->group) return runner->group->set_profiling(on != 0);
    return NB_OK;
}

int nb_runner_rank_times(nb_runner *runner, float *kernel_ms, float *wait_ms, int n) {
    if (check_runner(runner) || n < 1) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    for (int r = 0; r < n; ++r) {
        if (kernel_ms) kernel_ms[r] = 0.f;
        if (wait_ms) wait_ms[r] = 0.f;
    }
    if (runner->group) return runner->group->rank_times(kernel_ms, wait_ms, n);
    if (kernel_ms) kernel_ms[0] = runner->kernel_ms;
    return NB_OK;
}

int nb_runner_read_particles(nb_runner *runner, nb_particle *dst, size_t n) {
    if (!runner) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    if (runner->group) {
        if (!dst && n) {
            set_error("read_particles: dst is null");
            return NB_ERR_INVALID;
        }
        NB_GUARD({ return runner->group->read_particles(dst, n); })
    }
    return nb_sim_read_particles(runner->sim, dst, n);
}

int nb_runner_sim_params(const nb_runner *runner, nb_sim_params *out) {
    if (!runner || !out) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    if (runner->group) {
        *out = runner->group->params();
        return NB_OK;
    }
    return nb_sim_sim_params(runner->sim, out);
}

int nb_runner_step_num(const nb_runner *runner, uint64_t *out) {
    if (!runner || !out) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    if (runner->group) {
        *out = runner->group->step_num();
        return NB_OK;
    }
    return nb_sim_step_num(runner->sim, out);
}

// the analysis passes read the whole state of one simulator
static int refuse_group(const nb_runner *runner, const char *name) {
    if (!runner->group) return NB_OK;
    set_error("%s: not available on a several-GPU runner (nb_runner_create_multi*)", name);
    return NB_ERR_UNSUPPORTED;
}

int nb_runner_diagnostics(nb_runner *runner, uint32_t flags, nb_diagnostics *out) {
    if (int rc = check_runner(runner)) return rc;
    if (out && !(flags & ~(NB_DIAG_MOMENTS | NB_DIAG_POTENTIAL)))  // (a group is refused for valid arguments only)
        if (int rc = refuse_group(runner, "diagnostics")) return rc;
    return nb_sim_diagnostics(runner->sim, flags, out);
}

int nb_runner_radial_profile(nb_runner *runner, const nb_radial_params *params, nb_radial_profile *out,
                             nb_radial_bin *bins) {
    if (int rc = radial_check_params(params, out, bins)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "radial_profile")) return rc;
    return nb_sim_radial_profile(runner->sim, params, out, bins);
}

int nb_runner_field(nb_runner *runner, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                    nb_field_stats *stats) {
    if (int rc = field_check_args(points, m, flags, out)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "field")) return rc;
    return nb_sim_field(runner->sim, points, m, flags, out, stats);
}

int nb_runner_map(nb_runner *runner, const nb_map_params *params, uint32_t *counts, double *planes,
                  nb_map_stats *stats) {
    MapPlan plan{};
    if (int rc = map_check_params(params, &plan)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "map")) return rc;
    return nb_sim_map(runner->sim, params, counts, planes, stats);
}

int nb_runner_fof(nb_runner *runner, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of,
                  nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats) {
    if (int rc = fof_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "fof")) return rc;
    return nb_sim_fof(runner->sim, params, labels, group_of, groups, group_capacity, stats);
}

int nb_runner_hop(nb_runner *runner, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of,
                  double *density, nb_fof_group *groups, double *peak_density, size_t group_capacity,
                  nb_hop_boundary *boundaries, size_t boundary_capacity, nb_hop_stats *stats) {
    if (int rc = hop_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "hop")) return rc;
    return nb_sim_hop(runner->sim, params, labels, group_of, density, groups, peak_density, group_capacity, boundaries,
                      boundary_capacity, stats);
}

int nb_runner_bound(nb_runner *runner, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of,
                    double *energy, nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats) {
    if (int rc = bound_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "bound")) return rc;
    return nb_sim_bound(runner->sim, params, group_of, bound_of, energy, groups, group_capacity, stats);
}

int nb_runner_knn(nb_runner *runner, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in,
                  double *density, nb_knn_stats *stats) {
    if (int rc = knn_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "knn")) return rc;
    return nb_sim_knn(runner->sim, params, r2, kth, mass_in, density, stats);
}

int nb_runner_halo_profiles(nb_runner *runner, const nb_halo_params *params, nb_halo_head *heads,
                            nb_radial_bin *bins, nb_halo_stats *stats) {
    if (int rc = halo_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "halo_profiles")) return rc;
    return nb_sim_halo_profiles(runner->sim, params, heads, bins, stats);
}

int nb_runner_group_shapes(nb_runner *runner, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                           const double *centers, const double *velocities, const double *radius,
                           nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats) {
    if (int rc = shape_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "group_shapes")) return rc;
    return nb_sim_group_shapes(runner->sim, params, group_of, m, centers, velocities, radius, rows_out, selected_of,
                               stats);
}

int nb_runner_smooth_map(nb_runner *runner, const nb_smooth_params *params, const double *s, uint32_t *counts,
                         double *planes, nb_smooth_stats *stats) {
    NB_GUARD({
        SmoothPlan plan{};
        if (int rc = smooth_check_params(params, &plan)) return rc;
    })
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "smooth_map")) return rc;
    return nb_sim_smooth_map(runner->sim, params, s, counts, planes, stats);
}

int nb_runner_render(nb_runner *runner, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                     nb_render_stats *stats) {
    if (int rc = render_check_params(params)) return rc;
    if (int rc = check_runner(runner)) return rc;
    if (int rc = refuse_group(runner, "render")) return rc;
    return nb_sim_render(runner->sim, params, rgba, counts, stats);
}

nb_sim *nb_runner_sim(nb_runner *runner) { return runner ? runner->sim : nullptr; }

int nb_runner_destroy(nb_runner *runner) {
    if (!runner) return NB_OK;
    runner->group.reset();
    nb_sim_destroy(runner->sim);
    delete runner;
    return NB_OK;
}

}  // extern "C"
