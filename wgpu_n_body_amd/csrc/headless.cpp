// headless.cpp -- C++ counterpart of the reference's src/bin/headless.rs:14-35 (and of the
// criterion groups in benches/benchmark.rs:12-49) over the drop-in API of simulator.hpp.
//
//   headless [--sim naive|tree] [--n N] [--steps S] [--theta T] [--init uniform|disc|spherical]
//            [--seed K] [--device D | --devices D0,D1,...] [--g G] [--dt DT] [--dump FILE]
//            [--e E] [--diag K [--diag-potential 1]] [--frames DIR [--frame-every K] [--frame-size WxH]]
//
// --devices: the step sharded over several GPUs of this process (nb_runner_create_multi; both simulators);
// --let K (with --sim tree --devices): Morton domains + LET exchange, migration every K-th step (0: never);
// a device id may repeat.
//
// --diag K prints the diagnostics (nb_runner_diagnostics) of step 0 and of every K-th step, one line
// "Diagnostics: step S kinetic K potential U total E momentum px py pz angular_momentum lx ly lz"
// (%.9e; potential and total are nan unless --diag-potential 1 adds the O(N^2) pair potential).  The
// time they take is not part of any "Step Duration"; without --diag the output is unchanged.
//
// --frames DIR draws the state on the device (nb_runner_render: the reference's draw pass with its
// default camera, src/runners/online_renderer.rs:224-367) at step 0 and after every K-th step
// (--frame-every, default 1) and writes DIR/frame_<step, 6 digits>.ppm (binary P6, --frame-size,
// default 1280x720), with one line "Frame S: drawn D clipped C oversize O nonfinite B fragments F
// max_count M" each.  DIR must exist.  Frame time is not part of any "Step Duration"; without
// --frames the output is unchanged.  bin/visualize.rs's run: --sim tree --n 100000 --init disc
// --g 1e-5 --e 1e-4 --dt 0.0016 --theta 0.75 --frames DIR.
//
// --dump FILE writes the final state as a snapshot (the layout of
// wgpu_n_body_amd/snapshot.py: "NBSNAP01", u64 step, SimParams, Particle[n]).
//
// Defaults reproduce headless.rs: TreeSim, 4,000,000 bodies, theta 0.75, uniform_init,
// 10 steps, printing "Step Duration: {} us" per step.  (TreeSim needs the Barnes-Hut build;
// pass --sim naive --n 65536 for the all-pairs path.)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "simulator.hpp"

static bool write_snapshot(const std::string &path, const nbody::SimParams &sp,
                           const std::vector<nbody::Particle> &parts, uint64_t step) {
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = std::fwrite("NBSNAP01", 1, 8, f) == 8 && std::fwrite(&step, sizeof step, 1, f) == 1 &&
              std::fwrite(&sp, sizeof sp, 1, f) == 1 &&
              std::fwrite(parts.data(), sizeof(nbody::Particle), parts.size(), f) == parts.size();
    return std::fclose(f) == 0 && ok;
}

template <class Sim>
static void print_diag(nbody::OfflineHeadless<Sim> &runner, bool potential) {
    const nbody::Diagnostics d = runner.diagnostics(potential);
    std::printf("Diagnostics: step %llu kinetic %.9e potential %.9e total %.9e momentum %.9e %.9e %.9e "
                "angular_momentum %.9e %.9e %.9e\n",
                (unsigned long long)d.step_num, d.kinetic, d.potential, d.total, d.momentum[0], d.momentum[1],
                d.momentum[2], d.angular_momentum[0], d.angular_momentum[1], d.angular_momentum[2]);
}

struct FrameOptions {
    std::string dir;
    int every = 1;
    uint32_t width = 1280, height = 720;
};

template <class Sim>
static bool write_frame(nbody::OfflineHeadless<Sim> &runner, const FrameOptions &fo) {
    const nbody::Frame f = runner.render(nbody::default_render_params(fo.width, fo.height));
    char name[64];
    std::snprintf(name, sizeof name, "/frame_%06llu.ppm", (unsigned long long)f.stats.step_num);
    const std::string path = fo.dir + name;
    std::FILE *out = std::fopen(path.c_str(), "wb");
    if (!out) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    std::vector<uint8_t> rgb((size_t)f.width * f.height * 3);
    for (size_t p = 0; p < (size_t)f.width * f.height; ++p)
        for (int c = 0; c < 3; ++c) rgb[3 * p + c] = f.rgba[4 * p + c];
    const bool ok = std::fprintf(out, "P6\n%u %u\n255\n", f.width, f.height) > 0 &&
                    std::fwrite(rgb.data(), 1, rgb.size(), out) == rgb.size();
    if (std::fclose(out) != 0 || !ok) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    std::printf("Frame %llu: drawn %llu clipped %llu oversize %llu nonfinite %llu fragments %llu max_count %u\n",
                (unsigned long long)f.stats.step_num, (unsigned long long)f.stats.drawn,
                (unsigned long long)f.stats.clipped, (unsigned long long)f.stats.oversize,
                (unsigned long long)f.stats.nonfinite, (unsigned long long)f.stats.fragments, f.stats.max_count);
    return true;
}

template <class Sim>
static int run(const nbody::SimParams &sp, const nbody::AddParams &ap, const nbody::InitFn &init,
               int steps, int device, const std::vector<int> &devices, const std::string &dump, int let,
               int diag, bool diag_potential, const FrameOptions &frames) {
    std::puts("Initializing Simulation");
    nbody::OfflineHeadless<Sim> runner = devices.empty() ? nbody::OfflineHeadless<Sim>(sp, ap, init, device)
                                                         : nbody::OfflineHeadless<Sim>(sp, ap, init, devices, let);
    std::puts("Running Simulation");
    if (diag > 0) print_diag(runner, diag_potential);
    if (!frames.dir.empty() && !write_frame(runner, frames)) return 1;
    for (int i = 0; i < steps; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        runner.step();
        const auto us = std::chrono::duration_cast<std::chrono::microseconds>(
                            std::chrono::steady_clock::now() - t0).count();
        std::printf("Step Duration: %lld \xC2\xB5s\n", (long long)us);
        if (diag > 0 && (i + 1) % diag == 0) print_diag(runner, diag_potential);
        if (!frames.dir.empty() && (i + 1) % frames.every == 0 && !write_frame(runner, frames)) return 1;
    }
    std::puts("Finished Running");
    if (!dump.empty()) {
        const std::vector<nbody::Particle> parts = runner.read_particles();
        if (!write_snapshot(dump, sp, parts, runner.step_num())) {
            std::fprintf(stderr, "cannot write %s\n", dump.c_str());
            return 1;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    std::string sim = "tree", init = "uniform", dump;
    std::vector<int> devices;
    nbody::SimParams sp{4000000u, 0.000001f, 0.0001f, 0.016f};  // headless.rs:15-20
    float theta = 0.75f;
    int steps = 10, device = -1, let = -1, diag = 0;
    bool diag_potential = false;
    FrameOptions frames;
    uint64_t seed = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i], v = argv[i + 1];
        if (k == "--sim") sim = v;
        else if (k == "--n") sp.particle_num = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--steps") steps = std::atoi(v.c_str());
        else if (k == "--theta") theta = (float)std::atof(v.c_str());
        else if (k == "--init") init = v;
        else if (k == "--seed") seed = std::strtoull(v.c_str(), nullptr, 10);
        else if (k == "--device") device = std::atoi(v.c_str());
        else if (k == "--g") sp.g = (float)std::atof(v.c_str());
        else if (k == "--e") sp.e = (float)std::atof(v.c_str());
        else if (k == "--dt") sp.dt = (float)std::atof(v.c_str());
        else if (k == "--dump") dump = v;
        else if (k == "--let") let = std::atoi(v.c_str());  // with --devices and --sim tree: LET scheme, migrate every k-th step
        else if (k == "--diag") diag = std::atoi(v.c_str());
        else if (k == "--diag-potential") diag_potential = std::atoi(v.c_str()) != 0;
        else if (k == "--frames") frames.dir = v;
        else if (k == "--frame-every") frames.every = std::max(1, std::atoi(v.c_str()));
        else if (k == "--frame-size") {
            unsigned w = 0, h = 0;
            if (std::sscanf(v.c_str(), "%ux%u", &w, &h) != 2) {
                std::fprintf(stderr, "--frame-size takes WxH, not %s\n", v.c_str());
                return 2;
            }
            frames.width = w;
            frames.height = h;
        }
        else if (k == "--devices") {
            for (size_t a = 0; a <= v.size();) {
                const size_t b = std::min(v.find(',', a), v.size());
                devices.push_back(std::atoi(v.substr(a, b - a).c_str()));
                a = b + 1;
            }
        }
        else { std::fprintf(stderr, "unknown option %s\n", k.c_str()); return 2; }
    }
    const nbody::InitFn fn = init == "disc" ? nbody::inits::disc_init(seed)
                           : init == "spherical" ? nbody::inits::spherical_init(seed)
                                                 : nbody::inits::uniform_init(seed);
    try {
        if (sim == "naive")
            return run<nbody::NaiveSim>(sp, nbody::AddParams::NaiveSimParams(), fn, steps, device, devices, dump, -1, diag,
                                        diag_potential, frames);
        return run<nbody::TreeSim>(sp, nbody::AddParams::TreeSimParams(theta), fn, steps, device, devices, dump, let,
                                       diag, diag_potential, frames);
    } catch (const nbody::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
