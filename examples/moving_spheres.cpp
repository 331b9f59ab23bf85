// moving_spheres.cpp -- an animation on a resident scene: 10 000 spheres placed as the C2 benchmark scene places them, every one
// on a small orbit of its own; per frame ONE rtx_scene_update_objects (the spheres are refitted into the resident tree on the
// device, no host build, no re-upload) and one render, through the C++ host API (include/rtx.hpp).  The frames land in device
// memory; the last one is copied back and written as raw f64.  Usage: moving_spheres W H SPP [N_FRAMES = 30] [out.f64]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "rtx.hpp"

using namespace rtx;
using rtx::object::Material;
using rtx::object::Object;
using rtx::object::sphere::Sphere;

namespace {
struct Rng {                                              // SplitMix64
    std::uint64_t s;
    double next()
    {
        std::uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
    }
};
struct Ball { Vector3 c; double r, orbit, phase; Material m; };
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s W H SPP [N_FRAMES] [out.f64]\n", argv[0]); return 2; }
    const std::size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    const std::size_t spp = std::strtoul(argv[3], nullptr, 10), frames = argc > 4 ? std::strtoul(argv[4], nullptr, 10) : 30;
    const double pi = std::acos(-1.0);
    try {
        Rng rng{1};
        std::vector<Ball> balls;
        Scene scene(Config().with_rays_per_pixel(spp), Camera(Vector3(0, 0, 0), Vector3(1, 0, 0), pi / 2));
        for (int k = 0; k < 10000; ++k) {
            Ball b{Vector3(10.0 + 100.0 * rng.next(), -50.0 + 100.0 * rng.next(), -50.0 + 100.0 * rng.next()), 0.2 + 0.8 * rng.next(),
                   0.5 + 1.5 * rng.next(), 2.0 * pi * rng.next(), Material::colored(Vector3(0.2 + 0.7 * rng.next(), 0.2 + 0.7 * rng.next(), 0.2 + 0.7 * rng.next()))};
            if (k % 20 == 0) b.m = Material::light(Vector3(2.0, 2.0, 1.6));
            balls.push_back(b);
            scene.add_object(Object(Sphere(b.c, b.r), b.m));
        }
        Scene::Resident resident = scene.upload(0);

        double *d_frame = nullptr;
        const std::size_t n = w * h * 3;
        if (hipMalloc((void **)&d_frame, n * sizeof(double)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 3; }
        std::vector<std::uint64_t> indices(balls.size());
        for (std::size_t k = 0; k < balls.size(); ++k) indices[k] = k;
        std::vector<Object> moved;
        double update_ms = 0.0, render_ms = 0.0;
        unsigned refits = 0;
        for (std::size_t f = 0; f < frames; ++f) {
            const double t = 2.0 * pi * (double)(f + 1) / (double)(frames ? frames : 1);
            moved.clear();
            for (const Ball &b : balls)                    // a circle in the (y, z) plane around the sphere's first position
                moved.push_back(Object(Sphere(Vector3(b.c.x, b.c.y + b.orbit * (std::cos(t + b.phase) - std::cos(b.phase)),
                                                      b.c.z + b.orbit * (std::sin(t + b.phase) - std::sin(b.phase))), b.r), b.m));
            const auto t0 = std::chrono::steady_clock::now();
            refits += resident.update_objects(indices, moved) == RTX_UPDATED_REFIT ? 1u : 0u;
            const auto t1 = std::chrono::steady_clock::now();
            resident.render(w, h, d_frame);
            const auto t2 = std::chrono::steady_clock::now();
            update_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
            render_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
        }
        std::printf("%zu frames of %zu x %zu x %zu spp: %u refits, update %.3f ms and render %.3f ms per frame\n", frames, w, h, spp, refits,
                    update_ms / (double)(frames ? frames : 1), render_ms / (double)(frames ? frames : 1));
        if (argc > 5) {
            std::vector<double> frame(n);
            if (hipMemcpy(frame.data(), d_frame, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 4;
            std::FILE *out = std::fopen(argv[5], "wb");
            if (!out) return 3;
            std::fwrite(frame.data(), sizeof(double), n, out);
            std::fclose(out);
        }
        (void)hipFree(d_frame);
    } catch (const rtx::Panic &p) {
        std::fprintf(stderr, "rtx panic (status %d): %s\n", (int)p.status, p.what());
        return 1;
    }
    return 0;
}
