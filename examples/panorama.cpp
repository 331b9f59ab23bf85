// panorama.cpp -- an equirectangular 360-degree frame of a resident scene: a camera the reference's angular projection cannot
// express, through the path queries of the C++ host API (Scene::Resident::trace_paths, include/rtx.hpp).  Pixel (x, y) looks along
// longitude 2 pi (x + 0.5) / W - pi and latitude pi / 2 - pi (y + 0.5) / H from the eye; sample s of pixel p draws as the id pair
// (p, s), and the samples are folded as a render folds them: summed in sample order, divided by SPP.  The frame is written as raw f64
// [H][W][3].  Usage: panorama W H SPP out.f64
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
using rtx::object::triangle::Triangle;

int main(int argc, char **argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: %s W H SPP out.f64\n", argv[0]); return 2; }
    const std::size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    const std::size_t spp = std::strtoul(argv[3], nullptr, 10);
    const double pi = std::acos(-1.0);
    if (w == 0 || h == 0 || spp == 0) return 2;
    try {
        // the eye sits between the objects: every direction of the sphere sees something different
        Scene scene(Config().with_rays_per_pixel(spp), Camera(Vector3(0, 0, 0), Vector3(1, 0, 0), pi / 2));
        scene.add_object(Object(Sphere(Vector3(6, 0, 8), 5), Material::light(Vector3(1, 1, 1))));
        scene.add_object(Object(Sphere(Vector3(6, -1.2, 0), 1), Material::colored(Vector3(0.8, 0.2, 0.2))));
        scene.add_object(Object(Sphere(Vector3(-5, 1.2, 0), 1.5), Material(Vector3(0.9, 0.9, 0.9), Vector3::zeros(), 0.1)));
        scene.add_object(Object(Sphere(Vector3(0, -7, -1), 2), Material::light(Vector3(0.9, 0.6, 0.2))));
        scene.add_object(Object(Triangle({Vector3(-3, 4, -2), Vector3(3, 4, -2), Vector3(0, 4, 3)}), Material::colored(Vector3(0.2, 0.6, 0.9))));
        scene.add_object(Object(Triangle({Vector3(-8, -8, -3), Vector3(8, -8, -3), Vector3(0, 8, -3)}), Material::colored(Vector3(0.6, 0.6, 0.6))));
        Scene::Resident resident = scene.upload(0);

        // one sample of the whole frame per launch: entry p is pixel p, its ids (p, s)
        const std::size_t n = w * h;
        std::vector<RtxRay> rays(n);
        std::vector<uint64_t> ids(2 * n);
        for (std::size_t y = 0; y < h; ++y)
            for (std::size_t x = 0; x < w; ++x) {
                const double lon = 2.0 * pi * ((double)x + 0.5) / (double)w - pi, lat = pi / 2 - pi * ((double)y + 0.5) / (double)h;
                Vector3 d(std::cos(lat) * std::cos(lon), std::cos(lat) * std::sin(lon), std::sin(lat));
                const double len = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);      // (unit to the last bit: the ray walks the tree)
                d = Vector3(d.x / len, d.y / len, d.z / len);
                RtxRay &r = rays[y * w + x];
                r.position[0] = r.position[1] = r.position[2] = 0.0;
                r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z;
                ids[2 * (y * w + x)] = y * w + x;
            }
        RtxRay *d_rays = nullptr;
        uint64_t *d_ids = nullptr;
        double *d_rgb = nullptr;
        if (hipMalloc((void **)&d_rays, n * sizeof(RtxRay)) != hipSuccess || hipMalloc((void **)&d_ids, 2 * n * sizeof(uint64_t)) != hipSuccess ||
            hipMalloc((void **)&d_rgb, 3 * n * sizeof(double)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 3; }
        if (hipMemcpy(d_rays, rays.data(), n * sizeof(RtxRay), hipMemcpyHostToDevice) != hipSuccess) return 4;
        std::vector<double> frame(3 * n, 0.0), sample(3 * n);
        unsigned long long segments = 0;
        for (std::size_t s = 0; s < spp; ++s) {
            for (std::size_t p = 0; p < n; ++p) ids[2 * p + 1] = s;
            if (hipMemcpy(d_ids, ids.data(), 2 * n * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return 4;
            RtxStats st{};
            resident.trace_paths(d_rays, d_ids, n, d_rgb, nullptr, nullptr, &st);       // (with stats: synchronous)
            segments += st.segments;
            if (hipMemcpy(sample.data(), d_rgb, 3 * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 4;
            for (std::size_t k = 0; k < 3 * n; ++k) frame[k] = frame[k] + sample[k];
        }
        for (std::size_t k = 0; k < 3 * n; ++k) frame[k] = frame[k] / (double)spp;
        (void)hipFree(d_rays); (void)hipFree(d_ids); (void)hipFree(d_rgb);
        std::FILE *f = std::fopen(argv[4], "wb");
        if (!f) return 3;
        std::fwrite(frame.data(), sizeof(double), frame.size(), f);
        std::fclose(f);
        std::printf("panorama %zux%zu, %zu spp: %llu segments\n", w, h, spp, segments);
    } catch (const rtx::Panic &p) {
        std::fprintf(stderr, "rtx panic (status %d): %s\n", (int)p.status, p.what());
        return 1;
    }
    return 0;
}
