// adaptive.cpp -- adaptive sampling of a resident scene through the C++ host API (Scene::Resident::render_blocks_accumulate and trace_samples,
// include/rtx.hpp): BASE samples of every pixel, then up to MAX on the tenth of the pixels whose mean has the largest estimated
// variance.  Every sample is the render's own -- sample s of pixel p whichever call traced it -- so a refined pixel's mean is the
// MAX-spp render's pixel and every other one the BASE-spp render's, bit for bit.  Prints the samples traced against a uniform MAX-spp
// frame and writes the means as raw f64 [H][W][3].  Usage: adaptive W H out.f64 [BASE MAX]   (default 8 64)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
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
    if (argc < 4) { std::fprintf(stderr, "usage: %s W H out.f64 [BASE MAX]\n", argv[0]); return 2; }
    const std::size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    const std::size_t base = argc > 4 ? std::strtoul(argv[4], nullptr, 10) : 8, top = argc > 5 ? std::strtoul(argv[5], nullptr, 10) : 64;
    if (w == 0 || h == 0 || base < 2 || top < base) return 2;
    const double pi = std::acos(-1.0);
    try {
        Scene scene(Config(), Camera(Vector3(0, 0, 0), Vector3(1, 0, 0), pi / 2));
        scene.add_object(Object(Sphere(Vector3(6, 0, 8), 5), Material::light(Vector3(1, 1, 1))));
        scene.add_object(Object(Sphere(Vector3(6, -1.2, 0), 1), Material::colored(Vector3(0.8, 0.2, 0.2))));
        scene.add_object(Object(Sphere(Vector3(7, 1.6, 0.3), 1.5), Material(Vector3(0.9, 0.9, 0.9), Vector3::zeros(), 0.1)));
        scene.add_object(Object(Sphere(Vector3(5, -3, 2), 0.6), Material::light(Vector3(0.9, 0.6, 0.2))));
        scene.add_object(Object(Triangle({Vector3(-8, -8, -1.5), Vector3(30, -8, -1.5), Vector3(8, 20, -1.5)}), Material::colored(Vector3(0.6, 0.6, 0.6))));
        Scene::Resident resident = scene.upload(0);

        const std::size_t n = w * h;
        double *d_sum = nullptr, *d_sq = nullptr;
        if (hipMalloc((void **)&d_sum, 3 * n * sizeof(double)) != hipSuccess || hipMalloc((void **)&d_sq, 3 * n * sizeof(double)) != hipSuccess ||
            hipMemset(d_sum, 0, 3 * n * sizeof(double)) != hipSuccess || hipMemset(d_sq, 0, 3 * n * sizeof(double)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 3;
        }
        // BASE samples everywhere: the running sums of the samples and of their squares
        RtxStats st{};
        resident.render_blocks_accumulate(w, h, 8, 0, 1, 0, base, d_sum, d_sq, nullptr, &st);      // the full frame (with stats: synchronous)
        unsigned long long traced = st.primary_rays;
        std::vector<double> sum(3 * n), sq(3 * n);
        if (hipMemcpy(sum.data(), d_sum, 3 * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(sq.data(), d_sq, 3 * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 4;
        // the variance of each pixel's mean, summed over the channels: (sum_sq - sum^2 / n) / (n - 1) / n
        std::vector<double> var(n, 0.0);
        const double nb = (double)base;
        for (std::size_t p = 0; p < n; ++p)
            for (int c = 0; c < 3; ++c) var[p] += (sq[3 * p + c] - sum[3 * p + c] * sum[3 * p + c] / nb) / (nb - 1.0) / nb;
        std::vector<std::size_t> order(n);
        std::iota(order.begin(), order.end(), (std::size_t)0);
        const std::size_t chosen = n / 10;
        std::partial_sort(order.begin(), order.begin() + chosen, order.end(),
                          [&](std::size_t a, std::size_t b) { return var[a] > var[b] || (var[a] == var[b] && a < b); });
        std::vector<uint64_t> count(n, base);
        const std::size_t extra = top - base, m = chosen * extra;
        if (m != 0) {
            // the samples BASE .. MAX - 1 of the chosen pixels, sample-major, in one launch
            std::vector<uint64_t> ids(2 * m);
            for (std::size_t s = 0; s < extra; ++s)
                for (std::size_t k = 0; k < chosen; ++k) { ids[2 * (s * chosen + k)] = order[k]; ids[2 * (s * chosen + k) + 1] = base + s; }
            uint64_t *d_ids = nullptr;
            double *d_rgb = nullptr;
            if (hipMalloc((void **)&d_ids, 2 * m * sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&d_rgb, 3 * m * sizeof(double)) != hipSuccess ||
                hipMemcpy(d_ids, ids.data(), 2 * m * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return 4;
            resident.trace_samples(w, h, d_ids, m, d_rgb, nullptr, nullptr, &st);
            traced += st.primary_rays;
            std::vector<double> rgb(3 * m);
            if (hipMemcpy(rgb.data(), d_rgb, 3 * m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 4;
            for (std::size_t s = 0; s < extra; ++s)                                      // a pixel's samples in sample order: the render's fold
                for (std::size_t k = 0; k < chosen; ++k)
                    for (int c = 0; c < 3; ++c) sum[3 * order[k] + c] = sum[3 * order[k] + c] + rgb[3 * (s * chosen + k) + c];
            for (std::size_t k = 0; k < chosen; ++k) count[order[k]] = top;
            (void)hipFree(d_ids); (void)hipFree(d_rgb);
        }
        (void)hipFree(d_sum); (void)hipFree(d_sq);
        std::vector<double> frame(3 * n);
        for (std::size_t p = 0; p < n; ++p)
            for (int c = 0; c < 3; ++c) frame[3 * p + c] = sum[3 * p + c] / (double)count[p];
        std::FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 3;
        std::fwrite(frame.data(), sizeof(double), frame.size(), f);
        std::fclose(f);
        const unsigned long long uniform = (unsigned long long)n * top;
        std::printf("adaptive %zux%zu: %zu spp everywhere, %zu spp on %zu pixels: %llu samples traced, %llu for a uniform %zu-spp frame (%.1f %%)\n",
                    w, h, base, top, chosen, traced, uniform, top, 100.0 * (double)traced / (double)uniform);
    } catch (const rtx::Panic &p) {
        std::fprintf(stderr, "rtx panic (status %d): %s\n", (int)p.status, p.what());
        return 1;
    }
    return 0;
}
