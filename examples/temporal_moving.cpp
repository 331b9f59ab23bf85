// temporal_moving.cpp -- moving objects over a few low-sample frames with temporal accumulation that KEEPS their history, on the device,
// through the C++ host API (include/rtx.hpp).  The camera stands still; three spheres each run on a small orbit of their own in the
// (y, z) plane (the motion of moving_spheres.cpp).  Per frame: one Resident::update_objects, SPP new samples of every pixel into fresh
// sums (render_blocks_accumulate, samples [k SPP, (k + 1) SPP)), the pick buffer (primary_hits), rtx::object_motions of what the update
// was given, Resident::rewind_hits -- the pick with every hit on a moved sphere put back onto the sphere's previous position -- and
// Resident::temporal_accumulate on the REWOUND pick, so a moved sphere's pixels find their history; the unrewound pick is the next
// frame's history.  The last frame then goes through the guides (pixel_features), the denoiser (Resident::denoise) and
// render_to_image's quantisation (rtx_quantize_image_device).  Writes the last frame as a binary PPM and, when asked, the accumulated
// mean, its history length and the denoised frame as raw f64.
// Usage: temporal_moving W H out.ppm [N_FRAMES [SPP [out.f64]]]   (default 4 frames at 4 spp)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "rtx.hpp"

using namespace rtx;
using rtx::object::Material;
using rtx::object::Object;
using rtx::object::sphere::Sphere;
using rtx::object::triangle::Triangle;

#define HIP_OK(expr) do { if ((expr) != hipSuccess) { std::fprintf(stderr, "%s failed\n", #expr); return 3; } } while (0)

struct FrameBuffers { double *rgb = nullptr, *var = nullptr, *len = nullptr; RtxHit *hits = nullptr; };
struct Ball { std::uint64_t index; Vector3 c; double r, orbit, phase; Material m; };

// frame k's position of a ball: a circle in the (y, z) plane through its first position, 0.05 rad per frame
static Object ball_at(const Ball &b, std::size_t k)
{
    const double t = 0.05 * (double)k;
    return Object(Sphere(Vector3(b.c.x, b.c.y + b.orbit * (std::cos(t + b.phase) - std::cos(b.phase)),
                                 b.c.z + b.orbit * (std::sin(t + b.phase) - std::sin(b.phase))), b.r), b.m);
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s W H out.ppm [N_FRAMES [SPP [out.f64]]]\n", argv[0]); return 2; }
    const std::size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    const std::size_t frames = argc > 4 ? std::strtoul(argv[4], nullptr, 10) : 4, spp = argc > 5 ? std::strtoul(argv[5], nullptr, 10) : 4;
    if (w == 0 || h == 0 || frames == 0 || spp < 2) return 2;
    const double fov = std::acos(-1.0) / 2;
    try {
        Config config;
        config.rays_per_pixel = spp;                       // the guides are taken over a frame's own rays
        Scene scene(config, Camera(Vector3(0, 0, 0), Vector3(1, 0, 0), fov));
        scene.add_object(Object(Sphere(Vector3(6, 0, 8), 5), Material::light(Vector3(1, 1, 1))));
        scene.add_object(Object(Sphere(Vector3(6, -1.2, 0), 1), Material::colored(Vector3(0.8, 0.2, 0.2))));
        scene.add_object(Object(Sphere(Vector3(7, 1.6, 0.3), 1.5), Material(Vector3(0.9, 0.9, 0.9), Vector3::zeros(), 0.1)));
        scene.add_object(Object(Sphere(Vector3(5, -3, 2), 0.6), Material::light(Vector3(0.9, 0.6, 0.2))));
        scene.add_object(Object(Triangle({Vector3(-8, -8, -1.5), Vector3(30, -8, -1.5), Vector3(8, 20, -1.5)}), Material::colored(Vector3(0.6, 0.6, 0.6))));
        const std::vector<Ball> balls = {
            {1, Vector3(6, -1.2, 0), 1, 0.8, 0.3, Material::colored(Vector3(0.8, 0.2, 0.2))},
            {2, Vector3(7, 1.6, 0.3), 1.5, 0.5, 2.0, Material(Vector3(0.9, 0.9, 0.9), Vector3::zeros(), 0.1)},
            {3, Vector3(5, -3, 2), 0.6, 0.6, 4.0, Material::light(Vector3(0.9, 0.6, 0.2))}};
        std::vector<std::uint64_t> indices;
        for (const Ball &b : balls) indices.push_back(b.index);
        Scene::Resident resident = scene.upload(0);

        const std::size_t n = w * h, frame_bytes = 3 * n * sizeof(double);
        const RtxTemporalParams tparams = temporal_default_params();
        const RtxDenoiseParams dparams = denoise_default_params();
        const std::uint64_t work_bytes = denoise_work_bytes(w, h, dparams);
        double *d_sum = nullptr, *d_sq = nullptr, *d_tables = nullptr, *d_out = nullptr;
        FrameBuffers buf[2];                               // the history's two sets, used in turn
        RtxPixelFeatures *d_features = nullptr;
        void *d_work = nullptr;
        RtxHit *d_rewound = nullptr;
        std::int64_t *d_objects = nullptr;
        RtxObjectMotion *d_motions = nullptr;
        uint8_t *d_rgb8 = nullptr;
        HIP_OK(hipMalloc((void **)&d_sum, frame_bytes));
        HIP_OK(hipMalloc((void **)&d_sq, frame_bytes));
        HIP_OK(hipMalloc((void **)&d_out, frame_bytes));
        HIP_OK(hipMalloc((void **)&d_tables, (w + h + 2) * sizeof(double)));
        for (FrameBuffers &b : buf) {
            HIP_OK(hipMalloc((void **)&b.rgb, frame_bytes));
            HIP_OK(hipMalloc((void **)&b.var, frame_bytes));
            HIP_OK(hipMalloc((void **)&b.len, n * sizeof(double)));
            HIP_OK(hipMalloc((void **)&b.hits, n * sizeof(RtxHit)));
        }
        HIP_OK(hipMalloc((void **)&d_features, n * sizeof(RtxPixelFeatures)));
        HIP_OK(hipMalloc(&d_work, work_bytes));
        HIP_OK(hipMalloc((void **)&d_rewound, n * sizeof(RtxHit)));
        HIP_OK(hipMalloc((void **)&d_objects, balls.size() * sizeof(std::int64_t)));
        HIP_OK(hipMalloc((void **)&d_motions, balls.size() * sizeof(RtxObjectMotion)));
        HIP_OK(hipMalloc((void **)&d_rgb8, 3 * n));
        const std::vector<double> tables = temporal_tables(fov, w, h);          // one fov, one size: uploaded once
        HIP_OK(hipMemcpy(d_tables, tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice));

        std::vector<double> sum(3 * n), sq(3 * n);
        const RtxCamera prev_camera = Camera(Vector3(0, 0, 0), Vector3(1, 0, 0), fov).to_c();          // the camera stands still
        std::vector<Object> before, moved;
        for (const Ball &b : balls) before.push_back(ball_at(b, 0));
        const double ns = (double)spp;
        for (std::size_t k = 0; k < frames; ++k) {
            const RtxHit *seen = nullptr;                    // what the accumulation reads as this frame's pick
            if (k > 0) {
                moved.clear();
                for (const Ball &b : balls) moved.push_back(ball_at(b, k));
                resident.update_objects(indices, moved);
            }
            FrameBuffers &now = buf[k & 1], &last = buf[(k & 1) ^ 1];
            HIP_OK(hipMemset(d_sum, 0, frame_bytes));
            HIP_OK(hipMemset(d_sq, 0, frame_bytes));
            RtxStats st{};
            resident.render_blocks_accumulate(w, h, 8, 0, 1, k * spp, spp, d_sum, d_sq, nullptr, &st);          // (with stats: synchronous)
            resident.primary_hits(w, h, now.hits);
            seen = now.hits;
            if (k > 0) {
                const ObjectMotions motions = object_motions(indices, before, moved);
                if (!motions.objects.empty()) {
                    HIP_OK(hipMemcpy(d_objects, motions.objects.data(), motions.objects.size() * sizeof(std::int64_t), hipMemcpyHostToDevice));
                    HIP_OK(hipMemcpy(d_motions, motions.motions.data(), motions.motions.size() * sizeof(RtxObjectMotion), hipMemcpyHostToDevice));
                    resident.rewind_hits(now.hits, n, d_objects, d_motions, motions.objects.size(), d_rewound);
                    seen = d_rewound;
                }
                before = moved;
            }
            // the mean and the variance of the mean, (sum_sq - sum^2 / n) / (n - 1) / n: plain f64 arithmetic on the two sums
            HIP_OK(hipMemcpy(sum.data(), d_sum, frame_bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(sq.data(), d_sq, frame_bytes, hipMemcpyDeviceToHost));
            for (std::size_t i = 0; i < 3 * n; ++i) {
                const double s = sum[i];
                sum[i] = s / ns;
                sq[i] = (sq[i] - s * s / ns) / (ns - 1.0) / ns;
            }
            HIP_OK(hipMemcpy(d_sum, sum.data(), frame_bytes, hipMemcpyHostToDevice));                      // now the frame's mean ...
            HIP_OK(hipMemcpy(d_sq, sq.data(), frame_bytes, hipMemcpyHostToDevice));                        // ... and its variance
            if (k == 0)
                resident.temporal_accumulate(w, h, d_sum, d_sq, seen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tparams,
                                             now.rgb, now.var, now.len);
            else
                resident.temporal_accumulate(w, h, d_sum, d_sq, seen, last.rgb, last.var, last.len, last.hits, &prev_camera,
                                             d_tables, tparams, now.rgb, now.var, now.len);
            HIP_OK(hipDeviceSynchronize());
        }
        const FrameBuffers &last = buf[(frames - 1) & 1];
        resident.pixel_features(w, h, d_features);
        resident.denoise(w, h, last.rgb, last.var, d_features, dparams, d_out, nullptr, d_work);
        if (rtx_quantize_image_device(d_out, (uint32_t)w, (uint32_t)h, d_rgb8, 0, nullptr) != RTX_OK) {
            std::fprintf(stderr, "rtx_quantize_image_device: %s\n", rtx_last_error());
            return 1;
        }
        HIP_OK(hipDeviceSynchronize());
        std::vector<uint8_t> rgb8(3 * n);
        std::vector<double> acc(3 * n), len(n), out(3 * n);
        HIP_OK(hipMemcpy(rgb8.data(), d_rgb8, 3 * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(acc.data(), last.rgb, frame_bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(len.data(), last.len, n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out.data(), d_out, frame_bytes, hipMemcpyDeviceToHost));
        for (FrameBuffers &b : buf) { (void)hipFree(b.rgb); (void)hipFree(b.var); (void)hipFree(b.len); (void)hipFree(b.hits); }
        (void)hipFree(d_sum); (void)hipFree(d_sq); (void)hipFree(d_out); (void)hipFree(d_tables); (void)hipFree(d_features);
        (void)hipFree(d_work); (void)hipFree(d_rgb8); (void)hipFree(d_rewound); (void)hipFree(d_objects); (void)hipFree(d_motions);
        std::FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 3;
        std::fprintf(f, "P6\n%zu %zu\n255\n", w, h);
        std::fwrite(rgb8.data(), 1, rgb8.size(), f);
        std::fclose(f);
        if (argc > 6) {                                    // [accumulated mean][history length][denoised]
            f = std::fopen(argv[6], "wb");
            if (!f) return 3;
            std::fwrite(acc.data(), sizeof(double), acc.size(), f);
            std::fwrite(len.data(), sizeof(double), len.size(), f);
            std::fwrite(out.data(), sizeof(double), out.size(), f);
            std::fclose(f);
        }
        double mean_len = 0.0;
        for (double l : len) mean_len += l;
        std::printf("temporal_moving %zux%zu: %zu frames at %zu spp; mean history length %.2f of %zu\n", w, h, frames, spp,
                    mean_len / (double)n, frames);
    } catch (const rtx::Panic &p) {
        std::fprintf(stderr, "rtx panic (status %d): %s\n", (int)p.status, p.what());
        return 1;
    }
    return 0;
}
