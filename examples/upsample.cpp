// upsample.cpp -- a frame rendered at half the display resolution, denoised there and reconstructed at full resolution, on the device,
// through the C++ host API (include/rtx.hpp): SPP samples of every LOW pixel into running sums (Resident::render_blocks_accumulate),
// the guide buffers at both sizes (pixel_features), the a-trous filter on the low frame (Resident::denoise), the guided upsampling x2
// with the library's default parameters (Resident::upsample), then render_to_image's quantisation (rtx_quantize_image_device).
// Writes the W x H frame as a binary PPM and, when asked, as raw f64 [H][W][3].
// Usage: upsample W H out.ppm [SPP [out.f64]]   (W and H even: the output size; default 8 spp)
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

#define HIP_OK(expr) do { if ((expr) != hipSuccess) { std::fprintf(stderr, "%s failed\n", #expr); return 3; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s W H out.ppm [SPP [out.f64]]\n", argv[0]); return 2; }
    const std::size_t w = std::strtoul(argv[1], nullptr, 10), h = std::strtoul(argv[2], nullptr, 10);
    const std::size_t spp = argc > 4 ? std::strtoul(argv[4], nullptr, 10) : 8;
    RtxUpsampleParams up = upsample_default_params();
    up.factor = 2;
    if (w == 0 || h == 0 || w % up.factor || h % up.factor || spp < 2) return 2;
    const std::size_t wl = w / up.factor, hl = h / up.factor;
    const double pi = std::acos(-1.0);
    try {
        Config config;
        config.rays_per_pixel = spp;                       // the guides are taken over as many lens-jittered rays as the frame's
        Scene scene(config, Camera(Vector3(0, 0, 0), Vector3(1, 0, 0), pi / 2));
        scene.add_object(Object(Sphere(Vector3(6, 0, 8), 5), Material::light(Vector3(1, 1, 1))));
        scene.add_object(Object(Sphere(Vector3(6, -1.2, 0), 1), Material::colored(Vector3(0.8, 0.2, 0.2))));
        scene.add_object(Object(Sphere(Vector3(7, 1.6, 0.3), 1.5), Material(Vector3(0.9, 0.9, 0.9), Vector3::zeros(), 0.1)));
        scene.add_object(Object(Sphere(Vector3(5, -3, 2), 0.6), Material::light(Vector3(0.9, 0.6, 0.2))));
        scene.add_object(Object(Triangle({Vector3(-8, -8, -1.5), Vector3(30, -8, -1.5), Vector3(8, 20, -1.5)}), Material::colored(Vector3(0.6, 0.6, 0.6))));
        Scene::Resident resident = scene.upload(0);

        const std::size_t n = w * h, nl = wl * hl, lo_bytes = 3 * nl * sizeof(double), frame_bytes = 3 * n * sizeof(double);
        const RtxDenoiseParams dn = denoise_default_params();
        const std::uint64_t work_bytes = denoise_work_bytes(wl, hl, dn);
        double *d_sum = nullptr, *d_sq = nullptr, *d_lo = nullptr, *d_out = nullptr;
        RtxPixelFeatures *d_lo_features = nullptr, *d_features = nullptr;
        void *d_work = nullptr;
        uint8_t *d_rgb8 = nullptr;
        HIP_OK(hipMalloc((void **)&d_sum, lo_bytes));
        HIP_OK(hipMalloc((void **)&d_sq, lo_bytes));
        HIP_OK(hipMalloc((void **)&d_lo, lo_bytes));
        HIP_OK(hipMalloc((void **)&d_out, frame_bytes));
        HIP_OK(hipMalloc((void **)&d_lo_features, nl * sizeof(RtxPixelFeatures)));
        HIP_OK(hipMalloc((void **)&d_features, n * sizeof(RtxPixelFeatures)));
        HIP_OK(hipMalloc(&d_work, work_bytes));
        HIP_OK(hipMalloc((void **)&d_rgb8, 3 * n));
        HIP_OK(hipMemset(d_sum, 0, lo_bytes));
        HIP_OK(hipMemset(d_sq, 0, lo_bytes));
        // SPP samples of every low pixel, then the guides of the low and of the output frame (first hits only: no paths)
        RtxStats st{};
        resident.render_blocks_accumulate(wl, hl, 8, 0, 1, 0, spp, d_sum, d_sq, nullptr, &st);        // (with stats: synchronous)
        resident.pixel_features(wl, hl, d_lo_features);
        resident.pixel_features(w, h, d_features);
        // the mean and the variance of the mean, (sum_sq - sum^2 / n) / (n - 1) / n: plain f64 arithmetic on the two sums
        std::vector<double> sum(3 * nl), sq(3 * nl);
        HIP_OK(hipMemcpy(sum.data(), d_sum, lo_bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(sq.data(), d_sq, lo_bytes, hipMemcpyDeviceToHost));
        const double ns = (double)spp;
        for (std::size_t i = 0; i < 3 * nl; ++i) {
            const double s = sum[i];
            sum[i] = s / ns;
            sq[i] = (sq[i] - s * s / ns) / (ns - 1.0) / ns;
        }
        HIP_OK(hipMemcpy(d_sum, sum.data(), lo_bytes, hipMemcpyHostToDevice));                         // now the mean ...
        HIP_OK(hipMemcpy(d_sq, sq.data(), lo_bytes, hipMemcpyHostToDevice));                           // ... and its variance
        resident.denoise(wl, hl, d_sum, d_sq, d_lo_features, dn, d_lo, nullptr, d_work);
        resident.upsample(w, h, d_lo, nullptr, d_lo_features, d_features, up, d_out, nullptr);
        if (rtx_quantize_image_device(d_out, (uint32_t)w, (uint32_t)h, d_rgb8, 0, nullptr) != RTX_OK) {
            std::fprintf(stderr, "rtx_quantize_image_device: %s\n", rtx_last_error());
            return 1;
        }
        HIP_OK(hipDeviceSynchronize());
        std::vector<uint8_t> rgb8(3 * n);
        std::vector<double> out(3 * n);
        HIP_OK(hipMemcpy(rgb8.data(), d_rgb8, 3 * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out.data(), d_out, frame_bytes, hipMemcpyDeviceToHost));
        (void)hipFree(d_sum); (void)hipFree(d_sq); (void)hipFree(d_lo); (void)hipFree(d_out); (void)hipFree(d_lo_features);
        (void)hipFree(d_features); (void)hipFree(d_work); (void)hipFree(d_rgb8);
        std::FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 3;
        std::fprintf(f, "P6\n%zu %zu\n255\n", w, h);
        std::fwrite(rgb8.data(), 1, rgb8.size(), f);
        std::fclose(f);
        if (argc > 5) {
            f = std::fopen(argv[5], "wb");
            if (!f) return 3;
            std::fwrite(out.data(), sizeof(double), out.size(), f);
            std::fclose(f);
        }
        double mean = 0.0;
        for (std::size_t i = 0; i < 3 * n; ++i) mean += out[i];
        std::printf("upsample %zux%zu -> %zux%zu: %zu spp on a quarter of the pixels, factor %u; mean of the frame = %.6f\n", wl, hl, w, h, spp,
                    up.factor, mean / (double)(3 * n));
    } catch (const rtx::Panic &p) {
        std::fprintf(stderr, "rtx panic (status %d): %s\n", (int)p.status, p.what());
        return 1;
    }
    return 0;
}
