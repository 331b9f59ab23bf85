// rtx.hpp -- C++ host API over the C ABI of librtx_hip.so, mirroring the public surface of the
// reference crate `rtx` (src/lib.rs:1-5):
//
//     rtx::math::Vector3                                   src/math/vector.rs
//     rtx::Camera                                          src/raytracing/camera.rs
//     rtx::Config, rtx::Scene                              src/raytracing/scene.rs
//     rtx::object::{Object, Material, CustomShape,
//                   sphere::Sphere, plane::Plane, triangle::Triangle}
//                                                          src/raytracing/object.rs, object/*.rs
//
// Same names, argument meaning and error behaviour: the reference reports failures by panicking
// (scene.rs:168, object.rs:38,50); here a failed render throws rtx::Panic.  The reference is
// Rust and this image has no Rust toolchain, so this header is the compiled-language host side;
// INTEGRATION.md holds the Rust `extern "C"` shim a maintainer would add to the crate itself.
//
// Header-only; link with -lrtx_hip.  Nothing here computes pixels: Scene::render packs
// Scene.objects into RtxObject records and calls rtx_render.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rtx_hip.h"

namespace rtx {

struct Panic : std::runtime_error {                                 // the reference panics; we throw
    int32_t status;
    Panic(int32_t st, const std::string &what) : std::runtime_error(what), status(st) {}
};

namespace math {

struct Vector3 {                                                    // math/vector.rs:12-20
    double x = 0.0, y = 0.0, z = 0.0;
    Vector3() = default;
    Vector3(double x_, double y_, double z_) : x(x_), y(y_), z(z_) {}   // Vector3::new, vector.rs:67-69
    static Vector3 zeros() { return {0.0, 0.0, 0.0}; }              // vector.rs:81-83
    static Vector3 ones() { return {1.0, 1.0, 1.0}; }               // vector.rs:47-53
    static Vector3 x_axis() { return {1.0, 0.0, 0.0}; }             // Vector3::x(), vector.rs:55-57
    static Vector3 y_axis() { return {0.0, 1.0, 0.0}; }             // Vector3::y(), vector.rs:59-61
    static Vector3 z_axis() { return {0.0, 0.0, 1.0}; }             // Vector3::z(), vector.rs:63-65
    double dot(const Vector3 &o) const { return x * o.x + y * o.y + z * o.z; }          // vector.rs:85-87
    Vector3 operator-() const { return {-x, -y, -z}; }             // vector.rs:115-121
    Vector3 operator+(const Vector3 &o) const { return {x + o.x, y + o.y, z + o.z}; }   // vector/add.rs:16-24
    Vector3 operator-(const Vector3 &o) const { return {x - o.x, y - o.y, z - o.z}; }   // vector/sub.rs:16-24
    bool operator==(const Vector3 &o) const { return x == o.x && y == o.y && z == o.z; } // derive(PartialEq)
};

}  // namespace math

using math::Vector3;

namespace object {

// What the device can run for a shape.  The reference's trait has only distance()/normal()
// (object.rs:53-76), from which geometry cannot be recovered, so the drop-in adds one provided
// method: primitive().  A user-defined CustomShape that does not override it cannot be rendered
// (there is no CPU fallback) and Scene::render throws.
struct Primitive {
    uint32_t kind;                       // RTX_SPHERE / RTX_PLANE / RTX_TRIANGLE
    std::array<double, 9> geom;
};

struct CustomShape {                                                // object.rs:53-76
    virtual ~CustomShape() = default;
    virtual std::optional<Primitive> primitive() const { return std::nullopt; }
};

namespace sphere {
struct Sphere : CustomShape {                                       // object/sphere.rs:8-17
    Vector3 position;
    double radius;
    Sphere(Vector3 position_, double radius_) : position(position_), radius(radius_) {}
    std::optional<Primitive> primitive() const override
    {
        return Primitive{RTX_SPHERE, {position.x, position.y, position.z, radius, 0, 0, 0, 0, 0}};
    }
};
}  // namespace sphere

namespace plane {
struct Plane : CustomShape {                                        // object/plane.rs:8-17
    Vector3 position, normal;
    Plane(Vector3 position_, Vector3 normal_) : position(position_), normal(normal_) {}
    std::optional<Primitive> primitive() const override
    {
        return Primitive{RTX_PLANE, {position.x, position.y, position.z, normal.x, normal.y, normal.z, 0, 0, 0}};
    }
};
}  // namespace plane

namespace triangle {
struct Triangle : CustomShape {                                     // object/triangle.rs:8-17
    std::array<Vector3, 3> vertices;
    explicit Triangle(std::array<Vector3, 3> vertices_) : vertices(vertices_) {}
    std::optional<Primitive> primitive() const override
    {
        const auto &v = vertices;
        return Primitive{RTX_TRIANGLE, {v[0].x, v[0].y, v[0].z, v[1].x, v[1].y, v[1].z, v[2].x, v[2].y, v[2].z}};
    }
};
}  // namespace triangle

struct Material {                                                   // object.rs:78-86
    Vector3 base_color, emission_color;
    double roughness;
    Material(Vector3 base, Vector3 emission, double rough)          // Material::new, object.rs:92-94
        : base_color(base), emission_color(emission), roughness(rough) {}
    static Material colored(Vector3 color) { return {color, Vector3::zeros(), 1.0}; }       // object.rs:111-113
    static Material light(Vector3 light_color) { return {Vector3::zeros(), light_color, 1.0}; } // object.rs:130-132
    static Material mirror() { return {Vector3::ones(), Vector3::zeros(), 1.0}; }           // object.rs:133-135
};

struct Object {                                                     // object.rs:9-28
    std::shared_ptr<const CustomShape> shape;                       // Arc<Mutex<dyn CustomShape>>: immutable snapshot here
    Material material;
    template <class T>
    Object(T shape_, Material material_) : shape(std::make_shared<T>(std::move(shape_))), material(material_) {}
};

}  // namespace object

struct Config {                                                     // scene.rs:16-28; Default scene.rs:55-65
    std::size_t rays_per_pixel = 16;
    std::size_t max_bounces = 10;
    double focal_length = 10.0;
    double focal_offset = 1e-4;
    double non_focal_offset = 1e-1;
    uint64_t seed = 42;                                             // build-added
    uint32_t kernel = RTX_KERNEL_AUTO;                              // build-added
    Config with_rays_per_pixel(std::size_t v) const { Config c = *this; c.rays_per_pixel = v; return c; }   // scene.rs:39-41
    Config with_max_bounces(std::size_t v) const { Config c = *this; c.max_bounces = v; return c; }         // scene.rs:42-44
    Config with_focal_length(double v) const { Config c = *this; c.focal_length = v; return c; }            // scene.rs:45-47
    Config with_focal_offset(double v) const { Config c = *this; c.focal_offset = v; return c; }            // scene.rs:48-50
    Config with_non_focal_offset(double v) const { Config c = *this; c.non_focal_offset = v; return c; }    // scene.rs:51-53
    Config with_seed(uint64_t v) const { Config c = *this; c.seed = v; return c; }
    Config with_kernel(uint32_t v) const { Config c = *this; c.kernel = v; return c; }
};

class Camera {                                                      // camera.rs:7-15
public:
    double fov;                                                     // horizontal fov in radians (camera.rs:8)
    Vector3 position;
    Camera(Vector3 position_, Vector3 direction_, double fov_) : fov(fov_), position(position_), direction_(direction_)
    {                                                               // Camera::new, camera.rs:19-28
        derive(direction_);
    }
    Vector3 get_direction() const { return direction_; }            // camera.rs:30-32
    void set_direction(Vector3 direction)                           // camera.rs:35-40
    {
        derive(direction_);           // as the reference: matrices from the OLD direction, then store the new one
        direction_ = direction;
    }
    Vector3 to_cam_space(Vector3 v) const { return mul(c_.to_cam_space, v - position); }        // camera.rs:51-53
    Vector3 to_world_space(Vector3 v) const { return mul(c_.to_world_space, v) + position; }    // camera.rs:55-57
    Vector3 rotate_to_world_space(Vector3 v) const { return mul(c_.to_world_space, v); }        // camera.rs:65-67
    RtxCamera to_c() const
    {
        RtxCamera c = c_;
        c.fov = fov;
        c.position[0] = position.x; c.position[1] = position.y; c.position[2] = position.z;
        c.direction[0] = direction_.x; c.direction[1] = direction_.y; c.direction[2] = direction_.z;
        return c;
    }

private:
    Vector3 direction_;
    RtxCamera c_{};
    void derive(Vector3 d)
    {
        const double p[3] = {position.x, position.y, position.z}, dd[3] = {d.x, d.y, d.z};
        int32_t rc = rtx_camera_new(p, dd, fov, &c_);
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    }
    static Vector3 mul(const double m[9], Vector3 v)                // mat/mul.rs:42-50
    {
        return {v.x * m[0] + v.y * m[1] + v.z * m[2], v.x * m[3] + v.y * m[4] + v.z * m[5],
                v.x * m[6] + v.y * m[7] + v.z * m[8]};
    }
};

class Scene {                                                       // scene.rs:78-85
public:
    std::vector<object::Object> objects;
    Camera camera;
    Config config;

    Scene() : camera(Vector3(0, 0, 0), Vector3(1, 0, 0), 90.0) {}   // Default, scene.rs:86-94 (90f64, as the reference)
    Scene(Config config_, Camera camera_) : camera(std::move(camera_)), config(config_) {}   // Scene::new, scene.rs:112-118
    void add_object(object::Object o) { objects.push_back(std::move(o)); }                  // scene.rs:126-128

    // Scene::render, scene.rs:144-170: img[y][x].  `devices`: the GPUs the frame is partitioned over (interleaved row
    // bands, one gather on devices[0]; rtx_render_devices); empty = device 0.  The pixels do not depend on it.
    std::vector<std::vector<Vector3>> render(std::size_t width, std::size_t height, const std::vector<int32_t> &devices = {}) const
    {
        std::vector<double> flat(width * height * 3);
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = devices.empty() ? rtx_render(&sc, (uint32_t)width, (uint32_t)height, flat.data())
                                     : rtx_render_devices(&sc, (uint32_t)width, (uint32_t)height, devices.data(),
                                                          (uint32_t)devices.size(), flat.data());
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        std::vector<std::vector<Vector3>> img(height, std::vector<Vector3>(width));
        for (std::size_t y = 0; y < height; ++y)
            for (std::size_t x = 0; x < width; ++x) {
                const double *c = &flat[(y * width + x) * 3];
                img[y][x] = Vector3(c[0], c[1], c[2]);
            }
        return img;
    }

    // Scene::render_to_image, scene.rs:172-178: RGB8, row 0 = top of the image
    std::vector<uint8_t> render_to_image(std::size_t width, std::size_t height, const std::vector<int32_t> &devices = {}) const
    {
        std::vector<uint8_t> out(width * height * 3);
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = devices.empty() ? rtx_render_to_image(&sc, (uint32_t)width, (uint32_t)height, out.data())
                                     : rtx_render_to_image_devices(&sc, (uint32_t)width, (uint32_t)height, devices.data(),
                                                                   (uint32_t)devices.size(), out.data());
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        return out;
    }

    // closest_object (scene.rs:243-251) for each ray (rtx_closest_hits: upload to device 0, query, copy back).  A miss has
    // object == -1, distance == +inf and NaN position / normal.  Directions are used as given.
    std::vector<RtxHit> closest_hits(const std::vector<RtxRay> &rays) const
    {
        std::vector<RtxHit> hits(rays.size());
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = rtx_closest_hits(&sc, rays.data(), rays.size(), hits.data());
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        return hits;
    }

    // Occlusion: out[i] = 1 when some object's distance is normal, positive and < t_max[i] (rtx_any_hits); an empty t_max
    // means +inf for every ray (any hit at all).  Limits are compared as given: NaN, zero or negative is never occluded.
    std::vector<uint8_t> any_hits(const std::vector<RtxRay> &rays, const std::vector<double> &t_max = {}) const
    {
        if (!t_max.empty() && t_max.size() != rays.size()) throw Panic(RTX_ERR_INVALID_ARGUMENT, "any_hits: one limit per ray, or none");
        std::vector<uint8_t> out(rays.size());
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = rtx_any_hits(&sc, rays.data(), t_max.empty() ? nullptr : t_max.data(), rays.size(), out.data());
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        return out;
    }

    // The k nearest objects along each ray, sorted by (distance, object index) (rtx_multi_hits): hits[i * k + j] is entry j of ray i;
    // the entries behind counts[i] (optional) are closest_hits' miss.  t_max as for any_hits; 1 <= k <= RTX_MULTI_HIT_MAX.
    std::vector<RtxHit> multi_hits(const std::vector<RtxRay> &rays, std::uint32_t k, const std::vector<double> &t_max = {},
                                   std::vector<std::uint32_t> *counts = nullptr) const
    {
        if (!t_max.empty() && t_max.size() != rays.size()) throw Panic(RTX_ERR_INVALID_ARGUMENT, "multi_hits: one limit per ray, or none");
        std::vector<RtxHit> hits(rays.size() * k);
        if (counts) counts->assign(rays.size(), 0u);
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = rtx_multi_hits(&sc, rays.data(), t_max.empty() ? nullptr : t_max.data(), rays.size(), k, hits.data(),
                                    counts ? counts->data() : nullptr);
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        return hits;
    }

    // The denoising guide buffers of a width x height frame (rtx_pixel_features): per pixel [y][x] the first hits of render_pixel's own
    // lens-jittered rays, folded in sample order -- mean albedo / emission / normal, mean depth, coverage, sample 0's object.
    std::vector<RtxPixelFeatures> pixel_features(std::size_t width, std::size_t height) const
    {
        std::vector<RtxPixelFeatures> out(width * height);
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = rtx_pixel_features(&sc, (uint32_t)width, (uint32_t)height, out.data());
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        return out;
    }

    // render_ray (scene.rs:223-242) from each ray, with the config's max_bounces and seed (rtx_trace_paths): rgb[3 i .. 3 i + 2] =
    // the path's resulting_color, unclamped.  ids: empty (entry i draws as pixel i, sample 0) or 2 per ray, (pixel index, sample
    // index); segments (optional): the closest_object calls of each path.
    std::vector<double> trace_paths(const std::vector<RtxRay> &rays, const std::vector<uint64_t> &ids = {},
                                    std::vector<uint32_t> *segments = nullptr) const
    {
        if (!ids.empty() && ids.size() != 2 * rays.size()) throw Panic(RTX_ERR_INVALID_ARGUMENT, "trace_paths: two ids per ray, or none");
        std::vector<double> rgb(3 * rays.size());
        if (segments) segments->assign(rays.size(), 0u);
        std::vector<RtxObject> packed = pack();
        RtxScene sc = to_c(packed);
        int32_t rc = rtx_trace_paths(&sc, rays.data(), ids.empty() ? nullptr : ids.data(), rays.size(), rgb.data(),
                                     segments ? segments->data() : nullptr);
        if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
        return rgb;
    }

    std::vector<RtxObject> pack() const
    {
        std::vector<RtxObject> packed(objects.size());
        for (std::size_t i = 0; i < objects.size(); ++i) {
            const auto prim = objects[i].shape->primitive();
            if (!prim)
                throw Panic(RTX_ERR_UNSUPPORTED, "object " + std::to_string(i) +
                                                     ": CustomShape without primitive() cannot run on the GPU (no CPU fallback)");
            RtxObject &o = packed[i];
            o.kind = prim->kind;
            o.reserved = 0;
            for (int k = 0; k < 9; ++k) o.geom[k] = prim->geom[k];
            const object::Material &m = objects[i].material;
            o.base_color[0] = m.base_color.x; o.base_color[1] = m.base_color.y; o.base_color[2] = m.base_color.z;
            o.emission_color[0] = m.emission_color.x; o.emission_color[1] = m.emission_color.y;
            o.emission_color[2] = m.emission_color.z;
            o.roughness = m.roughness;
        }
        return packed;
    }

    class Resident;
    // Row N4 of SURVEY 8f (the use-case of the crate's wgpu path, gpu_state/buffer.rs:69-115): the scene stays on
    // `device`; camera / config changes do not re-upload it.
    Resident upload(int device = 0) const;

private:
    RtxScene to_c(const std::vector<RtxObject> &packed) const
    {
        RtxScene sc{};
        sc.config.rays_per_pixel = config.rays_per_pixel;
        sc.config.max_bounces = config.max_bounces;
        sc.config.focal_length = config.focal_length;
        sc.config.focal_offset = config.focal_offset;
        sc.config.non_focal_offset = config.non_focal_offset;
        sc.config.seed = config.seed;
        sc.config.kernel = config.kernel;
        sc.camera = camera.to_c();
        sc.n_objects = packed.size();
        sc.objects = packed.empty() ? nullptr : packed.data();
        return sc;
    }
};

// A scene resident in the HBM of one GPU (rtx_scene_upload ... rtx_scene_free).  Output goes to DEVICE memory the
// caller owns (h*w*3 doubles for a full frame), on the HIP stream it names; a row band per call is what one rank of
// a multi-GPU job renders.
class Scene::Resident {
public:
    Resident(const Resident &) = delete;
    Resident &operator=(const Resident &) = delete;
    Resident(Resident &&o) noexcept : h_(o.h_), n_objects_(o.n_objects_), device_(o.device_) { o.h_ = nullptr; }
    ~Resident() { if (h_) rtx_scene_free(h_); }

    void set_camera(const Camera &camera)                              // Camera::set_position / set_direction, camera.rs:35-40
    {
        const RtxCamera c = camera.to_c();
        check(rtx_scene_set_camera(h_, &c));
    }
    void set_config(const Config &config)
    {
        RtxConfig c{};
        c.rays_per_pixel = config.rays_per_pixel; c.max_bounces = config.max_bounces;
        c.focal_length = config.focal_length; c.focal_offset = config.focal_offset; c.non_focal_offset = config.non_focal_offset;
        c.seed = config.seed; c.kernel = config.kernel;
        check(rtx_scene_set_config(h_, &c));
    }
    void add_object(const object::Object &o)                           // Scene::add_object, scene.rs:126-128
    {
        Scene one;
        one.add_object(o);
        const std::vector<RtxObject> packed = one.pack();
        check(rtx_scene_append_objects(h_, packed.data(), packed.size()));
        n_objects_ += packed.size();
    }
    // Scene.objects[indices[i]] = objects[i] on the resident scene (rtx_scene_update_objects): moved spheres are refitted into the
    // resident tree on the device, materials and planes are rewritten in place; anything the tree cannot take (a kind change, a
    // triangle's geometry, a sphere beyond the range the tree was built for) or rebuild = true rebuilds as add_object does.
    // Returns RTX_UPDATED_NOTHING / RECORDS / REFIT / REBUILT.
    uint32_t update_objects(const std::vector<std::uint64_t> &indices, const std::vector<object::Object> &objects, bool rebuild = false,
                            void *hip_stream = nullptr)
    {
        return update_objects_mode(indices, objects, rebuild ? RTX_UPDATE_REBUILD : RTX_UPDATE_AUTO, hip_stream);
    }
    // The same with the mode spelled out: RTX_UPDATE_AUTO, RTX_UPDATE_REBUILD, or RTX_UPDATE_DEFORM -- AUTO, and a triangle that gets
    // new vertices and keeps its class (include/rtx_hip.h) is rewritten and refitted in place too (a deforming mesh, a moving part).
    uint32_t update_objects_mode(const std::vector<std::uint64_t> &indices, const std::vector<object::Object> &objects, uint32_t mode,
                                 void *hip_stream = nullptr)
    {
        if (indices.size() != objects.size()) throw std::invalid_argument("update_objects: indices and objects differ in length");
        Scene list;
        for (const object::Object &o : objects) list.add_object(o);
        const std::vector<RtxObject> packed = list.pack();
        uint32_t how = RTX_UPDATED_NOTHING;
        check(rtx_scene_update_objects(h_, indices.data(), packed.data(), packed.size(), mode, hip_stream, &how));
        return how;
    }
    // Hides (visible = false) or shows Scene.objects[indices[i]] in place (rtx_scene_set_visible): what the reference's users do with
    // retain / remove on the pub Vec, with the indices of all other objects unchanged and the tree kept.  A hidden object is never hit;
    // frames are those of the list without it.  Returns RTX_UPDATED_NOTHING / RECORDS / REFIT / REBUILT.
    uint32_t set_visible(const std::vector<std::uint64_t> &indices, bool visible, void *hip_stream = nullptr)
    {
        uint32_t how = RTX_UPDATED_NOTHING;
        check(rtx_scene_set_visible(h_, indices.data(), indices.size(), visible ? 1u : 0u, hip_stream, &how));
        return how;
    }
    // one entry per object of the resident list: false for a hidden one
    std::vector<bool> visible() const
    {
        std::vector<std::uint8_t> mask(n_objects_, 1);
        check(rtx_scene_get_visible(h_, mask.data()));
        return std::vector<bool>(mask.begin(), mask.end());
    }
    // rows row_begin, row_begin + row_stride, ... (n_rows of them) of the width x height image -> d_out_rgb[n_rows][width][3]
    RtxStats render_rows(std::size_t width, std::size_t height, std::size_t row_begin, std::size_t row_stride, std::size_t n_rows,
                         double *d_out_rgb, void *hip_stream = nullptr)
    {
        RtxStats st{};
        check(rtx_render_rows(h_, (uint32_t)width, (uint32_t)height, (uint32_t)row_begin, (uint32_t)row_stride, (uint32_t)n_rows,
                              d_out_rgb, hip_stream, &st));
        return st;
    }
    RtxStats render(std::size_t width, std::size_t height, double *d_out_rgb, void *hip_stream = nullptr)
    {
        return render_rows(width, height, 0, 1, height, d_out_rgb, hip_stream);
    }
    // what rank `part` of `n_parts` of a multi-GPU job renders: the blocks of `block_rows` rows part, part + n_parts, ...
    // (8 keeps the tree kernels' 8x8 ray tiles whole) -> d_out_rgb[band_rows(...)][width][3], rows in increasing image order
    static std::size_t band_rows(std::size_t height, std::size_t block_rows, std::size_t part, std::size_t n_parts)
    {
        return rtx_blocks_row_count((uint32_t)height, (uint32_t)block_rows, (uint32_t)part, (uint32_t)n_parts);
    }
    RtxStats render_blocks(std::size_t width, std::size_t height, std::size_t block_rows, std::size_t part, std::size_t n_parts,
                           double *d_out_rgb, void *hip_stream = nullptr)
    {
        RtxStats st{};
        check(rtx_render_blocks(h_, (uint32_t)width, (uint32_t)height, (uint32_t)block_rows, (uint32_t)part, (uint32_t)n_parts,
                                d_out_rgb, hip_stream, &st));
        return st;
    }
    // progressive sampling: the samples [sample_begin, sample_begin + n_samples) of every pixel of the same band ADDED to the running
    // sums d_sum and d_sum_sq (or nullptr) -- band_rows(...) * width * 3 doubles each, zero bytes before the first call; ranges that tile
    // [0, S) in order leave d_sum / S == render_blocks at rays_per_pixel = S, bit for bit; (8, 0, 1) is the full frame.  With stats =
    // nullptr the call returns once the work is enqueued
    void render_blocks_accumulate(std::size_t width, std::size_t height, std::size_t block_rows, std::size_t part, std::size_t n_parts,
                                  std::uint64_t sample_begin, std::uint64_t n_samples, double *d_sum, double *d_sum_sq = nullptr,
                                  void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_render_blocks_accumulate(h_, (uint32_t)width, (uint32_t)height, (uint32_t)block_rows, (uint32_t)part, (uint32_t)n_parts,
                                           sample_begin, n_samples, d_sum, d_sum_sq, hip_stream, stats));
    }
    // refinement to a noise threshold, decided on the device (rtx_render_blocks_refine): every pixel of render_blocks_accumulate's band
    // whose summed variance of the mean exceeds (threshold * (mean + floor))^2 and that has fewer than max_samples samples gets n_more
    // further samples per round, folded into d_sum / d_sum_sq; d_extra (one zeroed uint32 per pixel) counts each pixel's samples beyond
    // sample_begin.  Returns {pixels that traced, samples traced, pixels still selected}: [2] == 0 is the stop signal
    std::array<std::uint64_t, 3> refine(std::size_t width, std::size_t height, std::size_t block_rows, std::size_t part, std::size_t n_parts,
                                        std::uint64_t sample_begin, std::uint32_t n_more, std::uint32_t max_samples, std::uint32_t rounds,
                                        double threshold, double floor, double *d_sum, double *d_sum_sq, std::uint32_t *d_extra,
                                        void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        std::array<std::uint64_t, 3> result{};
        check(rtx_render_blocks_refine(h_, (uint32_t)width, (uint32_t)height, (uint32_t)block_rows, (uint32_t)part, (uint32_t)n_parts,
                                       sample_begin, n_more, max_samples, rounds, threshold, floor, d_sum, d_sum_sq, d_extra,
                                       result.data(), hip_stream, stats));
        return result;
    }
    void set_scratch_limit(std::uint64_t bytes) { check(rtx_scene_set_scratch_limit(h_, bytes)); }
    // closest_object for n rays of DEVICE memory (d_rays[n] -> d_hits[n], not overlapping), on the HIP stream it names; with
    // stats = nullptr the call returns once the work is enqueued
    void closest_hits(const RtxRay *d_rays, std::size_t n, RtxHit *d_hits, void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_closest_hits(h_, d_rays, n, d_hits, hip_stream, stats));
    }
    // occlusion for n rays of DEVICE memory: d_out[i] = 1 when something lies before d_t_max[i] (nullptr: anywhere along the ray)
    void any_hits(const RtxRay *d_rays, const double *d_t_max, std::size_t n, uint8_t *d_out, void *hip_stream = nullptr,
                  RtxStats *stats = nullptr)
    {
        check(rtx_scene_any_hits(h_, d_rays, d_t_max, n, d_out, hip_stream, stats));
    }
    // the k nearest objects along each of n rays of DEVICE memory, sorted: d_hits[n * k] (ray i's list at i * k), d_counts[n] or
    // nullptr, d_t_max[n] or nullptr (no limit)
    void multi_hits(const RtxRay *d_rays, const double *d_t_max, std::size_t n, std::uint32_t k, RtxHit *d_hits,
                    std::uint32_t *d_counts = nullptr, void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_multi_hits(h_, d_rays, d_t_max, n, k, d_hits, d_counts, hip_stream, stats));
    }
    // the same for the pick buffer's rays: d_hits[height][width][k], d_counts[height][width] or nullptr
    void primary_multi_hits(std::size_t width, std::size_t height, std::uint32_t k, RtxHit *d_hits, std::uint32_t *d_counts = nullptr,
                            void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_primary_multi_hits(h_, (uint32_t)width, (uint32_t)height, k, d_hits, d_counts, hip_stream, stats));
    }
    // render_ray from n rays of DEVICE memory: d_rgb[3 n] = each path's colour, d_ids (nullptr: (i, 0)) the (pixel, sample) pairs that
    // key the RNG, d_segments (or nullptr) the closest_object calls of each path
    void trace_paths(const RtxRay *d_rays, const uint64_t *d_ids, std::size_t n, double *d_rgb, uint32_t *d_segments = nullptr,
                     void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_trace_paths(h_, d_rays, d_ids, n, d_rgb, d_segments, hip_stream, stats));
    }
    // sparse samples of the render: entry i is sample d_ids[2 i + 1] of pixel d_ids[2 i] (= y * width + x) of the width x height frame,
    // bit for bit the render's; d_rgb[3 n], d_segments (or nullptr) as trace_paths.  An entry outside the frame: NaN, 0 segments
    void trace_samples(std::size_t width, std::size_t height, const uint64_t *d_ids, std::size_t n, double *d_rgb,
                       uint32_t *d_segments = nullptr, void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_trace_samples(h_, (uint32_t)width, (uint32_t)height, d_ids, n, d_rgb, d_segments, hip_stream, stats));
    }
    // the pick buffer: d_hits[height][width] = the hit of each pixel's primary ray without the focal / non-focal offsets
    void primary_hits(std::size_t width, std::size_t height, RtxHit *d_hits, void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_primary_hits(h_, (uint32_t)width, (uint32_t)height, d_hits, hip_stream, stats));
    }
    // the denoising guide buffers: d_features[height][width] = each pixel's folded first hits over the render's own rays
    void pixel_features(std::size_t width, std::size_t height, RtxPixelFeatures *d_features, void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_pixel_features(h_, (uint32_t)width, (uint32_t)height, d_features, hip_stream, stats));
    }
    // the same for the band of part `part` of `n_parts` (blocks of block_rows rows, as render_blocks): rtx_blocks_row_count() rows
    void pixel_features_blocks(std::size_t width, std::size_t height, std::uint32_t block_rows, std::uint32_t part, std::uint32_t n_parts,
                               RtxPixelFeatures *d_features, void *hip_stream = nullptr, RtxStats *stats = nullptr)
    {
        check(rtx_scene_pixel_features_blocks(h_, (uint32_t)width, (uint32_t)height, block_rows, part, n_parts, d_features, hip_stream, stats));
    }
    // the denoiser on this scene's device (rtx_denoise_device; it reads no scene): the full frame d_rgb[height][width][3] with its
    // guides d_features (pixel_features) and, or null, the variance of the mean d_var -> d_out (and d_var_out, or null).  d_work:
    // rtx::denoise_work_bytes(width, height, params) bytes.  Only enqueues on hip_stream.
    void denoise(std::size_t width, std::size_t height, const double *d_rgb, const double *d_var, const RtxPixelFeatures *d_features,
                 const RtxDenoiseParams &params, double *d_out, double *d_var_out, void *d_work, void *hip_stream = nullptr)
    {
        check(rtx_denoise_device(d_rgb, d_var, d_features, (uint32_t)width, (uint32_t)height, &params, d_out, d_var_out, d_work, device_, hip_stream));
    }
    // guided upsampling on this scene's device (rtx_upsample_device; it reads no scene): the low frame d_lo_rgb[height / s][width / s][3]
    // (s = params.factor; d_lo_var its variance of the mean, or null) with the guides of the low and of the width x height output frame
    // (pixel_features at both sizes, the same camera) -> d_out[height][width][3] (and d_var_out, or null).  One launch, only enqueued.
    void upsample(std::size_t width, std::size_t height, const double *d_lo_rgb, const double *d_lo_var, const RtxPixelFeatures *d_lo_features,
                  const RtxPixelFeatures *d_features, const RtxUpsampleParams &params, double *d_out, double *d_var_out,
                  void *hip_stream = nullptr)
    {
        check(rtx_upsample_device(d_lo_rgb, d_lo_var, d_lo_features, d_features, (uint32_t)width, (uint32_t)height, &params, d_out, d_var_out,
                                  device_, hip_stream));
    }
    // temporal accumulation on this scene's device (rtx_temporal_accumulate_device; it reads no scene): this frame's d_rgb, d_var (or
    // null) and pick buffer d_hits with the previous frame's accumulated d_hist_* (all null: the first frame), its camera and the
    // uploaded rtx::temporal_tables of that camera -> d_out_rgb, d_out_var (or null), d_out_len, d_motion (or null).  Only enqueues.
    void temporal_accumulate(std::size_t width, std::size_t height, const double *d_rgb, const double *d_var, const RtxHit *d_hits,
                             const double *d_hist_rgb, const double *d_hist_var, const double *d_hist_len, const RtxHit *d_hist_hits,
                             const RtxCamera *prev_camera, const double *d_prev_tables, const RtxTemporalParams &params, double *d_out_rgb,
                             double *d_out_var, double *d_out_len, double *d_motion = nullptr, void *hip_stream = nullptr)
    {
        check(rtx_temporal_accumulate_device(d_rgb, d_var, d_hits, d_hist_rgb, d_hist_var, d_hist_len, d_hist_hits, prev_camera, d_prev_tables,
                                             (uint32_t)width, (uint32_t)height, &params, d_out_rgb, d_out_var, d_out_len, d_motion, device_,
                                             hip_stream));
    }
    // rewinds a pick buffer on this scene's device (rtx_rewind_hits_device; it reads no scene): the n_hits records at d_hits, with every
    // hit on one of the m moved objects (d_objects ascending, d_motions: rtx::object_motions, uploaded) replaced by the record of the
    // same material point on the object's previous geometry -> d_out, which temporal_accumulate then takes as d_hits.  Only enqueues.
    void rewind_hits(const RtxHit *d_hits, std::size_t n_hits, const std::int64_t *d_objects, const RtxObjectMotion *d_motions, std::size_t m,
                     RtxHit *d_out, void *hip_stream = nullptr)
    {
        check(rtx_rewind_hits_device(d_hits, n_hits, d_objects, d_motions, m, 0u, d_out, device_, hip_stream));
    }

private:
    friend class Scene;
    Resident(RtxSceneHandle h, std::size_t n_objects, int device) : h_(h), n_objects_(n_objects), device_(device) {}
    static void check(int32_t rc) { if (rc != RTX_OK) throw Panic(rc, rtx_last_error()); }
    RtxSceneHandle h_;
    std::size_t n_objects_;
    int device_;
};

inline Scene::Resident Scene::upload(int device) const
{
    std::vector<RtxObject> packed = pack();
    RtxScene sc = to_c(packed);
    RtxSceneHandle h = nullptr;
    int32_t rc = rtx_scene_upload(&sc, device, &h);
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    return Resident(h, packed.size(), device);
}

// The denoiser of include/rtx_hip.h ("Denoising"): an edge-avoiding a-trous filter guided by a frame's pixel features and, when there
// is one, by the variance of its mean.
inline RtxDenoiseParams denoise_default_params()
{
    RtxDenoiseParams p;
    rtx_denoise_default_params(&p);
    return p;
}
inline std::uint64_t denoise_work_bytes(std::size_t width, std::size_t height, const RtxDenoiseParams &params)
{
    return rtx_denoise_work_bytes((uint32_t)width, (uint32_t)height, &params);
}
// host form (rtx_denoise: device 0, copies both ways): rgb [height][width][3], features from Scene::pixel_features, var (may be empty: no
// colour term) the per-channel variance of the mean -> the denoised frame; var_out (optional, needs var): the filtered variance
inline std::vector<double> denoise(const std::vector<double> &rgb, const std::vector<RtxPixelFeatures> &features, std::size_t width,
                                   std::size_t height, const RtxDenoiseParams &params = denoise_default_params(),
                                   const std::vector<double> &var = {}, std::vector<double> *var_out = nullptr)
{
    if (rgb.size() != 3 * width * height || features.size() != width * height || (!var.empty() && var.size() != rgb.size()))
        throw Panic(RTX_ERR_INVALID_ARGUMENT, "denoise: rgb, var and features must hold width * height pixels");
    std::vector<double> out(rgb.size());
    if (var_out) var_out->assign(var.empty() ? 0 : rgb.size(), 0.0);
    int32_t rc = rtx_denoise(rgb.data(), var.empty() ? nullptr : var.data(), features.data(), (uint32_t)width, (uint32_t)height, &params,
                             out.data(), (var_out && !var.empty()) ? var_out->data() : nullptr);
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    return out;
}

// The guided upsampling of include/rtx_hip.h ("Guided upsampling"): a frame rendered at 1 / factor of the output size, reconstructed at
// the output size under the guides of both sizes.
inline RtxUpsampleParams upsample_default_params()
{
    RtxUpsampleParams p;
    rtx_upsample_default_params(&p);
    return p;
}
// host form (rtx_upsample: device 0, copies both ways): lo_rgb [height / s][width / s][3] and lo_features of the low frame, features of
// the width x height output frame (both from Scene::pixel_features, the same camera), lo_var (may be empty) the low frame's variance of
// the mean -> the output frame; var_out (optional, needs lo_var): its variance
inline std::vector<double> upsample(const std::vector<double> &lo_rgb, const std::vector<RtxPixelFeatures> &lo_features,
                                    const std::vector<RtxPixelFeatures> &features, std::size_t width, std::size_t height,
                                    const RtxUpsampleParams &params = upsample_default_params(), const std::vector<double> &lo_var = {},
                                    std::vector<double> *var_out = nullptr)
{
    const std::size_t s = params.factor ? params.factor : 1, n_lo = (width / s) * (height / s);
    if (lo_rgb.size() != 3 * n_lo || lo_features.size() != n_lo || features.size() != width * height || (!lo_var.empty() && lo_var.size() != lo_rgb.size()))
        throw Panic(RTX_ERR_INVALID_ARGUMENT, "upsample: lo_rgb, lo_var and lo_features must hold (width / factor) * (height / factor) pixels, features width * height");
    std::vector<double> out(3 * width * height);
    if (var_out) var_out->assign(lo_var.empty() ? 0 : out.size(), 0.0);
    int32_t rc = rtx_upsample(lo_rgb.data(), lo_var.empty() ? nullptr : lo_var.data(), lo_features.data(), features.data(), (uint32_t)width,
                              (uint32_t)height, &params, out.data(), (var_out && !lo_var.empty()) ? var_out->data() : nullptr);
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    return out;
}

// Temporal accumulation of include/rtx_hip.h ("Temporal accumulation"): the previous frames' samples, reprojected and blended in where
// the same surface is still seen.
inline RtxTemporalParams temporal_default_params()
{
    RtxTemporalParams p;
    rtx_temporal_default_params(&p);
    return p;
}
// the sines of a camera's pixel map, Tx[width + 1] then Ty[height + 1]: what Resident::temporal_accumulate takes, uploaded
inline std::vector<double> temporal_tables(double fov, std::size_t width, std::size_t height)
{
    std::vector<double> t(width + height + 2);
    int32_t rc = rtx_temporal_tables(fov, (uint32_t)width, (uint32_t)height, t.data());
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    return t;
}
// one frame's buffers on the host: what temporal_accumulate takes as its history and returns as the next one
struct TemporalFrame {
    std::vector<double> rgb, var, len;                      // var: empty when no variance is tracked
    std::vector<RtxHit> hits;
    std::vector<double> motion;                             // filled when asked for
};
// host form (rtx_temporal_accumulate: device 0, copies both ways): rgb [height][width][3], var (may be empty), this frame's pick buffer;
// history: null on the first frame, else the previous call's result with the camera it was taken with
inline TemporalFrame temporal_accumulate(const std::vector<double> &rgb, const std::vector<double> &var, const std::vector<RtxHit> &hits,
                                         std::size_t width, std::size_t height, const TemporalFrame *history = nullptr,
                                         const RtxCamera *prev_camera = nullptr,
                                         const RtxTemporalParams &params = temporal_default_params(), bool want_motion = false)
{
    const std::size_t n = width * height;
    if (rgb.size() != 3 * n || hits.size() != n || (!var.empty() && var.size() != 3 * n))
        throw Panic(RTX_ERR_INVALID_ARGUMENT, "temporal_accumulate: rgb, var and hits must hold width * height pixels");
    if (history && (history->rgb.size() != 3 * n || history->len.size() != n || history->hits.size() != n ||
                    (!history->var.empty() && history->var.size() != 3 * n)))
        throw Panic(RTX_ERR_INVALID_ARGUMENT, "temporal_accumulate: the history must hold width * height pixels");
    TemporalFrame out;
    out.rgb.resize(3 * n); out.len.resize(n); out.hits = hits;
    if (!var.empty()) out.var.resize(3 * n);
    if (want_motion) out.motion.resize(2 * n);
    int32_t rc = rtx_temporal_accumulate(rgb.data(), var.empty() ? nullptr : var.data(), hits.data(), history ? history->rgb.data() : nullptr,
                                         (history && !history->var.empty()) ? history->var.data() : nullptr,
                                         history ? history->len.data() : nullptr, history ? history->hits.data() : nullptr, prev_camera,
                                         (uint32_t)width, (uint32_t)height, &params, out.rgb.data(), var.empty() ? nullptr : out.var.data(),
                                         out.len.data(), want_motion ? out.motion.data() : nullptr);
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    return out;
}

// What moved between two frames (rtx_object_motions; host only): the objects `indices` had the records `before` when the previous
// frame's pick was taken and have the records `now` -- what update_objects was given since.  Of a repeated index the first `before` and
// the last `now` count; unchanged geometry is left out.
struct ObjectMotions {
    std::vector<std::int64_t> objects;                      // ascending
    std::vector<RtxObjectMotion> motions;
};
inline ObjectMotions object_motions(const std::vector<std::uint64_t> &indices, const std::vector<object::Object> &before,
                                    const std::vector<object::Object> &now)
{
    if (indices.size() != before.size() || indices.size() != now.size())
        throw std::invalid_argument("object_motions: indices, before and now differ in length");
    Scene was, is;
    for (const object::Object &o : before) was.add_object(o);
    for (const object::Object &o : now) is.add_object(o);
    const std::vector<RtxObject> pw = was.pack(), pi = is.pack();
    ObjectMotions out;
    out.objects.resize(indices.size());
    out.motions.resize(indices.size());
    std::uint64_t m = 0;
    int32_t rc = rtx_object_motions(indices.data(), pw.data(), pi.data(), indices.size(), out.objects.data(), out.motions.data(), &m);
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    out.objects.resize(m);
    out.motions.resize(m);
    return out;
}
// host form (rtx_rewind_hits: device 0, copies both ways): a pick buffer, rewound on the moved objects
inline std::vector<RtxHit> rewind_hits(const std::vector<RtxHit> &hits, const ObjectMotions &moved)
{
    std::vector<RtxHit> out(hits.size());
    int32_t rc = rtx_rewind_hits(hits.data(), hits.size(), moved.objects.empty() ? nullptr : moved.objects.data(),
                                 moved.motions.empty() ? nullptr : moved.motions.data(), moved.objects.size(), out.data());
    if (rc != RTX_OK) throw Panic(rc, rtx_last_error());
    return out;
}

}  // namespace rtx
