/*
 * rtx_hip.h -- C ABI of librtx_hip.so: the MI355X (gfx950) implementation of the
 * Scene::render() hot path of Schatten2021/rust-raytracing (crate `rtx` 0.1.0).
 *
 * The reference has no FFI of its own (no `extern`, no `unsafe`); the boundary this library
 * replaces is the Rust method
 *     Scene::render(&self, width: usize, height: usize) -> Vec<Vec<Vector3>>
 *                                                         (src/raytracing/scene.rs:144-170)
 * and everything below it: render_pixel / get_ray_dir / render_ray / closest_object / ray_hit /
 * random_bounce_dir (scene.rs:194-292), Object::distance / normal_at (object.rs:37-51),
 * Sphere / Plane / Triangle distance + normal (object/sphere.rs:19-33, plane.rs:20-35,
 * triangle.rs:20-127) and the Vector3 ops they use (src/math/vector*.rs).  A Rust shim
 * binds these entry points with a plain `extern "C"` block (INTEGRATION.md shows it).
 *
 * Plain C: fixed-width integers, doubles, caller-owned memory, no C++ or torch types.
 * All entry points return 0 on success; on failure they return a non-zero RtxStatus and
 * rtx_last_error() (thread-local) describes the failure.  There is NO CPU fallback: without
 * a usable gfx950 device every render entry point fails with RTX_ERR_NO_DEVICE.
 *
 * Threads: Scene::render(&self) is re-entrant in the reference (clones share the shapes behind Arc<Mutex>,
 * object.rs:9-15); here rtx_render / rtx_render_to_image may be called from any number of threads at once (each call
 * owns its device buffers; the library keeps no global mutable state besides the thread-local error string).  An
 * RtxSceneHandle owns scratch memory and is for one thread at a time; upload one handle per rendering thread or rank.
 * Streams: a handle's device buffers are shared by all of its renders, so its work is ordered on one stream at a time --
 * a call that brings a different stream than the previous call first waits for the previous stream to drain.
 * (on the device: an event the handle owns, recorded at the end of every render -- the caller's previous stream may be
 * gone by then and is never touched again).
 * With stats == NULL rtx_render_rows / rtx_render_blocks are asynchronous; an internal error of such a render (the launch's
 * watchdog word: the sweep kernel's round bound, a full survivors' queue) is reported by the next call on the handle that
 * finds it, at the latest by rtx_scene_free.
 */
#ifndef RTX_HIP_H
#define RTX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_HIP_VERSION 100  /* 0.1.0, the crate version this drop-in tracks (Cargo.toml:3) */

typedef enum RtxStatus {
    RTX_OK = 0,
    RTX_ERR_INVALID_ARGUMENT = 1,
    RTX_ERR_NO_DEVICE = 2,       /* no HIP device / not gfx950 */
    RTX_ERR_HIP = 3,             /* a HIP runtime call failed; see rtx_last_error() */
    RTX_ERR_UNSUPPORTED = 4,     /* e.g. an object kind the device path has no primitive for */
    RTX_ERR_OUT_OF_MEMORY = 5
} RtxStatus;

/* Shape tags of the three built-in shapes (object/sphere.rs, plane.rs, triangle.rs).
 * User-defined CustomShape impls (object.rs:53-76) have no device primitive -> RTX_ERR_UNSUPPORTED. */
enum { RTX_SPHERE = 0, RTX_PLANE = 1, RTX_TRIANGLE = 2 };

/* Kernel selection (RtxConfig.kernel). */
enum {
    RTX_KERNEL_AUTO  = 0,  /* RTX_KERNEL_BVH when a tree was built at upload (more than 4 finite spheres and/or more than
                              4 triangles with a footprint) and at most 64 spheres/triangles stay outside it;
                              RTX_KERNEL_BVH_REGROUP instead when the tree holds a triangle mesh (>= 1024 triangles);
                              RTX_KERNEL_WAVEFRONT for such a mesh when the call renders >= 2^20 rays;
                              else RTX_KERNEL_MIXED.  All kernels produce the same bits, AUTO picks the fastest */
    RTX_KERNEL_EXACT = 1,  /* every shape test in f64, reference operation order */
    RTX_KERNEL_MIXED = 2,  /* f32 conservative LDS filter + exact f64 re-evaluation of candidates;
                              produces the same bits as RTX_KERNEL_EXACT */
    RTX_KERNEL_MIXED_VERIFY = 3, /* debug: MIXED that also runs the exact sweep per segment and counts
                              disagreements in RtxStats.filter_mismatches (must stay 0) */
    RTX_KERNEL_BVH = 4,    /* spheres and triangles found by traversal of a flat BVH built at upload (SURVEY 8f N2:
                              3-D sphere boxes; (x, y) footprints for triangles, which keeps the reference's phantom
                              hits), exact f64 leaf tests; planes and shapes outside the tree tested for every
                              segment; same bits as RTX_KERNEL_EXACT.  RtxStats.box_tests counts child boxes tested.  The
                              kernels of this id are the sphere tree's; a tree that holds triangles runs RTX_KERNEL_BVH_REGROUP's,
                              whichever of the two ids is asked for ("Product and lab" below) */
    RTX_KERNEL_BVH_REGROUP = 5, /* the same tree under a different schedule: lanes whose traversal ended wait until enough
                              of them can go on together, instead of every lane waiting for the wave's longest traversal;
                              the kernel of trees that hold triangles (a sphere tree runs RTX_KERNEL_BVH's); same bits */
    RTX_KERNEL_WAVEFRONT = 6   /* the same tree walked by a kernel of its own per bounce level (f32 only; level 0 of a mesh:
                              one wave-uniform walk per 8x8 tile of primary rays), the f64 exact tests + ray_hit in a
                              second kernel, the ray state structure-of-arrays in HBM between them.  For a mesh the
                              levels after the first run in RTX_KERNEL_BVH_REGROUP's kernel, fed from the level-1 queue.
                              For trees that hold triangles (level 0 needs the tiled ray queue and a depth <= 42); any
                              other tree with triangles takes RTX_KERNEL_BVH_REGROUP; same bits */
};

/* One entry of Scene.objects (scene.rs:80), flattened: Object{shape, material} (object.rs:9-15)
 * with Material{base_color, emission_color, roughness} (object.rs:78-86).  136 bytes. */
typedef struct RtxObject {
    uint32_t kind;               /* RTX_SPHERE | RTX_PLANE | RTX_TRIANGLE */
    uint32_t reserved;           /* must be 0 */
    double   geom[9];            /* sphere: position.xyz, radius           (sphere.rs:9-12)
                                    plane:  position.xyz, normal.xyz       (plane.rs:9-12)
                                    triangle: vertices[0..3].xyz           (triangle.rs:9-11) */
    double   base_color[3];
    double   emission_color[3];
    double   roughness;
} RtxObject;

/* Config (scene.rs:16-28) plus the two fields the build adds. */
typedef struct RtxConfig {
    uint64_t rays_per_pixel;
    uint64_t max_bounces;
    double   focal_length;
    double   focal_offset;
    double   non_focal_offset;
    uint64_t seed;               /* counter-RNG key; the reference's fastrand stream is unseedable */
    uint32_t kernel;             /* RTX_KERNEL_* */
    uint32_t tuning;             /* RTX_TUNE_* bits: A/B switches for tests and lab runs; 0 = what ships */
} RtxConfig;

/* RtxConfig.tuning.  Every combination renders the same bits (tests/test_gpu_parity.py::test_ab_knobs_keep_the_bits);
 * the library reads no environment variable for any of this.  The two tree-build fields (TRI_LEAF, BVH_MEDIAN) are read
 * when the tree is built (rtx_scene_upload / rtx_scene_append_objects / rtx_render), the others per render.
 *
 * Product and lab.  librtx_hip.so holds the kernels RTX_KERNEL_AUTO can reach plus RTX_KERNEL_EXACT / RTX_KERNEL_MIXED.
 * librtx_hip_lab.so -- the same sources with -DRTX_LAB, the same ABI, the same dispatch, loaded by the lab tests and A/B tools --
 * adds the rtx_debug_* hooks and the A/B forms behind the RTX_TUNE_LAB_MASK bits.  In both libraries
 *   - a tuning word with a bit this header does not name is refused with RTX_ERR_UNSUPPORTED by every entry point that takes a
 *     config; the product library refuses the bits of RTX_TUNE_LAB_MASK the same way;
 *   - RTX_KERNEL_BVH, RTX_KERNEL_BVH_REGROUP and RTX_KERNEL_WAVEFRONT each run the tree kernel that exists for the scene's tree
 *     (sphere tree: trace_sph_packet_kernel / trace_bvh_spheres_kernel; a tree that holds triangles: trace_bvh_mesh_kernel, as
 *     RTX_KERNEL_WAVEFRONT with the packet kernels in front; no tree: the LDS sweep); RtxStats.kernel reports the id whose
 *     kernels ran.
 * Bits 1, 19, 21, 22, 24 and 26 are retired with the experiments they selected (profiles/LAB_NOTEBOOK.md): refused, never to be reused. */
enum {
    RTX_TUNE_NO_TILES    = 1u << 0,  /* BVH kernels: ray queue in image rows instead of 8x8 pixel tiles (no packets then) */
    RTX_TUNE_NO_QNODES   = 1u << 2,  /* 96-byte footprint nodes instead of the 64-byte quantised ones */
    RTX_TUNE_NO_PACKETS  = 1u << 3,  /* primary rays walk per lane instead of one wave-uniform walk per tile */
    RTX_TUNE_WF_PURE     = 1u << 4,  /* RTX_KERNEL_WAVEFRONT on a pure (x, y)-footprint tree: every level in that form */
    RTX_TUNE_ONE_STAGE   = 1u << 5,  /* sphere trees: primary and bounced rays in one launch whatever the ray count */
    RTX_TUNE_TWO_STAGE   = 1u << 6,  /* sphere trees: two stages even below 2^20 rays per launch */
    RTX_TUNE_BVH_MEDIAN  = 1u << 7,  /* tree build: median splits instead of the binned SAH */
    RTX_TUNE_TRI_LEAF_SHIFT = 8,     /* bits 8..11: triangles per leaf, 1..6 (0 = default: 5 pure footprint tree, 2 joint) */
    RTX_TUNE_THRESH_SHIFT   = 12,    /* bits 12..18: lanes that wait before the regrouping kernels' f64 phase runs, 1..64
                                        (0 = default) */
    RTX_TUNE_PK_LDS_STACK = 1u << 20, /* mesh packets: the wave-uniform stack in LDS (round 2) instead of in the lanes of a VGPR */
    RTX_TUNE_INLINE_LEAVES = 1u << 25, /* sphere trees, 64-byte nodes: a node's leaf children are bounded inside the node visit (the
                                        earlier form) instead of being pushed and visited when popped, leaf visits apart from node visits */
    RTX_TUNE_NO_CUT = 1u << 23,      /* sphere trees: every round of a lock-step wave lasts until its longest walk ends (round 2's
                                        form) instead of leaving the last few walkers to continue beside the next segments */
    RTX_TUNE_HALVES = 1u << 27,      /* sphere trees, two stages: the launch as two halves of the samples in flight on two streams
                                      * (bit-identical, measured slower: not the default) */
    RTX_TUNE_NO_HALVES = 1u << 28,   /* ... never (today's default, spelled out) */
    RTX_TUNE_NO_TILE_LISTS = 1u << 29  /* sphere trees, two stages: every packet of primary rays walks the tree (rounds 3's form) instead of
                                        * running over its tile's list of reachable spheres */
};

#define RTX_TUNE_LAB_MASK (RTX_TUNE_NO_QNODES | RTX_TUNE_NO_PACKETS | RTX_TUNE_WF_PURE | RTX_TUNE_PK_LDS_STACK | RTX_TUNE_INLINE_LEAVES)
#define RTX_TUNE_KNOWN_MASK (RTX_TUNE_LAB_MASK | RTX_TUNE_NO_TILES | RTX_TUNE_ONE_STAGE | RTX_TUNE_TWO_STAGE | RTX_TUNE_BVH_MEDIAN | \
                             (15u << RTX_TUNE_TRI_LEAF_SHIFT) | (127u << RTX_TUNE_THRESH_SHIFT) | RTX_TUNE_NO_CUT | RTX_TUNE_HALVES | \
                             RTX_TUNE_NO_HALVES | RTX_TUNE_NO_TILE_LISTS)

/* Camera (camera.rs:7-15).  to_world_space / to_cam_space are the three ROWS of each matrix
 * (mat.rs:11-18), row-major.  Only fov, position and to_world_space are read by render
 * (scene.rs:145,196,214-221; camera.rs:65-67). */
typedef struct RtxCamera {
    double fov;
    double position[3];
    double direction[3];
    double to_cam_space[9];
    double to_world_space[9];
} RtxCamera;

/* Scene (scene.rs:78-85). */
typedef struct RtxScene {
    RtxConfig        config;
    RtxCamera        camera;
    uint64_t         n_objects;
    const RtxObject *objects;    /* Scene.objects, in order (order decides ties, scene.rs:250) */
} RtxScene;

/* Counters of one render call (optional out-parameter). */
typedef struct RtxStats {
    uint64_t primary_rays;       /* rows * width * rays_per_pixel */
    uint64_t segments;           /* closest_object queries (scene.rs:231) */
    uint64_t exact_tests;        /* f64 shape evaluations (EXACT: segments * n_objects) */
    uint64_t filter_tests;       /* f32 filter evaluations (MIXED only) */
    double   trace_ms;           /* device time of the trace kernel(s), hipEvent on the launch stream */
    double   resolve_ms;         /* device time of the per-pixel sample fold */
    uint64_t filter_mismatches;  /* RTX_KERNEL_MIXED_VERIFY only */
    uint64_t box_tests;          /* RTX_KERNEL_BVH only: ray/box slab tests (32 B node each) */
    uint32_t trace_launches;
    uint32_t kernel;             /* the RTX_KERNEL_* that ran (resolves RTX_KERNEL_AUTO) */
    /* the two-stage form of RTX_KERNEL_BVH on a sphere tree (else 0): what its stage 1 -- the primary rays, one segment
     * each -- accounts for of the totals above */
    double   stage1_ms;
    uint64_t stage1_box_tests;
    uint64_t stage1_filter_tests;
    uint64_t stage1_exact_tests;
} RtxStats;

typedef struct RtxSceneHandle_ *RtxSceneHandle;

/* Ray queries (rtx_scene_closest_hits, rtx_scene_primary_hits, rtx_closest_hits): one ray, and the answer of closest_object
 * (scene.rs:243-251) for it. */
typedef struct RtxRay {
    double position[3];
    double direction[3];         /* used as given: no hidden norm() (the shape tests normalise where the reference does) */
} RtxRay;

typedef struct RtxHit {
    double  position[3];         /* position + direction * distance (scene.rs:234); NaN when nothing is hit */
    double  normal[3];           /* Object::normal_at(position) of the winner (object.rs:37-39); NaN when nothing is hit */
    double  distance;            /* the winning Object::distance; +inf when nothing is hit */
    int64_t object;              /* the winner's index in Scene.objects (the first minimal distance wins); -1: nothing is hit */
} RtxHit;

/* Denoising guide buffers (rtx_scene_pixel_features, rtx_scene_pixel_features_blocks, rtx_pixel_features): one pixel's first hits over
 * render_pixel's own lens-jittered rays, folded as the render folds its samples. */
typedef struct RtxPixelFeatures {
    double  albedo[3];           /* mean Material.base_color of the samples' first hits (a miss adds zero) */
    double  emission[3];         /* mean Material.emission_color, likewise */
    double  normal[3];           /* mean Object::normal_at(hit point), likewise; NOT renormalised */
    double  depth;               /* mean distance over the samples that hit; +inf when none did */
    double  coverage;            /* samples that hit / rays_per_pixel */
    int64_t object;              /* sample 0's winner in Scene.objects; -1: it missed (or rays_per_pixel == 0) */
} RtxPixelFeatures;

/* The layouts a binding has to reproduce (rust/src/raytracing/hip.rs: #[repr(C)]; rust-raytracing_amd/abi.py: ctypes;
 * tests/test_abi_and_host.py checks both against these numbers). */
#ifdef __cplusplus
#define RTX_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define RTX_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif
RTX_STATIC_ASSERT(sizeof(RtxObject) == 136 && offsetof(RtxObject, geom) == 8 && offsetof(RtxObject, base_color) == 80 &&
                  offsetof(RtxObject, emission_color) == 104 && offsetof(RtxObject, roughness) == 128, "RtxObject layout");
RTX_STATIC_ASSERT(sizeof(RtxConfig) == 56 && offsetof(RtxConfig, focal_length) == 16 && offsetof(RtxConfig, seed) == 40 &&
                  offsetof(RtxConfig, kernel) == 48 && offsetof(RtxConfig, tuning) == 52, "RtxConfig layout");
RTX_STATIC_ASSERT(sizeof(RtxCamera) == 200 && offsetof(RtxCamera, position) == 8 && offsetof(RtxCamera, direction) == 32 &&
                  offsetof(RtxCamera, to_cam_space) == 56 && offsetof(RtxCamera, to_world_space) == 128, "RtxCamera layout");
RTX_STATIC_ASSERT(sizeof(RtxScene) == 272 && offsetof(RtxScene, camera) == 56 && offsetof(RtxScene, n_objects) == 256 &&
                  offsetof(RtxScene, objects) == 264, "RtxScene layout");
RTX_STATIC_ASSERT(sizeof(RtxStats) == 104 && offsetof(RtxStats, trace_ms) == 32 && offsetof(RtxStats, box_tests) == 56 &&
                  offsetof(RtxStats, trace_launches) == 64 && offsetof(RtxStats, kernel) == 68 && offsetof(RtxStats, stage1_ms) == 72 &&
                  offsetof(RtxStats, stage1_exact_tests) == 96, "RtxStats layout");
RTX_STATIC_ASSERT(sizeof(RtxRay) == 48 && offsetof(RtxRay, direction) == 24, "RtxRay layout");
RTX_STATIC_ASSERT(sizeof(RtxHit) == 64 && offsetof(RtxHit, normal) == 24 && offsetof(RtxHit, distance) == 48 &&
                  offsetof(RtxHit, object) == 56, "RtxHit layout");
RTX_STATIC_ASSERT(sizeof(RtxPixelFeatures) == 96 && offsetof(RtxPixelFeatures, emission) == 24 && offsetof(RtxPixelFeatures, normal) == 48 &&
                  offsetof(RtxPixelFeatures, depth) == 72 && offsetof(RtxPixelFeatures, coverage) == 80 &&
                  offsetof(RtxPixelFeatures, object) == 88, "RtxPixelFeatures layout");

/* -- library ----------------------------------------------------------------------------- */
int32_t     rtx_version(void);
const char *rtx_last_error(void);
int32_t     rtx_device_count(void);     /* number of usable gfx950 devices (0 when none) */
int32_t     rtx_lab_build(void);        /* 0: librtx_hip.so (the product); 1: librtx_hip_lab.so (built with -DRTX_LAB, see RtxConfig.tuning) */

/* Camera::new (camera.rs:19-28, derive_to_world_space_mat :42-49, Mat3x3::inverse
 * specific_math.rs:10-14).  Host-side, f64, reference operation order. */
int32_t rtx_camera_new(const double position[3], const double direction[3], double fov, RtxCamera *out);

/* Scene::render (scene.rs:144-170).  out_rgb: height*width*3 doubles, out_rgb[(y*width+x)*3+c]
 * == reference img[y][x].{x,y,z}; unclamped; row 0 is the reference's row 0.
 * Uploads the scene to device 0, renders, copies back. */
int32_t rtx_render(const RtxScene *scene, uint32_t width, uint32_t height, double *out_rgb);

/* Scene::render_to_image (scene.rs:172-178): `* 256`, saturating `as u8`, vertical flip.
 * out_rgb8: height*width*3 bytes. */
int32_t rtx_render_to_image(const RtxScene *scene, uint32_t width, uint32_t height, uint8_t *out_rgb8);

/* Scene::render / render_to_image on several GPUs of one node (BASELINE north_star: "tile-partitioned across the 8 GPUs
 * ... single gather over xGMI at the end"): still ONE call that returns the whole frame (scene.rs:144-170).  The scene is
 * packed once and replicated; device devices[k] renders the blocks of 8 rows k, k + n, ... (rtx_render_blocks; one host
 * thread and one stream per device, no exchange during the render: pixels are independent, scene.rs:149-160); the bands --
 * for render_to_image already quantised to 3 bytes per pixel -- are gathered on devices[0] with one peer copy each
 * (hipMemcpyPeerAsync: every peer pushes over its own xGMI link; no communicator to set up), de-interleaved there and
 * copied to the host once.  Pixel values do not depend on n_devices or the order of
 * the list.  An entry may repeat (two bands on one device) -- that is how the path is tested on a one-GPU box.
 * rtx_render(scene, w, h, out) == rtx_render_devices(scene, w, h, {0}, 1, out). */
int32_t rtx_render_devices(const RtxScene *scene, uint32_t width, uint32_t height,
                           const int32_t *devices, uint32_t n_devices, double *out_rgb);
int32_t rtx_render_to_image_devices(const RtxScene *scene, uint32_t width, uint32_t height,
                                    const int32_t *devices, uint32_t n_devices, uint8_t *out_rgb8);

/* -- split form: upload once, render many (rows / devices), output stays on the device ------ */
int32_t rtx_scene_upload(const RtxScene *scene, int32_t device, RtxSceneHandle *out);
int32_t rtx_scene_free(RtxSceneHandle scene);      /* non-zero: an earlier asynchronous render on it had failed (see "Streams") */

/* Replace the Config of an uploaded scene (rays_per_pixel, seed, kernel, ...). */
int32_t rtx_scene_set_config(RtxSceneHandle scene, const RtxConfig *config);

/* Upper bound of the per-render scratch this handle allocates on its device (sample records, ray queues), in bytes;
 * 0 = the default (24 GiB, never more than 3/4 of the memory free at render time).  A frame that needs more is traced in
 * sample batches -- same bits (the fold continues across batches).  For several handles, ranks or frameworks sharing a GPU.
 * What a launch allocates whatever its batch (a queue chunk per resident wave, counters, stack columns: 0.15-0.3 GB on a
 * 256-CU part) is taken off the limit before the batch is sized.  The floor is ONE sample of the band per launch: a limit
 * below that size is exceeded by that one sample's records + the fixed part (a frame cannot be cut finer).
 * The largest single launch the default yields, by what a ray of the launch holds: 32 B (the LDS sweep, the exhaustive kernel, the
 * mesh megakernel): ~800 M rays; 101 B (a sphere tree's two stages: + the survivors' queue): ~255 M; 408 B (the wavefront form: + two
 * sets of ray state, two record queues, candidates): ~63 M -- and never 2^32 ray slots or more.  Observed by tests/test_launch_sizes.py,
 * which holds such launches to the bits of small ones: one launch for 165.9 M rays (1920 x 1080 x 80) of the first two families and for
 * 180.4 M (16384 x 11008 x 1) of the second; the wavefront form takes 33.2 M (16 spp) in one launch and 132.7 M (64 spp) in three. */
int32_t rtx_scene_set_scratch_limit(RtxSceneHandle scene, uint64_t bytes);

/* Scene::add_object (scene.rs:126-128) on an uploaded scene: the objects are appended in order (they get the next scene
 * indices, so earlier objects still win ties, scene.rs:250), the shape arrays, filter records and the BVH are rebuilt on
 * the host and replace the resident ones; config, camera and scratch stay.  Waits for renders in flight on the handle's
 * device.  On failure (e.g. an unsupported kind) the resident scene is unchanged. */
int32_t rtx_scene_append_objects(RtxSceneHandle scene, const RtxObject *objects, uint64_t n_objects);

/* Scene.objects[indices[i]] = objects[i] for i = 0 .. n-1, in order, on an uploaded scene (the reference: shapes sit behind
 * Arc<Mutex<..>> and `material` is a pub field, object.rs:9-15, so Scene.objects[i] is mutable between renders).  `indices` and
 * `objects` are HOST arrays; when an index repeats, its last entry wins.  After a successful call every entry point of the handle
 * returns, bit for bit, what a freshly uploaded handle would return for the updated list with the same config and camera (RtxStats
 * counters may differ): every kernel decides hits in f64 and the tree only selects candidates, so a tree that keeps its topology and
 * gets new boxes finds the same winners.
 *   *how (may be NULL) reports the path:
 *   RTX_UPDATED_REBUILT   rtx_scene_append_objects' path on the modified list (host build, every array replaced).  Taken when mode is
 *                         RTX_UPDATE_REBUILD, an entry changes an object's kind or a triangle's geometry (but see "Triangles"), a new sphere is not finite,
 *                         its box leaves the range the resident tree was built for, its reach |c - centre| + |r| or the resident
 *                         sphere_cmax is not below 1e14, or the refit finds a 64-byte node it cannot encode.
 *   RTX_UPDATED_REFIT     a sphere of the tree gets new geometry: its records are rewritten and the boxes above it refitted, on the device,
 *                         one small kernel launch per tree level.  The topology is the old one: after large moves the frame is the
 *                         same but slower than after a rebuild ("Moving objects").
 *   RTX_UPDATED_RECORDS   anything else (materials of any kind -- an entry that repeats a sphere's resident geometry bit for bit is a
 *                         material update --, plane geometry, spheres of a scene without a sphere sub-tree): the records alone.
 *   RTX_UPDATED_NOTHING   n == 0.
 * Errors, found before the first device write (the resident scene is unchanged): RTX_ERR_INVALID_ARGUMENT -- a null argument, an
 * index >= n_objects, an unknown mode; RTX_ERR_UNSUPPORTED -- an unknown kind, a non-zero `reserved`.
 * "Streams" applies: the device work is enqueued on `stream` behind whatever earlier calls enqueued on the handle.  The call returns
 * after its own device work has completed (it reads back a status word and the new sphere_cmax).
 *   Triangles.  Under RTX_UPDATE_AUTO a triangle entry with new vertices ALWAYS rebuilds, and keeps doing so: callers written against
 * that mode see the path (*how) and the cost they saw before -- compatibility, nothing else.  RTX_UPDATE_DEFORM is AUTO plus the
 * in-place update of such triangles (a deforming mesh, a rigid part that moves between frames).  A triangle has a class, decided by
 * the host exactly as the upload decides it: NONE -- it can never be hit (degenerate, a non-finite normal or n.v0, or n.v0 <
 * -(1 + 1e-9)) and has no filter record; ALWAYS -- it has a record and is tested for every segment (a non-finite vertex, or a
 * projection with |det| <= 1e-6 |r| |s|); QUALIFIED(f) -- it may enter the tree with its footprint in the plane that leaves out axis f
 * (the rows Triangle::contains' elimination reads).  A triangle with new vertices is updated in place when its class and f are the
 * resident ones and, where it is qualified, every finite face of its new footprint lies within the range the resident tree was built
 * for.  *how is then RTX_UPDATED_REFIT when at least one such triangle has its record in the tree (its records and f32 footprint are
 * rewritten, the rectangles / boxes above it and their 64-byte forms refitted level by level, tri_extent taken again), and
 * RTX_UPDATED_RECORDS when all of them lie outside the tree.  Any other triangle with new vertices (a class or f change either way, a
 * non-finite vertex, a footprint beyond the range), a footprint node whose 64-byte form cannot be encoded, and everything that
 * rebuilds under AUTO give RTX_UPDATED_REBUILT.  The contract above holds for every path. */
enum { RTX_UPDATE_AUTO = 0, RTX_UPDATE_REBUILD = 1, RTX_UPDATE_DEFORM = 2 };   /* mode */
enum { RTX_UPDATED_NOTHING = 0, RTX_UPDATED_RECORDS = 1, RTX_UPDATED_REFIT = 2, RTX_UPDATED_REBUILT = 3 };   /* *how */
int32_t rtx_scene_update_objects(RtxSceneHandle scene, const uint64_t *indices, const RtxObject *objects, uint64_t n,
                                 uint32_t mode, void *stream, uint32_t *how);

/* Hides (visible == 0) or shows (visible == 1) Scene.objects[indices[i]] of an uploaded scene, in place: the reference's users
 * `retain` / `remove` objects of the pub Vec Scene.objects between renders, or skip one for a while; here the object keeps its index
 * and its slot in the tree.  `indices` is a HOST array; repeated indices are fine; an entry already in the requested state is a no-op.
 *   The contract.  After any sequence of calls on a handle, everything the handle produces -- frames under every kernel id,
 * closest-hit and any-hit queries, the pick buffer, path radiance, sparse samples, progressive sums, a refinement round, pixel
 * features -- equals, byte for byte, what a fresh upload of the list L_nan produces: the handle's current object list with the nine
 * `geom` words of every hidden object set to NaN (all-NaN geometry is "never hit" in the reference for each kind: sphere.rs:22-29 with
 * scene.rs:249's is_normal, plane.rs:21-31, triangle.rs:37-101).  L_nan has the same length, so:
 *   - indices are stable: a hit never reports a hidden object, and no other object's index moves;
 *   - frames, and hits after the monotone index map, also equal a fresh upload of the list with the hidden objects DELETED
 *     (closest_object's tie-break only needs relative order, and rng_key(seed, pix, sample) does not read an object index);
 *   - RtxStats counters may differ, as they may after an update.
 *   *how (may be NULL) reports the path with rtx_scene_update_objects' values: RTX_UPDATED_NOTHING -- no state changes;
 * RTX_UPDATED_RECORDS -- only planes and shapes outside the tree change state; RTX_UPDATED_REFIT -- a shape with a slot in the tree
 * changes state: its records are rewritten and the nodes above it refitted on the device, where a leaf whose entries are all hidden and
 * an interior child with nothing alive below become the empty slot every walk ignores (and get their words back when something below
 * is shown); RTX_UPDATED_REBUILT -- a shape being SHOWN has geometry (given by rtx_scene_update_objects while it was hidden) that
 * rtx_scene_update_objects would not take in place under RTX_UPDATE_DEFORM, the resident sphere_cmax is not below 1e14, or a 64-byte
 * node has no encoding.
 *   With the other entry points.  rtx_scene_update_objects on a hidden index updates the object and its material record and writes no
 * geometry record: the object stays hidden and its new geometry is judged when it is shown (a kind change rebuilds as ever).
 * rtx_scene_append_objects: the new objects are visible.  Any rebuild -- append, RTX_UPDATE_REBUILD, every fallback -- packs the list
 * with its real geometries and then hides the hidden set on the fresh arrays, so hidden objects keep a slot and can be shown in place.
 * The one-shot host forms and rtx_render_devices take an RtxScene, not a handle: they know no hidden set.
 *   Errors, found before the first device write (the scene is unchanged): RTX_ERR_INVALID_ARGUMENT -- a null `indices` with n > 0, an
 * index >= n_objects, visible > 1.  "Streams" applies exactly as for rtx_scene_update_objects; the call returns after its own device
 * work has completed. */
int32_t rtx_scene_set_visible(RtxSceneHandle scene, const uint64_t *indices, uint64_t n, uint32_t visible, void *stream, uint32_t *how);
int32_t rtx_scene_get_visible(RtxSceneHandle scene, uint8_t *mask /* n_objects bytes, 1 = visible */);

/* Replace the Camera of an uploaded scene without re-uploading the objects (the reference's analogue is
 * Scene.camera being a pub field, scene.rs:82, with Camera::set_direction camera.rs:35-40).  Only fov, position and
 * to_world_space are read by render. */
int32_t rtx_scene_set_camera(RtxSceneHandle scene, const RtxCamera *camera);

/*
 * Renders image rows row_begin, row_begin+row_stride, ... (n_rows of them, all < height) of the
 * width x height image into d_out_rgb, a DEVICE buffer of n_rows*width*3 doubles (row k of the
 * buffer is image row row_begin + k*row_stride).  Pixel values do not depend on the
 * partition: a pixel's RNG key is its index in the full image.  stream is a hipStream_t
 * (NULL = the device's null stream).  The call enqueues all work on `stream`; it returns
 * after the work is enqueued when stats == NULL, and after it completed (stream
 * synchronised, stats filled) otherwise.
 */
int32_t rtx_render_rows(RtxSceneHandle scene, uint32_t width, uint32_t height,
                        uint32_t row_begin, uint32_t row_stride, uint32_t n_rows,
                        double *d_out_rgb, void *stream, RtxStats *stats);

/*
 * The same for a band made of BLOCKS of rows -- what one rank / device of a multi-GPU job renders.  The frame is cut into
 * blocks of block_rows rows (block b = image rows [b * block_rows, min((b + 1) * block_rows, height))), dealt out
 * round-robin: part `part` of `n_parts` owns blocks part, part + n_parts, ...  d_out_rgb: DEVICE buffer of
 * rtx_blocks_row_count(height, block_rows, part, n_parts) * width * 3 doubles, the part's rows in increasing image order.
 * block_rows = 8 keeps the BVH kernels' 8x8 ray tiles whole (a tile of rtx_render_rows' single-row bands is 8 columns x
 * 8 * n_parts image rows: the packet walks lose a quarter to a third of their rate on it); the interleaving still balances
 * the uneven per-pixel cost (1080 rows on 8 parts: 17 or 16 blocks each).  Pixels do not depend on the partition.
 * rtx_render_blocks(h, w, hgt, 1, r, n, ...) == rtx_render_rows(h, w, hgt, r, n, rows, ...).
 */
uint32_t rtx_blocks_row_count(uint32_t height, uint32_t block_rows, uint32_t part, uint32_t n_parts);
int32_t rtx_render_blocks(RtxSceneHandle scene, uint32_t width, uint32_t height,
                          uint32_t block_rows, uint32_t part, uint32_t n_parts,
                          double *d_out_rgb, void *stream, RtxStats *stats);

/*
 * Progressive sampling: the samples [sample_begin, sample_begin + n_samples) of every pixel of rtx_render_blocks' band (the same
 * partition, the same row order; the rows form is block_rows = 1, the full frame (8, 0, 1)), ADDED to the caller's running sums.
 * d_sum and d_sum_sq (may be NULL) are DEVICE buffers of rtx_blocks_row_count(...) * width * 3 doubles, read and written; they must
 * not overlap.  For every pixel p of the band and s = sample_begin, ..., in order, with c = the render's sample s of that pixel
 * (render_pixel's ray for the key rng_key(seed, y * width + x, s), then render_ray):
 *     d_sum[3 p + k]    = d_sum[3 p + k] + c_k
 *     d_sum_sq[3 p + k] = d_sum_sq[3 p + k] + c_k * c_k        (a rounded multiply, then a rounded add: never fused)
 * Nothing is divided and RtxConfig.rays_per_pixel is not read; every other field of the handle's config, and its camera, is read as a
 * render reads it.
 *  - The contract with the full render: with buffers that start as all-zero bytes and calls whose ranges tile [0, S) in increasing
 *    order, d_sum / (double)S is the frame rtx_render_blocks gives at rays_per_pixel = S, bit for bit -- for any split of the range,
 *    any scratch limit (sample batches inside a call) and any kernel id.  It needs a buffer that holds zero bytes or an earlier call's
 *    output: the fold skips zero samples (which leave a sum that started at +0.0 unchanged), so a caller's -0.0 stays -0.0 where the
 *    full fold would make it +0.0.
 *  - n_samples == 0, and a scene without objects (every sample is zero): nothing is touched.
 *  - sample_begin + n_samples > 2^32 - 1, a NULL d_sum, 2^32 - 16 pixels per call or more: RTX_ERR_INVALID_ARGUMENT.
 *  - The tile lists of the primary rays are rebuilt by every call (the camera may have changed since the previous range).
 * Streams, stats == NULL asynchrony, the watchdog word and RtxConfig.tuning follow rtx_render_blocks (RTX_TUNE_HALVES is not used: the
 * call takes the batch path).  stats: primary_rays = pixels * n_samples and the render's fields.  (DESIGN.md "Progressive and
 * adaptive sampling".)
 */
int32_t rtx_render_blocks_accumulate(RtxSceneHandle scene, uint32_t width, uint32_t height,
                                     uint32_t block_rows, uint32_t part, uint32_t n_parts,
                                     uint64_t sample_begin, uint64_t n_samples,
                                     double *d_sum, double *d_sum_sq, void *stream, RtxStats *stats);

/* -- ray queries on an uploaded scene ----------------------------------------------------------
 * Each answer is exactly what the reference's closest_object(position, direction) returns over Scene.objects (the first minimal
 * distance wins, is_normal && is_sign_positive filter), filled in as RtxHit describes; a scene without objects hits nothing.
 * RtxConfig.kernel of the handle picks the path: RTX_KERNEL_EXACT tests every shape of every ray in f64; any other id walks the
 * scene's tree (query_closest_kernel, DESIGN.md "Ray queries") where it has one -- the same bits.  Rays the walk's f32 bounds were
 * not derived for (|d.d - 1| > 2^-40 or a non-finite component, an origin beyond the tree's far range) are swept exhaustively:
 * slower, the same bits.  The "Streams" rules apply; RtxConfig.tuning bits of RTX_TUNE_LAB_MASK are refused as for renders.
 * With stats == NULL the call returns once the work is enqueued on `stream`; else it synchronises and fills stats: segments = n,
 * exact_tests, filter_tests, box_tests, trace_ms, trace_launches = 1, kernel = RTX_KERNEL_BVH (a tree walk) or RTX_KERNEL_EXACT.
 *
 * rtx_scene_closest_hits: d_rays / d_hits are DEVICE arrays of n entries (must not overlap); n < 2^32. */
int32_t rtx_scene_closest_hits(RtxSceneHandle scene, const RtxRay *d_rays, uint64_t n, RtxHit *d_hits,
                               void *stream, RtxStats *stats);

/* The pick buffer: per pixel of a width x height frame, the hit of the ray render_pixel builds when focal_offset =
 * non_focal_offset = 0 (scene.rs:196-209): position = camera.position, direction = ((p + get_ray_dir(x/w, y/h, vfov) *
 * focal_length) - p).norm().  d_hits: DEVICE array [y][x], row 0 = the reference's row 0 (as rtx_render); width * height < 2^32.
 * Independent of the RNG, the seed and both offsets of the handle's config. */
int32_t rtx_scene_primary_hits(RtxSceneHandle scene, uint32_t width, uint32_t height, RtxHit *d_hits,
                               void *stream, RtxStats *stats);

/* One-shot host form (as rtx_render is to rtx_render_rows): uploads to device 0, queries, copies back.  rays / hits: HOST arrays. */
int32_t rtx_closest_hits(const RtxScene *scene, const RtxRay *rays, uint64_t n, RtxHit *hits);

/* Occlusion (any-hit) queries: shadow rays, ambient occlusion, line of sight.  For ray i with limit t_max[i]:
 *   occluded[i] = 1 iff some object of Scene.objects has Object::distance(position, direction) = Some(t) with t.is_normal() &&
 *   t.is_sign_positive() (closest_object's filter, scene.rs:249) and t < t_max[i] (strict); else 0
 * -- exactly (rtx_scene_closest_hits' distance < t_max[i]), without the search for the nearest surface: the limit prunes the walk,
 * and a ray stops at the first surface that certainly lies before it (DESIGN.md "Occlusion queries").
 *  - t_max is compared as given: +inf asks for any hit at all; NaN, zero or a negative limit is never occluded (0, nothing is tested).
 *  - d_t_max == NULL means +inf for every ray.
 *  - Directions are used as given, exactly as for closest hits.  A surface the ray starts on is found like any other -- the
 *    reference's |t| ~ 1e-16 self-hits included: callers who do not want that offset their origins.  No hidden epsilon, no t_min.
 *  - A scene without objects answers 0 everywhere (one memset, no launch: stats has segments = n and nothing else).
 * d_rays: n RtxRay; d_t_max: n doubles or NULL; d_occluded: n bytes, 1 / 0.  DEVICE arrays, pairwise non-overlapping; n < 2^32.
 * Streams, stats == NULL asynchrony, RtxConfig.tuning bits of RTX_TUNE_LAB_MASK, RTX_KERNEL_EXACT (every shape of every ray in f64,
 * up to the first one before the limit): as rtx_scene_closest_hits.  stats: segments = n, exact_tests, filter_tests, box_tests (the
 * tests actually made), trace_ms, trace_launches = 1, kernel = RTX_KERNEL_BVH | RTX_KERNEL_EXACT. */
int32_t rtx_scene_any_hits(RtxSceneHandle scene, const RtxRay *d_rays, const double *d_t_max, uint64_t n, uint8_t *d_occluded,
                           void *stream, RtxStats *stats);

/* One-shot host form (upload to device 0, query, copy back), as rtx_closest_hits.  rays / t_max (or NULL) / occluded: HOST arrays. */
int32_t rtx_any_hits(const RtxScene *scene, const RtxRay *rays, const double *t_max, uint64_t n, uint8_t *occluded);

/* Multi-hit queries: the k nearest surfaces along each ray -- select-through picking, x-ray and thickness views, transparency done by
 * the caller, counting the surfaces between two points.  For ray i, with L_i = the objects of Scene.objects whose
 * Object::distance(position, direction) = Some(t) has t.is_normal() && t.is_sign_positive() (closest_object's filter, scene.rs:249)
 * and t < t_max[i] (strict), sorted by (t, index in Scene.objects):
 *   d_hits[i * k + j], j < min(k, |L_i|) = the j-th element, filled in as RtxHit describes for closest hits (distance, object,
 *       position = position + direction * distance, normal = normal_at(position) of that object);
 *   d_hits[i * k + j], j >= min(k, |L_i|) = the "nothing" record of a closest-hit miss (NaN position and normal, +inf distance, -1);
 *   d_counts[i] = min(k, |L_i|)                                                               (d_counts may be NULL)
 * -- entry j is what closest_object returns once the winners of entries 0 .. j-1 have been retain()ed out of Scene.objects: the
 * stable order of min_by + total_cmp, applied k times.  Every distance is the reference's f64 test, bit for bit.
 *  - 1 <= k <= RTX_MULTI_HIT_MAX, else RTX_ERR_INVALID_ARGUMENT; n < 2^32; i * k + j is 64-bit arithmetic.
 *  - One entry per object: a sphere gives its entry root only, and nothing when the ray starts inside it (sphere.rs:29).
 *  - Equal distances come in index order.  Hidden objects (rtx_scene_set_visible) are absent, as from every product of the handle.
 *  - t_max is compared as given, as for rtx_scene_any_hits: d_t_max == NULL means +inf for every ray; NaN, zero or a negative limit
 *    gives count 0 and k nothing records, and nothing is tested.  The list for a limit is the prefix of the unlimited list below it.
 *  - Directions are used as given; no epsilon, no t_min: the |t| ~ 1e-16 self-hits are found like any other hit.
 *  - With k = 1 and d_t_max == NULL the record is rtx_scene_closest_hits' record, byte for byte; count > 0 is rtx_scene_any_hits'
 *    answer for the same limit.  A scene without objects writes the nothing records.
 * d_rays: n RtxRay; d_t_max: n doubles or NULL; d_hits: n * k RtxHit; d_counts: n uint32_t or NULL.  DEVICE arrays, pairwise
 * non-overlapping.  While a ray is walked its k records hold the lane's sorted list (DESIGN.md "Multi-hit queries"): their content is
 * undefined until the call's work on the stream has finished.  Streams, stats == NULL asynchrony, RtxConfig.tuning bits of
 * RTX_TUNE_LAB_MASK, RTX_KERNEL_EXACT (every shape of every ray in f64), the exhaustive sweep for rays the f32 bounds were not
 * derived for: as rtx_scene_closest_hits.  stats: segments = n, exact_tests, filter_tests, box_tests, trace_ms, trace_launches = 1,
 * kernel = RTX_KERNEL_BVH | RTX_KERNEL_EXACT. */
#define RTX_MULTI_HIT_MAX 32
int32_t rtx_scene_multi_hits(RtxSceneHandle scene, const RtxRay *d_rays, const double *d_t_max, uint64_t n, uint32_t k,
                             RtxHit *d_hits, uint32_t *d_counts, void *stream, RtxStats *stats);

/* The same for the pick buffer's rays: rtx_scene_primary_hits' zero-offset primary ray of every pixel, no limit.  d_hits: DEVICE array
 * [y][x][j] of width * height * k records; d_counts: [y][x] or NULL; width * height < 2^32; stats: segments = width * height. */
int32_t rtx_scene_primary_multi_hits(RtxSceneHandle scene, uint32_t width, uint32_t height, uint32_t k,
                                     RtxHit *d_hits, uint32_t *d_counts, void *stream, RtxStats *stats);

/* One-shot host form (upload to device 0, query, copy back), as rtx_closest_hits.  rays / t_max (or NULL) / hits / counts (or NULL):
 * HOST arrays. */
int32_t rtx_multi_hits(const RtxScene *scene, const RtxRay *rays, const double *t_max, uint64_t n, uint32_t k,
                       RtxHit *hits, uint32_t *counts);

/* Path-radiance queries: render_ray (scene.rs:223-242), the bounce loop that turns a ray into a colour, for the caller's rays -- the
 * path tracer without the reference's camera (panoramas, stereo pairs, light probes at pick() / query() points, debug rays).
 * For entry i, with the handle's RtxConfig supplying max_bounces and seed (rays_per_pixel, focal_* and the camera are not read):
 *  - ray = Ray::new(position, direction), the direction used as given (no hidden norm()); resulting_color = 0, light_color = 1.
 *  - Up to max_bounces + 1 times: stop if light_color == zeros; closest_object -- on None, stop; else position += direction * dst
 *    and ray_hit (scene.rs:260-278).
 *  - d_rgb[3 i .. 3 i + 2] = resulting_color, unclamped.  d_segments[i] = the closest_object calls the path made; d_segments may
 *    be NULL.
 *  - Randomness: key = rng_key(config.seed, d_ids[2 i], d_ids[2 i + 1]), a (pixel index, sample index) pair; d_ids == NULL means
 *    (i, 0).  Bounce b draws indices 6 + 2 b and 7 + 2 b; indices 0..5 stay the lens jitter's.  So a caller who brings
 *    render_pixel's own ray for (pixel, sample) gets that sample of rtx_render bit for bit, and summing S samples in sample order
 *    and dividing by S gives the render's pixel.  A path's result depends only on its ray, its id pair and the scene -- never on
 *    n, on its position in the batch or on its neighbours.
 *  - A scene without objects (scene.rs:224): zeros, nothing is asked -- one memset of d_rgb (and of d_segments), no launch,
 *    stats->segments = 0.
 *  - A segment whose ray the walk's f32 bounds were not derived for (a non-unit or non-finite direction, a far or NaN origin) is
 *    swept exhaustively, as for closest hits; bounced directions are normalised, so later segments walk.  RTX_KERNEL_EXACT: every
 *    segment swept -- the same bits.  No self-hit pre-test and no epsilon, as for the other queries.
 * d_rays: n RtxRay; d_ids: 2 n uint64 or NULL; d_rgb: 3 n doubles; d_segments: n uint32 or NULL.  DEVICE arrays, pairwise
 * non-overlapping; n < 2^32.  Streams, stats == NULL asynchrony, RtxConfig.tuning bits of RTX_TUNE_LAB_MASK: as rtx_scene_any_hits.
 * stats: primary_rays = n, segments = all closest_object calls, exact_tests, filter_tests, box_tests, trace_ms,
 * trace_launches = 1, kernel = RTX_KERNEL_BVH | RTX_KERNEL_EXACT.  (DESIGN.md "Path queries".) */
int32_t rtx_scene_trace_paths(RtxSceneHandle scene, const RtxRay *d_rays, const uint64_t *d_ids, uint64_t n,
                              double *d_rgb, uint32_t *d_segments, void *stream, RtxStats *stats);

/* One-shot host form (upload to device 0, trace, copy back), as rtx_closest_hits.  rays / ids (or NULL) / rgb / segments (or NULL):
 * HOST arrays. */
int32_t rtx_trace_paths(const RtxScene *scene, const RtxRay *rays, const uint64_t *ids, uint64_t n, double *rgb, uint32_t *segments);

/* Sparse samples of the render: entry i names (pixel, sample) = (d_ids[2 i], d_ids[2 i + 1]), pixel = y * width + x in the full
 * width x height frame, and gets that sample of rtx_render bit for bit -- what an adaptive sampler traces where the variance is.
 *  - The kernel builds render_pixel's own ray (scene.rs:196-207: the key rng_key(seed, pixel, sample), draws 0..5, the handle's
 *    non_focal_offset, focal_offset, focal_length and camera), then runs render_ray exactly as rtx_scene_trace_paths does (draws from
 *    6 on): d_rgb[3 i .. 3 i + 2] = resulting_color, d_segments[i] (d_segments may be NULL) = its closest_object calls.
 *  - The result does not depend on n, on the entry's place in the batch or on its neighbours; repeated ids are allowed.  Adding a
 *    pixel's samples in sample order to the sums of rtx_render_blocks_accumulate continues that fold.
 *  - An entry with pixel >= width * height or sample >= 2^32 gets NaN colour and 0 segments; nothing is traced for it.
 *  - A scene without objects: one memset of d_rgb (and of d_segments), no launch, the ids are not read -- as rtx_scene_trace_paths.
 * d_ids: 2 n uint64 (required); d_rgb: 3 n doubles; d_segments: n uint32 or NULL.  DEVICE arrays, pairwise non-overlapping; n < 2^32;
 * 0 < width * height < 2^32 - 16.  Streams, stats == NULL asynchrony, RTX_KERNEL_EXACT, RtxConfig.tuning bits of RTX_TUNE_LAB_MASK and
 * stats: as rtx_scene_trace_paths.  (DESIGN.md "Progressive and adaptive sampling".) */
int32_t rtx_scene_trace_samples(RtxSceneHandle scene, uint32_t width, uint32_t height, const uint64_t *d_ids, uint64_t n,
                                double *d_rgb, uint32_t *d_segments, void *stream, RtxStats *stats);

/* Refinement to a noise threshold, decided on the device: every pixel of rtx_render_blocks_accumulate's band (the same partition, the
 * same row order) that the rule below selects gets further samples of the render, folded into the caller's running sums, for up to
 * `rounds` rounds -- no ids, no colours and no choice travel through the host.
 *  - d_sum, d_sum_sq: that call's DEVICE buffers (both required).  d_extra: one uint32 per pixel of the band, in the same order: the
 *    samples the pixel has had beyond sample_begin.  A caller accumulates [0, sample_begin), zeroes d_extra with a memset, then calls
 *    this, again and again if it likes.  The three buffers must not overlap.
 *  - The rule.  Pixel p has n = sample_begin + d_extra[p] samples, sums S[3] and sums of squares Q[3].  It is selected iff
 *    n < max_samples && (n < 2 || e > b * b), with dn = (double)n and
 *        v_k = Q_k - S_k * S_k / dn                      (k = 0, 1, 2)
 *        e   = ((v_0 + v_1) + v_2) / (dn - 1.0) / dn     the summed per-channel variance of the mean
 *        m   = ((S_0 + S_1) + S_2) / dn
 *        b   = threshold * (m + floor)
 *    every operation a separately rounded f64 operation in exactly this order (plain numpy reproduces the decision bit for bit); a
 *    comparison with a NaN is false, so a NaN pixel is selected only while n < 2.
 *  - A round.  A selected pixel traces min(n_more, max_samples - n) further samples, numbered n, n + 1, ...: each the render's own
 *    (render_pixel's ray for the key rng_key(seed, y * width + x, s), then render_ray, as rtx_scene_trace_samples runs it), and after
 *    each sample c: d_sum[3 p + k] += c_k, then d_sum_sq[3 p + k] += c_k * c_k (the multiply rounded, then the add; plain adds, which
 *    on buffers that hold zero bytes or earlier outputs give the bits of rtx_render_blocks_accumulate's fold).  d_extra[p] advances by
 *    the samples traced.  Then the rule is evaluated again; the pixel goes on for up to `rounds` rounds in this call.
 *  - A pixel's sequence depends on nothing but its own samples: one call with rounds = k equals k calls with rounds = 1, for any
 *    partition; and a pixel with n samples holds the render's samples 0 .. n - 1 folded in order, so d_sum / n is the render's pixel at
 *    rays_per_pixel = n, bit for bit.
 *  - result: a HOST array of 3 uint64, or NULL: [0] pixels that traced at least one sample, [1] samples traced, [2] pixels the rule
 *    still selects after the call -- 0 means converged or capped everywhere: the caller's stop signal.
 *  - max_samples <= sample_begin: nothing is selected, nothing is touched.  A scene without objects: nothing is touched, nothing is
 *    launched, result is all zeros (as rtx_render_blocks_accumulate).
 *  - RTX_ERR_INVALID_ARGUMENT: a NULL d_sum, d_sum_sq or d_extra; overlapping buffers; n_more == 0 or rounds == 0; threshold or floor
 *    NaN or negative; sample_begin > 2^32 - 1; a bad partition; 2^32 - 16 pixels per call or more.
 * RtxConfig.rays_per_pixel is not read.  No sample records, survivors' queue or tile lists are allocated: the scratch limit does not
 * apply.  Streams, the watchdog word, RtxConfig.tuning bits of RTX_TUNE_LAB_MASK and RTX_KERNEL_EXACT (every segment swept): as
 * rtx_scene_trace_samples.  With result == NULL && stats == NULL the call only enqueues; else it synchronises.  stats: primary_rays =
 * samples traced; segments, exact_tests, filter_tests, box_tests, trace_ms, trace_launches = 1 and kernel as rtx_scene_trace_samples.
 * (DESIGN.md "Refinement to a threshold".) */
int32_t rtx_render_blocks_refine(RtxSceneHandle scene, uint32_t width, uint32_t height,
                                 uint32_t block_rows, uint32_t part, uint32_t n_parts,
                                 uint64_t sample_begin, uint32_t n_more, uint32_t max_samples, uint32_t rounds,
                                 double threshold, double floor,
                                 double *d_sum, double *d_sum_sq, uint32_t *d_extra,
                                 uint64_t *result, void *stream, RtxStats *stats);

/* One-shot host form (upload to device 0, trace, copy back), as rtx_closest_hits.  ids / rgb / segments (or NULL): HOST arrays. */
int32_t rtx_trace_samples(const RtxScene *scene, uint32_t width, uint32_t height, const uint64_t *ids, uint64_t n, double *rgb,
                          uint32_t *segments);

/* Denoising guide buffers: the per-pixel first-hit albedo, emission, normal and depth (the "auxiliary feature" / AOV buffers a
 * denoiser reads next to the beauty frame), taken over the SAME lens-jittered primary rays as the render, so that depth-of-field blur
 * and edge coverage in the guides line up with the image (the pick buffer of rtx_scene_primary_hits uses the zero-offset ray: it is
 * sharp where the render is blurred).  For pixel (x, y) of the width x height frame, with S = the handle's rays_per_pixel, for
 * s = 0 .. S - 1 in order:
 *  - the ray is exactly render_pixel's (scene.rs:196-207): key = rng_key(seed, y * width + x, s), draws 0..5; non_focal_offset,
 *    focal_offset, focal_length and the camera come from the handle; max_bounces is not read.
 *  - closest_object of that ray.  On Some((dst, obj)): albedo sum += base_color, emission sum += emission_color, normal sum +=
 *    obj.normal_at(position + direction * dst), depth sum += dst, hits += 1 -- component-wise f64 adds from +0.0, in sample order.  On
 *    None nothing is added.
 * Then albedo, emission, normal = sum / (double)S (a division, as the render's fold: iter_ops.rs:4-8); coverage = (double)hits /
 * (double)S; depth = depth sum / (double)hits, +inf when hits == 0; object = sample 0's winner, -1 when it missed.  S == 0: 0 / 0 = NaN
 * for the four means (as the render's NaN pixels), depth = +inf, object = -1.  S >= 2^32: RTX_ERR_INVALID_ARGUMENT.
 *  - `emission` is, bit for bit, the pixel rtx_render_rows produces with max_bounces = 0 and the same config: a one-segment render_ray
 *    returns 0 + 1 * emission_color, and the fold is the same left sum from zero divided by S (0 + 1 * e differs from e only for
 *    e = -0.0, and added to a sum that started at +0.0 both give the same sum).
 *  - d_features: DEVICE array [y][x], row 0 = the reference's row 0.  The blocks form writes the rows of part `part` of `n_parts`
 *    (blocks of block_rows rows dealt out round-robin) in increasing image order, exactly as rtx_render_blocks does:
 *    rtx_blocks_row_count(height, block_rows, part, n_parts) * width records.  Pixels do not depend on the partition;
 *    rtx_scene_pixel_features(h, w, hgt, ...) == rtx_scene_pixel_features_blocks(h, w, hgt, 8, 0, 1, ...).  Pixels per call < 2^32 - 16,
 *    as for renders.
 *  - A scene without objects is no special case: the launch runs and every sample misses (zeros, depth +inf, object -1, coverage 0).
 * Streams, stats == NULL asynchrony, RtxConfig.tuning bits of RTX_TUNE_LAB_MASK, RTX_KERNEL_EXACT (every ray swept, the same bits): as
 * rtx_scene_closest_hits.  stats: primary_rays = segments = pixels * S, exact_tests, filter_tests, box_tests, trace_ms,
 * trace_launches = 1, kernel = RTX_KERNEL_BVH | RTX_KERNEL_EXACT.  (DESIGN.md "Pixel features".) */
int32_t rtx_scene_pixel_features(RtxSceneHandle scene, uint32_t width, uint32_t height, RtxPixelFeatures *d_features,
                                 void *stream, RtxStats *stats);
int32_t rtx_scene_pixel_features_blocks(RtxSceneHandle scene, uint32_t width, uint32_t height,
                                        uint32_t block_rows, uint32_t part, uint32_t n_parts,
                                        RtxPixelFeatures *d_features, void *stream, RtxStats *stats);

/* One-shot host form (upload to device 0, query, copy back), as rtx_closest_hits.  features: HOST array of width * height records. */
int32_t rtx_pixel_features(const RtxScene *scene, uint32_t width, uint32_t height, RtxPixelFeatures *features);

/* Device epilogue of render_to_image on a full device image (scene.rs:175-178):
 * d_rgb height*width*3 doubles -> d_rgb8 height*width*3 bytes, flipped vertically. */
int32_t rtx_quantize_image_device(const double *d_rgb, uint32_t width, uint32_t height,
                                  uint8_t *d_rgb8, int32_t device, void *stream);

/* Denoising a low-sample frame: an edge-avoiding a-trous (dilated B3-spline) wavelet filter over a full [y][x] f64 frame in device
 * memory, guided by the frame's RtxPixelFeatures and, when the caller has it, by the per-pixel variance of the mean, which is filtered
 * along with the colour (the spatial filter of SVGF; its temporal part is rtx_temporal_accumulate_device, below, whose outputs feed
 * this call unchanged).  What a 4 to 64 spp frame of rtx_render_blocks_accumulate goes
 * through before rtx_quantize_image_device.  The call takes no scene handle.  Only the FULL frame: a band cannot be filtered without
 * its neighbours' rows, so the bands of a multi-device render are gathered first; multi-device denoising is out of scope.
 *
 * This comment is the specification: every operation below is one separately rounded f64 operation (IEEE add, subtract, multiply,
 * divide; never fused), in exactly the written order and bracketing, so plain numpy (tests/denoise_model.py) gives the same bits.
 * Comparisons with a NaN are false.  "finite" means neither NaN nor an infinity.  Pixel p = (x, y), row 0 = the reference's row 0;
 * c = d_rgb[3 p ..], var = d_var[3 p ..], and e = emission, a = albedo, n = normal, z = depth of d_features[p].  D = the flag
 * RTX_DENOISE_DEMODULATE; V = (d_var != NULL).
 *
 * Preparation, per pixel and channel k:
 *     D:      u_k = a_k > albedo_min ? (c_k - e_k) / a_k : (c_k - e_k)        V: v_k = a_k > albedo_min ? var_k / (a_k * a_k) : var_k
 *     not D:  u_k = c_k                                                      V: v_k = var_k
 *     V:      nv = (v_0 + v_1) + v_2            -- taken again from the new v after every pass
 *
 * Pass i = 0 .. passes - 1 has step s = 2^i and maps (u, v, nv) to (u', v', nv') for every pixel at once (all reads see the pass's
 * input).  For centre p:
 *   - a centre with a u_p component that is not finite keeps u' = u_p, v' = v_p.  Else:
 *   - V: gv = g / gw with g = gw = +0.0 and, for dy = -1, 0, 1 (outer) and dx = -1, 0, 1 (inner), for every q = p + (dx, dy) inside
 *     the frame: g = g + m * nv_q, gw = gw + m, m = {1, 2, 1}[dx + 1] * {1, 2, 1}[dy + 1];   cden = (sigma_color * sigma_color) * gv +
 *     epsilon
 *   - sc_k = sv_k = sw = +0.0, then for dy = -2 .. 2 (outer) and dx = -2 .. 2 (inner) the tap q = p + s * (dx, dy):
 *       h  = b[dx + 2] * b[dy + 2], b = {1/16, 1/4, 3/8, 1/4, 1/16}                                  (dyadic: exact)
 *       the centre tap (dx = dy = 0): w = h.  Any other tap: skipped when q is outside the frame, else
 *       wn = 1 when normal_power_log2 == RTX_DENOISE_NO_NORMAL, else t = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z;
 *            t = t > 0 ? t : 0;  normal_power_log2 times: t = t * t;  wn = t
 *       wz = 1 when sigma_depth == +inf; else, both z_p and z_q finite: r = (z_p - z_q) / (sigma_depth * (z_p + z_q)),
 *            wz = 1 / (1 + r * r); neither finite: wz = 1; exactly one finite: wz = 0
 *       wa = 1 when sigma_albedo == +inf; else d_k = a_p,k - a_q,k, da = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2,
 *            wa = 1 / (1 + da / (sigma_albedo * sigma_albedo))
 *       wc = 1 when not V or sigma_color == +inf; else d_k = u_p,k - u_q,k, d2 = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2,
 *            wc = 1 / (1 + d2 / cden)
 *       w  = (((h * wn) * wz) * wa) * wc
 *       the tap is skipped when !(w > 0) (which removes a NaN weight too) or when a component of u_q is not finite; a tap that is
 *       kept adds  sc_k = sc_k + w * u_q,k,   sw = sw + w,   V: sv_k = sv_k + (w * w) * v_q,k
 *   - u'_k = sc_k / sw;   V: v'_k = sv_k / (sw * sw), nv' = (v'_0 + v'_1) + v'_2.     (The centre tap is always kept: sw >= 9/64.)
 *
 * After the last pass:  D: d_out[3 p + k] = a_k > albedo_min ? u_k * a_k + e_k : u_k + e_k  (the multiply is rounded, then the add);
 * not D: d_out = u.  d_var_out (V only) likewise: D && a_k > albedo_min ? v_k * (a_k * a_k) : v_k.  With passes == 0 d_out is a byte
 * copy of d_rgb and d_var_out one of d_var: no arithmetic at all.
 *
 * Buffers.  d_rgb, d_out: width * height * 3 doubles.  d_var (may be NULL: no colour term, no variance is tracked) and d_var_out (may
 * be NULL; must be NULL when d_var is): the same.  d_features: width * height records.  d_work: rtx_denoise_work_bytes(width, height,
 * params) bytes, 16-byte aligned (may be NULL when that is 0): the packed 128-byte pixel records {u, v, nv, z, n, a} of a pass's input
 * and output -- one buffer for one pass, two for more.  The library allocates nothing and reads nothing it has not written itself in
 * d_out, d_var_out and d_work.  rtx_denoise_device only enqueues on `stream` (a hipStream_t; NULL = the device's null stream): one
 * preparation launch and one launch per pass.
 * RTX_ERR_INVALID_ARGUMENT, decided before any device is looked for: a NULL params, d_rgb, d_features, d_out, or d_work where work
 * bytes are needed; a d_var_out without d_var; a misaligned d_work; any overlap among the input, output and work buffers; width *
 * height == 0 or >= 2^32 - 16; passes > RTX_DENOISE_MAX_PASSES; a flag bit other than RTX_DENOISE_DEMODULATE; normal_power_log2 > 8
 * and not RTX_DENOISE_NO_NORMAL; reserved != 0; a sigma that is NaN or <= 0 (+inf is allowed: it deletes the term); epsilon or
 * albedo_min NaN, negative or infinite.  rtx_denoise_work_bytes returns 0 for arguments the call would refuse.
 * (DESIGN.md 3.14 "Denoising".) */
#define RTX_DENOISE_MAX_PASSES 8
#define RTX_DENOISE_DEMODULATE 1u
#define RTX_DENOISE_NO_NORMAL  0xFFFFFFFFu
typedef struct RtxDenoiseParams {
    uint32_t passes;             /* 0..RTX_DENOISE_MAX_PASSES; pass i uses step 2^i */
    uint32_t flags;              /* RTX_DENOISE_DEMODULATE or 0 */
    uint32_t normal_power_log2;  /* 0..8: the clamped normal dot product is squared this many times; RTX_DENOISE_NO_NORMAL: no normal term */
    uint32_t reserved;           /* must be 0 */
    double   sigma_color;        /* > 0, in standard deviations of the pixel's own noise; +inf: no colour term */
    double   sigma_depth;        /* > 0, relative depth difference at which the weight is 1/2; +inf: no depth term */
    double   sigma_albedo;       /* > 0, albedo distance at which the weight is 1/2; +inf: no albedo term */
    double   epsilon;            /* >= 0, finite: added to the colour term's denominator */
    double   albedo_min;         /* >= 0, finite: channels with albedo at or below it are not demodulated */
} RtxDenoiseParams;
RTX_STATIC_ASSERT(sizeof(RtxDenoiseParams) == 56 && offsetof(RtxDenoiseParams, flags) == 4 && offsetof(RtxDenoiseParams, normal_power_log2) == 8 &&
                  offsetof(RtxDenoiseParams, reserved) == 12 && offsetof(RtxDenoiseParams, sigma_color) == 16 &&
                  offsetof(RtxDenoiseParams, sigma_depth) == 24 && offsetof(RtxDenoiseParams, sigma_albedo) == 32 &&
                  offsetof(RtxDenoiseParams, epsilon) == 40 && offsetof(RtxDenoiseParams, albedo_min) == 48, "RtxDenoiseParams layout");

/* The defaults (DESIGN.md 3.14 records how they were chosen): 5 passes, RTX_DENOISE_DEMODULATE, normal_power_log2 = 0, sigma_color = 2,
 * sigma_depth = 0.1, sigma_albedo = 0.5, epsilon = 1e-10, albedo_min = 1e-3. */
void     rtx_denoise_default_params(RtxDenoiseParams *out);
uint64_t rtx_denoise_work_bytes(uint32_t width, uint32_t height, const RtxDenoiseParams *params);
int32_t  rtx_denoise_device(const double *d_rgb, const double *d_var, const RtxPixelFeatures *d_features, uint32_t width, uint32_t height,
                            const RtxDenoiseParams *params, double *d_out, double *d_var_out, void *d_work, int32_t device, void *stream);
/* One-shot host form (device 0: allocates, copies, denoises, copies back), as rtx_closest_hits.  Every pointer is a HOST array; var and
 * var_out may be NULL as above. */
int32_t  rtx_denoise(const double *rgb, const double *var, const RtxPixelFeatures *features, uint32_t width, uint32_t height,
                     const RtxDenoiseParams *params, double *out, double *var_out);

/* Temporal accumulation: a frame of a sequence on one resident scene (rtx_scene_set_camera, rtx_scene_update_objects,
 * rtx_scene_set_visible between frames) takes over the previous frame's accumulated samples wherever the same surface is still seen.
 * For every pixel: where was its surface point in the previous frame (reprojection through the previous camera), did the previous
 * frame see the same surface there (object, normal and tangent-plane tests on the four surrounding pixels), and if so the history is
 * blended in, with the variance of the mean and a history length carried along.  d_out_rgb and d_out_var are what rtx_denoise_device
 * takes as d_rgb and d_var; d_out_rgb, d_out_var, d_out_len and this frame's d_hits are the next frame's history.  d_hits and
 * d_hist_hits are pick buffers of rtx_scene_primary_hits (the sharp zero-offset rays: position, normal, object) of this and of the
 * previous frame, both of the same width x height.  The call takes no scene handle, allocates nothing and only enqueues ONE launch on
 * `stream` (a hipStream_t; NULL = the device's null stream).
 *
 * This comment is the specification: every operation below is one separately rounded f64 operation (IEEE add, subtract, multiply,
 * divide, square root; never fused), in exactly the written order and bracketing, so plain Python floats (tests/temporal_model.py)
 * give the same bits.  Comparisons with a NaN are false.  "finite" means neither NaN nor an infinity.  a . b = (a.x * b.x + a.y * b.y)
 * + a.z * b.z.  Pixel p = (x, y), row 0 = the reference's row 0.
 *
 * Tables (rtx_temporal_tables; host only, no device is looked for): Tx[i] = sin(fov * (i / width - 0.5)), i = 0 .. width, followed by
 * Ty[j] = sin(vfov * (j / height - 0.5)), j = 0 .. height, vfov = height / width * fov -- (width + 1) + (height + 1) doubles; the
 * divisions are of the integers as doubles; sin is the host libm's.  These are the sines of the render's own pixel map (scene.rs:145,
 * :153-157, :214-215; entry i is pixel i's own ray, one entry more than the image has pixels), from the same code.  The caller uploads
 * them once per (fov, size).  RTX_ERR_INVALID_ARGUMENT: NULL tables, fov not in (0, pi] (pi: the double 3.141592653589793; beyond
 * it the tables stop being monotone), width * height == 0 or >= 2^32 - 16.
 *
 * Per pixel, with P = d_hits[p].position, n = d_hits[p].normal, o = d_hits[p].object, c = d_rgb[3 p ..], v = d_var[3 p ..]
 * (V = (d_var != NULL): the variance is tracked):
 *  1. NO HISTORY when the call has none (the first frame: every d_hist_* is NULL), or o < 0, or a component of P is not finite, or
 *     where a step below says so.  Then d_out_rgb = c, d_out_var = v, d_out_len = 1: copies of the bytes, no arithmetic (a NaN keeps
 *     its payload, -0.0 its sign).
 *  2. e = P - prev_camera->position (per component);  cc.x = e . row 0, cc.y = e . row 1, cc.z = e . row 2 of prev_camera->
 *     to_cam_space, each as (e.x * r[0] + e.y * r[1]) + e.z * r[2] (camera.rs:51-53, mat/mul.rs:42-50).  !(cc.z > 0): no history (a
 *     point behind the previous camera; the NaN matrix of a camera that looks along +-z).
 *  3. The inverse of get_ray_dir, whose direction is proportional to (sin ax, sin ay, cos ax * cos ay), without inverse trigonometry:
 *       a = cc.x * cc.x;  b = cc.y * cc.y;  L = (a + b) + cc.z * cc.z;  q = L * L - 4 * (a * b);  q = q > 0 ? q : 0
 *       m = 2 / (L + sqrt(q));  k = sqrt(m);  sx = cc.x * k;  sy = cc.y * k
 *     fx from Tx (n = width) and sx:  lo = 0, hi = n;  while (hi - lo > 1) { mid = (lo + hi) >> 1;  if (T[mid] <= s) lo = mid; else
 *     hi = mid; }   den = T[lo + 1] - T[lo];   fx = lo + (den > 0 ? (s - T[lo]) / den : 0)   (the first and the last interval
 *     extrapolate; a NaN s gives a NaN fx); fy likewise from Ty (n = height) and sy.
 *     !(fx >= -0.5 && fx <= width - 0.5) or !(fy >= -0.5 && fy <= height - 0.5): no history.  An integer fx is a pixel's own ray
 *     (pixels are sampled at their corners).  Between the pixels' own rays the interpolation is linear in the SINE, not in the angle:
 *     fx is off by up to 1e-4 px at 1920 wide and fov pi/2, 0.02 px at 8 wide, and 0.25 px in the outermost columns at fov = pi,
 *     where the sine is flat; the pixels' own rays come back to 1e-12 px (3e-10 px at fov = pi and 1920 wide).
 *  4. i0 = floor(fx), tx = fx - i0, j0 = floor(fy), ty = fy - j0; sw = h_k = hv_k = hn = +0.0.  For dy = 0, 1 (outer) and dx = 0, 1
 *     (inner) the tap q = (i0 + dx, j0 + dy) with w = {1 - tx, tx}[dx] * {1 - ty, ty}[dy] is kept when ALL of:  q is inside the
 *     frame;  w > 0;  d_hist_hits[q].object == o;  d_hist_len[q] >= 1;  the three d_hist_rgb[3 q ..] are finite, and with V the three
 *     d_hist_var[3 q ..];  with n_q = d_hist_hits[q].normal:  t = n . n_q,  t > 0  and  t * t >= normal_min2 * ((n . n) * (n_q . n_q));
 *     with Q = d_hist_hits[q].position:  g = Q - P,  d = g . n,  d * d <= (plane_tol2 * (e . e)) * (n . n).  Here normal_min2 =
 *     normal_min * normal_min and plane_tol2 = plane_tolerance * plane_tolerance, each one rounded multiply.  (No square root and no
 *     division in a test.  A zero normal fails t > 0: such a pixel never takes history.  The plane test keeps a plane seen at a
 *     grazing angle and drops the pixels an object moved by rtx_scene_update_objects has covered or uncovered.)  A kept tap adds
 *       sw = sw + w;   h_k = h_k + w * hist_rgb_q,k;   V: hv_k = hv_k + w * hist_var_q,k;   hn = hn + w * hist_len_q
 *  5. !(sw > min_weight): no history.  Else  N = hn / sw;  alpha = 1 / (N + 1);  alpha = alpha > alpha_min ? alpha : alpha_min;
 *     beta = 1 - alpha;   d_out_rgb_k = beta * (h_k / sw) + alpha * c_k;   V: d_out_var_k = (beta * beta) * (hv_k / sw) + (alpha *
 *     alpha) * v_k;   len = N + 1;  d_out_len = len < max_history ? len : max_history.
 *  d_motion (may be NULL; 2 doubles per pixel): (fx, fy) for every pixel that passed step 3 -- whether or not a tap was then kept --
 *  and the quiet NaN pair otherwise.  A current colour or variance that is not finite is blended as it is: the output is not finite,
 *  and the next frame's taps drop it.  d_hist_len need not be finite (+inf: the history's weight is 1 - alpha_min).
 * With a static camera and scene, alpha_min = 0 and a large max_history this is the running mean of the frames and d_out_var the
 * variance of that mean.
 *
 * Buffers (all DEVICE memory): d_rgb, d_var (may be NULL), d_hist_rgb, d_hist_var, d_out_rgb, d_out_var (may be NULL): width * height * 3
 * doubles; d_hits, d_hist_hits: width * height RtxHit; d_hist_len, d_out_len: width * height doubles; d_prev_tables: the tables of
 * (prev_camera->fov, width, height); prev_camera: a HOST struct, read before the call returns -- only its fov (checked), position and
 * to_cam_space.  Nothing of the first frame's NULL history, camera and tables is read.
 * RTX_ERR_INVALID_ARGUMENT, decided before any device is looked for: NULL params, d_rgb, d_hits, d_out_rgb or d_out_len; a history
 * that is only partly given (d_hist_rgb, d_hist_len, d_hist_hits, prev_camera and d_prev_tables go together); d_var without
 * d_hist_var on a frame with history, or the reverse; d_out_var without d_var; any overlap among the inputs and outputs; width * height
 * == 0 or >= 2^32 - 16; alpha_min not in [0, 1]; max_history NaN, < 1 or infinite; plane_tolerance NaN, negative or infinite;
 * normal_min not in [0, 1]; min_weight not in [0, 1); flags or reserved != 0; prev_camera->fov not in (0, pi].
 * Per-object motion is not part of this call: a moved object's history is dropped where the tests catch it, unless d_hits was first
 * rewound by rtx_rewind_hits_device (below).  Out of scope: SVGF's 3 x 3 fallback search; multi-device frames (gather first, as for the denoiser); frames of different
 * sizes (rtx_upsample_device, below, takes a low frame to the display's size after this call).  (DESIGN.md 3.15 "Temporal accumulation".) */
typedef struct RtxTemporalParams {
    double   alpha_min;          /* in [0, 1]: the least weight of the new frame (0: the running mean) */
    double   max_history;        /* >= 1, finite: where the history length stops growing */
    double   plane_tolerance;    /* >= 0, finite: a tap's distance from the tangent plane, relative to the distance from the previous camera */
    double   normal_min;         /* in [0, 1]: the least cosine between the two normals */
    double   min_weight;         /* in [0, 1): the bilinear weight that must survive the tests */
    uint32_t flags;              /* must be 0 */
    uint32_t reserved;           /* must be 0 */
} RtxTemporalParams;
RTX_STATIC_ASSERT(sizeof(RtxTemporalParams) == 48 && offsetof(RtxTemporalParams, max_history) == 8 &&
                  offsetof(RtxTemporalParams, plane_tolerance) == 16 && offsetof(RtxTemporalParams, normal_min) == 24 &&
                  offsetof(RtxTemporalParams, min_weight) == 32 && offsetof(RtxTemporalParams, flags) == 40 &&
                  offsetof(RtxTemporalParams, reserved) == 44, "RtxTemporalParams layout");

/* The defaults (DESIGN.md 3.15 records how they were chosen): alpha_min = 0.5, max_history = 32, plane_tolerance = 0.005,
 * normal_min = 0.9, min_weight = 0.01. */
void     rtx_temporal_default_params(RtxTemporalParams *out);
int32_t  rtx_temporal_tables(double fov, uint32_t width, uint32_t height, double *tables);
int32_t  rtx_temporal_accumulate_device(const double *d_rgb, const double *d_var, const RtxHit *d_hits, const double *d_hist_rgb,
                                        const double *d_hist_var, const double *d_hist_len, const RtxHit *d_hist_hits,
                                        const RtxCamera *prev_camera, const double *d_prev_tables, uint32_t width, uint32_t height,
                                        const RtxTemporalParams *params, double *d_out_rgb, double *d_out_var, double *d_out_len,
                                        double *d_motion, int32_t device, void *stream);
/* One-shot host form (device 0: allocates, copies, accumulates, copies back; builds the tables itself from prev_camera->fov).  Every
 * pointer is a HOST array; the same arguments may be NULL, the same are refused. */
int32_t  rtx_temporal_accumulate(const double *rgb, const double *var, const RtxHit *hits, const double *hist_rgb, const double *hist_var,
                                 const double *hist_len, const RtxHit *hist_hits, const RtxCamera *prev_camera, uint32_t width,
                                 uint32_t height, const RtxTemporalParams *params, double *out_rgb, double *out_var, double *out_len,
                                 double *motion);

/* Rewinding a pick buffer: the step before rtx_temporal_accumulate_device in a frame in which objects MOVED (rtx_scene_update_objects
 * between the two frames).  The accumulation reprojects a pixel's CURRENT surface point; a moved object was somewhere else when the
 * previous pick was taken, so its history is dropped or -- after a sideways move -- taken from another point of its surface.  This call
 * replaces every hit on a moved object by the record of the SAME MATERIAL POINT on the object's geometry of the previous frame: the
 * position and Object::normal_at that geometry has there.  The rewound buffer is what the accumulation takes as d_hits (it reads only
 * position, normal and object); its d_motion then holds true screen-space motion, object motion included.  The UNREWOUND pick stays
 * the next frame's d_hist_hits, which is why there is no in-place form.  The call takes no scene handle, allocates nothing and only
 * enqueues ONE launch on `stream` (a hipStream_t; NULL = the device's null stream).
 *
 * This comment is the specification, under the rules of the temporal comment above: every operation is one separately rounded f64
 * operation (add, subtract, multiply, divide, square root; never fused) in the written order and bracketing, so plain Python floats
 * (tests/rewind_model.py) give the same bits; comparisons with a NaN are false; "finite" is neither NaN nor an infinity;
 * a . b = (a.x * b.x + a.y * b.y) + a.z * b.z;  |a| = sqrt((a.x * a.x + a.y * a.y) + a.z * a.z);  norm(a) = (a.x / |a|, a.y / |a|,
 * a.z / |a|), three true divisions (vector.rs:97-107).
 *
 * d_objects holds the m indices of the moved objects, STRICTLY ASCENDING; d_motions[k] belongs to d_objects[k].  Per hit
 * H = d_hits[p], with o = H.object and P = H.position, in this order:
 *  1. UNMOVED when m == 0 or o < 0: d_out[p] = the 64 bytes of H (a NaN keeps its payload).  Else the search
 *       lo = 0, hi = m;  while (hi - lo > 1) { mid = (lo + hi) >> 1;  if (d_objects[mid] <= o) lo = mid; else hi = mid; }
 *     UNMOVED when d_objects[lo] != o.  Else M = d_motions[lo].  (A list that is not ascending is the caller's error in the device
 *     form: the hit is rewound by whichever entry the search ends on, or not at all; no index outside [0, m) is read.)
 *  2. LOST -- d_out[p] = H with object = -1, every other byte copied, so that step 1 of the accumulation gives "no history" -- when
 *     M.kind is RTX_MOTION_LOST or none of the three shape kinds (M.reserved is not read); when a component of P is not finite; where
 *     step 3 says so; when a component of the rewound P' is not finite.
 *  3. P', by M.kind, from now = M.now and before = M.before (the words of RtxObject.geom; the device never compares the two):
 *     sphere (c = now[0..2], r = now[3]; c' = before[0..2], r' = before[3]):   s = r' / r;  !(s > 0) or s infinite: LOST (a zero, negative
 *       or NaN radius on either side; a ratio that overflows);   g = P - c;   P'_k = c'_k + g_k * s.
 *     plane (q = now[0..2]; q' = before[0..2]):   t = q' - q;   P'_k = P_k + t_k.   The translation of the anchor: a plane that turned
 *       gets its previous normal in step 4, and the accumulation's own normal test decides.
 *     triangle (A, B, C = now[0..2], [3..5], [6..8]; A', B', C' of before):   e1 = B - A;  e2 = C - A;  w = P - A;   d11 = e1 . e1;
 *       d12 = e1 . e2;  d22 = e2 . e2;  w1 = w . e1;  w2 = w . e2;   det = d11 * d22 - d12 * d12;   !(det > 0) or det infinite: LOST;
 *       u = (d22 * w1 - d12 * w2) / det;   v = (d11 * w2 - d12 * w1) / det;   e1' = B' - A';  e2' = C' - A';
 *       P'_k = (A'_k + u * e1'_k) + v * e2'_k.   (u, v) are P's affine coordinates in the plane of the current triangle (the least-squares
 *       ones where rounding left P off it); the reference's phantom hits outside the triangle extend affinely, which is intended.
 *  4. n' = Object::normal_at(P') of the object with geometry `before`, in the reference's order (object.rs:37-39 over sphere.rs:31-33,
 *     plane.rs:33-35, triangle.rs:104-107): the shape's normal, normalised AGAIN --
 *       sphere:  norm(norm(P' - c'));    plane:  norm(before[3..5]);    triangle:  norm(norm(e1' x e2')),
 *       a x b = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x).
 *     A normal that is not finite is written as it comes (the accumulation's t > 0 test drops such a pixel).
 *  5. d_out[p] = { position = P', normal = n', distance = H.distance (this frame's ray's; the accumulation does not read it),
 *     object = o }.
 * With before == now bitwise: a plane's P' == P as values and as bits except that a component -0.0 comes back as +0.0 (t = +0.0); a
 * sphere's P'_k = c_k + (P_k - c_k) (s == 1 exactly), which is P_k to within 2^-53 * (|P_k - c_k| + |P'_k|) but not always its bits;
 * a triangle's P' is the projection of P onto its plane, through u and v.  rtx_object_motions leaves such entries out.
 *
 * Buffers (DEVICE memory): d_hits, d_out: n_hits RtxHit, both 16-BYTE ALIGNED (every hipMalloc'd array and every whole-record offset
 * into one is; the records move as 16-byte vectors) -- an RtxHit array that is only 8-byte aligned is refused, here, not in the
 * accumulation; d_objects: m int64; d_motions: m RtxObjectMotion (8-byte aligned).  With m == 0 both lists may be NULL and the call
 * is a copy.  RTX_ERR_INVALID_ARGUMENT, decided before any device is looked for: NULL d_hits or d_out, or one that is not 16-byte
 * aligned; m > 0 with a NULL d_objects or d_motions; n_hits == 0 or >= 2^32 - 16; m >= 2^31; flags != 0; any overlap among the
 * inputs and the output.
 * Out of scope: a device-side record of what moved; the rotation of a plane about its anchor; skinned or camera-relative motion.
 * (DESIGN.md 3.16 "Rewinding moved objects".) */
#define RTX_MOTION_LOST 0xFFFFFFFFu   /* RtxObjectMotion.kind: the object has no previous geometry to rewind to (none of RTX_SPHERE .. RTX_TRIANGLE) */
typedef struct RtxObjectMotion {
    uint32_t kind;               /* RTX_SPHERE | RTX_PLANE | RTX_TRIANGLE: the object's kind in both frames; or RTX_MOTION_LOST */
    uint32_t reserved;           /* must be 0 */
    double   now[9];             /* RtxObject.geom as resident when d_hits was picked */
    double   before[9];          /* RtxObject.geom when the previous frame's pick (d_hist_hits) was taken */
} RtxObjectMotion;
RTX_STATIC_ASSERT(sizeof(RtxObjectMotion) == 152 && offsetof(RtxObjectMotion, reserved) == 4 && offsetof(RtxObjectMotion, now) == 8 &&
                  offsetof(RtxObjectMotion, before) == 80, "RtxObjectMotion layout");

int32_t  rtx_rewind_hits_device(const RtxHit *d_hits, uint64_t n_hits, const int64_t *d_objects, const RtxObjectMotion *d_motions,
                                uint64_t m, uint32_t flags, RtxHit *d_out, int32_t device, void *stream);
/* One-shot host form (device 0: allocates, copies, rewinds, copies back).  Every pointer is a HOST array of any alignment; flags are 0.
 * Refused as the device form refuses, and additionally: a list that is not strictly ascending, a kind that is none of the three shapes
 * and not RTX_MOTION_LOST, a reserved word that is not 0. */
int32_t  rtx_rewind_hits(const RtxHit *hits, uint64_t n_hits, const int64_t *objects, const RtxObjectMotion *motions, uint64_t m,
                         RtxHit *out);
/* What a caller handed to rtx_scene_update_objects since the previous frame -> the sorted list the two calls above take.  Host only: no
 * device is looked for.  Entry i says that object indices[i] had the record before[i] and now has now[i]; only kind and geom are
 * read.  before[i].kind == RTX_MOTION_LOST says that the object was hidden, or did not exist, when the previous pick was taken.  Of an
 * index that is given more than once, the FIRST entry's `before` and the LAST entry's `now` are kept (several updates between two
 * frames, in call order).  Then, per index: the kinds differ, or `before` is RTX_MOTION_LOST: kind = RTX_MOTION_LOST, now and before
 * all 0.  Else, when the geometry words the kind reads (sphere 4, plane 6, triangle 9) are bitwise the same in both: the index is left
 * out (a material update moves nothing).  Else kind = the kind, now and before = all 9 words of the two geom arrays.  reserved = 0.
 * The output is in ascending index order; *m_out entries (at most n; objects_out and motions_out hold n) are written.
 * RTX_ERR_INVALID_ARGUMENT: n > 0 with a NULL indices, before, now, objects_out or motions_out; NULL m_out; n >= 2^31; an index
 * >= 2^63; a now[i].kind that is none of the three shapes; a before[i].kind that is none of them and not RTX_MOTION_LOST. */
int32_t  rtx_object_motions(const uint64_t *indices, const RtxObject *before, const RtxObject *now, uint64_t n, int64_t *objects_out,
                            RtxObjectMotion *motions_out, uint64_t *m_out);

/* Guided upsampling: a frame rendered at 1/s of the output resolution (wl x hl = width / s x height / s, the same camera) is
 * reconstructed at width x height, guided by the RtxPixelFeatures of both sizes (a joint bilateral upsampling: the four low pixels
 * around an output pixel, tent weights times the denoiser's normal, depth and albedo weights).  What makes the construction exact is the
 * reference's pixel map: render() gives pixel x of a w-wide frame the angle fov * (x / w - 0.5) -- pixel corners -- with
 * vfov = h / w * fov, so pixel (X, Y) of the wl x hl frame has the zero-offset ray of pixel (s X, s Y) of the width x height frame bit
 * for bit (X / wl and s X / width are correctly rounded quotients of the same rational, and so are hl / wl and height / width): the low
 * frame is a sampling of the output frame's own lattice {(s X, s Y)}.  That identity needs s to divide both sizes, which is why any
 * other width or height is refused.  Only the lens jitter of the two frames differs (the RNG key uses y * width + x).
 * The call takes no scene handle, allocates nothing and only enqueues ONE launch on `stream` (a hipStream_t; NULL = the device's null
 * stream).  d_lo_rgb is what rtx_render_blocks_accumulate, rtx_temporal_accumulate_device or rtx_denoise_device left of the low frame,
 * d_lo_var its variance of the mean; d_out feeds rtx_quantize_image_device.
 *
 * This comment is the specification: every operation below is one separately rounded f64 operation (IEEE add, subtract, multiply,
 * divide; never fused), in exactly the written order and bracketing, so plain numpy (tests/upsample_model.py) gives the same bits.
 * Comparisons with a NaN are false.  "finite" means neither NaN nor an infinity.  s = factor; D = the flag RTX_UPSAMPLE_DEMODULATE;
 * V = (d_lo_var != NULL).  The output pixel is p = (x, y) with a = albedo, e = emission, n = normal, z = depth of d_features[y * width
 * + x]; low pixel Q = (X, Y) has a_Q, e_Q, n_Q, z_Q of d_lo_features[Y * wl + X], c_Q = d_lo_rgb[3 (Y * wl + X) ..], var_Q likewise.
 *
 * A tap's values, per channel k (the denoiser's preparation):
 *     D:      u_Q,k = a_Q,k > albedo_min ? (c_Q,k - e_Q,k) / a_Q,k : c_Q,k - e_Q,k
 *             V: v_Q,k = a_Q,k > albedo_min ? var_Q,k / (a_Q,k * a_Q,k) : var_Q,k
 *     not D:  u_Q,k = c_Q,k                                       V: v_Q,k = var_Q,k
 * Channel k of tap Q is USABLE when u_Q,k is finite and, under D, a_Q,k > albedo_min (a channel whose albedo is zero carries no
 * irradiance, only c - e, which is about 0).
 *
 * X0 = x / s, Y0 = y / s (integer division), rx = x - s * X0, ry = y - s * Y0, fx = (double)rx / (double)s, fy = (double)ry / (double)s.
 *   - A lattice pixel (rx == 0 && ry == 0): u_k = u_Q,k and v_k = v_Q,k of Q = (X0, Y0), moved without arithmetic, where the channel is
 *     usable; else u_k = v_k = +0.0.
 *   - Any other pixel: tc_k = tw_k = tv_k = sc_k = sw_k = sv_k = +0.0, then for j = 0, 1 (outer) and i = 0, 1 (inner) the tap
 *     Q = (X0 + i, Y0 + j):
 *       h  = (i ? fx : 1 - fx) * (j ? fy : 1 - fy)                                                      (the tent weight)
 *       the tap is skipped when Q lies outside the low frame or h == 0; else
 *       wn, wz, wa = the denoiser's three weights (above: "wn = 1 when normal_power_log2 == RTX_DENOISE_NO_NORMAL, else ...", "wz = 1
 *            when sigma_depth == +inf; else ...", "wa = 1 when sigma_albedo == +inf; else ..."), word for word, with n_p, z_p, a_p =
 *            n, z, a of the output pixel and n_q, z_q, a_q = n_Q, z_Q, a_Q
 *       w  = ((h * wn) * wz) * wa
 *       per usable channel k:  tc_k = tc_k + h * u_Q,k,  tw_k = tw_k + h,  V: tv_k = tv_k + (h * h) * v_Q,k
 *       and, when w > 0, also: sc_k = sc_k + w * u_Q,k,  sw_k = sw_k + w,  V: sv_k = sv_k + (w * w) * v_Q,k
 *     then per channel k:
 *       sw_k > min_weight * tw_k:   u_k = sc_k / sw_k,  V: v_k = sv_k / (sw_k * sw_k)       (the guided sum)
 *       else tw_k > 0:              u_k = tc_k / tw_k,  V: v_k = tv_k / (tw_k * tw_k)       (the tent sum: no tap resembles p enough)
 *       else:                       u_k = v_k = +0.0                                        (no usable tap)
 * Output.  D: d_out[3 p + k] = a_k > albedo_min ? u_k * a_k + e_k : e_k (the multiply is rounded, then the add); V: d_var_out[3 p + k]
 * = a_k > albedo_min ? v_k * (a_k * a_k) : +0.0.  Not D: d_out = u, d_var_out = v.  The second arm under D is e_k, not the denoiser's
 * u_k + e_k: a surface whose albedo is zero in a channel returns exactly its emission there (render_ray multiplies the light by the base
 * colour), and a pixel whose samples all miss has a = e = 0, so a black channel and a missed pixel come out as the render would give
 * them, whatever their neighbours hold.  With s == 1 every pixel is a lattice pixel: without D, d_out is a byte copy of d_lo_rgb
 * wherever that is finite.
 * d_var_out is the variance of the weighted mean of independent taps; neighbouring OUTPUT pixels share taps, and the result ignores
 * that correlation: it is not the variance a filter over d_out may assume independent.
 *
 * Buffers.  d_lo_rgb: wl * hl * 3 doubles; d_lo_var (may be NULL) the same; d_lo_features: wl * hl records; d_features: width * height
 * records; d_out: width * height * 3 doubles; d_var_out (may be NULL; must be NULL when d_lo_var is) the same.
 * RTX_ERR_INVALID_ARGUMENT, decided before any device is looked for: a NULL params, d_lo_rgb, d_lo_features, d_features or d_out; a
 * d_var_out without d_lo_var; any overlap among the inputs and outputs; width * height == 0 or >= 2^32 - 16; factor == 0 or >
 * RTX_UPSAMPLE_MAX_FACTOR; width or height not a multiple of factor; a flag bit other than RTX_UPSAMPLE_DEMODULATE; reserved != 0;
 * normal_power_log2 > 8 and not RTX_DENOISE_NO_NORMAL; a sigma that is NaN or <= 0 (+inf is allowed: it deletes the term, no
 * arithmetic); albedo_min or min_weight NaN, negative or infinite.
 * Out of scope: factors that are not integers or do not divide the frame; multi-device frames (gather first); more than 2 x 2 taps;
 * upsampling history or pick buffers.  (DESIGN.md 3.17 "Guided upsampling".) */
#define RTX_UPSAMPLE_MAX_FACTOR 8
#define RTX_UPSAMPLE_DEMODULATE 1u
typedef struct RtxUpsampleParams {
    uint32_t factor;             /* s, 1..RTX_UPSAMPLE_MAX_FACTOR: output pixels per low pixel along each axis */
    uint32_t flags;              /* RTX_UPSAMPLE_DEMODULATE or 0 */
    uint32_t normal_power_log2;  /* 0..8 or RTX_DENOISE_NO_NORMAL, the denoiser's meaning */
    uint32_t reserved;           /* must be 0 */
    double   sigma_depth;        /* > 0, relative depth difference at which the weight is 1/2; +inf: no depth term */
    double   sigma_albedo;       /* > 0, albedo distance at which the weight is 1/2; +inf: no albedo term */
    double   albedo_min;         /* >= 0, finite: channels with albedo at or below it are not demodulated and carry no irradiance */
    double   min_weight;         /* >= 0, finite: below this share of the tent weight the guided sum is not trusted */
} RtxUpsampleParams;
RTX_STATIC_ASSERT(sizeof(RtxUpsampleParams) == 48 && offsetof(RtxUpsampleParams, flags) == 4 && offsetof(RtxUpsampleParams, normal_power_log2) == 8 &&
                  offsetof(RtxUpsampleParams, reserved) == 12 && offsetof(RtxUpsampleParams, sigma_depth) == 16 &&
                  offsetof(RtxUpsampleParams, sigma_albedo) == 24 && offsetof(RtxUpsampleParams, albedo_min) == 32 &&
                  offsetof(RtxUpsampleParams, min_weight) == 40, "RtxUpsampleParams layout");

/* The defaults (DESIGN.md 3.17 records how they were chosen): factor 2, RTX_UPSAMPLE_DEMODULATE, normal_power_log2 = 2, sigma_depth =
 * 0.05, sigma_albedo = 0.5, albedo_min = 1e-3, min_weight = 1e-3. */
void     rtx_upsample_default_params(RtxUpsampleParams *out);
int32_t  rtx_upsample_device(const double *d_lo_rgb, const double *d_lo_var, const RtxPixelFeatures *d_lo_features,
                             const RtxPixelFeatures *d_features, uint32_t width, uint32_t height, const RtxUpsampleParams *params,
                             double *d_out, double *d_var_out, int32_t device, void *stream);
/* One-shot host form (device 0: allocates, copies, upsamples, copies back), as rtx_denoise.  Every pointer is a HOST array; lo_var and
 * var_out may be NULL as above. */
int32_t  rtx_upsample(const double *lo_rgb, const double *lo_var, const RtxPixelFeatures *lo_features, const RtxPixelFeatures *features,
                      uint32_t width, uint32_t height, const RtxUpsampleParams *params, double *out, double *var_out);

/* Test hook (lab library; the product returns RTX_ERR_UNSUPPORTED -- same sources and flags, so the arithmetic it shows is the
 * product's): evaluates one f64 operation per element on the device (op 0: a/b, 1: sqrt(a),
 * 2: sin(a), 3: cos(a), 4 / 5: sincos(a)'s two results; 6: the packet walks' v_writelane -- out[i] = (int)b[0] in lane (int)b[1]
 * of every wave, (int)a[i] elsewhere; 7 / 8: v_min_f64 / v_max_f64 on the raw bits of a[i], b[i] -- the child sort's (key, link)
 * pairs are denormal f64 patterns when the key is +0.0 and must come back bit for bit; 9 / 10: the sin / cos the path itself uses
 * for Vector3::random_direction's angle in [0, 2 pi] -- rtx_math.h sincos_2pi; 11-16: the trace kernels' ray index -> pixel arithmetic
 * (rtx_device.h) on 32-bit integers held in doubles, the divisors built on the host and passed as a kernel argument as the renders
 * pass theirs -- 11: fastdiv(a[i], make_fastdiv(b[0])); 12 / 13: ray_index_to_pixel's local pixel / sample of ray index a[i] in a band
 * of b[0] pixels; 14 / 15 / 16: ray_index_to_pixel_tiled's local pixel / sample / 1.0 unless the lane is the padding of a partial 8x8
 * tile, in a band of b[0] columns x b[1] rows; 17-21: the HOST forms, evaluated without a device -- 17: fastdiv(a[i],
 * make_fastdiv(b[0])); 18: image_row of local row a[i] for row_begin, row_stride, row_block = b[0], b[1], b[2]; 19 / 20 / 21: m, s1, s2
 * of make_fastdiv(a[i])); a, b, out are HOST arrays of n doubles.  Used by tests/ to check that the
 * device's / and sqrt are correctly rounded, to measure how far its sin/cos are from libm, and to hold the index arithmetic to
 * "exact for every 32-bit n" at ray counts no test can afford to allocate. */
int32_t rtx_debug_math(int32_t op, const double *a, const double *b, double *out, uint64_t n);

/* Test hook (lab library; the product returns RTX_ERR_UNSUPPORTED): the TRANSCRIPT of every path of one image row, as the exhaustive
 * f64 kernel (RTX_KERNEL_EXACT) walks it -- per segment the ray closest_object was asked about (scene.rs:232: position, direction),
 * the winning distance and the winner's index in Scene.objects (scene.rs:243-251; -1 and +inf: no object, the path ends).  Images
 * compare hit SEQUENCES (a colour is a product of materials); a transcript compares the arithmetic itself, every bounce direction
 * and hit point to the last bit (tests: equal to the oracle's transcript when the oracle uses the device's sin / cos routine).
 * steps: HOST array [width][rays_per_pixel][max_steps]; counts: HOST array [width][rays_per_pixel], the path's number of segments
 * (steps beyond max_steps are counted, not stored). */
typedef struct RtxPathStep {
    double  position[3];
    double  direction[3];
    double  distance;
    int64_t object;
} RtxPathStep;
int32_t rtx_debug_paths(RtxSceneHandle scene, uint32_t width, uint32_t height, uint32_t row, uint32_t max_steps,
                        RtxPathStep *steps, uint32_t *counts);

/* Test hooks of the sample store, the fold and the gather epilogues (lab library; the product returns RTX_ERR_UNSUPPORTED).  Each runs
 * the product's own device function or launcher on the caller's data: every argument is a HOST array, the hook allocates on device 0,
 * copies, launches, copies back and synchronises.  tests/test_support_kernels.py holds them to plain references, bit for bit.
 *
 * rtx_debug_store_samples: entry i < n is the sample rgb[3 i .. 3 i + 2] of ray-queue slot slots[i]; one thread per entry calls the
 * trace kernels' store_sample (rtx_device.h) on it, with `records` (n_records records of 4 doubles) as the launch's sample buffer and
 * `mask` (n_words 32-bit words) as its non-zero mask with base nonzero_base: a sample that is not zero leaves {r, g, b, 0.0} in record
 * slots[i] and sets bit nonzero_base + slots[i] of the mask, a zero sample touches neither.  records and mask are read (the caller
 * pre-fills them) and written back whole.  The slots must be distinct and every record and bit inside the buffers: else
 * RTX_ERR_INVALID_ARGUMENT, nothing runs. */
int32_t rtx_debug_store_samples(const double *rgb, const uint64_t *slots, uint64_t n, uint64_t nonzero_base, double *records,
                                uint64_t n_records, uint32_t *mask, uint64_t n_words);

/* rtx_debug_resolve: launch_resolve -- the launcher every render calls -- on a band of width x n_rows pixels whose ray queue runs in
 * image rows (tiles_x = 0: per_sample = width * n_rows slots per sample) or over 8x8 pixel tiles (tiles_x = ceil(width / 8): per_sample =
 * tiles_x * ceil(n_rows / 8) * 64, the padding of partial tiles included).  records: n_samples * per_sample records of 4 doubles in queue
 * order; mask: one bit per record (bit 0 of word 0 = record 0), ceil(n_samples * per_sample / 32) words; both may be null when n_samples
 * is 0.  first: the fold starts from zero, else from acc; last: out[3 p + c] = sum / rays_per_pixel, else the sum goes to acc (p = k *
 * width + x, local row k).  acc (acc_doubles >= 3 * width * n_rows doubles; may be null when first and last) and out (out_doubles >= 3 *
 * width * n_rows; may be null unless last) are read and written back whole: what lies behind the pixels must come back untouched.  On the device one more sample's worth of NaN
 * records under set bits lies behind the caller's records and mask, so a fold that reads a sample too many shows in the frame. */
int32_t rtx_debug_resolve(const double *records, const uint32_t *mask, uint32_t width, uint32_t n_rows, uint32_t tiles_x,
                          uint32_t n_samples, uint64_t rays_per_pixel, int32_t first, int32_t last, double *acc, uint64_t acc_doubles,
                          double *out, uint64_t out_doubles);

/* rtx_debug_resolve_moments: launch_resolve as rtx_render_blocks_accumulate calls it -- first = last = 0, the caller's sums as the
 * accumulator, a squares buffer -- on the caller's host arrays: sum[3 p + c] += the set-bit records of pixel p in sample order,
 * sum_sq[3 p + c] += their squares (sum_sq may be null: the sums alone).  records, mask, width, n_rows, tiles_x, n_samples as
 * rtx_debug_resolve, the NaN records under set bits behind the caller's data included; sum / sum_sq (at least 3 * width * n_rows doubles)
 * are read and written back whole. */
int32_t rtx_debug_resolve_moments(const double *records, const uint32_t *mask, uint32_t width, uint32_t n_rows, uint32_t tiles_x,
                                  uint32_t n_samples, double *sum, uint64_t sum_doubles, double *sum_sq, uint64_t sum_sq_doubles);

/* rtx_debug_gather: the epilogues of rtx_render_devices / rtx_render_to_image_devices on a caller's staging buffer.  form 0:
 * launch_deinterleave, parts = n bands of cap_rows rows of width * 3 doubles (band p = the blocks of `block` image rows p, p + n, ... in
 * order) -> full, height * width * 3 doubles; form 1: launch_deinterleave_u8, the same on bytes, flip != 0: output row y is image row
 * height - 1 - y; form 2: launch_quantize_values, parts = a band of height x width x 3 doubles -> full, as many bytes (`* 256`,
 * saturating `as u8`, rows in place; n, cap_rows, block and flip are not read).  cap_rows below a part's row count is refused. */
int32_t rtx_debug_gather(int32_t form, const void *parts, uint32_t width, uint32_t height, uint32_t n, uint32_t cap_rows,
                         uint32_t block, int32_t flip, void *full);

/* rtx_debug_path_bounds (lab library; the product returns RTX_ERR_UNSUPPORTED): what the tree walks' f32 bounds decide for single
 * (ray, object) pairs.  Every result is decided in f64; WHICH shapes reach the f64 test is decided by f32 slab tests and f32 distance
 * bounds with hand-derived margins, and a margin that is too small shows only for rays within a few f32 ulps of a box
 * face, a tangent or an edge.  For entry i < n the host finds the path root -> leaf of Scene.objects[objects[i]] in the scene's resident
 * tree; one device thread then runs the walks' own device functions along that path with the bound best_up[i]: per step the slab test
 * of the object's child, then the leaf bounds of the object's own record.  rays, objects, best_up and out are HOST arrays; the hook
 * copies, launches once, copies back and synchronises.
 * form: bit 0 -- an origin beyond origin_limit is walked with the f64 slab test (Ray64), else with the slack of Ray32S;
 *       bit 1 -- the 64-byte nodes (a sphere tree: the sphere_node_step_q3 visit on an empty stack, the entered children read back from
 *                its stack -- it has no f64 form; a pure (x, y)-footprint tree: qrect_entry), else the 128-byte nodes (box_entry32, or
 *                rect_entry32 where the node is a footprint node); RTX_ERR_INVALID_ARGUMENT when the tree has no 64-byte nodes;
 *       bits 8-9 -- the leaf test: 0 the phased walks' (sphere_leaf_step_at on a one-record leaf; tri_filter_sign + tri_bounds),
 *                1 sphere_step's inline leaf and 2 mesh_step's inline leaf (sphere or triangle), each through a 128-byte node whose only
 *                child is a one-record leaf of the object in an unbounded box; 3 sph_packet_leaf_test, the packet kernel's test of one
 *                sphere record (a triangle: flag 64).
 * out: 8 words per entry --
 *   [0] flags: bits 0-1 the ray form the origin selects (0 Ray32: |o|_inf <= origin_limit, 1 Ray32S with its slack, 2 Ray64, 3 NO WALK:
 *       beyond 2^27 origin_limit, a NaN origin or a direction that is not of unit length -- the kernels sweep, words 1..7 are 0);
 *       4 the object is in the tree (else words 1..7 are 0: planes, shapes kept outside the tree); 8 the leaf test made it a CANDIDATE
 *       under best_up[i]; 16 CERTAIN: the same leaf test started from best_up = +inf lowered the bound; 32 a triangle; 64 the form
 *       does not exist for this element (words 1..7 are then not meaningful)
 *   [1] the path's length in node visits   [2] how many of them entered the object's child under best_up[i]
 *   [3] the largest entry distance those slab tests returned (f32 bits; -inf: none -- the 64-byte sphere visit returns none)
 *   [4] t_lo (f32 bits; +inf: not a candidate under either bound)   [5] t_hi: the bound after the leaf test from +inf (+inf: not certain)
 *   [6] best_up[i] after the leaf test   [7] the first step that did not enter (~0: none).
 * Optional HOST outputs (null: not wanted) -- the resident data those functions read, so that a model of the f32 arithmetic can be
 * run on the same bits:
 *   scene_info[16]: the centre the f32 records are relative to (3), sphere_cmax, origin_limit, inv_max, tri_extent, the tree's flags
 *       (rtx_debug_host_scene, stats[7]), depth, wide nodes, triangle records in the tree, spheres; written even when n is 0
 *   records: 16 words per entry -- a sphere's leaf record {c - centre, |r| rounded up}, zeros behind it -- with form bit 11 (0x800,
 *       which selects nothing else) words 4-7 and 8-11 are its filter record {c - centre, |c - centre|^2 - r^2} as the leaf holds it
 *       (bvh_leaf_f32) and as the sweep holds it (sphere_f32, un-interleaved); a triangle's A, B (the filter record) and g0, g1
 *       (tri_bounds' record); zeros for an object outside the tree
 *   path_data: 16 words per entry and step, path_steps steps per entry (further steps are not stored) -- word 0 the layout, word 15
 *       the node's link: 0 a 128-byte child {lo.xyz, hi.xyz}; 1 a footprint child {lo.x, lo.y, hi.x, hi.y}; 2 a 64-byte sphere child
 *       {o.xyz, s.xyz} and the child's six bytes {lo.xyz, hi.xyz} as integers; 3 a 64-byte footprint child {ox, oy, sx, sy} and the
 *       words {lo.x | hi.x << 16, lo.y | hi.y << 16}.
 * tests/test_walk_bounds.py holds these to the f64 text of the reference's distance functions on rays aimed at the margins. */
int32_t rtx_debug_path_bounds(RtxSceneHandle scene, const RtxRay *rays, const uint32_t *objects, const float *best_up, uint64_t n,
                              uint32_t form, uint32_t *out, double *scene_info, uint32_t *records, uint32_t *path_data,
                              uint32_t path_steps);

/* Test hook, needs no GPU: runs the host half of rtx_scene_upload (scene packing, filter records, the SAH build of
 * the flat BVH -- SURVEY 8f row N2; the reference's analogue is gpu_state.rs:53-77) and checks the tree's
 * invariants: every child box inside its parent's, every sphere / triangle-footprint inside its leaf's box, every
 * shape of the tree in exactly one leaf, links and layout flags consistent, depth as recorded.  stats[16]:
 * 0 spheres, 1 triangles, 2 triangle filter records, 3 of them in the tree, 4 wide nodes, 5 depth, 6 binary nodes,
 * 7 flags (1 spheres in the tree, 2 triangles in the tree, 4 nothing but (x, y)-footprint triangles: every node is a footprint node, 8 the 64-byte footprint-node form exists, 16 the 64-byte form of a sphere tree exists), 8 sphere leaf entries seen, 9 triangle leaf entries seen,
 * 10 largest leaf, 11 flat (footprint) nodes, 12 stack entries bound (3*depth+2), 13 tree triangles whose footprint lies in
 * the (x, y) plane, 14 those with an (x, z) or (y, z) footprint (zero-pivot row swaps, triangle.rs:60-71,81-87), 15 nodes that also exist in the 64-byte quantised form (flag 8). */
int32_t rtx_debug_host_scene(const RtxScene *scene, uint64_t *stats);

/* Test hook of the lab library (the product returns RTX_ERR_UNSUPPORTED), needs no GPU: the host half of rtx_scene_update_objects.
 * Packs `scene`, decides the update's path as the entry point does, applies it with the host reference of the device kernel
 * (refit_packed: the same header text, csrc/rtx_refit.h) -- or re-packs, for REBUILT -- and runs rtx_debug_host_scene's walk over
 * the result and the updated object list (same stats[16]).  *how: RTX_UPDATED_*.  digests[8]: FNV-1a-64 of the wide nodes, the
 * 64-byte sphere nodes, the leaf records (bvh_leaf_f32 then bvh_leaf_cr), sphere_f32, the sphere, plane and material records, and
 * the bits of sphere_cmax.  The high 16 bits of `mode`, when non-zero, are a split point s: entries [0, s) are applied as one
 * update and [s, n) as a second one on its result (*how is then the larger of the two). */
int32_t rtx_debug_host_refit(const RtxScene *scene, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                             uint64_t *stats, uint32_t *how, uint64_t *digests);

/* Test hook of the lab library: downloads the resident arrays of `scene` and digests them in rtx_debug_host_refit's order. */
int32_t rtx_debug_resident_digests(RtxSceneHandle scene, uint64_t *digests);

/* rtx_debug_host_refit with the arrays a triangle update writes (lab library; no GPU; the split point in the high 16 bits of `mode`
 * too).  digests[16]: [0..7] as rtx_debug_host_refit; [8] the triangle records (tris), [9] tri_f32, [10] tri_geo, [11] the 64-byte
 * footprint nodes, [12] the bits of tri_extent; [13..15] 0.  info[8]: the centre the f32 records are offsets from (3 values),
 * tri_extent, sphere_cmax, abs_pad, the range (scale) the tree was built for (< 0: no tree), 0. */
int32_t rtx_debug_host_refit_mesh(const RtxScene *scene, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                                  uint64_t *stats, uint32_t *how, uint64_t *digests, double *info);

/* Test hook of the lab library (the product returns RTX_ERR_UNSUPPORTED), needs no GPU: the host half of a handle's life with
 * rtx_scene_set_visible.  Packs `scene`, then runs n_steps steps; step s has kind step_kind[s] and the entries
 * [step_begin[s], step_begin[s + 1]) of `indices` / `objects` (step_begin has n_steps + 1 values):
 *   0 hide, 1 show (indices);  2 + mode: rtx_scene_update_objects under RTX_UPDATE_* `mode` (indices, objects);  5 append (objects).
 * how[s]: the step's RTX_UPDATED_*.  stats[16]: rtx_debug_host_scene's walk over the result, which for a hidden shape asks no
 * containing box and for every visible one still asks its leaf's box and exactly one leaf.  digests[16], info[8] (may be NULL): as
 * rtx_debug_host_refit_mesh, info[7] the number of wide nodes.  mask (may be NULL): one byte per object of the final list, 1 = visible.
 * dump (may be NULL; dump_words >= 4 * 17 * wide nodes): per wide node and child 17 words -- [0] link and [1] count as they are now,
 * [2..7] the bits of lo.xyz, hi.xyz (a footprint child: z unbounded; the nothing box when empty), [8] link and [9] count of the pack,
 * [10] the pack's leaf entries and [11..16] their object indices. */
int32_t rtx_debug_host_set_visible(const RtxScene *scene, const uint32_t *step_kind, const uint64_t *step_begin, uint64_t n_steps,
                                   const uint64_t *indices, const RtxObject *objects, uint32_t *how, uint64_t *stats, uint64_t *digests,
                                   double *info, uint8_t *mask, uint32_t *dump, uint64_t dump_words);

/* Test hook of the lab library: the 16 digests of rtx_debug_host_refit_mesh, from the downloaded resident arrays of `scene`. */
int32_t rtx_debug_resident_mesh_digests(RtxSceneHandle scene, uint64_t *digests);

/* rtx_debug_tile_lists (lab library; the product returns RTX_ERR_UNSUPPORTED): the per-tile candidate lists of the primary rays that
 * the LAST render call on `scene` used -- built by it, or by an earlier call of the same frame -- (build_mesh_tile_lists_kernel, DESIGN.md 3.3 "Tile lists"), read out of the handle's
 * own buffer and carved as the launch carved it.  The handle remembers that call's form and tile grid; the hook synchronises the
 * device.  All arrays are HOST arrays.
 * info[8]: [0] the form -- 0 the call built no lists (no packet path, RTX_TUNE_NO_TILE_LISTS, two halves in flight, no render yet;
 *       the lab's forms whose primary rays walk per lane), 1 a sphere tree's lists in the sphere packets' 32-byte entries {the leaf's
 *       f32 record (4 words), the sphere's index, t_lb, 0, 0}, 2 the {entry, t_lb} pairs of a footprint or joint tree (entry: a filter
 *       record, or with bit 31 a sphere leaf entry);  [1] tiles per row of the band's 8 x 8 tile grid, [2] tiles -- tile t holds the
 *       band's local rows 8 (t / info[1]) ... and columns 8 (t % info[1]) ...;  [3] the cap: entries a tile's list may hold;
 *       [4] words of a stored entry (8 or 2);  [5] the launches this handle's render calls have asked to BUILD lists so far (a call
 *       that renders the frame of the call before it -- same camera, band and scene -- finds them in the buffer and adds none:
 *       DESIGN.md 3.3);  [6..7] 0.
 * counts and entries may both be NULL (info alone); else they hold max_tiles >= info[2] tiles.
 * counts[t]: entries of tile t's list; 0xFFFFFFFF: the tile has no list (its packets walk the tree).
 * entries: 12 words per slot, [tile][cap][12]; the slots below counts[t] are written, the others 0 --
 *   [0..7] the stored words (form 2: two, the others 0);  [8] the bits of t_lb, the f32 lower bound of the distance the sweep stops by;
 *   [9] the index in Scene.objects the entry stands for, through the tables the kernels read (a sphere: bvh_prims, sphere_id; a filter
 *       record: tri_fidx and the triangle table), 0xFFFFFFFF where they name none;  [10] 1 a filter record, 0 a sphere;  [11] 0.
 * tests/test_tile_lists_gpu.py holds the lists to the f64 text on the extreme rays of every tile's ray family. */
int32_t rtx_debug_tile_lists(RtxSceneHandle scene, uint32_t *info, uint32_t *counts, uint32_t *entries, uint64_t max_tiles);

/* rtx_debug_sweep_filter (lab library; the product returns RTX_ERR_UNSUPPORTED): what the LDS sweep's two f32 filters
 * (trace_mixed_kernel) decide for single rays.  One device thread per entry runs the sweep's own filter_from_ray,
 * filter_disc2 and filter_disc1, tri_filter_from_ray (the idle parameters when the scene has no triangle filter record, as the sweep
 * sets them) and tri_filter_sign on the handle's resident sphere_f32 and tri_f32.  rays, objects and out are HOST arrays; the hook
 * copies, launches once, copies back and synchronises.
 * pairs (objects != NULL): entry i is ray i and Scene.objects[objects[i]], whose filter record is found through sphere_id, or through
 *   tri_fidx and the triangle table.  out: 24 words per entry --
 *   [0] flags: 1 a triangle; 2 the object has a filter record (else every other word is 0: planes, triangles that can never be hit);
 *       4 the ray's filter of that kind is pass-all; 8 the record is a CANDIDATE (the sign bit the sweep tests is clear)
 *   [1..8] a sphere: the eight FilterParams words {d.xyz, -p.d, 2p.xyz, E - p.p}; a triangle: the seven TriFilterParams words
 *       {d.xyz, -p.xyz, A} and 0
 *   [9..16] the record as the kernel read it: a sphere's {c - centre, |c - centre|^2 - r^2}, taken out of its pair, then 0; a triangle's
 *       A = {n, n.(v0 - centre)} and B = {cx, cy, hx, hy}
 *   [17] a sphere: D of filter_disc2 on the resident pair (this sphere's half); a triangle: tri_filter_sign's word, bits(sx) | bits(sy)
 *   [18] a sphere: D of filter_disc1 on the record of [9..12]   [19] the record's index (sphere_f32 / tri_f32)   [20..23] 0.
 * counts (objects == NULL): out holds 4 words per ray -- [0] the records of the WHOLE padded sphere array (n_spheres rounded up to a
 *   multiple of 4) and [1] of the n_tri_filter triangle records whose sign bit is clear: what the sweep queues for the ray;
 *   [2] 4: the sphere filter is pass-all, 16: the triangle filter is; [3] 0.
 * scene_info[16] (may be NULL; written even when n is 0): the centre the records are relative to (3), sphere_cmax, tri_extent,
 *   n_spheres, n_tri_filter, the sweep's queue sizes Q and kOverflowQ of the shipped instance, planes, triangles, objects, triangle
 *   records in the tree, 0, 0, 0.
 * tests/test_sweep_filters.py holds both filters to the f64 text on rays aimed at them. */
int32_t rtx_debug_sweep_filter(RtxSceneHandle scene, const RtxRay *rays, const uint32_t *objects, uint64_t n, uint32_t *out,
                               double *scene_info);

#ifdef __cplusplus
}
#endif
#endif
