//! FFI declarations of `librtx_hip.so` -- a field-for-field mirror of `include/rtx_hip.h`.
//! UNCOMPILED here (no Rust toolchain in the image that wrote it); the layouts are checked against the header's
//! `RTX_STATIC_ASSERT`s by `tests/test_abi_and_host.py::test_rust_shim_matches_the_header`.
#![allow(dead_code)]
use std::os::raw::{c_char, c_void};

pub const RTX_SPHERE: u32 = 0;
pub const RTX_PLANE: u32 = 1;
pub const RTX_TRIANGLE: u32 = 2;
pub const RTX_KERNEL_AUTO: u32 = 0;

/// One entry of `Scene.objects` (scene.rs:80): `Object{shape, material}` flattened.  136 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxObject {
    pub kind: u32,
    pub reserved: u32,
    pub geom: [f64; 9],
    pub base_color: [f64; 3],
    pub emission_color: [f64; 3],
    pub roughness: f64,
}

/// `Config` (scene.rs:16-28) + seed, kernel.  56 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxConfig {
    pub rays_per_pixel: u64,
    pub max_bounces: u64,
    pub focal_length: f64,
    pub focal_offset: f64,
    pub non_focal_offset: f64,
    pub seed: u64,
    pub kernel: u32,
    /// `RTX_TUNE_*` bits: A/B switches for tests and lab runs; 0 = what ships.
    pub tuning: u32,
}

/// `Camera` (camera.rs:7-15); the matrices as three rows, row-major.  200 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxCamera {
    pub fov: f64,
    pub position: [f64; 3],
    pub direction: [f64; 3],
    pub to_cam_space: [f64; 9],
    pub to_world_space: [f64; 9],
}

/// `Scene` (scene.rs:78-85).  272 bytes.
#[repr(C)]
pub struct RtxScene {
    pub config: RtxConfig,
    pub camera: RtxCamera,
    pub n_objects: u64,
    pub objects: *const RtxObject,
}

/// Counters of one `rtx_render_rows` call.  104 bytes.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtxStats {
    pub primary_rays: u64,
    pub segments: u64,
    pub exact_tests: u64,
    pub filter_tests: u64,
    pub trace_ms: f64,
    pub resolve_ms: f64,
    pub filter_mismatches: u64,
    pub box_tests: u64,
    pub trace_launches: u32,
    pub kernel: u32,
    pub stage1_ms: f64,
    pub stage1_box_tests: u64,
    pub stage1_filter_tests: u64,
    pub stage1_exact_tests: u64,
}

/// One ray of a closest-hit query (`rtx_scene_closest_hits`, `rtx_closest_hits`); the direction is used as given.  48 bytes.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtxRay {
    pub position: [f64; 3],
    pub direction: [f64; 3],
}

/// The answer of `closest_object` (scene.rs:243-251) for one ray: hit point, `normal_at` there, distance, index in
/// `Scene.objects` (-1, +inf and NaNs when nothing is hit).  64 bytes.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtxHit {
    pub position: [f64; 3],
    pub normal: [f64; 3],
    pub distance: f64,
    pub object: i64,
}

/// One pixel of the denoising guide buffers (`rtx_scene_pixel_features`): the first hits of `render_pixel`'s own rays, folded in
/// sample order -- mean `base_color`, `emission_color`, `normal_at` (not renormalised), mean distance of the samples that hit (+inf:
/// none), hits / rays_per_pixel, and sample 0's winner in `Scene.objects` (-1: it missed).  96 bytes.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtxPixelFeatures {
    pub albedo: [f64; 3],
    pub emission: [f64; 3],
    pub normal: [f64; 3],
    pub depth: f64,
    pub coverage: f64,
    pub object: i64,
}

/// `RtxTemporalParams` (include/rtx_hip.h, "Temporal accumulation"): fill it with `rtx_temporal_default_params`.  48 bytes.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtxTemporalParams {
    pub alpha_min: f64,
    pub max_history: f64,
    pub plane_tolerance: f64,
    pub normal_min: f64,
    pub min_weight: f64,
    pub flags: u32,
    pub reserved: u32,
}

/// `RtxObjectMotion.kind` of an object with no previous geometry to rewind to (include/rtx_hip.h, "Rewinding a pick buffer").
pub const RTX_MOTION_LOST: u32 = 0xFFFF_FFFF;

/// `RtxObjectMotion`: one moved object's geometry now and when the previous frame's pick was taken.  152 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxObjectMotion {
    pub kind: u32,
    pub reserved: u32,
    pub now: [f64; 9],
    pub before: [f64; 9],
}

/// `RtxUpsampleParams` (include/rtx_hip.h, "Guided upsampling"): fill it with `rtx_upsample_default_params`.  48 bytes.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtxUpsampleParams {
    pub factor: u32,
    pub flags: u32,
    pub normal_power_log2: u32,
    pub reserved: u32,
    pub sigma_depth: f64,
    pub sigma_albedo: f64,
    pub albedo_min: f64,
    pub min_weight: f64,
}
pub const RTX_UPSAMPLE_MAX_FACTOR: u32 = 8;
pub const RTX_UPSAMPLE_DEMODULATE: u32 = 1;

#[repr(C)]
pub struct RtxSceneHandleOpaque {
    _private: [u8; 0],
}
pub type RtxSceneHandle = *mut RtxSceneHandleOpaque;

extern "C" {
    pub fn rtx_version() -> i32;
    pub fn rtx_last_error() -> *const c_char;
    pub fn rtx_device_count() -> i32;
    pub fn rtx_lab_build() -> i32;
    pub fn rtx_camera_new(position: *const f64, direction: *const f64, fov: f64, out: *mut RtxCamera) -> i32;
    pub fn rtx_render(scene: *const RtxScene, width: u32, height: u32, out_rgb: *mut f64) -> i32;
    pub fn rtx_render_to_image(scene: *const RtxScene, width: u32, height: u32, out_rgb8: *mut u8) -> i32;
    pub fn rtx_render_devices(scene: *const RtxScene, width: u32, height: u32, devices: *const i32, n_devices: u32, out_rgb: *mut f64) -> i32;
    pub fn rtx_render_to_image_devices(scene: *const RtxScene, width: u32, height: u32, devices: *const i32, n_devices: u32, out_rgb8: *mut u8) -> i32;
    pub fn rtx_scene_upload(scene: *const RtxScene, device: i32, out: *mut RtxSceneHandle) -> i32;
    pub fn rtx_scene_free(scene: RtxSceneHandle) -> i32;
    pub fn rtx_scene_set_config(scene: RtxSceneHandle, config: *const RtxConfig) -> i32;
    pub fn rtx_scene_set_scratch_limit(scene: RtxSceneHandle, bytes: u64) -> i32;
    pub fn rtx_scene_append_objects(scene: RtxSceneHandle, objects: *const RtxObject, n_objects: u64) -> i32;
    pub fn rtx_scene_update_objects(scene: RtxSceneHandle, indices: *const u64, objects: *const RtxObject, n: u64, mode: u32,
                                    stream: *mut c_void, how: *mut u32) -> i32;
    pub fn rtx_scene_set_camera(scene: RtxSceneHandle, camera: *const RtxCamera) -> i32;
    pub fn rtx_render_rows(scene: RtxSceneHandle, width: u32, height: u32, row_begin: u32, row_stride: u32, n_rows: u32, d_out_rgb: *mut f64, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_blocks_row_count(height: u32, block_rows: u32, part: u32, n_parts: u32) -> u32;
    pub fn rtx_render_blocks(scene: RtxSceneHandle, width: u32, height: u32, block_rows: u32, part: u32, n_parts: u32, d_out_rgb: *mut f64, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_render_blocks_accumulate(scene: RtxSceneHandle, width: u32, height: u32, block_rows: u32, part: u32, n_parts: u32, sample_begin: u64, n_samples: u64, d_sum: *mut f64, d_sum_sq: *mut f64, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_scene_closest_hits(scene: RtxSceneHandle, d_rays: *const RtxRay, n: u64, d_hits: *mut RtxHit, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_scene_primary_hits(scene: RtxSceneHandle, width: u32, height: u32, d_hits: *mut RtxHit, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_closest_hits(scene: *const RtxScene, rays: *const RtxRay, n: u64, hits: *mut RtxHit) -> i32;
    pub fn rtx_scene_any_hits(scene: RtxSceneHandle, d_rays: *const RtxRay, d_t_max: *const f64, n: u64, d_occluded: *mut u8, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_any_hits(scene: *const RtxScene, rays: *const RtxRay, t_max: *const f64, n: u64, occluded: *mut u8) -> i32;
    pub fn rtx_scene_multi_hits(scene: RtxSceneHandle, d_rays: *const RtxRay, d_t_max: *const f64, n: u64, k: u32, d_hits: *mut RtxHit, d_counts: *mut u32, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_scene_primary_multi_hits(scene: RtxSceneHandle, width: u32, height: u32, k: u32, d_hits: *mut RtxHit, d_counts: *mut u32, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_multi_hits(scene: *const RtxScene, rays: *const RtxRay, t_max: *const f64, n: u64, k: u32, hits: *mut RtxHit, counts: *mut u32) -> i32;
    pub fn rtx_scene_trace_paths(scene: RtxSceneHandle, d_rays: *const RtxRay, d_ids: *const u64, n: u64, d_rgb: *mut f64, d_segments: *mut u32, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_trace_paths(scene: *const RtxScene, rays: *const RtxRay, ids: *const u64, n: u64, rgb: *mut f64, segments: *mut u32) -> i32;
    pub fn rtx_scene_trace_samples(scene: RtxSceneHandle, width: u32, height: u32, d_ids: *const u64, n: u64, d_rgb: *mut f64, d_segments: *mut u32, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_render_blocks_refine(scene: RtxSceneHandle, width: u32, height: u32, block_rows: u32, part: u32, n_parts: u32, sample_begin: u64, n_more: u32, max_samples: u32, rounds: u32, threshold: f64, floor: f64, d_sum: *mut f64, d_sum_sq: *mut f64, d_extra: *mut u32, result: *mut u64, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_trace_samples(scene: *const RtxScene, width: u32, height: u32, ids: *const u64, n: u64, rgb: *mut f64, segments: *mut u32) -> i32;
    pub fn rtx_scene_pixel_features(scene: RtxSceneHandle, width: u32, height: u32, d_features: *mut RtxPixelFeatures, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_scene_pixel_features_blocks(scene: RtxSceneHandle, width: u32, height: u32, block_rows: u32, part: u32, n_parts: u32, d_features: *mut RtxPixelFeatures, stream: *mut c_void, stats: *mut RtxStats) -> i32;
    pub fn rtx_pixel_features(scene: *const RtxScene, width: u32, height: u32, features: *mut RtxPixelFeatures) -> i32;
    pub fn rtx_debug_resolve_moments(records: *const f64, mask: *const u32, width: u32, n_rows: u32, tiles_x: u32, n_samples: u32, sum: *mut f64, sum_doubles: u64, sum_sq: *mut f64, sum_sq_doubles: u64) -> i32;
    pub fn rtx_quantize_image_device(d_rgb: *const f64, width: u32, height: u32, d_rgb8: *mut u8, device: i32, stream: *mut c_void) -> i32;
    pub fn rtx_temporal_default_params(out: *mut RtxTemporalParams);
    pub fn rtx_temporal_tables(fov: f64, width: u32, height: u32, tables: *mut f64) -> i32;
    pub fn rtx_temporal_accumulate_device(d_rgb: *const f64, d_var: *const f64, d_hits: *const RtxHit, d_hist_rgb: *const f64, d_hist_var: *const f64, d_hist_len: *const f64, d_hist_hits: *const RtxHit, prev_camera: *const RtxCamera, d_prev_tables: *const f64, width: u32, height: u32, params: *const RtxTemporalParams, d_out_rgb: *mut f64, d_out_var: *mut f64, d_out_len: *mut f64, d_motion: *mut f64, device: i32, stream: *mut c_void) -> i32;
    pub fn rtx_rewind_hits_device(d_hits: *const RtxHit, n_hits: u64, d_objects: *const i64, d_motions: *const RtxObjectMotion, m: u64, flags: u32, d_out: *mut RtxHit, device: i32, stream: *mut c_void) -> i32;
    pub fn rtx_rewind_hits(hits: *const RtxHit, n_hits: u64, objects: *const i64, motions: *const RtxObjectMotion, m: u64, out: *mut RtxHit) -> i32;
    pub fn rtx_object_motions(indices: *const u64, before: *const RtxObject, now: *const RtxObject, n: u64, objects_out: *mut i64, motions_out: *mut RtxObjectMotion, m_out: *mut u64) -> i32;
    pub fn rtx_upsample_default_params(out: *mut RtxUpsampleParams);
    pub fn rtx_upsample_device(d_lo_rgb: *const f64, d_lo_var: *const f64, d_lo_features: *const RtxPixelFeatures, d_features: *const RtxPixelFeatures, width: u32, height: u32, params: *const RtxUpsampleParams, d_out: *mut f64, d_var_out: *mut f64, device: i32, stream: *mut c_void) -> i32;
    pub fn rtx_upsample(lo_rgb: *const f64, lo_var: *const f64, lo_features: *const RtxPixelFeatures, features: *const RtxPixelFeatures, width: u32, height: u32, params: *const RtxUpsampleParams, out: *mut f64, var_out: *mut f64) -> i32;
    pub fn rtx_temporal_accumulate(rgb: *const f64, var: *const f64, hits: *const RtxHit, hist_rgb: *const f64, hist_var: *const f64, hist_len: *const f64, hist_hits: *const RtxHit, prev_camera: *const RtxCamera, width: u32, height: u32, params: *const RtxTemporalParams, out_rgb: *mut f64, out_var: *mut f64, out_len: *mut f64, motion: *mut f64) -> i32;
}

/// The reference reports failures by panicking (scene.rs:168, object.rs:38,50); so does the shim.
pub fn check(rc: i32) {
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(rtx_last_error()) }.to_string_lossy().into_owned();
        panic!("rtx_hip (status {rc}): {msg}");
    }
}

// ---- what the device path needs and the reference's types cannot carry -------------------------------------------------
// `Config` and `Scene` are plain `pub` structs that users build with struct literals (scene.rs:16-28, :78-85), so the shim
// adds NO field to them -- and NO process-wide state either: `Scene::render(&self)` is re-entrant in the reference and may run
// on several threads at once (clones share the shapes behind Arc<Mutex>, object.rs:9-15), so two scenes must be able to render
// with different seeds / device lists concurrently.  The two settings the device path adds travel PER CALL:
//   * the render seed: the reference draws from fastrand's never-seeded thread-local generator on one thread per row
//     (math/vector.rs:31-38, scene.rs:151) -- every run renders a different image.  `None` keeps that behaviour (a fresh
//     key per call); `Some(k)` makes a render reproducible (it never was).
//   * the GPUs a frame is partitioned over (blocks of rows, one gather); empty: device 0.
// `SceneHipExt` (patches/scene_render.rs implements it for `Scene`) takes them as arguments; the reference's own
// `Scene::render(&self, w, h)` delegates to it with this THREAD's defaults, which `with_render_defaults` scopes.
use std::cell::RefCell;

#[derive(Clone, Debug, Default)]
pub struct RenderOptions {
    pub seed: Option<u64>,
    pub devices: Vec<i32>,
}

impl RenderOptions {
    pub fn seeded(seed: u64) -> Self { RenderOptions { seed: Some(seed), devices: Vec::new() } }
    pub fn on(devices: &[i32]) -> Self { RenderOptions { seed: None, devices: devices.to_vec() } }
    /// The key of THIS call: the fixed seed, or a fresh one (the reference's "a different image every run").
    pub fn key(&self) -> u64 { self.seed.unwrap_or_else(|| fastrand::u64(..)) }
}

thread_local! {
    static DEFAULTS: RefCell<RenderOptions> = RefCell::new(RenderOptions::default());
}

/// What `Scene::render(&self, w, h)` -- the reference's signature, which has no room for options -- uses on this thread.
pub fn render_defaults() -> RenderOptions {
    DEFAULTS.with(|d| d.borrow().clone())
}

/// Runs `f` with `opts` as this thread's defaults and restores the previous ones afterwards (also when `f` panics, as the
/// reference's render does on failure): `hip::with_render_defaults(RenderOptions::seeded(7), || scene.render(w, h))`.
pub fn with_render_defaults<R>(opts: RenderOptions, f: impl FnOnce() -> R) -> R {
    struct Restore(Option<RenderOptions>);
    impl Drop for Restore {
        fn drop(&mut self) {
            if let Some(prev) = self.0.take() { DEFAULTS.with(|d| *d.borrow_mut() = prev); }
        }
    }
    let _restore = Restore(Some(DEFAULTS.with(|d| std::mem::replace(&mut *d.borrow_mut(), opts))));
    f()
}

/// The per-call form of the render entry points (implemented for `Scene` in patches/scene_render.rs).
pub trait SceneHipExt {
    type Pixel;
    /// `Scene::render` with everything the device path adds passed explicitly.
    fn render_with(&self, width: usize, height: usize, opts: &RenderOptions) -> Vec<Vec<Self::Pixel>>;
    /// A reproducible render: the same seed gives the same image on any partition of the frame.
    fn render_seeded(&self, width: usize, height: usize, seed: u64) -> Vec<Vec<Self::Pixel>> {
        self.render_with(width, height, &RenderOptions::seeded(seed))
    }
    /// The frame partitioned over `devices` (blocks of 8 rows round-robin, one gather on `devices[0]`).
    fn render_on(&self, width: usize, height: usize, devices: &[i32]) -> Vec<Vec<Self::Pixel>> {
        self.render_with(width, height, &RenderOptions::on(devices))
    }
}
