// rtx_host.h -- what the device-facing host translation units (rtx_api.hip, rtx_api_update.hip, rtx_api_debug.hip) share: the
// HIP error check, the scene handle, and the helpers they call across files (rtx::host, hidden: rtx_pack.h).
#pragma once

#include "rtx_launch.h"
#include "rtx_pack.h"

using namespace rtx;
using namespace rtx::host;

#define RTX_HIP_CHECK(expr)                                                                              \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(e_ == hipErrorOutOfMemory ? RTX_ERR_OUT_OF_MEMORY : RTX_ERR_HIP,                 \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                              \
    } while (0)

struct RtxSceneHandle_ {
    int device = 0;
    int n_cus = 0;
    RtxConfig cfg{};
    RtxCamera cam{};
    SceneView sv{};
    std::vector<RtxObject> objects;                       // Scene.objects as uploaded (rtx_scene_append_objects re-packs them)
    std::vector<uint8_t> hidden;                          // rtx_scene_set_visible: one byte per object (1: hidden; empty: none ever was)
    std::vector<void *> scene_allocs;
    // rtx_scene_update_objects: the host tables of the resident pack, and their device side -- made at the first REFIT or RECORDS
    // call, dropped by any rebuild (upload_packed)
    RefitTables refit;
    struct UpdateBufs {
        bool valid = false;
        uint32_t *levels = nullptr; float *box32 = nullptr; double *reach = nullptr;
        bool mesh_valid = false;                                // the triangle half: made at the first DEFORM call that moves a triangle
        uint32_t *all_levels = nullptr; float *tribox32 = nullptr; double *tri_reach = nullptr;
        bool keep_valid = false;                                // the kept words (rtx_refit.h): made by the first visibility call after a pack
        uint32_t *keep = nullptr;
        UpdateEntry *h_entries = nullptr; size_t h_cap = 0;     // pinned staging of the update list
        UpdateEntry *d_entries = nullptr; size_t d_cap = 0;
        unsigned long long *d_status = nullptr, *h_status = nullptr;   // {status bits, the bits of the new sphere_cmax, of the new tri_extent}; h_status pinned
    } upd;
    // scratch, grown on demand
    double *samples = nullptr;  size_t samples_bytes = 0;
    double *acc = nullptr;      size_t acc_bytes = 0;
    double *tables = nullptr;   size_t tables_doubles = 0;
    double *h_tables = nullptr; size_t h_tables_doubles = 0;
    double *state = nullptr;    size_t state_bytes = 0;
    void *wf_state = nullptr;   size_t wf_bytes = 0;       // the wavefront kernels' ray state
    void *tile_lists = nullptr; size_t tile_lists_bytes = 0;   // what each tile's primary rays can reach (build_mesh_tile_lists_kernel)
    // The lists depend on the tree, the camera and the frame's geometry alone, so a call that renders the frame of the call before it
    // (a progressive render's next samples, an adaptive round, the same band again) builds none: tl_key says what the buffer holds.
    // scene_gen: bumped by whatever can change the tree, the shapes, the camera, the config or the scratch cap (touch_scene); any
    // doubt -- a buffer that grew, a launch that failed, a call without lists -- clears tl_key.valid and the next call builds.
    uint64_t scene_gen = 0;
    struct TileListKey {
        bool valid = false;
        uint64_t scene_gen = 0;
        RtxCamera cam{};
        uint32_t width = 0, height = 0, row_begin = 0, row_stride = 0, row_block = 0, n_rows = 0, tiles_x = 0;
        uint32_t kernel = 0, tuning = 0;                      // the list form: RTX_KERNEL_BVH a sphere tree's entries, RTX_KERNEL_WAVEFRONT a mesh's pairs
        const void *buffer = nullptr; size_t bytes = 0;       // the handle's buffer and what the plan carved of it
    } tl_key;
#ifdef RTX_LAB
    // (lab) rtx_debug_tile_lists: the shape of the lists the last render call handed its launch -- 0 none, 1 a sphere tree's
    // TileEntry lists, 2 the {entry, t_lb} pairs of a mesh or joint tree --, its tile grid; the launches this handle's calls
    // asked to BUILD lists (info[5]: a call that finds its frame's lists in the buffer adds none)
    uint32_t tl_form = 0, tl_tiles_x = 0, tl_tiles = 0, tl_builds = 0;
#endif
    PathStep *transcript = nullptr; uint32_t *transcript_counts = nullptr; uint32_t transcript_steps = 0;   // (lab) rtx_debug_paths, set for one call
    Counters *counters = nullptr;
    unsigned long long *work_counter = nullptr;
    SceneView *d_sv = nullptr;  bool sv_dirty = true;     // device copy of sv (kernels take it by pointer)
    RowsView *d_rv = nullptr;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };      // [3]: the end of the sphere kernel's stage 1 (stats only)
    // The second half's own stream and buffers when a launch runs as two halves in flight (render_band, "halves"): created on first use.
    struct SecondHalf {
        hipStream_t stream = nullptr;
        hipEvent_t fork = nullptr, join = nullptr, stage1_done = nullptr;
        Counters *counters = nullptr, *counters_stage1 = nullptr;
        unsigned long long *work_counter = nullptr;
        RowsView *d_rv = nullptr;
        double *state = nullptr;    size_t state_bytes = 0;
        void *queue = nullptr;      size_t queue_bytes = 0;
    } half2;
    Counters *counters_stage1 = nullptr;                   // the counters as stage 1 left them (stats only)
    // The handle's device buffers (descriptors, tables, counters, scratch) are shared by all of its renders, so they
    // are ordered on ONE stream at a time: when a call brings a different stream the previous one is drained first.
    size_t scratch_limit = 0;                             // rtx_scene_set_scratch_limit (0 = default)
    hipStream_t last_stream = nullptr;                    // compared, never used: the caller may have destroyed it since
    bool have_last_stream = false;
    hipEvent_t ev_done = nullptr;                         // recorded at the end of every render, on the stream it ran on
    bool have_done = false;
    // Round-bound watchdog of the sweep kernel (ctr[1].pad_): copied to this pinned word after every launch and looked
    // at by the next entry point that finds the copy complete (and by rtx_scene_free), so that the asynchronous
    // stats == NULL path reports it too.
    unsigned long long *h_watchdog = nullptr;
    hipEvent_t ev_watchdog = nullptr;
    bool watchdog_pending = false;
    // what the trig tables currently hold
    uint32_t t_w = 0, t_h = 0, t_rb = 0, t_rs = 0, t_blk = 0, t_nr = 0;
    double t_fov = 0.0;
    bool t_valid = false;
};

RTX_HOST_BEGIN

// Called by every entry point and helper that may change what the tile lists were built from (the resident arrays, h->sv, the camera,
// the config, the scratch cap), before it changes anything: the lists in the handle's buffer are then nobody's (tl_key).
inline void touch_scene(RtxSceneHandle_ *h) { ++h->scene_gen; h->tl_key.valid = false; }

// the non-zero mask of a launch's sample records (store_sample, rtx_device.h): one bit per ray-queue slot, in whole 32-bit words
inline size_t nonzero_mask_bytes(uint64_t n_rays) { return (size_t)((n_rays + 31) / 32) * sizeof(uint32_t); }

// The samples a call traces and where their fold goes.  A render: [0, rays_per_pixel) from zero into out = sum / rays_per_pixel.
// rtx_render_blocks_accumulate (sum != null): [begin, begin + n) on top of what the caller's sum (and sum_sq, or null) hold; nothing
// is divided and no accumulator of the handle's is used -- the caller's buffers have its layout.
struct SampleRange { uint64_t begin = 0, n = 0; double *sum = nullptr, *sum_sq = nullptr; };

// From adopt_stream on, work may be enqueued on `stream`, and last_stream already names it: whatever way the call leaves -- a failed
// HIP call after some launches, the watchdog return, the empty-scene answer -- the event a later call on ANOTHER stream waits
// for (adopt_stream) is recorded behind everything enqueued so far, so that call never reuses the handle's scratch early.
struct DoneGuard {
    RtxSceneHandle_ *h; hipStream_t stream;
    ~DoneGuard() {
        if (hipEventRecord(h->ev_done, stream) == hipSuccess) h->have_done = true;
        else { (void)hipGetLastError(); (void)hipDeviceSynchronize(); h->have_done = false; }   // (no event: drain instead)
    }
};

// The angles of get_ray_dir's trig tables, in the reference's operation order: what the render's own tables (ensure_tables, rtx_api.hip)
// and rtx_temporal_tables (rtx_temporal.hip) take the host libm's sines of -- one text, so the two cannot drift.
inline double table_vertical_fov(double fov, uint32_t width, uint32_t height) { return (double)height / (double)width * fov; }   // scene.rs:145
inline double table_angle(double fov, uint32_t i, uint32_t n)
{
    const double u = (double)i / (double)n;                 // scene.rs:153 (v, of the image row), :157 (u)
    return fov * (u - 0.5);                                 // scene.rs:214-215
}

// rtx_api.hip
int usable_device_count();
int32_t check_device(int32_t device, const char *who);      // a usable gfx950 `device`, or the status with the error text set
struct Range { const void *base; size_t bytes; };            // one of the caller's arrays (a null base: an optional one that was not given)
bool ranges_overlap(const Range *r, int n);
void drop_update_tables(RtxSceneHandle_ *h);
int32_t upload_packed(RtxSceneHandle_ *h, const PackedScene &p);
int32_t check_watchdog(RtxSceneHandle_ *h, bool wait);
int32_t adopt_stream(RtxSceneHandle_ *h, hipStream_t stream);
int32_t render_band(RtxSceneHandle_ *h, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_stride, uint32_t row_block,
                    uint32_t n_rows, double *d_out_rgb, void *stream_, RtxStats *stats, const SampleRange *accumulate = nullptr);

RTX_HOST_END
