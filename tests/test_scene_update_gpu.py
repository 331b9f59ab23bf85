"""rtx_scene_update_objects on the device.  After an update every entry point of the handle must return, bit for bit, what a freshly
uploaded handle returns for the updated object list ("Fresh"): frames under AUTO, the exhaustive and the LDS-sweep kernels (and both
forms of the sphere kernel), closest-hit and occlusion queries on 2000 rays, the pick buffer -- and (_same_entry_points) path
radiance, sparse samples, the block band, progressive sums on top of the caller's earlier sums, a refinement round, the pixel
features and, on the lab library, the path transcripts.  And the arrays scene_update_kernel leaves on the device must be the ones
the host reference leaves (tests/test_scene_update.py checked those): FNV digests of the resident arrays against
rtx_debug_host_refit's.  Every comparison is equality of bytes.  tests/test_update_bounds.py aims rays at the refitted bounds."""
import numpy as np
import pytest

import update_cases as uc
from helpers import check_equal, fuzz_rays

W, H = 48, 27
CFG = dict(rays_per_pixel=3, max_bounces=3, seed=11)
GPU_SCENES = ["s%d" % n for n in uc.GPU_SPHERE_COUNTS] + ["mixed"]
CAM = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), np.pi / 2)


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _scene(rtx, objs, **over):
    return rtx.Scene.from_packed(rtx.Config(**dict(CFG, **over)), rtx.Camera(*CAM), objs)


def _configs(rtx, sphere_tree_only):
    out = [("auto", dict()), ("exact", dict(kernel=rtx.RTX_KERNEL_EXACT)), ("mixed", dict(kernel=rtx.RTX_KERNEL_MIXED))]
    if sphere_tree_only:
        out += [("one-stage", dict(tuning=rtx.RTX_TUNE_ONE_STAGE)), ("two-stage", dict(tuning=rtx.RTX_TUNE_TWO_STAGE))]
    return out


def _frame(hnd, stream=None, want_stats=True):
    import torch
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize(0)                       # (the fill runs on torch's stream, the render maybe on another)
    hnd.render_rows(W, H, 0, 1, H, buf.data_ptr(), stream=stream, want_stats=want_stats)
    return buf


def _same_everything(rtx, hnd, fresh, objs_now, what, frames_only=False, stages=True):
    sphere_tree_only = stages and not (uc.has(objs_now, 1) or uc.has(objs_now, 2))
    for name, over in _configs(rtx, sphere_tree_only):
        cfg = rtx.Config(**dict(CFG, **over))
        hnd.set_config(cfg)
        fresh.set_config(cfg)
        a, b = _frame(hnd).cpu().numpy(), _frame(fresh).cpu().numpy()
        assert a.tobytes() == b.tobytes(), (what, name, int((a != b).any(axis=2).sum()))
    if frames_only:
        return
    o, d = fuzz_rays(np.random.default_rng(5), objs_now, 2000)
    check_equal(hnd.query(o, d), fresh.query(o, d), what + ": query")
    assert np.array_equal(hnd.occluded(o, d), fresh.occluded(o, d)), what
    lim = np.random.default_rng(6).uniform(0.0, 12.0, len(o))
    assert np.array_equal(hnd.occluded(o, d, lim), fresh.occluded(o, d, lim)), what
    check_equal([np.asarray(x).reshape(W * H, -1) for x in hnd.pick(W, H)], [np.asarray(x).reshape(W * H, -1) for x in fresh.pick(W, H)],
                what + ": pick")


def _dev_bytes(t):
    return t.cpu().numpy().tobytes()


def _sums_before(hnd):
    """a caller's progressive accumulators: the samples [0, 3) of the scene the handle holds now, with second moments"""
    import torch
    total = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    sq = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize(0)
    hnd.render_accumulate(W, H, 0, 3, total.data_ptr(), sq.data_ptr())
    return total, sq


def _entry_points(hnd, objs_now, sums):
    """{name: bytes} of the entry points _same_everything does not call, under the handle's current config.  `sums`: the (sum,
    sum_sq) buffers a caller already holds; they are cloned, the clones accumulated into"""
    import torch
    import rust_raytracing_amd as rtx
    out = {}
    dev = torch.device("cuda", 0)
    # path radiance on the caller's rays, with (pixel, sample) ids
    o, d = fuzz_rays(np.random.default_rng(7), objs_now, 2000)
    ids = np.stack([np.random.default_rng(8).integers(0, 1 << 20, len(o)), np.random.default_rng(9).integers(0, 64, len(o))], axis=1).astype(np.uint64)
    out["radiance"] = hnd.radiance(o, d, ids=ids).tobytes()
    # about 1000 sparse samples of the frame
    rng = np.random.default_rng(10)
    pid = np.stack([rng.integers(0, W * H, 1000), rng.integers(0, 8, 1000)], axis=1).astype(np.uint64)
    d_ids = torch.from_numpy(pid.view(np.int64)).to(dev)
    d_rgb = torch.zeros(3 * len(pid), dtype=torch.float64, device=dev)
    d_seg = torch.zeros(len(pid), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    hnd.trace_samples(W, H, d_ids.data_ptr(), len(pid), d_rgb.data_ptr(), d_seg.data_ptr())
    out["trace_samples"] = _dev_bytes(d_rgb) + _dev_bytes(d_seg)
    # the band of part 1 of 3, blocks of 8 rows
    band = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    hnd.render_blocks(W, H, 8, 1, 3, band.data_ptr())
    out["render_blocks"] = _dev_bytes(band)
    # progressive sums: [0, 2) then [2, 3) on top of what the caller's buffers held before the update
    total, sq = sums[0].clone(), sums[1].clone()
    torch.cuda.synchronize(dev)
    hnd.render_accumulate(W, H, 0, 2, total.data_ptr(), sq.data_ptr())
    hnd.render_accumulate(W, H, 2, 1, total.data_ptr(), sq.data_ptr())
    out["render_accumulate"] = _dev_bytes(total) + _dev_bytes(sq)
    # one refinement round from three samples of this scene, tests/refine_cases.py's threshold and floor
    t2, q2 = torch.zeros_like(total), torch.zeros_like(sq)
    extra = torch.zeros((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    hnd.render_accumulate(W, H, 0, 3, t2.data_ptr(), q2.data_ptr())
    counts, _ = hnd.render_refine(W, H, 3, 3, 12, 0.5, 0.01, t2.data_ptr(), q2.data_ptr(), extra.data_ptr(), rounds=1)
    assert counts[0] > 0, "the refinement round selected nothing: the comparison would be empty"
    out["render_refine"] = _dev_bytes(t2) + _dev_bytes(q2) + _dev_bytes(extra) + np.array(counts, dtype=np.uint64).tobytes()
    # pixel features, whole and as a band
    item = rtx.FEATURE_DTYPE.itemsize
    feat = torch.zeros(W * H * item, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hnd.pixel_features(W, H, feat.data_ptr())
    out["features"] = _dev_bytes(feat)
    feat = torch.zeros(W * H * item, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hnd.pixel_features_blocks(W, H, 8, 1, 3, feat.data_ptr())
    out["pixel_features_blocks"] = _dev_bytes(feat)
    if hnd.lab:
        steps, counts = hnd.debug_paths(W, H, H // 2, 8)
        out["debug_paths"] = steps.tobytes() + counts.tobytes()
    return out


def _same_entry_points(hnd, fresh, objs_now, sums, what):
    a, b = _entry_points(hnd, objs_now, sums), _entry_points(fresh, objs_now, sums)
    assert set(a) == set(b)
    for k in a:
        assert len(a[k]) == len(b[k]) and len(a[k]) > 0, (what, k)
        if a[k] != b[k]:
            x, y = np.frombuffer(a[k], dtype=np.uint8), np.frombuffer(b[k], dtype=np.uint8)
            raise AssertionError("%s: %s differs from a fresh upload's in %d bytes, the first at %d" % (what, k, int((x != y).sum()), int(np.nonzero(x != y)[0][0])))


def _pairs():
    return [(s, c) for s in GPU_SCENES for c in uc.cases_for(uc.scene(s))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", _pairs())
def test_an_updated_scene_is_a_fresh_scene(gpu, name, case):
    objs = uc.scene(name)
    idx, new, want = uc.update(objs, case)
    now = uc.apply(objs, idx, new)
    # the device's arrays against the host reference's (the lab library carries the digest hooks)
    _, _, host = gpu.debug_host_refit(_scene(gpu, objs), idx, new)
    lab = _scene(gpu, objs).upload(0, lab=True)
    assert lab.update_objects(idx, new) == want
    assert lab.debug_resident_digests() == host, (name, case)
    lab.close()
    # the product library: every entry point against a fresh upload of the updated list
    hnd = _scene(gpu, objs).upload(0)
    old = _frame(hnd).cpu().numpy()                 # (a render before the update: scratch, tables and descriptor are in use)
    assert hnd.update_objects(idx, new) == want
    fresh = _scene(gpu, now).upload(0)
    if case in ("all", "inbox", "plane"):           # the case is worth its name: the updated scene's frame is another frame
        assert _frame(fresh).cpu().numpy().tobytes() != old.tobytes()
    _same_everything(gpu, hnd, fresh, now, "%s/%s" % (name, case))
    hnd.close()
    fresh.close()


@pytest.mark.gpu
def test_twenty_whole_scene_updates_in_a_row(gpu):
    """an animation: every sphere moves in every step; the arrays are the host reference's after each step (a refit depends on the
    topology and the geometry it ends with, so step k is held to the host refit of (base, update k)), the last frame is Fresh's"""
    objs = uc.scene("s300")
    lab = _scene(gpu, objs).upload(0, lab=True)
    hnd = _scene(gpu, objs).upload(0)
    now = objs
    for k in range(20):
        idx, new, want = uc.update(objs, "inbox" if k % 2 else "all", seed=100 + k)
        assert lab.update_objects(idx, new) == want == "refit"
        assert hnd.update_objects(idx, new) == "refit"
        _, _, host = gpu.debug_host_refit(_scene(gpu, objs), idx, new)
        assert lab.debug_resident_digests() == host, k
        now = uc.apply(objs, idx, new)
    fresh = _scene(gpu, now).upload(0)
    _same_everything(gpu, hnd, fresh, now, "step 20")
    _same_everything(gpu, lab, fresh, now, "step 20 (lab)", frames_only=True)
    for h in (lab, hnd, fresh):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s9", "s300", "mixed"])
def test_fallbacks_rebuild_and_errors_change_nothing(gpu, name):
    objs = uc.scene(name)
    for case in uc.fallbacks_for(objs):
        idx, new, want = uc.update(objs, case)
        hnd = _scene(gpu, objs).upload(0)
        assert hnd.update_objects(idx, new, mode="rebuild" if case == "rebuild" else "auto") == want == "rebuilt", case
        now = uc.apply(objs, idx, new)
        fresh = _scene(gpu, now).upload(0)
        _same_everything(gpu, hnd, fresh, now, "%s/%s" % (name, case), frames_only=True, stages=False)
        # a refit after the rebuild works on the new tree (the tables follow every pack)
        if case == "rebuild":
            i2, n2, w2 = uc.update(now, "third", seed=9)
            assert hnd.update_objects(i2, n2) == w2
            fresh.close()
            fresh = _scene(gpu, uc.apply(now, i2, n2)).upload(0)
            _same_everything(gpu, hnd, fresh, uc.apply(now, i2, n2), "%s/refit after rebuild" % name, frames_only=True)
        hnd.close()
        fresh.close()
    # errors are found before the first device write
    hnd = _scene(gpu, objs).upload(0)
    fresh = _scene(gpu, objs).upload(0)
    idx, new, _ = uc.update(objs, "third")
    bad_idx = idx.copy()
    bad_idx[-1] = len(objs)
    bad_kind = new.copy()
    bad_kind["kind"][-1] = 9
    bad_res = new.copy()
    bad_res["reserved"][-1] = 2
    for i, o, m, status in ((bad_idx, new, "auto", gpu.abi.RTX_ERR_INVALID_ARGUMENT), (idx, bad_kind, "auto", gpu.abi.RTX_ERR_UNSUPPORTED),
                            (idx, bad_res, "auto", gpu.abi.RTX_ERR_UNSUPPORTED), (idx, new, 5, gpu.abi.RTX_ERR_INVALID_ARGUMENT)):
        with pytest.raises(gpu.RtxError) as e:
            hnd.update_objects(i, o, mode=m)
        assert e.value.status == status
    assert hnd.update_objects(idx[:0], new[:0]) == "nothing"
    _same_everything(gpu, hnd, fresh, objs, "%s after errors" % name, frames_only=True)
    hnd.close()
    fresh.close()


@pytest.mark.gpu
def test_an_update_waits_for_the_frame_enqueued_before_it(gpu):
    """an asynchronous render on one stream, the update on another: the earlier frame is the pre-update scene's, the next one the
    updated scene's ("Streams": the update's writes are ordered behind what the handle enqueued before)"""
    import torch
    objs = uc.scene("s3000")
    idx, new, _ = uc.update(objs, "inbox")
    cfg = dict(rays_per_pixel=16)
    before = _scene(gpu, objs, **cfg).upload(0)
    after = _scene(gpu, uc.apply(objs, idx, new), **cfg).upload(0)
    want_before, want_after = _frame(before).cpu().numpy(), _frame(after).cpu().numpy()
    assert want_before.tobytes() != want_after.tobytes()
    hnd = _scene(gpu, objs, **cfg).upload(0)
    s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    early = _frame(hnd, stream=s1.cuda_stream, want_stats=False)
    assert hnd.update_objects(idx, new, stream=s2.cuda_stream) == "refit"
    late = _frame(hnd, stream=s2.cuda_stream, want_stats=False)
    torch.cuda.synchronize(0)
    assert early.cpu().numpy().tobytes() == want_before.tobytes()
    assert late.cpu().numpy().tobytes() == want_after.tobytes()
    for h in (before, after, hnd):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [("s65", "all"), ("s300", "inbox"), ("mixed", "material"), ("mixed", "plane")])
def test_the_remaining_entry_points_after_an_update(gpu, name, case):
    """include/rtx_hip.h promises Fresh's bits from EVERY entry point: path radiance on 2000 fuzz rays with ids, 1000 sparse samples,
    the band of part 1 of 3, progressive sums [0, 2) + [2, 3) with moments on top of sums the caller accumulated BEFORE the update
    (Fresh starts from copies: the update must not disturb the caller's accumulators), one refinement round, the pixel features
    whole and as a band -- on the product library; the same and one row of path transcripts on the lab library"""
    objs = uc.scene(name)
    idx, new, want = uc.update(objs, case)
    now = uc.apply(objs, idx, new)
    for lab in (False, True):
        hnd = _scene(gpu, objs).upload(0, lab=lab)
        sums = _sums_before(hnd)
        held = [_dev_bytes(t) for t in sums]
        assert hnd.update_objects(idx, new) == want
        fresh = _scene(gpu, now).upload(0, lab=lab)
        _same_entry_points(hnd, fresh, now, sums, "%s/%s%s" % (name, case, " (lab)" if lab else ""))
        assert [_dev_bytes(t) for t in sums] == held            # (the caller's own buffers: read, cloned, never written)
        hnd.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", uc.ONEPOINT_SCENES)
def test_the_fallback_the_device_finds_rebuilds_over_half_written_arrays(gpu, name):
    """collapse8 / onepoint_tiny pass plan_update; mode A has rewritten the records and mode B part of the boxes when a 64-byte node
    without an encoding sets kUpdateStatusNoQ3; the host reads the status word and rebuilds: "rebuilt", the host reference's arrays
    (a fresh pack's, tests/test_scene_update.py), and Fresh's bits from frames, query, occluded and pick -- lab and product.

    What this test found (first run, MI355X): nothing wrong -- "rebuilt" and Fresh's bits on all four scenes.  With the status word
    ignored on the host (a scratch build) every case fails on `how`: the update reports "refit" over a tree whose 64-byte nodes are
    partly the old ones."""
    objs = uc.scene(name)
    for case in uc.DEVICE_FALLBACK_CASES:
        idx, new, want = uc.update(objs, case)
        now = uc.apply(objs, idx, new)
        how, _, host = gpu.debug_host_refit(_scene(gpu, objs), idx, new)
        assert how == want == "rebuilt"
        fresh = _scene(gpu, now).upload(0)
        for lab in (True, False):
            hnd = _scene(gpu, objs).upload(0, lab=lab)
            _frame(hnd)                                      # (a render before the update: scratch, tables and descriptor are in use)
            assert hnd.update_objects(idx, new) == "rebuilt", (name, case, lab)
            if lab:
                assert hnd.debug_resident_digests() == host, (name, case)
            _same_everything(gpu, hnd, fresh, now, "%s/%s%s" % (name, case, " (lab)" if lab else ""))
            hnd.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s9", "s300"])
def test_the_tree_without_64_byte_nodes_refits_and_a_forced_rebuild_brings_them_back(gpu, name):
    """after collapse8 the handle holds a sphere tree WITHOUT the 64-byte form -- no upload of these suites makes one: a `third` move
    on it is a refit with q3nodes == null in mode B (the arrays are the host reference's of the two updates, everything is
    Fresh's); mode = "rebuild" of an update that spreads the eight spheres out again brings flags & 16 back"""
    objs = uc.scene(name)
    i1, n1, _ = uc.update(objs, "collapse8")
    mid = uc.apply(objs, i1, n1)
    i2, n2, _ = uc.update(mid, "third", seed=4)
    now = uc.apply(mid, i2, n2)
    _, stats, host = gpu.debug_host_refit(_scene(gpu, objs), np.concatenate([i1, i2]), np.concatenate([n1, n2]), split=len(i1))
    assert stats["flags"] & 16 == 0
    back = objs[i1.astype(np.int64)].copy()
    how, stats, host_back = gpu.debug_host_refit(_scene(gpu, now), i1, back, mode="rebuild")
    assert how == "rebuilt" and stats["flags"] & 16 and stats["quantised_nodes"] == stats["wide_nodes"]
    last = uc.apply(now, i1, back)
    fresh, fresh_last = _scene(gpu, now).upload(0), _scene(gpu, last).upload(0)
    for lab in (True, False):
        hnd = _scene(gpu, objs).upload(0, lab=lab)
        assert hnd.update_objects(i1, n1) == "rebuilt"
        assert hnd.update_objects(i2, n2) == "refit", (name, lab)
        if lab:
            assert hnd.debug_resident_digests() == host, name
        _same_everything(gpu, hnd, fresh, now, "%s/third after collapse8%s" % (name, " (lab)" if lab else ""), frames_only=lab)
        assert hnd.update_objects(i1, back, mode="rebuild") == "rebuilt"
        if lab:
            assert hnd.debug_resident_digests() == host_back, name
        _same_everything(gpu, hnd, fresh_last, last, "%s/spread out again%s" % (name, " (lab)" if lab else ""), frames_only=True)
        hnd.close()
    fresh.close()
    fresh_last.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s65", "s300"])
def test_every_sphere_at_one_point(gpu, name):
    """onepoint: every sphere at one corner of the move box with r = 1e-4 -- a refit that keeps the 64-byte form; every box of the
    tree coincides, so every ray that enters one enters all: frames (AUTO, exact, sweep, one- and two-stage) and queries are Fresh's"""
    objs = uc.scene(name)
    idx, new, want = uc.update(objs, "onepoint")
    now = uc.apply(objs, idx, new)
    _, stats, host = gpu.debug_host_refit(_scene(gpu, objs), idx, new)
    assert stats["flags"] & 16
    lab = _scene(gpu, objs).upload(0, lab=True)
    assert lab.update_objects(idx, new) == want == "refit"
    assert lab.debug_resident_digests() == host, name
    lab.close()
    hnd = _scene(gpu, objs).upload(0)
    assert hnd.update_objects(idx, new) == "refit"
    fresh = _scene(gpu, now).upload(0)
    _same_everything(gpu, hnd, fresh, now, "%s/onepoint" % name)
    hnd.close()
    fresh.close()


def _appended(objs):
    """10 more spheres inside the box the scene's spheres span: jittered copies of existing ones"""
    _, extra, _ = uc.update(objs, "third", seed=5)
    assert len(extra) >= 10
    return extra[:10].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s65", "mixed"])
def test_an_update_after_append_objects(gpu, name):
    """rtx_scene_append_objects replaces every array and the refit tables with them: a `third` update drawn from the APPENDED list
    (appended indices among them) is a refit of the new tree -- the host reference's arrays for the appended scene, Fresh's bits.
    A refit there and back before the append makes the first pack's device tables (box32, reach, the level lists) exist when the
    append replaces the pack: tables that outlived it would be too short for the appended spheres.

    What this test found (first run, MI355X): nothing wrong; upload_packed drops the tables with every pack."""
    objs = uc.scene(name)
    extra = _appended(objs)
    longer = np.concatenate([objs, extra])
    idx, new, want = uc.update(longer, "third", seed=6)
    assert (idx >= len(objs)).any() and (idx < len(objs)).any()
    now = uc.apply(longer, idx, new)
    _, _, host = gpu.debug_host_refit(_scene(gpu, longer), idx, new)
    fresh_longer, fresh = _scene(gpu, longer).upload(0), _scene(gpu, now).upload(0)
    for lab in (True, False):
        hnd = _scene(gpu, objs).upload(0, lab=lab)
        i0, n0, _ = uc.update(objs, "one")
        # there and back: the device tables of the FIRST pack exist when the append replaces the pack
        assert hnd.update_objects(i0, n0) == "refit" and hnd.update_objects(i0, objs[i0.astype(np.int64)].copy()) == "refit"
        hnd.append_objects(extra)
        _same_everything(gpu, hnd, fresh_longer, longer, "%s/appended" % name, frames_only=True)
        assert hnd.update_objects(idx, new) == want == "refit", (name, lab)
        if lab:
            assert hnd.debug_resident_digests() == host, name
        _same_everything(gpu, hnd, fresh, now, "%s/third after append%s" % (name, " (lab)" if lab else ""), frames_only=lab)
        hnd.close()
    fresh_longer.close()
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s65", "mixed"])
def test_updates_between_other_calls_of_the_handle(gpu, name):
    """set_camera and set_config between two updates; a material update (RECORDS) between two refits; on the joint scene a plane
    update right after a forced rebuild.  Frames after each step, everything at the end."""
    objs = uc.scene(name)
    cam2 = ((0.5, -0.25, 0.1), (1.0, 0.1, -0.05), np.pi / 2.5)

    def fresh_of(o, cam=CAM):
        return gpu.Scene.from_packed(gpu.Config(**CFG), gpu.Camera(*cam), o).upload(0)

    def step(hnd, now, cam, what, last=False):
        fresh = fresh_of(now, cam)
        _same_everything(gpu, hnd, fresh, now, "%s/%s" % (name, what), frames_only=not last)
        fresh.close()

    hnd = _scene(gpu, objs).upload(0)
    i, n, want = uc.update(objs, "third", seed=1)
    assert hnd.update_objects(i, n) == want == "refit"
    now = uc.apply(objs, i, n)
    step(hnd, now, CAM, "third")
    hnd.set_camera(gpu.Camera(*cam2))
    hnd.set_config(gpu.Config(**dict(CFG, rays_per_pixel=2, seed=5)))
    i, n, want = uc.update(objs, "inbox", seed=2)
    assert hnd.update_objects(i, n) == want == "refit"
    now = uc.apply(now, i, n)
    step(hnd, now, cam2, "inbox after set_camera and set_config")
    i, n, want = uc.update(now, "material", seed=3)
    assert hnd.update_objects(i, n) == want == "records"
    now = uc.apply(now, i, n)
    step(hnd, now, cam2, "material between two refits")
    i, n, want = uc.update(objs, "all", seed=4)
    assert hnd.update_objects(i, n) == want == "refit"
    now = uc.apply(now, i, n)
    if name == "mixed":
        step(hnd, now, cam2, "all after material")
        i, n, _ = uc.update(now, "third", seed=7)
        assert hnd.update_objects(i, n, mode="rebuild") == "rebuilt"
        now = uc.apply(now, i, n)
        i, n, want = uc.update(now, "plane")
        assert hnd.update_objects(i, n) == want == "records"
        now = uc.apply(now, i, n)
    step(hnd, now, cam2, "the end", last=True)
    hnd.close()
