"""rtx_scene_update_objects on the device.  After an update every entry point of the handle must return, bit for bit, what a freshly
uploaded handle returns for the updated object list ("Fresh"): frames under AUTO, the exhaustive and the LDS-sweep kernels (and both
forms of the sphere kernel), closest-hit and occlusion queries on 2000 rays, the pick buffer.  And the arrays scene_update_kernel
leaves on the device must be the ones the host reference leaves (tests/test_scene_update.py checked those): FNV digests of the
resident arrays against rtx_debug_host_refit's.  Every comparison is equality of bytes."""
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
