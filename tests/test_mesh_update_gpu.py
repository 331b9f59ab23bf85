"""RTX_UPDATE_DEFORM on the device: triangles that get new vertices and keep their class are rewritten and refitted in place.  After
the update every entry point of the handle must return, bit for bit, what a freshly uploaded handle returns for the updated object
list ("Fresh") -- frames under AUTO, the exhaustive and the LDS-sweep kernels (on the two larger scenes also the wavefront form, the
regrouping mesh kernel and the tile-free launch: the packets, the tile lists, the queue-fed stage), 2000-ray closest-hit and
occlusion queries, the pick buffer, and on one pair per scene every other entry point -- and the arrays scene_update_kernel leaves
on the device must be the ones the host reference leaves (tests/test_mesh_update.py checked those): the 16 FNV digests of the
resident arrays against rtx_debug_host_refit_mesh's.  Every comparison is equality of bytes.  The scenes, the cases and the class
rule that predicts `how`: tests/mesh_update_cases.py."""
import numpy as np
import pytest

import mesh_update_cases as mc
import test_scene_update_gpu as su
from test_scene_update_gpu import CFG, H, W, _dev_bytes, _frame, _same_everything, _scene, _sums_before

BIG = ("t1100", "cubes25")                          # where the wavefront / regroup / tile-free forms are compared too


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _same_big_forms(rtx, hnd, fresh, what):
    for name, over in (("wavefront", dict(kernel=rtx.RTX_KERNEL_WAVEFRONT)), ("regroup", dict(kernel=rtx.RTX_KERNEL_BVH_REGROUP)),
                       ("no-tiles", dict(tuning=rtx.RTX_TUNE_NO_TILES))):
        cfg = rtx.Config(**dict(CFG, **over))
        hnd.set_config(cfg)
        fresh.set_config(cfg)
        a, b = _frame(hnd).cpu().numpy(), _frame(fresh).cpu().numpy()
        assert a.tobytes() == b.tobytes(), (what, name, int((a != b).any(axis=2).sum()))
    hnd.set_config(rtx.Config(**CFG))
    fresh.set_config(rtx.Config(**CFG))


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", mc.pairs())
def test_a_deformed_scene_is_a_fresh_scene(gpu, name, case):
    objs, idx, new, want, mode = mc.case_of(name, case)
    now = mc.apply(objs, idx, new)
    # the device's arrays against the host reference's (the lab library carries the digest hooks)
    how, _, host, _ = gpu.debug_host_refit_mesh(_scene(gpu, objs), idx, new, mode=mode)
    assert how == want
    lab = _scene(gpu, objs).upload(0, lab=True)
    assert lab.update_objects(idx, new, mode=mode) == want
    assert lab.debug_resident_mesh_digests() == host, (name, case)
    lab.close()
    # the product library: every entry point against a fresh upload of the updated list
    hnd = _scene(gpu, objs).upload(0)
    old = _frame(hnd).cpu().numpy()                 # (a render before the update: scratch, tables, tile lists and descriptor are in use)
    old_pick = [np.asarray(x).tobytes() for x in hnd.pick(W, H)]
    assert hnd.update_objects(idx, new, mode=mode) == want
    fresh = _scene(gpu, now).upload(0)
    if case == "shrink":                            # the case is worth its name: the updated scene's frame is another frame
        if old.any():
            assert _frame(fresh).cpu().numpy().tobytes() != old.tobytes()
        else:                                       # (t6: no lit triangle in view, a black frame -- there the primary hits are other hits)
            assert name == "t6" and [np.asarray(x).tobytes() for x in fresh.pick(W, H)] != old_pick
    _same_everything(gpu, hnd, fresh, now, "%s/%s" % (name, case))
    if name in BIG:
        _same_big_forms(gpu, hnd, fresh, "%s/%s" % (name, case))
    hnd.close()
    fresh.close()


class _EmptyRoundAllowed:
    """A handle as the sphere suite's _entry_points sees it on t6 and t40.  From the tests' camera t6 is black and the lit pixels of
    t40 have three equal samples: no pixel has a variance, so no threshold selects one, and the helper's guard ("the refinement
    round selected nothing") cannot hold on these scenes whatever the update did.  The round still runs, and its sums, counts and
    extra-sample buffer are still compared with Fresh's; only the count the guard reads is given as 1 when it was 0 -- for both
    handles alike, and the true counts are compared here."""

    def __init__(self, hnd):
        self._hnd, self.true_counts = hnd, None

    def __getattr__(self, k):
        return getattr(self._hnd, k)

    def render_refine(self, *a, **kw):
        counts, stats = self._hnd.render_refine(*a, **kw)
        self.true_counts = tuple(counts)
        return (max(counts[0], 1),) + tuple(counts[1:]), stats


DARK = ("t6", "t40")


def _same_entry_points(name, hnd, fresh, now, sums, what):
    if name not in DARK:
        return su._same_entry_points(hnd, fresh, now, sums, what)
    a, b = _EmptyRoundAllowed(hnd), _EmptyRoundAllowed(fresh)
    su._same_entry_points(a, b, now, sums, what)
    assert a.true_counts == b.true_counts and a.true_counts is not None, what


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [("t6", "shrink"), ("t40", "jitter"), ("t300", "slide"), ("t1100", "shrink"), ("cubes25", "slide"),
                                       ("mixed", "with_spheres")])
def test_the_remaining_entry_points_after_a_deform(gpu, name, case):
    """path radiance with ids, sparse samples, the block band, progressive sums on top of sums taken BEFORE the update, a refinement
    round, the pixel features -- product and lab; on the lab library also one row of path transcripts"""
    objs, idx, new, want, mode = mc.case_of(name, case)
    now = mc.apply(objs, idx, new)
    for lab in (False, True):
        hnd = _scene(gpu, objs).upload(0, lab=lab)
        sums = _sums_before(hnd)
        held = [_dev_bytes(t) for t in sums]
        assert hnd.update_objects(idx, new, mode=mode) == want
        fresh = _scene(gpu, now).upload(0, lab=lab)
        _same_entry_points(name, hnd, fresh, now, sums, "%s/%s%s" % (name, case, " (lab)" if lab else ""))
        assert [_dev_bytes(t) for t in sums] == held
        hnd.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["t300", "cubes25"])
def test_ten_deform_steps_in_a_row(gpu, name):
    """an animation: slide and shrink alternate, each step drawn from the scene the step before left.  After each step the arrays
    are the host reference's: a refit depends on the topology, the kept centre and the geometry it ends with, so the host is given
    the base scene, the steps before as ONE update (the last entry of an index wins) and this step as a second one.  The last
    frame, the queries and the pick buffer are Fresh's."""
    base = mc.cached_scene(name)
    lab = _scene(gpu, base).upload(0, lab=True)
    hnd = _scene(gpu, base).upload(0)
    now, all_idx, all_new = base, [], []
    for k in range(10):
        idx, new, want, mode = mc.update(now, "shrink" if k % 2 else "slide", seed=100 + k, name=name)
        m = mc.kept(base, idx, new)                 # (the class is judged against the kept centre: the base scene's)
        idx, new = idx[m], new[m]
        assert lab.update_objects(idx, new, mode=mode) == want == "refit", k
        assert hnd.update_objects(idx, new, mode=mode) == "refit", k
        now = mc.apply(now, idx, new)
        all_idx.append(idx)
        all_new.append(new)
        # the host reference of the sequence so far: the steps before as ONE update (the last entry of an index wins, and a refit
        # depends on the topology and the geometry it ends with), then this step
        prev_idx, prev_new = np.concatenate(all_idx[:-1] + [idx[:0]]), np.concatenate(all_new[:-1] + [new[:0]])
        how, _, host, _ = gpu.debug_host_refit_mesh(_scene(gpu, base), np.concatenate([prev_idx, idx]), np.concatenate([prev_new, new]),
                                                    mode=mode, split=len(prev_idx))
        assert how == "refit"
        assert lab.debug_resident_mesh_digests() == host, (name, k)
    fresh = _scene(gpu, now).upload(0)
    _same_everything(gpu, hnd, fresh, now, "%s step 10" % name)
    _same_everything(gpu, lab, fresh, now, "%s step 10 (lab)" % name, frames_only=True)
    for h in (lab, hnd, fresh):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.SCENES)
def test_fallbacks_rebuild_and_errors_change_nothing(gpu, name):
    for case in mc.fallbacks_for(name):
        objs, idx, new, want, mode = mc.case_of(name, case)
        hnd = _scene(gpu, objs).upload(0)
        assert hnd.update_objects(idx, new, mode=mode) == want == "rebuilt", case
        now = mc.apply(objs, idx, new)
        fresh = _scene(gpu, now).upload(0)
        _same_everything(gpu, hnd, fresh, now, "%s/%s" % (name, case), frames_only=True, stages=False)
        if case == "flip":                          # a deform after the rebuild works on the new tree (the tables follow every pack)
            i2, n2, w2, m2 = mc.update(now, "shrink", seed=9, name=name)
            assert hnd.update_objects(i2, n2, mode=m2) == w2
            fresh.close()
            fresh = _scene(gpu, mc.apply(now, i2, n2)).upload(0)
            _same_everything(gpu, hnd, fresh, mc.apply(now, i2, n2), "%s/deform after rebuild" % name, frames_only=True)
        hnd.close()
        fresh.close()
    # errors are found before the first device write
    objs, idx, new, _, mode = mc.case_of(name, "shrink")
    hnd = _scene(gpu, objs).upload(0)
    fresh = _scene(gpu, objs).upload(0)
    bad_idx = idx.copy()
    bad_idx[-1] = len(objs)
    bad_kind = new.copy()
    bad_kind["kind"][-1] = 9
    bad_res = new.copy()
    bad_res["reserved"][-1] = 2
    for i, o, m, status in ((bad_idx, new, mode, gpu.abi.RTX_ERR_INVALID_ARGUMENT), (idx, bad_kind, mode, gpu.abi.RTX_ERR_UNSUPPORTED),
                            (idx, bad_res, mode, gpu.abi.RTX_ERR_UNSUPPORTED), (idx, new, 7, gpu.abi.RTX_ERR_INVALID_ARGUMENT)):
        with pytest.raises(gpu.RtxError) as e:
            hnd.update_objects(i, o, mode=m)
        assert e.value.status == status
    assert hnd.update_objects(idx[:0], new[:0], mode=mode) == "nothing"
    _same_everything(gpu, hnd, fresh, objs, "%s after errors" % name, frames_only=True)
    hnd.close()
    fresh.close()


@pytest.mark.gpu
def test_a_deform_waits_for_the_frame_enqueued_before_it(gpu):
    """an asynchronous render on one stream, the update on another: the earlier frame is the pre-update scene's, the next one the
    updated scene's ("Streams": the update's writes are ordered behind what the handle enqueued before)"""
    import torch
    objs, idx, new, want, mode = mc.case_of("t1100", "shrink")
    cfg = dict(rays_per_pixel=16)
    before = _scene(gpu, objs, **cfg).upload(0)
    after = _scene(gpu, mc.apply(objs, idx, new), **cfg).upload(0)
    want_before, want_after = _frame(before).cpu().numpy(), _frame(after).cpu().numpy()
    assert want_before.tobytes() != want_after.tobytes()
    hnd = _scene(gpu, objs, **cfg).upload(0)
    s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    early = _frame(hnd, stream=s1.cuda_stream, want_stats=False)
    assert hnd.update_objects(idx, new, mode=mode, stream=s2.cuda_stream) == want == "refit"
    late = _frame(hnd, stream=s2.cuda_stream, want_stats=False)
    torch.cuda.synchronize(0)
    assert early.cpu().numpy().tobytes() == want_before.tobytes()
    assert late.cpu().numpy().tobytes() == want_after.tobytes()
    for h in (before, after, hnd):
        h.close()
