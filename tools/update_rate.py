#!/usr/bin/env python3
"""What moving objects costs on a resident scene: wall time of SceneHandle.update_objects (rtx_scene_update_objects) against the
only way there was before it, rtx_scene_free + rtx_scene_upload of the modified list, and what a refitted tree costs per frame.

  update   per scene (C2: scenes.random_spheres(10000, 1); M1: random_spheres(1000000, 1)) and share of the spheres (one sphere,
           1 %, 100 %), the wall time of one call, host work and the final synchronisation included:
             refit     every named sphere moved inside the box of the centres (RTX_UPDATED_REFIT)
             records   the same spheres, materials only (RTX_UPDATED_RECORDS)
             rebuild   the refit leg's list under RTX_UPDATE_REBUILD (host build + upload of every array)
             reupload  close() + Scene.upload() of the modified list: the one leg a library without the entry point can run
  frames   C2 at 1920x1080 and --spp samples, every sphere displaced by 1, 5 and 20 units in a random direction (centres clipped to
           the box): the frame's device time (RtxStats trace_ms + resolve_ms) after a refit and after a fresh upload of the same
           geometry -- the price of keeping the old topology

  q3loss   C2 at 1920x1080: the 8 spheres nearest to the first go to one point with radius 1e-9 -- the refit finds a 64-byte node it
           cannot encode, the update falls back to a rebuild, and that rebuild has no 64-byte form for ANY node:
           the frame's device time on it against the scene as uploaded, alternating; then after an ordinary move (a refit, still
           without the form) and after RTX_UPDATE_REBUILD of the first list (the form is back) -- what a few co-located tiny
           spheres cost every later frame

  mesh     triangles that move under RTX_UPDATE_DEFORM (include/rtx_hip.h, "Triangles"): C3 (scenes.random_triangles(100000)) and T1M
           (random_triangles(1000000)); every named triangle is translated as a whole and clipped into the vertices' box, and only
           triangles that keep their class are named (a translation keeps the elimination's rows and the projection; n.v0 is checked):
             deform    one triangle, 1 %, all of them under RTX_UPDATE_DEFORM (RTX_UPDATED_REFIT)
             auto      the same entries under RTX_UPDATE_AUTO: the rebuild every triangle move was before the mode existed
             reupload  close() + Scene.upload() of the modified list
           and C3 at 1920x1080, --spp samples, every triangle translated by 0.1, 0.5 and 2 triangle sizes (the median edge): the
           frame's device time after the refit and after a fresh upload of the same geometry, alternating

  visibility   hiding and showing objects in place (SceneHandle.set_visible, rtx_scene_set_visible) on C2, C3, M1 and T1M: one object, 1 % and
           50 % of them, the wall time of one call:
             hide / show   the named objects hidden (shown again outside the clock), and the reverse
             reupload      close() + Scene.upload() of the list WITHOUT them: the shorter list, every later index shifted
             nan           update_objects with all-NaN geometry for them: "never hit" without the entry point (a rebuild; a NaN sphere
                           costs every sphere its sub-tree)
           and C2 / C3 at 1920x1080, --spp samples: the frame's device time after hiding 1 % and 50 %, after a fresh upload of the
           shortened list (what the kept topology costs), and after the NaN update (C2 at 1 % only: what losing the tree costs)

    tools/update_rate.py [--scenes C2,M1] [--legs update,frames,q3loss,mesh,visibility] [--reps 3] [--spp 4]

The package is the one of the tree the tool lies in; in a checkout of the parent commit (copy the tool there) only the reupload leg runs
(of the mesh leg: its auto and reupload forms).
One JSON line per measurement: the best of --reps timed runs after one warm-up, with the slowest run and the spread between them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCENES = {"C2": 10000, "M1": 1000000}


def moved(objs, idx, rng, step=None):
    """objs[idx] with new centres inside the box of all centres: uniform, or displaced by `step` in a random direction and clipped"""
    g = objs["geom"]
    rmax = float(np.abs(g[:, 3]).max())
    lo, hi = g[:, :3].min(axis=0) + rmax, g[:, :3].max(axis=0) - rmax
    new = objs[idx].copy()
    if step is None:
        new["geom"][:, :3] = lo + (hi - lo) * rng.random((len(idx), 3))
    else:
        d = rng.normal(size=(len(idx), 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        new["geom"][:, :3] = np.clip(new["geom"][:, :3] + step * d, lo, hi)
    return new


def tri_cull_side(g):
    """n.v0 < -(1 + 1e-9) per triangle (9 doubles each), with make_triangle's operations: such a triangle has no filter record"""
    v0, r, s = g[:, 0:3], g[:, 3:6] - g[:, 0:3], g[:, 6:9] - g[:, 0:3]
    n = np.stack([r[:, 1] * s[:, 2] - r[:, 2] * s[:, 1], r[:, 2] * s[:, 0] - r[:, 0] * s[:, 2], r[:, 0] * s[:, 1] - r[:, 1] * s[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        n = n / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])[:, None]
        return (n[:, 0] * v0[:, 0] + n[:, 1] * v0[:, 1] + n[:, 2] * v0[:, 2]) < -(1.0 + 1e-9)


def translated(objs, idx, rng, step):
    """objs[idx], each triangle moved as a whole by `step` in a random direction, the move cut so that it stays inside the box of all
    vertices shrunk by 1 % (no footprint can then leave the range the tree was built for) -> (the entries, mask: the class is kept)"""
    v = objs["geom"].reshape(-1, 3, 3)
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    lo, hi = lo + 0.01 * (hi - lo), hi - 0.01 * (hi - lo)
    new = objs[idx].copy()
    w = new["geom"].reshape(len(idx), 3, 3)
    d = rng.normal(size=(len(idx), 3))
    d *= step / np.linalg.norm(d, axis=1)[:, None]
    room_lo, room_hi = np.minimum(lo - w.min(axis=1), 0.0), np.maximum(hi - w.max(axis=1), 0.0)
    d = np.clip(d, room_lo, room_hi)
    new["geom"] = (w + d[:, None, :]).reshape(len(idx), 9)
    return new, tri_cull_side(new["geom"]) == tri_cull_side(objs["geom"][idx])


def mesh_legs(rtx, scenes, cam, args, emit_):
    import torch
    has_deform = hasattr(rtx.abi, "RTX_UPDATE_DEFORM")           # (a checkout of the parent commit: the auto and reupload forms alone)
    for name, n in (("C3", 100000), ("T1M", 1000000)):
        objs = scenes.random_triangles(n)
        cfg = rtx.Config(rays_per_pixel=args.spp, seed=scenes.RENDER_SEED)
        e = objs["geom"].reshape(-1, 3, 3)
        size = float(np.median(np.linalg.norm(e - np.roll(e, 1, axis=1), axis=2)))
        hnd = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
        for share, count in (("1", 1), ("1%", n // 100), ("100%", n)):
            rng = np.random.default_rng(7)
            cand = np.sort(rng.permutation(n)[:count])
            new, keep = translated(objs, cand, rng, 0.5 * size)
            idx, new = cand[keep].astype(np.uint64), new[keep]
            if len(idx) == 0:                                    # (the one triangle drawn changes its class: take the next that does not)
                new, keep = translated(objs, np.arange(n), rng, 0.5 * size)
                idx, new = np.arange(n)[keep][:1].astype(np.uint64), new[keep][:1]
            back = objs[idx.astype(np.int64)].copy()
            state = {"k": 0}

            def there_or_back():                                 # alternate, so that every timed call really moves the triangles
                state["k"] += 1
                return new if state["k"] % 2 else back

            for form, mode, want in ((("deform", "deform", "refit"),) if has_deform else ()) + (("auto", "auto", "rebuilt"),):
                how = []
                best, worst = timed(lambda a, _m=mode: how.append(hnd.update_objects(idx, a, mode=_m)), args.reps, there_or_back)
                emit_(scene=name, leg="mesh", form=form, triangles=n, updated=len(idx), share=share, how=sorted(set(how)), expected=want,
                      ms=round(best, 4), worst_ms=round(worst, 4), spread=round(worst / best - 1.0, 3), reps=args.reps)
            box = {"hnd": hnd}

            def reupload(a):
                mod = objs.copy()
                mod[idx.astype(np.int64)] = a
                box["hnd"].close()
                box["hnd"] = rtx.Scene.from_packed(cfg, cam, mod).upload(0)

            best, worst = timed(reupload, args.reps, there_or_back)
            hnd = box["hnd"]
            hnd.close()
            hnd = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            emit_(scene=name, leg="mesh", form="reupload", triangles=n, updated=len(idx), share=share, ms=round(best, 4), worst_ms=round(worst, 4),
                  spread=round(worst / best - 1.0, 3), reps=args.reps)
        hnd.close()
        if name != "C3" or not has_deform:
            continue
        w, h = 1920, 1080
        buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")

        def frame_ms(handle):
            out = []
            for k in range(args.reps + 1):
                st = handle.render_rows(w, h, 0, 1, h, buf.data_ptr())
                out.append(st.trace_ms + st.resolve_ms)
            return min(out[1:]), max(out[1:])

        base = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
        b, wst = frame_ms(base)
        emit_(scene=name, leg="mesh-frames", form="as uploaded", step=0, spp=args.spp, ms=round(b, 4), worst_ms=round(wst, 4), spread=round(wst / b - 1.0, 3))
        base.close()
        for sizes in (0.1, 0.5, 2.0):
            new, keep = translated(objs, np.arange(n), np.random.default_rng(11), sizes * size)
            idx, new = np.arange(n)[keep].astype(np.uint64), new[keep]
            mod = objs.copy()
            mod[idx.astype(np.int64)] = new
            refit = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            how = refit.update_objects(idx, new, mode="deform")
            fresh = rtx.Scene.from_packed(cfg, cam, mod).upload(0)
            for run in (1, 2):                                   # alternating
                for form, handle in (("after " + how, refit), ("fresh upload", fresh)):
                    b, wst = frame_ms(handle)
                    emit_(scene=name, leg="mesh-frames", form=form, run=run, step_in_triangle_sizes=sizes, updated=len(idx), spp=args.spp,
                          ms=round(b, 4), worst_ms=round(wst, 4), spread=round(wst / b - 1.0, 3))
            refit.render_rows(w, h, 0, 1, h, buf.data_ptr())
            img = buf.cpu().numpy().copy()
            fresh.render_rows(w, h, 0, 1, h, buf.data_ptr())
            emit_(scene=name, leg="mesh-frames", form="same bits", step_in_triangle_sizes=sizes, equal=bool(np.array_equal(img, buf.cpu().numpy())))
            refit.close()
            fresh.close()


def visibility_legs(rtx, scenes, cam, args, emit_):
    import torch
    has_visible = hasattr(rtx.SceneHandle, "set_visible")           # (a checkout of the parent commit: the reupload and nan forms alone)
    w, h = 1920, 1080
    for name, make, n in (("C2", lambda: scenes.random_spheres(10000, 1), 10000), ("C3", lambda: scenes.random_triangles(100000), 100000),
                          ("M1", lambda: scenes.random_spheres(1000000, 1), 1000000), ("T1M", lambda: scenes.random_triangles(1000000), 1000000)):
        if name not in args.vis_scenes.split(","):
            continue
        objs = make()
        cfg = rtx.Config(rays_per_pixel=args.spp, seed=scenes.RENDER_SEED)
        for share, count in (("1", 1), ("1%", n // 100), ("50%", n // 2)):
            idx = np.sort(np.random.default_rng(7).permutation(n)[:count]).astype(np.uint64)
            keep = np.ones(n, dtype=bool)
            keep[idx.astype(np.int64)] = False
            real = objs[idx.astype(np.int64)].copy()
            nan = real.copy()
            nan["geom"] = np.nan
            hnd = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            if has_visible:
                for form, visible in (("hide", False), ("show", True)):
                    how = []
                    best, worst = timed(lambda _a, _v=visible: how.append(hnd.set_visible(idx, _v)), args.reps, lambda _v=visible: hnd.set_visible(idx, not _v))
                    emit_(scene=name, leg="visibility", form=form, objects=n, changed=count, share=share, how=sorted(set(how)), ms=round(best, 4),
                          worst_ms=round(worst, 4), spread=round(worst / best - 1.0, 3), reps=args.reps)
                hnd.set_visible(idx, True)
            how = []
            best, worst = timed(lambda _a: how.append(hnd.update_objects(idx, nan)), args.reps, lambda: hnd.update_objects(idx, real, mode="rebuild"))
            emit_(scene=name, leg="visibility", form="nan", objects=n, changed=count, share=share, how=sorted(set(how)), ms=round(best, 4),
                  worst_ms=round(worst, 4), spread=round(worst / best - 1.0, 3), reps=args.reps)
            box = {"hnd": hnd}

            def reupload(_a):
                box["hnd"].close()
                box["hnd"] = rtx.Scene.from_packed(cfg, cam, objs[keep]).upload(0)

            best, worst = timed(reupload, args.reps)
            box["hnd"].close()
            emit_(scene=name, leg="visibility", form="reupload", objects=n, changed=count, share=share, ms=round(best, 4), worst_ms=round(worst, 4),
                  spread=round(worst / best - 1.0, 3), reps=args.reps)
            if name not in ("C2", "C3") or share == "1":
                continue
            buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")

            def frame_ms(handle, reps=args.reps):
                out = []
                for k in range(reps + 1):
                    st = handle.render_rows(w, h, 0, 1, h, buf.data_ptr())
                    out.append(st.trace_ms + st.resolve_ms)
                return min(out[1:]), max(out[1:])

            handles = []
            if has_visible:
                hid = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
                handles.append(("after hide: " + hid.set_visible(idx, False), hid, args.reps))
            handles.append(("fresh upload of the shortened list", rtx.Scene.from_packed(cfg, cam, objs[keep]).upload(0), args.reps))
            if share == "1%":
                lost = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
                handles.append(("after the NaN update: " + lost.update_objects(idx, nan), lost, 1))
            for run in (1, 2):                                   # alternating
                for form, handle, reps in handles:
                    if run == 2 and reps == 1:
                        continue                                 # (the frame without a tree is slow: taken once)
                    b, wst = frame_ms(handle, reps)
                    emit_(scene=name, leg="visibility-frames", form=form, run=run, share=share, spp=args.spp, ms=round(b, 4), worst_ms=round(wst, 4),
                          spread=round(wst / b - 1.0, 3))
            if has_visible:
                handles[0][1].render_rows(w, h, 0, 1, h, buf.data_ptr())
                img = buf.cpu().numpy().copy()
                handles[1][1].render_rows(w, h, 0, 1, h, buf.data_ptr())
                emit_(scene=name, leg="visibility-frames", form="same bits as the shortened list", share=share, equal=bool(np.array_equal(img, buf.cpu().numpy())))
            for _, handle, _ in handles:
                handle.close()


def timed(fn, reps, setup=None):
    """wall ms of fn(): (best, worst) of `reps` runs after one warm-up; setup() runs before each, outside the clock"""
    import torch
    out = []
    for k in range(reps + 1):
        arg = setup() if setup else None
        torch.cuda.synchronize(0)
        t0 = time.perf_counter()
        fn(arg)
        torch.cuda.synchronize(0)
        out.append((time.perf_counter() - t0) * 1e3)
    out = out[1:]
    return min(out), max(out)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="C2,M1")
    ap.add_argument("--legs", default="update,frames")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--vis-scenes", default="C2,C3,M1,T1M", help="the scenes of the visibility leg")
    args = ap.parse_args()
    import torch

    import rust_raytracing_amd as rtx
    from rust_raytracing_amd import scenes
    cam = rtx.Camera(*scenes.CAMERA)
    has_update = hasattr(rtx.SceneHandle, "update_objects")          # (a checkout of the parent commit: the reupload leg alone)
    legs = args.legs.split(",")
    if "mesh" in legs:
        mesh_legs(rtx, scenes, cam, args, emit)
        legs = [k for k in legs if k != "mesh"]
        if not legs:
            return
    if "visibility" in legs:
        visibility_legs(rtx, scenes, cam, args, emit)
        legs = [k for k in legs if k != "visibility"]
        if not legs:
            return
    for name in args.scenes.split(","):
        objs = scenes.random_spheres(SCENES[name], 1)
        cfg = rtx.Config(rays_per_pixel=args.spp, seed=scenes.RENDER_SEED)
        n = len(objs)
        if "update" in legs:
            hnd = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            current = objs.copy()                                # what the handle holds
            for share, count in (("1", 1), ("1%", max(1, n // 100)), ("100%", n)):
                rng = np.random.default_rng(7)
                idx = np.sort(rng.permutation(n)[:count]).astype(np.uint64)

                def fresh_move(_rng=rng, _idx=idx):
                    return moved(objs, _idx, _rng)

                def material(_rng=rng, _idx=idx):
                    new = current[_idx.astype(np.int64)].copy()
                    new["base_color"] = _rng.uniform(0.1, 0.9, (len(_idx), 3))
                    return new

                if has_update:
                    for leg, setup, mode, want in (("refit", fresh_move, "auto", "refit"), ("records", material, "auto", "records"),
                                                   ("rebuild", fresh_move, "rebuild", "rebuilt")):
                        how = []

                        def call(new, _mode=mode):
                            how.append(hnd.update_objects(idx, new, mode=_mode))
                            current[idx.astype(np.int64)] = new

                        best, worst = timed(call, args.reps, setup)
                        assert set(how) == {want}, (leg, how)
                        emit(scene=name, leg="update", form=leg, spheres=n, updated=count, share=share, ms=round(best, 4), worst_ms=round(worst, 4),
                             spread=round(worst / best - 1.0, 3), reps=args.reps)
                state = {"hnd": hnd}

                def reupload(new, _idx=idx):
                    mod = objs.copy()
                    mod[_idx.astype(np.int64)] = new
                    state["hnd"].close()
                    state["hnd"] = rtx.Scene.from_packed(cfg, cam, mod).upload(0)

                best, worst = timed(reupload, args.reps, fresh_move)
                hnd = state["hnd"]
                emit(scene=name, leg="update", form="reupload", spheres=n, updated=count, share=share, ms=round(best, 4), worst_ms=round(worst, 4),
                     spread=round(worst / best - 1.0, 3), reps=args.reps)
            hnd.close()
        if "frames" in legs and name == "C2" and has_update:
            w, h = 1920, 1080
            buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")

            def frame_ms(handle):
                out = []
                for k in range(args.reps + 1):
                    st = handle.render_rows(w, h, 0, 1, h, buf.data_ptr())
                    out.append(st.trace_ms + st.resolve_ms)
                return min(out[1:]), max(out[1:])

            base = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            b, wst = frame_ms(base)
            emit(scene=name, leg="frames", form="as uploaded", step=0, spp=args.spp, ms=round(b, 4), worst_ms=round(wst, 4), spread=round(wst / b - 1.0, 3))
            base.close()
            for step in (1.0, 5.0, 20.0):
                idx = np.arange(n, dtype=np.uint64)
                new = moved(objs, idx, np.random.default_rng(11), step)
                refit = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
                assert refit.update_objects(idx, new) == "refit"
                fresh = rtx.Scene.from_packed(cfg, cam, new).upload(0)
                for run in (1, 2):                               # alternating
                    for form, handle in (("after refit", refit), ("fresh upload", fresh)):
                        b, wst = frame_ms(handle)
                        emit(scene=name, leg="frames", form=form, run=run, step=step, spp=args.spp, ms=round(b, 4), worst_ms=round(wst, 4),
                             spread=round(wst / b - 1.0, 3))
                refit.render_rows(w, h, 0, 1, h, buf.data_ptr())
                img_refit = buf.cpu().numpy().copy()
                fresh.render_rows(w, h, 0, 1, h, buf.data_ptr())
                emit(scene=name, leg="frames", form="same bits", step=step, equal=bool(np.array_equal(img_refit, buf.cpu().numpy())))
                refit.close()
                fresh.close()

        if "q3loss" in legs and name == "C2" and has_update:
            w, h = 1920, 1080
            buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")

            def frame_ms(handle):
                out = []
                for k in range(args.reps + 1):
                    st = handle.render_rows(w, h, 0, 1, h, buf.data_ptr())
                    out.append(st.trace_ms + st.resolve_ms)
                return min(out[1:]), max(out[1:])

            def flags_of(o):
                return rtx.debug_host_scene(rtx.Scene.from_packed(cfg, cam, o))["flags"]      # (host only; & 16: the 64-byte form exists)

            c = objs["geom"][:, :3]
            idx = np.argsort(np.linalg.norm(c - c[0], axis=1), kind="stable")[:8].astype(np.uint64)
            tiny = objs[idx.astype(np.int64)].copy()
            tiny["geom"][:, :3] = c[0]
            tiny["geom"][:, 3] = 1.0e-9
            collapsed = objs.copy()
            collapsed[idx.astype(np.int64)] = tiny
            plain = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            hnd = rtx.Scene.from_packed(cfg, cam, objs).upload(0)
            how = hnd.update_objects(idx, tiny)
            assert how == "rebuilt", how
            for run in (1, 2):                                   # alternating
                for form, handle, o in (("as uploaded", plain, objs), ("8 spheres collapsed: rebuilt by the fallback", hnd, collapsed)):
                    b, wst = frame_ms(handle)
                    emit(scene=name, leg="q3loss", form=form, run=run, spp=args.spp, flags=flags_of(o), ms=round(b, 4), worst_ms=round(wst, 4),
                         spread=round(wst / b - 1.0, 3))
            # a later ordinary move is a refit of the tree without the form; spreading the eight out again under RTX_UPDATE_REBUILD ends it
            moved_idx = np.arange(100, 200, dtype=np.uint64)
            how = hnd.update_objects(moved_idx, moved(objs, moved_idx, np.random.default_rng(3), 1.0))
            b, wst = frame_ms(hnd)
            emit(scene=name, leg="q3loss", form="then 100 spheres moved: " + how, spp=args.spp, ms=round(b, 4), worst_ms=round(wst, 4), spread=round(wst / b - 1.0, 3))
            how = hnd.update_objects(np.concatenate([idx, moved_idx]), objs[np.concatenate([idx, moved_idx]).astype(np.int64)].copy(), mode="rebuild")
            b, wst = frame_ms(hnd)
            emit(scene=name, leg="q3loss", form="then the first list again under RTX_UPDATE_REBUILD: " + how, spp=args.spp, flags=flags_of(objs),
                 ms=round(b, 4), worst_ms=round(wst, 4), spread=round(wst / b - 1.0, 3))
            plain.close()
            hnd.close()

if __name__ == "__main__":
    main()
