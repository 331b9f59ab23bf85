"""Refinement to a noise threshold, decided on the device (rtx_render_blocks_refine): the pixels of a band whose summed variance of the
mean exceeds (threshold * (mean + floor))^2 get further samples of the render, folded into the caller's sums, round after round.

The yardstick is refine_cases.Simulation -- the rule and the folds in plain numpy over per-sample colours that come from the exhaustive
kernel's path transcripts (the oracle's on the CPU) -- and, for the render's bits, rtx_render_rows and rtx_scene_trace_samples.  Every
comparison is exact (helpers.same / bytes)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import DEFAULT_CAM, hip_scene, same
from progressive_cases import band_rows, case
from refine_cases import CENSUS, RULES, Simulation, census, colours, selected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_hip.h")
RUST_SHIM = os.path.join(ROOT, "rust", "src", "raytracing", "hip.rs")
FN = "rtx_render_blocks_refine"
CASE_NAMES = ("spheres", "joint")
GUARD = 96                                           # elements of NaN / 0xFFFFFFFF behind each buffer: must come back untouched
NAN = float("nan")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


# ----------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_census_of_both_cases(oracle, name):
    """from the oracle's samples alone: what each rounds = 1 pass selects and traces, and the final sample counts -- the cases are known
    to be discriminating before a GPU runs them: round 1 selects between 5 % and 95 % of the pixels, the final counts take at least
    three values, and a partial last round stops some pixel at the cap"""
    rule = RULES[name]
    colour = colours(name, oracle=oracle)
    passes, finals = census(colour, rule)
    print(name, rule, "passes (pixels, samples):", passes, "final counts:", finals)
    pixels = colour.shape[0] * colour.shape[1]
    assert 0.05 * pixels <= passes[0][0] <= 0.95 * pixels
    assert len(finals) >= 3
    assert any(0 < s < p * rule["n_more"] for p, s in passes), "no pass was cut by the cap"
    assert sum(finals.values()) == pixels and sum(s for _, s in passes) == sum((n - rule["sample_begin"]) * c for n, c in finals.items())
    assert (passes, finals) == CENSUS[name]


def test_header_abi_libraries_and_rust_shim_carry_the_entry_point(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % FN, hdr)
    assert m, FN
    sym = [s for s in rtx.abi.SYMBOLS if s[0] == FN]
    assert len(sym) == 1 and len(sym[0][2]) == len(m.group(1).split(",")) == 18
    shim = re.search(r"\bpub fn %s\s*\(([^)]*)\)" % FN, open(RUST_SHIM).read())
    assert shim and len(shim.group(1).split(",")) == 18
    for lab in (False, True):
        assert getattr(rtx.load_library(lab), FN) is not None, lab
    lib = rtx.load_library()
    assert lib.rtx_render_blocks_refine(None, 8, 8, 8, 0, 1, 0, 1, 2, 1, 0.5, 0.01, None, None, None, None, None, None) == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    assert b"null scene" in lib.rtx_last_error()


def test_a_caller_of_resident_refine_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "rtx.hpp"\n'
                   "std::uint64_t go(rtx::Scene::Resident &r, double *sum, double *sq, std::uint32_t *extra) {\n"
                   "    RtxStats st;\n"
                   "    std::array<std::uint64_t, 3> a = r.refine(64, 40, 8, 0, 1, 8, 8, 64, 1, 0.05, 0.01, sum, sq, extra);\n"
                   "    std::array<std::uint64_t, 3> b = r.refine(64, 40, 8, 1, 2, 8, 8, 64, 4, 0.05, 0.01, sum, sq, extra, nullptr, &st);\n"
                   "    return a[2] + b[1] + st.primary_rays;\n"
                   "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_product_library_gained_no_kernel_and_the_sphere_query_kernel_no_spill(rtx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    rows = kernel_instances.kernels(rtx.abi.LIB_PATH)
    names = sorted(r["name"] for r in rows)
    assert len(names) <= 25, names
    sph = [r for r in rows if r["name"] == "query_closest_kernel<false>"]
    assert len(sph) == 1, sph
    print("query_closest_kernel<false>:", sph[0])
    assert sph[0]["vgpr_spill"] == 0 and sph[0]["vgpr"] <= 128, sph[0]


def test_the_rule_in_numpy_on_hand_made_pixels():
    """the yardstick's own rule on pixels worked out by hand: n < 2 always, the cap never, a NaN never (n >= 2), zero variance never,
    and e > b * b strictly"""
    total = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [NAN, 1.0, 1.0], [3.0, 0.0, 0.0], [3.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    sq = np.array([[9.0, 9.0, 9.0], [2.0, 2.0, 2.0], [9.0, 9.0, 9.0], [9.0, 0.0, 0.0], [9.0, 0.0, 0.0], [9.0, 0.0, 0.0]])
    n = np.array([1, 2, 2, 3, 3, 12])
    # pixel 3: v = 9 - 9 / 3 = 6, e = 6 / 2 / 3 = 1, m = 1; threshold 1, floor 0: b * b = 1, e > 1 is false; pixel 1: v = 0
    assert selected(total, sq, n, 12, 1.0, 0.0).tolist() == [True, False, False, False, False, False]
    assert selected(total, sq, n, 12, 0.5, 0.0).tolist() == [True, False, False, True, True, False]
    assert selected(total, sq, n, 3, 0.5, 0.0).tolist() == [True, False, False, False, False, False]


# ----------------------------------------------------------------------------------------------------------------- GPU
def _handle(gpu, name, kernel=None, spp=None):
    objs, w, h, cam, cfg = case(name)
    if spp is not None:
        cfg = dict(cfg, rays_per_pixel=spp)
    return hip_scene(gpu, objs, cam=cam, kernel=kernel, **cfg).upload(0)


class Band:
    """the three device buffers of a band with their guards, and the calls on them"""

    def __init__(self, gpu, hnd, w, h, part=(8, 0, 1)):
        import torch
        self.torch, self.hnd, self.w, self.h, self.part = torch, hnd, w, h, part
        self.rows = band_rows(h, *part)
        self.n = len(self.rows) * w
        self.total = torch.full((self.n * 3 + GUARD,), NAN, dtype=torch.float64, device="cuda:0")
        self.sq = torch.full((self.n * 3 + GUARD,), NAN, dtype=torch.float64, device="cuda:0")
        self.extra = torch.full((self.n + GUARD,), -1, dtype=torch.int32, device="cuda:0")
        self.total[:self.n * 3] = 0.0
        self.sq[:self.n * 3] = 0.0
        self.extra[:self.n] = 0
        torch.cuda.synchronize()

    def base(self, sample_begin):
        if sample_begin:
            self.hnd.render_accumulate(self.w, self.h, 0, sample_begin, self.total.data_ptr(), self.sq.data_ptr(), *self.part)
        return self

    def set(self, total, sq, extra):
        t = self.torch
        self.total[:self.n * 3] = t.from_numpy(np.ascontiguousarray(total, dtype=np.float64).ravel()).to("cuda:0")
        self.sq[:self.n * 3] = t.from_numpy(np.ascontiguousarray(sq, dtype=np.float64).ravel()).to("cuda:0")
        self.extra[:self.n] = t.from_numpy(np.ascontiguousarray(extra, dtype=np.uint32).view(np.int32).ravel()).to("cuda:0")
        t.cuda.synchronize()
        return self

    def refine(self, rule, rounds=1, **kw):
        return self.hnd.render_refine(self.w, self.h, rule["sample_begin"], rule["n_more"], rule["max_samples"], rule["threshold"], rule["floor"],
                                      self.total.data_ptr(), self.sq.data_ptr(), self.extra.data_ptr(), rounds, *self.part, **kw)

    def host(self):
        """(sum, sum_sq [rows][w][3], extra [rows][w]); the guards must be as they were"""
        self.torch.cuda.synchronize()
        total, sq, extra = self.total.cpu().numpy(), self.sq.cpu().numpy(), self.extra.cpu().numpy().view(np.uint32)
        assert np.isnan(total[self.n * 3:]).all() and np.isnan(sq[self.n * 3:]).all() and (extra[self.n:] == 0xFFFFFFFF).all(), "a guard was written"
        shape = (len(self.rows), self.w)
        return total[:self.n * 3].reshape(shape + (3,)).copy(), sq[:self.n * 3].reshape(shape + (3,)).copy(), extra[:self.n].reshape(shape).copy()

    def equals(self, sim):
        total, sq, extra = self.host()
        return same(total, sim.total) and same(sq, sim.sq) and np.array_equal(extra, sim.extra)


def _converged(gpu, name, kernel=None, rounds=1, part=(8, 0, 1)):
    """base + calls until result[2] == 0, each held to the simulation -> (handle, band, simulation, calls)"""
    objs, w, h, cam, cfg = case(name)
    rule = RULES[name]
    colour = colours(name, gpu=gpu)[band_rows(h, *part)]
    hnd = _handle(gpu, name, kernel)
    band = Band(gpu, hnd, w, h, part).base(rule["sample_begin"])
    sim = Simulation(colour, **rule)
    assert band.equals(sim), (name, "the base")
    calls = 0
    while True:
        counts, st = band.refine(rule, rounds)
        want = sim.call(rounds)
        calls += 1
        print(name, kernel, "call", calls, "rounds", rounds, "counts", counts, "want", want)
        assert counts == want, (name, kernel, calls)
        assert band.equals(sim), (name, kernel, calls)
        assert st.primary_rays == want[1] and st.trace_launches == 1 and st.segments >= want[1]
        assert st.kernel == (gpu.RTX_KERNEL_EXACT if kernel == gpu.RTX_KERNEL_EXACT else gpu.RTX_KERNEL_BVH)
        if counts[2] == 0:
            break
        assert calls < 16
    return hnd, band, sim, calls


@pytest.mark.gpu
@pytest.mark.parametrize("exact", (False, True))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_base_plus_repeated_calls_follow_the_simulation(gpu, name, exact):
    """accumulate [0, sample_begin), then rounds = 1 calls until result[2] == 0: after every call the sums, the squares' sums, the counts
    and the three results are the simulation's; the passes are the census the CPU test pins (the GPU's transcripts give the oracle's
    samples); a further call touches nothing"""
    hnd, band, sim, calls = _converged(gpu, name, gpu.RTX_KERNEL_EXACT if exact else None)
    passes, finals = CENSUS[name]
    assert calls == len(passes) - 1
    values, counts = np.unique(sim.count(), return_counts=True)
    assert {int(v): int(c) for v, c in zip(values, counts)} == finals
    before = band.host()
    counts, st = band.refine(RULES[name])
    assert counts == (0, 0, 0) and st.primary_rays == 0
    after = band.host()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    hnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_one_call_with_four_rounds_equals_the_repeated_calls(gpu, name):
    hnd, band, sim, calls = _converged(gpu, name)
    assert calls >= 3
    want = band.host()
    hnd.close()
    hnd, many, sim4, calls4 = _converged(gpu, name, rounds=4)
    assert calls4 == 1
    got = many.host()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), name
    # and without result and stats the call only enqueues: the same buffers after a synchronisation
    objs, w, h, cam, cfg = case(name)
    quiet = Band(gpu, hnd, w, h).base(RULES[name]["sample_begin"])
    assert quiet.refine(RULES[name], 4, want_stats=False, want_result=False) == (None, None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(quiet.host(), want)), name
    hnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_parts_equal_the_frames_rows(gpu, name):
    hnd, band, sim, _ = _converged(gpu, name, rounds=4)
    full = band.host()
    hnd.close()
    objs, w, h, cam, cfg = case(name)
    for part in ((8, 0, 2), (8, 1, 2)):
        rows = band_rows(h, *part)
        assert 0 < len(rows) < h
        hnd, piece, _, _ = _converged(gpu, name, rounds=4, part=part)
        got = piece.host()
        hnd.close()
        assert all(a.tobytes() == b[rows].tobytes() for a, b in zip(got, full)), (name, part)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_refined_pixel_holds_the_renders_bits(gpu, name):
    """for every final count n: d_sum / n on the pixels with that count == rtx_render_rows at rays_per_pixel = n there; and d_sum, d_sum_sq
    == the folds of rtx_scene_trace_samples' colours of (p, 0 .. n - 1)"""
    import torch
    objs, w, h, cam, cfg = case(name)
    hnd, band, sim, _ = _converged(gpu, name, rounds=4)
    total, sq, extra = band.host()
    n = RULES[name]["sample_begin"] + extra.astype(np.int64)
    assert len(np.unique(n)) >= 3
    for count in np.unique(n):
        hnd.set_config(gpu.Config(**dict(cfg, rays_per_pixel=int(count))))
        img = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        hnd.render_rows(w, h, 0, 1, h, img.data_ptr())
        img = img.cpu().numpy()
        at = n == count
        assert same((total / float(count))[at], img[at]), (name, int(count))
    top = int(n.max())
    ids = np.stack([np.tile(np.arange(w * h, dtype=np.uint64), top), np.repeat(np.arange(top, dtype=np.uint64), w * h)], axis=1)
    d_ids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    d_rgb = torch.empty(len(ids) * 3, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    hnd.trace_samples(w, h, d_ids.data_ptr(), len(ids), d_rgb.data_ptr())
    rgb = d_rgb.cpu().numpy().reshape(top, h, w, 3)
    fold, fold_sq = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for s in range(top):
        on = (n > s)[..., None]
        fold = np.where(on, fold + rgb[s], fold)
        fold_sq = np.where(on, fold_sq + rgb[s] * rgb[s], fold_sq)
    assert same(total, fold) and same(sq, fold_sq), name
    hnd.close()


@pytest.mark.gpu
def test_edges_no_ops_and_refusals(gpu):
    import torch
    name = "spheres"
    objs, w, h, cam, cfg = case(name)
    rule = RULES[name]
    colour = colours(name, gpu=gpu)
    hnd = _handle(gpu, name)
    # max_samples <= sample_begin: nothing is touched, NaN-filled buffers stay NaN-filled
    band = Band(gpu, hnd, w, h).set(np.full((h, w, 3), NAN), np.full((h, w, 3), NAN), np.full((h, w), 7))
    for cap in (0, rule["sample_begin"]):
        counts, st = band.refine(dict(rule, max_samples=cap))
        assert counts == (0, 0, 0) and st.primary_rays == 0 and st.trace_launches == 0
    total, sq, extra = band.host()
    assert np.isnan(total).all() and np.isnan(sq).all() and (extra == 7).all()
    # threshold = 0 with floor = 0: every pixel with e > 0 is selected, no other
    zero = dict(rule, threshold=0.0, floor=0.0)
    band = Band(gpu, hnd, w, h).base(rule["sample_begin"])
    sim = Simulation(colour, **zero)
    sel = sim.select()
    with np.errstate(all="ignore"):
        dn = float(rule["sample_begin"])
        v = sim.sq - sim.total * sim.total / dn
        e = ((v[..., 0] + v[..., 1]) + v[..., 2]) / (dn - 1.0) / dn
    assert np.array_equal(sel, e > 0) and 0 < sel.sum() < sel.size
    counts, _ = band.refine(zero)
    assert counts == sim.call(1) and counts[0] == int(sel.sum()) and band.equals(sim)
    assert np.array_equal(band.host()[2] != 0, sel)
    # pixels preset to NaN sums: selected while n < 2, never from n = 2 on
    for begin, extra0, expect in ((0, 0, True), (1, 0, True), (0, 1, True), (2, 0, False), (1, 1, False), (0, 5, False)):
        nan_rule = dict(rule, sample_begin=begin)
        total0, sq0, ex0 = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.uint32)
        mark = np.zeros((h, w), dtype=bool)
        mark[::3, ::5] = True
        total0[mark], sq0[mark], ex0[mark] = NAN, NAN, extra0
        ex0[~mark] = rule["max_samples"]                                          # the others are at the cap: only the NaN pixels can move
        band = Band(gpu, hnd, w, h).set(total0, sq0, ex0)
        sim = Simulation(colour, **dict(nan_rule, total=total0, sq=sq0, extra=ex0))
        counts, _ = band.refine(nan_rule)
        want = sim.call(1)
        assert counts == want and band.equals(sim), (begin, extra0)
        assert (counts[0] == int(mark.sum())) == expect and (counts[0] == 0) == (not expect), (begin, extra0, counts)
    # refusals touch nothing: null buffers, overlaps, n_more / rounds == 0, a NaN or negative threshold or floor, sample_begin >= 2^32
    band = Band(gpu, hnd, w, h).set(np.full((h, w, 3), NAN), np.full((h, w, 3), NAN), np.full((h, w), 7))
    t, q, x = band.total.data_ptr(), band.sq.data_ptr(), band.extra.data_ptr()
    good = dict(sample_begin=0, n_more=1, max_samples=4, threshold=0.5, floor=0.01, rounds=1)
    bad = [dict(good, n_more=0), dict(good, rounds=0), dict(good, threshold=NAN), dict(good, threshold=-0.5), dict(good, floor=NAN),
           dict(good, floor=-1e-300), dict(good, sample_begin=1 << 32), dict(good, block_rows=0), dict(good, part=2, n_parts=2)]
    ptrs = [(None, q, x), (t, None, x), (t, q, None), (t, t + 8, x), (t, q, t + 16), (t, q, q)]
    for kw, (a, b, c) in [(k, (t, q, x)) for k in bad] + [(good, p) for p in ptrs]:
        kw = dict(kw)
        args = [kw.pop(k) for k in ("sample_begin", "n_more", "max_samples", "threshold", "floor")]
        with pytest.raises(gpu.RtxError) as err:
            hnd.render_refine(w, h, *args, a, b, c, **kw)
        assert err.value.status == gpu.abi.RTX_ERR_INVALID_ARGUMENT, (kw, a, b, c)
    total, sq, extra = band.host()
    assert np.isnan(total).all() and np.isnan(sq).all() and (extra == 7).all()
    # a scene without objects: nothing is touched, nothing is launched, the result is zeros
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=4), gpu.Camera(*DEFAULT_CAM), np.zeros(0, dtype=gpu.OBJECT_DTYPE)).upload(0)
    band = Band(gpu, empty, w, h)
    counts, st = band.refine(dict(rule, sample_begin=0))
    assert counts == (0, 0, 0) and st.primary_rays == 0 and st.trace_launches == 0
    total, sq, extra = band.host()
    assert not total.any() and not sq.any() and not extra.any()
    empty.close()
    # the handle renders correctly afterwards
    hnd.set_config(gpu.Config(**dict(cfg, rays_per_pixel=rule["sample_begin"])))
    img = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    hnd.render_rows(w, h, 0, 1, h, img.data_ptr())
    fresh = Simulation(colour, **rule)
    assert same(img.cpu().numpy(), fresh.total / float(rule["sample_begin"]))
    hnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_progressive_converge_equals_the_raw_calls(gpu, name):
    import torch
    objs, w, h, cam, cfg = case(name)
    rule = RULES[name]
    hnd, band, sim, calls = _converged(gpu, name)
    want_total, want_sq, want_extra = band.host()
    prog = hnd.progressive(w, h)
    prog.add(rule["sample_begin"])
    got = []
    while True:
        got.append(prog.converge(rule["threshold"], rule["floor"], step=rule["n_more"], max_samples=rule["max_samples"]))
        assert prog._uniform == rule["sample_begin"] and int(prog.count.min()) >= prog._uniform and int(prog.count.max()) <= rule["max_samples"]
        if got[-1][2] == 0:
            break
        assert len(got) < 16
    passes, finals = CENSUS[name]
    assert [g[:2] for g in got] == passes[:-1] and len(got) == calls
    assert prog.sum.cpu().numpy().tobytes() == want_total.tobytes() and prog.sum_sq.cpu().numpy().tobytes() == want_sq.tobytes()
    count = prog.count.cpu().numpy()
    assert np.array_equal(count, rule["sample_begin"] + want_extra.astype(np.int64))
    assert prog.traced == w * h * rule["sample_begin"] + sum(s for _, s in passes)
    mean = prog.mean()
    for n in np.unique(count):
        hnd.set_config(gpu.Config(**dict(cfg, rays_per_pixel=int(n))))
        img = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        hnd.render_rows(w, h, 0, 1, h, img.data_ptr())
        at = count == n
        assert same(mean[at], img.cpu().numpy()[at]), (name, int(n))
    # one converge() with rounds = 4 on a fresh accumulator: the same state; refine() and variance() still work on it
    again = hnd.progressive(w, h)
    again.add(rule["sample_begin"])
    assert again.converge(rule["threshold"], rule["floor"], step=rule["n_more"], max_samples=rule["max_samples"], rounds=4)[2] == 0
    assert again.sum.cpu().numpy().tobytes() == want_total.tobytes() and np.array_equal(again.count.cpu().numpy(), count)
    again.refine([0, 5], 1)
    assert int(again.count.view(-1)[5]) == int(count.reshape(-1)[5]) + 1 and again.variance().shape == (h, w, 3)
    hnd.close()
