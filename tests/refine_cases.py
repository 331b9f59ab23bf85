"""The cases of tests/test_refine.py (rtx_render_blocks_refine) and their yardstick: simulate(), the rule and the folds of the header
comment in plain numpy, over the per-sample colours of a frame.  Those colours come from path transcripts replayed over the materials as
progressive_cases.replay does -- rtx_debug_paths of the exhaustive kernel on the GPU, oracle.trace_row under oracle.device_sincos() on the
CPU -- so the yardstick runs neither the refinement's take nor its fold.  A case's colours are computed once."""
import numpy as np

from helpers import hip_scene
from progressive_cases import case, left_fold

# the rule of each case; "spheres" runs query_closest_kernel<false>, "joint" (spheres and triangles in one tree) <true>
RULES = {
    "spheres": dict(sample_begin=4, n_more=3, max_samples=12, threshold=0.5, floor=0.01),
    "joint": dict(sample_begin=2, n_more=3, max_samples=9, threshold=0.5, floor=0.01),
}
# what the oracle's samples give under those rules (test_the_census_of_both_cases recomputes it on the CPU): per pass of rounds = 1
# (pixels selected, samples traced), then {final sample count: pixels}
CENSUS = {
    "spheres": ([(279, 837), (130, 390), (70, 140), (0, 0)], {4: 1125, 7: 149, 10: 60, 12: 70}),
    "joint": ([(260, 780), (101, 303), (56, 56), (0, 0)], {2: 1276, 5: 159, 8: 45, 9: 56}),
}
MAX_STEPS = 12                                       # max_bounces = 10: at most 11 closest_object calls per path


def _replay_row(steps, counts, em, base, out):
    """out[x][s] = the colour of path (x, s) of a row: its transcript's winners replayed over the materials (scene.rs:276-277)"""
    winners = steps["object"]
    width, spp = counts.shape
    for x in range(width):
        for s in range(spp):
            result, light = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
            for k in range(int(counts[x, s])):
                obj = int(winners[x, s, k])
                if obj < 0:
                    break
                result = [result[c] + light[c] * em[obj][c] for c in range(3)]
                light = [light[c] * base[obj][c] for c in range(3)]
            out[x, s] = result


_COLOURS = {}


def colours(name, gpu=None, oracle=None):
    """colour [h][w][max_samples][3]: every sample 0 .. max_samples - 1 of every pixel of the case's frame (a sample depends on (seed,
    pixel, sample index, scene), not on rays_per_pixel).  gpu: from the lab library's exhaustive-kernel transcripts; oracle: from the CPU
    oracle's, with the device's sin / cos"""
    key = (name, "gpu" if gpu is not None else "cpu")
    if key in _COLOURS:
        return _COLOURS[key]
    objs, w, h, cam, cfg = case(name)
    cfg = dict(cfg, rays_per_pixel=RULES[name]["max_samples"])
    em, base = objs["emission_color"].tolist(), objs["base_color"].tolist()
    colour = np.zeros((h, w, cfg["rays_per_pixel"], 3), dtype=np.float64)
    if gpu is not None:
        lab = hip_scene(gpu, objs, cam=cam, kernel=gpu.RTX_KERNEL_EXACT, **cfg).upload(0, lab=True)
        for row in range(h):
            st, cnt = lab.debug_paths(w, h, row, MAX_STEPS)
            assert cnt.max() < MAX_STEPS
            _replay_row(st, cnt, em, base, colour[row])
        lab.close()
    else:
        sc = oracle.make_scene(objs, cam, **cfg)
        with oracle.device_sincos():
            for row in range(h):
                st, cnt = oracle.trace_row(sc, w, h, row, MAX_STEPS)
                assert cnt.max() < MAX_STEPS
                _replay_row(st, cnt, em, base, colour[row])
    colour.setflags(write=False)
    _COLOURS[key] = colour
    return colour


def selected(total, sq, n, max_samples, threshold, floor):
    """the rule, per pixel: total / sq [..][3] float64, n [..] integer counts -> bool [..].  Every numpy operation below is one rounded f64
    operation, in the order the header states them; a comparison with a NaN is False"""
    n = np.asarray(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        dn = n.astype(np.float64)
        s0, s1, s2 = total[..., 0], total[..., 1], total[..., 2]
        v0 = sq[..., 0] - s0 * s0 / dn
        v1 = sq[..., 1] - s1 * s1 / dn
        v2 = sq[..., 2] - s2 * s2 / dn
        e = ((v0 + v1) + v2) / (dn - 1.0) / dn
        m = ((s0 + s1) + s2) / dn
        b = np.float64(threshold) * (m + np.float64(floor))
        return (n < max_samples) & ((n < 2) | (e > b * b))


class Simulation:
    """simulate(): the state of a band under rtx_render_blocks_refine.  colour [rows][w][>= max_samples][3] are the band's samples;
    total / sq start as the plain folds of the samples [0, sample_begin) unless given (the edge tests bring their own), extra as zeros.
    call(rounds) is one call: (pixels that traced, samples traced, pixels still selected)."""

    def __init__(self, colour, sample_begin, n_more, max_samples, threshold, floor, total=None, sq=None, extra=None):
        self.colour = colour
        self.rule = (int(max_samples), float(threshold), float(floor))
        self.sample_begin, self.n_more = int(sample_begin), int(n_more)
        base = colour[:, :, :self.sample_begin]
        self.total = left_fold(base) if total is None else np.array(total, dtype=np.float64)
        self.sq = left_fold(base * base) if sq is None else np.array(sq, dtype=np.float64)
        self.extra = np.zeros(colour.shape[:2], dtype=np.uint32) if extra is None else np.array(extra, dtype=np.uint32)

    def count(self):
        return self.sample_begin + self.extra.astype(np.int64)

    def select(self):
        return selected(self.total, self.sq, self.count(), *self.rule)

    def call(self, rounds=1):
        traced = np.zeros(self.extra.shape, dtype=bool)
        samples = 0
        for _ in range(int(rounds)):
            sel = self.select()                                   # decided once per round, from the sums at the round's start
            for _ in range(self.n_more):
                n = self.count()
                act = sel & (n < self.rule[0])
                if not act.any():
                    break
                c = self.colour[act, n[act]]                      # sample n of each active pixel
                self.total[act] = self.total[act] + c
                self.sq[act] = self.sq[act] + c * c               # the multiply rounded, then the add
                self.extra[act] += 1
                traced |= act
                samples += int(act.sum())
        return int(traced.sum()), samples, int(self.select().sum())


def census(colour, rule, limit=64):
    """(passes, finals): rounds = 1 calls until nothing is selected -- per pass (pixels that traced, samples traced), a last (0, 0) --
    and {final sample count: pixels}"""
    sim = Simulation(colour, **rule)
    passes = []
    for _ in range(limit):
        pixels, samples, still = sim.call(1)
        passes.append((pixels, samples))
        if pixels == 0:
            assert still == 0
            break
    values, counts = np.unique(sim.count(), return_counts=True)
    return passes, {int(v): int(c) for v, c in zip(values, counts)}
