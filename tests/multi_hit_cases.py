"""The cases of tests/test_multi_hit_bounds.py: bounds_cases' aimed rays on scenes that hold every object twice.

The multi-hit walks (rtx_scene_multi_hits) prune against round_up32 of the k-th distance of the ray's list once it is
full.  bounds_cases aims every ray at the f32 margin of ONE object, its target; here the scene is test_multi_hit_queries.doubled() of
the case's scene, so the target is a PAIR of equal shapes with equal distances.  With m distinct objects nearer than the target the
pair sits at ranks (2m, 2m + 1) of the ray's list, and at k = 2m + 1 the list is full as soon as one copy is in: the bound is then
round_up32(t) of the aimed object itself, and the other copy -- the same t, perhaps the lower index -- must still be entered, queued,
pass multi_flush's `<= bound` and displace the first.  Such a (ray, k) is called TIGHT: test_walk_bounds' "tight" regime, produced by
the real walk.  Nothing new is computed from the text: the answer for both copies is the case's own t / reported.

doubled_scene(name): the doubled scene, twin[], and lo[j] < hi[j], the two indices of the case's object j.
ladder(t, reported): the per-ray limits, aimed at the target's own t.  Six rungs where the text reports the target -- +inf, the f64
    after t, t, the f64 before t, round_up32(t) as an f64 (bound0 is then exactly the f32 the full list's bound would be) and the f64
    after that (bound0 one f32 ulp higher) --, four where it does not (+inf, 1e30, 1.0, NaN).  The rung is (i + i / 6) % 6 resp.
    (i + i / 4) % 4 of the ray index i: cycled by the index, moved on by one after every cycle, because bounds_cases' direction regimes
    are i % 6 themselves and every regime has to meet every rung.
subsample(name, regime): 256 seeded rays of a case, up to 224 of them drawn among `aimed & reported`, the others among the rest (the
    unreported targets and the surface regime's second pairs) -- the rays the oracle's full lists are computed for.
oracle_case(oracle, name, regime): those lists (test_multi_hit_queries.oracle_lists on the doubled scene), once per process.
rank_of(objects, lo, hi): per ray the positions of both copies in an (n, k) array of object indices (-1: not there)."""
import functools

import numpy as np

import bounds_cases as bc
import bounds_model as bm
from test_multi_hit_queries import doubled, oracle_lists

INF, NAN = np.inf, np.nan
SUBSAMPLE = 256
SUBSAMPLE_REPORTED = 224
RUNGS = ("+inf", "after t", "t", "before t", "round_up32(t)", "after round_up32(t)")


def _seed(name):
    return 20 + sum(map(ord, name))


@functools.lru_cache(maxsize=None)
def doubled_scene(name):
    import rust_raytracing_amd as rtx
    objs = dict(bc.scenes(rtx.OBJECT_DTYPE))[name]
    n = len(objs)
    both, twin = doubled(objs, _seed(name))
    old = np.random.default_rng(_seed(name)).permutation(2 * n) % n      # doubled()'s own shuffle: entry i is a copy of object old[i]
    assert both.tobytes() == objs[old].tobytes()
    order = np.argsort(old, kind="stable")
    lo, hi = order[0::2], order[1::2]
    assert np.array_equal(old[lo], np.arange(n)) and np.array_equal(old[hi], np.arange(n)) and (lo < hi).all()
    assert np.array_equal(twin[lo], hi) and np.array_equal(twin[hi], lo)
    return both, twin, lo, hi


@functools.lru_cache(maxsize=None)
def doubled_pack(name):
    return bm.pack_for(doubled_scene(name)[0])


def ladder(t, reported):
    """(t_max (n,), rung (n,)) -- module docstring"""
    n = len(t)
    i = np.arange(n)
    tt = np.where(reported, t, 1.0)
    up = bm.round_up32(tt).astype(np.float64)
    hit = np.stack([np.full(n, INF), np.nextafter(tt, INF), tt, np.nextafter(tt, 0.0), up, np.nextafter(up, INF)])
    miss = np.array([INF, 1e30, 1.0, NAN])
    rung = np.where(reported, (i + i // 6) % 6, (i + i // 4) % 4)
    return np.where(reported, hit[rung % 6, i], miss[rung % 4]), rung


@functools.lru_cache(maxsize=None)
def subsample(name, regime):
    cs = bc.case(name, regime)
    rng = np.random.default_rng(_seed(name + "/" + regime))
    first = np.nonzero(cs["aimed"] & cs["reported"])[0]
    rest = np.nonzero(~(cs["aimed"] & cs["reported"]))[0]
    n_rest = min(len(rest), SUBSAMPLE - min(len(first), SUBSAMPLE_REPORTED))
    n_first = min(len(first), SUBSAMPLE - n_rest)
    sel = np.concatenate([rng.choice(first, n_first, replace=False), rng.choice(rest, n_rest, replace=False)])
    return np.sort(sel)


_LISTS = {}


def oracle_case(oracle, name, regime):
    """(sel, lists): the subsample and the oracle's full sorted (t, index) lists of its rays on the doubled scene"""
    if (name, regime) not in _LISTS:
        cs = bc.case(name, regime)
        sel = subsample(name, regime)
        _LISTS[(name, regime)] = (sel, oracle_lists(oracle, doubled_scene(name)[0], cs["o"][sel], cs["d"][sel]))
    return _LISTS[(name, regime)]


def rank_of(objects, lo, hi):
    """(p_lo, p_hi) (n,): the column of lo[i] / hi[i] in row i of objects (n, k), -1 where it is not there"""
    at_lo, at_hi = objects == lo[:, None], objects == hi[:, None]
    return np.where(at_lo.any(axis=1), at_lo.argmax(axis=1), -1), np.where(at_hi.any(axis=1), at_hi.argmax(axis=1), -1)


def list_objects(lists, k):
    """the first k indices and distances of each of the oracle's lists as (n, k) arrays (-1 / +inf behind the list)"""
    obj = np.full((len(lists), k), -1, dtype=np.int64)
    dist = np.full((len(lists), k), INF)
    for r, l in enumerate(lists):
        for j, (t, idx) in enumerate(l[:k]):
            obj[r, j], dist[r, j] = idx, t
    return obj, dist


def tight_k(p_lo, p_hi):
    """the k at which a ray is tight: both copies adjacent at columns (k - 1, k), 0 where they are not in the list"""
    return np.where((p_lo >= 0) & (p_hi == p_lo + 1), p_lo + 1, 0)
