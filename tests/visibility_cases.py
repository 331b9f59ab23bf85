"""The scenes, the hide sets and the contract of rtx_scene_set_visible for tests/test_visibility.py (host, no GPU) and
tests/test_visibility_gpu.py: one builder, as tests/update_cases.py is for the moves.

The contract (include/rtx_hip.h): after any sequence of calls a handle produces what a fresh upload of L_nan produces -- the current
list with the nine geom words of every hidden object set to NaN -- and frames, and hits through the monotone index map, are also
those of the list with the hidden objects deleted.  `l_nan`, `deleted` and `index_map` state those lists.

The tree the hide sets are aimed at is read from the dump of rtx_debug_host_set_visible (per wide node and child: the link and count
words, the box, the pack's link and count, the objects of the pack's leaf entries).  `check_slots` restates from the contract alone
-- not from csrc/rtx_refit.h -- what the dump of a handle with a hidden set must show:
  * a slot reads empty (count 0xFFFFFFFF) exactly when the pack's slot was empty or no object below it is visible;
  * any other slot has the pack's link and count words, a box that contains every visible shape below it (a sphere's c +- |r|, a
    triangle's vertices on the axes the box bounds), and a box that lies within the pack's box of that slot: hiding never grows one.
"""
import numpy as np

import mesh_update_cases as mc
import update_cases as uc
from rust_raytracing_amd.abi import RTX_PLANE, RTX_SPHERE, RTX_TRIANGLE

SPHERE_SCENES = ("s9", "s65", "s300")
MESH_SCENES = ("t6", "t40", "t300", "cubes25")
SCENES = SPHERE_SCENES + ("mixed",) + MESH_SCENES
EMPTY, TRI_LEAF, FLAT = 0xFFFFFFFF, 0x10000, 0x80000000
HIDE_CASES = ("one", "leaf", "leaf_but_one", "node4", "third", "all_tree", "plane", "outside")
# the cases hide_sets() finds per scene, stated so that collecting the tests loads no library (the host suite holds hide_sets to it):
# sphere leaves hold one sphere -- no partly hidden leaf --, every shape of a sphere scene is in the tree, t6 has no tree
_SPHERES = ("one", "leaf", "node4", "third", "all_tree")
_MESH = ("one", "leaf", "leaf_but_one", "node4", "third", "all_tree", "outside")
CASES_OF = {"s9": _SPHERES, "s65": _SPHERES, "s300": _SPHERES, "mixed": HIDE_CASES, "t6": ("one", "third", "outside"), "t40": _MESH,
            "t300": _MESH, "cubes25": _MESH}
PAIRS = [(name, case) for name in SCENES for case in CASES_OF[name]]

_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = uc.scene(name) if name in SPHERE_SCENES or name == "mixed" else mc.scene(name)
    return _cache[name].copy()


def l_nan(objs, hidden):
    out = objs.copy()
    out["geom"][np.asarray(sorted(hidden), dtype=np.int64)] = np.nan
    return out


def deleted(objs, hidden):
    keep = np.ones(len(objs), dtype=bool)
    keep[np.asarray(sorted(hidden), dtype=np.int64)] = False
    return objs[keep]


def index_map(n, hidden):
    """old index -> index in the deleted list (-1: hidden), and the inverse"""
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(sorted(hidden), dtype=np.int64)] = False
    fwd = np.where(keep, np.cumsum(keep) - 1, -1)
    return fwd, np.nonzero(keep)[0]


# ---- the tree, from the dump -----------------------------------------------------------------------------------------------------------
class Tree:
    """children[node][c] = ("empty",) | ("leaf", [objects]) | ("node", child index), from the PACK's words of a dump"""

    def __init__(self, dump):
        self.dump = dump
        self.children = []
        referenced = set()
        for k in range(len(dump)):
            row = []
            for c in range(4):
                link, count, n = int(dump[k, c, 8]), int(dump[k, c, 9]), int(dump[k, c, 10])
                if count == EMPTY:
                    row.append(("empty",))
                elif count == 0:
                    row.append(("node", link & ~FLAT))
                    referenced.add(link & ~FLAT)
                else:
                    row.append(("leaf", [int(x) for x in dump[k, c, 11:11 + n]]))
            self.children.append(row)
        roots = [k for k in range(len(dump)) if k not in referenced]
        assert len(roots) <= 1
        self.root = roots[0] if roots else None

    def below(self, node):
        out = []
        for ch in self.children[node]:
            if ch[0] == "leaf":
                out += ch[1]
            elif ch[0] == "node":
                out += self.below(ch[1])
        return out

    def objects(self):
        return set(self.below(self.root)) if self.root is not None else set()

    def leaves(self):
        return [ch[1] for row in self.children for ch in row if ch[0] == "leaf"]

    def depth_of(self, node, at=None, d=1):
        at = self.root if at is None else at
        if at == node:
            return d
        for ch in self.children[at]:
            if ch[0] == "node":
                r = self.depth_of(node, ch[1], d + 1)
                if r:
                    return r
        return 0


def tree_of(rtx, sc):
    out = rtx.debug_host_set_visible(sc, [], dump=True)
    return Tree(out[5])


def hide_sets(tree, objs, seed=0):
    """{case: sorted object indices} of the hide cases that exist on this scene"""
    rng = np.random.default_rng(1000 + seed)
    in_tree = tree.objects()
    out = {}
    shapes = np.nonzero(objs["kind"] != RTX_PLANE)[0]
    out["one"] = [int(sorted(in_tree)[len(in_tree) // 2])] if in_tree else [int(shapes[0])]
    leaves = tree.leaves()
    multi = [l for l in leaves if len(l) > 1]
    if leaves:
        out["leaf"] = sorted(max(leaves, key=len))
    if multi:
        big = max(multi, key=len)
        out["leaf_but_one"] = sorted(big[1:])
    # a wide node that is not the root, with four used slots where the tree has one (else the fullest): everything below it
    inner = [k for k in range(len(tree.children)) if k != tree.root]
    if inner:
        k = max(inner, key=lambda q: (sum(ch[0] != "empty" for ch in tree.children[q]), tree.depth_of(q)))
        out["node4"] = sorted(tree.below(k))
    out["third"] = sorted(int(x) for x in rng.choice(len(objs), max(len(objs) // 3, 1), replace=False))
    if in_tree:
        out["all_tree"] = sorted(in_tree)
    planes = np.nonzero(objs["kind"] == RTX_PLANE)[0]
    if len(planes):
        out["plane"] = [int(planes[0])]
    outside = [int(k) for k in shapes if int(k) not in in_tree]
    if outside:
        out["outside"] = outside[:2]
    return out


def how_of(tree, idx, hidden_before=(), hide=True):
    """the path the header prescribes for hiding (showing) `idx` with `hidden_before` hidden, when every shown shape is taken in place"""
    before = set(int(k) for k in hidden_before)
    changed = [k for k in set(int(i) for i in idx) if (k in before) != hide]
    if not changed:
        return "nothing"
    return "refit" if any(k in tree.objects() for k in changed) else "records"


# ---- the contract on the dump --------------------------------------------------------------------------------------------------------
def _f32(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


def _shape_box(o):
    g = o["geom"]
    if o["kind"] == RTX_SPHERE:
        r = abs(g[3])
        return g[:3] - r, g[:3] + r
    v = g.reshape(3, 3)
    return v.min(axis=0), v.max(axis=0)


def check_slots(tree, objs, hidden, dump):
    """`dump`: of a handle whose list is `objs` (real geometries) with `hidden` hidden; `tree`: of the pack those arrays come from"""
    hidden = set(int(k) for k in hidden)
    n_empty = n_live = 0
    for k, row in enumerate(tree.children):
        for c, ch in enumerate(row):
            link, count = int(dump[k, c, 0]), int(dump[k, c, 1])
            below = ch[1] if ch[0] == "leaf" else (tree.below(ch[1]) if ch[0] == "node" else [])
            alive = [o for o in below if o not in hidden]
            if not alive:
                assert count == EMPTY, ("a slot with nothing visible below is not empty", k, c, below)
                n_empty += 1
                continue
            n_live += 1
            assert (link, count) == (int(tree.dump[k, c, 8]), int(tree.dump[k, c, 9])), ("a live slot lost the pack's words", k, c)
            lo, hi = _f32(dump[k, c, 2:5]), _f32(dump[k, c, 5:8])
            plo, phi = _f32(tree.dump[k, c, 2:5]), _f32(tree.dump[k, c, 5:8])
            assert (lo >= plo).all() and (hi <= phi).all(), ("a box grew by hiding", k, c)
            for o in alive:
                slo, shi = _shape_box(objs[o])
                bounded = np.isfinite(lo) & np.isfinite(hi)
                assert (lo[bounded] <= slo[bounded]).all() and (hi[bounded] >= shi[bounded]).all(), ("a visible shape outside its slot's box", k, c, o)
    return n_empty, n_live


# ---- rays aimed through a hidden sphere at a visible one ----------------------------------------------------------------------------------
def rays_through(objs, hidden, n=200, seed=3):
    """origins beyond a hidden sphere H on the line through its centre and the centre of a visible sphere V, directed at V: H lies
    between the origin and V, so a stale f32 record of H that were still `certain` would bound the walk in front of V"""
    rng = np.random.default_rng(seed)
    sph = [int(k) for k in np.nonzero(objs["kind"] == RTX_SPHERE)[0]]
    hid = [k for k in sph if k in set(hidden)]
    vis = [k for k in sph if k not in set(hidden)]
    if not hid or not vis:
        return np.zeros((0, 3)), np.zeros((0, 3))
    o, d = [], []
    for _ in range(n):
        h, v = objs["geom"][rng.choice(hid)], objs["geom"][rng.choice(vis)]
        axis = v[:3] - h[:3]
        ln = np.linalg.norm(axis)
        if ln == 0.0:
            continue
        axis /= ln
        o.append(h[:3] - axis * (abs(h[3]) * 1.5 + 0.25))
        d.append(axis)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)
