"""TEST TOOLING: a numpy long-double evaluator of the reference's hit semantics over the Python scene
tree, the yardstick of the ray queries (include/rt.h rt_scene_cast).

Written from Geometry.hs: `sphere` (58-94) and `sphereUV` (100-104), `planeShape`, `parallelogram`,
`cuboid`, `triangle` (108-176), `group` and `bvhNode` (335-363: the closest hit in the open interval,
the earlier leaf in depth-first order on equal t), `transform` (382-391) and `moving` (449-456).  It is
independent of rt_trace.h and of the oracle: every leaf (Sphere, PlaneShape) is tested by brute force
with the ray taken through the leaf's own chain of inverse transforms and motion shifts, outermost
first, in np.longdouble.  `ConstantMedium` subtrees are skipped (a query sees surfaces only), but they
take their depth-first orders as raytrace_amd.scene.flatten counts them.

`evaluate` also returns, per ray, what makes a comparison with a rounded implementation meaningful:
the winner's conditioning c (|n . d| for plane shapes, sqrt(disc) / r for spheres), the gap to the
second candidate, the winner's inside-test margin, and whether a LOSING leaf whose plane / sphere is met
at or before the winner had an inside-test or discriminant margin within m of zero or |n . d| within
1e-9 of the 1e-8 threshold.  `included` applies the exclusion rules to them.
"""
import numpy as np

from raytrace_amd import geometry as G

LD = np.longdouble
SPHERE, QUAD, TRI = 0, 1, 2


class Leaves:
    """The surface leaves of a scene tree, grouped by (chain, kind) for vector evaluation."""

    def __init__(self, world):
        self.chains = []      # chain id -> tuple of ops, outermost first: ("T", inv34, m34) | ("M", v0, v1)
        chain_ids = {}
        rows = []             # (chain id, kind, order, material, params)
        order = [0]

        def count(node):
            if isinstance(node, (G.Sphere, G.PlaneShape)):
                return 1
            if isinstance(node, G.ConstantMedium):
                return 1 + count(node.child)
            return sum(count(c) for c in G.children_of(node))

        def chain_id(ops):
            key = tuple(id(n) for n, _ in ops)
            if key not in chain_ids:
                chain_ids[key] = len(self.chains)
                self.chains.append(tuple(op for _, op in ops))
            return chain_ids[key]

        def walk(node, ops, mat):
            if isinstance(node, G.WithMaterial):
                walk(node.child, ops, node.material if mat is None else mat)  # the outermost `<$` wins
            elif isinstance(node, G.Group):
                for c in node.children:
                    walk(c, ops, mat)
            elif isinstance(node, G.BvhNode):
                walk(node.left, ops, mat)
                walk(node.right, ops, mat)
            elif isinstance(node, G.Transform):
                walk(node.child, ops + [(node, ("T", np.array(node.inv34, LD), np.array(node.m34, LD)))], mat)
            elif isinstance(node, G.Moving):
                walk(node.child, ops + [(node, ("M", np.array(node.v0, LD), np.array(node.v1, LD)))], mat)
            elif isinstance(node, G.ConstantMedium):
                order[0] += count(node)
            elif isinstance(node, G.Sphere):
                rows.append((chain_id(ops), SPHERE, order[0], mat, list(node.center) + [node.radius] + [0.0] * 11))
                order[0] += 1
            elif isinstance(node, G.PlaneShape):
                quad = node.kind == G.PARALLELOGRAM
                uv = [0.0, 0.0, 1.0, 0.0, 0.0, 1.0] if quad else list(node.uv0) + list(node.uv1) + list(node.uv2)
                rows.append((chain_id(ops), QUAD if quad else TRI, order[0], mat, list(node.q) + list(node.u) + list(node.v) + uv))
                order[0] += 1
            else:
                raise TypeError(type(node).__name__)

        walk(world, [], None)
        self.n = len(rows)
        self.chain = np.array([r[0] for r in rows], np.int64)
        self.kind = np.array([r[1] for r in rows], np.int64)
        self.order = np.array([r[2] for r in rows], np.int64)
        self.material = [r[3] for r in rows]
        self.params = np.array([r[4] for r in rows], LD).reshape(-1, 15)
        self.index_of_order = {int(o): i for i, o in enumerate(self.order)}
        lo = np.array([b[0] for b in world.bbox], np.float64)
        hi = np.array([b[1] for b in world.bbox], np.float64)
        self.box = (lo, hi)
        self.extent = float(max(np.abs(lo).max(), np.abs(hi).max()))


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _apply(m, v, point):
    r = v @ m[:, :3].T
    return r + m[:, 3] if point else r


def _chain_ray(ops, o, d, time):
    """The ray in the leaf's frame (transform: inv_m on origin and direction; moving: origin - shift)."""
    for op in ops:
        if op[0] == "T":
            o, d = _apply(op[1], o, True), _apply(op[1], d, False)
        else:
            shift = (1 - time)[:, None] * op[1] + time[:, None] * op[2]
            o = o - shift
    return o, d


def _chain_back(ops, p, n, time):
    """A hit's point and normal back to the world, innermost op first."""
    for op in reversed(ops):
        if op[0] == "T":
            p, n = _apply(op[2], p, True), _apply(op[2], n, False)
        else:
            p = p + ((1 - time)[:, None] * op[1] + time[:, None] * op[2])
    return p, n


def _test_group(kind, prm, o, d, tmin, tmax):
    """Leaves prm (L, 15) of one kind against rays (N, 3): (L, N) arrays t (the parameter the leaf's
    plane / sphere is met at, NaN-free), ok (the reference accepts the hit in (tmin, tmax)), margin
    (the inside-test / discriminant margin, >= 0 inside), c (conditioning), near (|n . d| within 1e-9
    of 1e-8)."""
    o, d = o[None], d[None]
    with np.errstate(all="ignore"):
        if kind == SPHERE:
            cen, r = prm[:, None, 0:3], prm[:, None, 3]
            oc = cen - o
            h = _dot(d, oc)
            disc = h * h - (_dot(oc, oc) - r * r)
            sq = np.sqrt(np.maximum(disc, 0))
            r1, r2 = h - sq, h + sq
            in1 = (tmin < r1) & (r1 < tmax)
            t = np.where(in1, r1, r2)
            ok = (disc >= 0) & (tmin < t) & (t < tmax)
            margin = disc / (r * r)
            c = sq / np.abs(r)
            near = np.zeros(t.shape, bool)
        else:
            q, u, v = prm[:, None, 0:3], prm[:, None, 3:6], prm[:, None, 6:9]
            cp = _cross(u, v)
            ncp = np.sqrt(_dot(cp, cp))
            nrm = cp / ncp[..., None]
            nS = nrm / ncp[..., None]
            denom = _dot(nrm, d)
            t = _dot(nrm, q - o) / denom
            prel = (o + t[..., None] * d) - q
            a = _dot(nS, _cross(prel, v))
            b = _dot(nS, _cross(u, prel))
            margin = np.minimum(np.minimum(a, b), np.minimum(1 - a, 1 - b) if kind == QUAD else 1 - a - b)
            big = np.abs(denom) > LD(1e-8)
            ok = big & (tmin < t) & (t < tmax) & (margin >= 0)
            c = np.abs(denom)
            near = np.abs(np.abs(denom) - LD(1e-8)) <= LD(1e-9)
            t = np.where(np.isfinite(t), t, LD(np.inf))
            margin = np.where(np.isfinite(margin), margin, LD(-1))
    return t, ok, margin, c, near


def evaluate(leaves: Leaves, origins, directions, tmin, tmax, time, m):
    """The reference's hit of every ray origin + t dir / |dir| in (tmin, tmax) at `time` (arrays of n),
    and the comparison data for margin m.  Returns a dict of arrays (float fields np.longdouble)."""
    o = np.asarray(origins, LD).reshape(-1, 3)
    n = len(o)
    d = np.broadcast_to(np.asarray(directions, LD), (n, 3))
    d = d / np.sqrt(_dot(d, d))[:, None]
    tmin = np.broadcast_to(np.asarray(tmin, LD), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, LD), (n,))
    time = np.broadcast_to(np.asarray(time, LD), (n,))
    inf = LD(np.inf)
    best_t = np.full(n, inf)
    best_ord = np.full(n, np.iinfo(np.int64).max)
    best = np.full(n, -1)
    best_margin = np.full(n, inf)
    best_c = np.full(n, inf)
    second_t = np.full(n, inf)
    # borderline losers: kept per ray as the smallest t of one (compared with the winner at the end)
    border_t = np.full(n, inf)
    border_ord = np.full(n, -1)
    CH = 128
    for ch in range(len(leaves.chains)):
        oc, dc = _chain_ray(leaves.chains[ch], o, d, time)
        for kind in (SPHERE, QUAD, TRI):
            idx = np.nonzero((leaves.chain == ch) & (leaves.kind == kind))[0]
            for k0 in range(0, len(idx), CH):
                ii = idx[k0:k0 + CH]
                t, ok, margin, c, near = _test_group(kind, leaves.params[ii], oc, dc, tmin, tmax)
                ords = leaves.order[ii][:, None]
                tc = np.where(ok, t, inf)
                # the chunk's winner per ray: smallest t, then smallest order
                key_t = tc.min(0)
                cand = tc == key_t[None]
                o_sel = np.where(cand & ok, ords, np.iinfo(np.int64).max).min(0)
                row = np.argmax(cand & ok & (ords == o_sel[None]), 0)
                ar = np.arange(n)
                # second candidate of the chunk: smallest t of the others
                t_wo = tc.copy()
                t_wo[row, ar] = inf
                sec = t_wo.min(0)
                better = (key_t < best_t) | ((key_t == best_t) & (o_sel < best_ord) & (key_t < inf))
                # the loser of (old best, chunk winner) is a second candidate
                loser = np.where(better, best_t, key_t)
                second_t = np.minimum(second_t, np.minimum(loser, sec))
                best_margin = np.where(better, margin[row, ar], best_margin)
                best_c = np.where(better, c[row, ar], best_c)
                best = np.where(better, ii[row], best)
                best_ord = np.where(better, o_sel, best_ord)
                best_t = np.where(better, key_t, best_t)
                # borderline leaves: margin within m of zero (either sign), or |n . d| near its threshold,
                # met inside the interval
                bl = ((np.abs(margin) <= m) | near) & (t > tmin[None]) & (t < tmax[None])
                bt = np.where(bl, t, inf)
                brow = np.argmin(bt, 0)
                bmin = bt[brow, ar]
                upd = bmin < border_t
                border_ord = np.where(upd, leaves.order[ii][brow], border_ord)
                border_t = np.where(upd, bmin, border_t)
    hit = best >= 0
    with np.errstate(invalid="ignore"):
        gap = np.where(hit, second_t - best_t, inf)
    res = dict(hit=hit, t=best_t, leaf=np.where(hit, best_ord, -1), index=best, margin=best_margin, c=best_c,
               gap=gap, tmin=tmin, tmax=tmax)
    # a borderline LOSER at or before the winner (a miss: anywhere in the interval)
    limit = np.where(hit, best_t + m * np.maximum(best_t, 1), tmax)
    res["border"] = (border_t <= limit) & (border_ord != res["leaf"])
    # the winner's record
    point = np.zeros((n, 3), LD)
    normal = np.zeros((n, 3), LD)
    uv = np.zeros((n, 2), LD)
    front = np.zeros(n, bool)
    kind_w = np.full(n, -1)
    radius = np.full(n, inf)
    uvscale = np.full(n, inf)   # min(|u|, |v|) of a plane shape
    for i in np.nonzero(hit)[0]:
        li = best[i]
        ops = leaves.chains[leaves.chain[li]]
        oc, dc = _chain_ray(ops, o[i:i + 1], d[i:i + 1], time[i:i + 1])
        prm, t = leaves.params[li], best_t[i]
        p = oc + t * dc
        k = leaves.kind[li]
        kind_w[i] = k
        if k == SPHERE:
            out = (p - prm[0:3]) / prm[3]
            fr = _dot(dc, out) <= 0
            nn = np.where(fr, out, -out)
            with np.errstate(all="ignore"):
                uv[i] = [np.arctan2(out[0, 0], out[0, 2]) / (2 * LD(np.pi)) + LD(0.5), np.arccos(-out[0, 1]) / LD(np.pi)]
            radius[i] = abs(prm[3])
        else:
            q, u, v = prm[0:3], prm[3:6], prm[6:9]
            cp = _cross(u, v)
            ncp = np.sqrt(_dot(cp, cp))
            nrm = cp / ncp
            fr = _dot(nrm, dc[0]) < 0
            nn = (nrm if fr else -nrm)[None]
            prel = p[0] - q
            a, b = _dot(nrm / ncp, _cross(prel, v)), _dot(nrm / ncp, _cross(u, prel))
            uv0, uv1, uv2 = prm[9:11], prm[11:13], prm[13:15]
            uv[i] = (1 - a - b) * uv0 + a * uv1 + b * uv2
            uvscale[i] = min(np.sqrt(_dot(u, u)), np.sqrt(_dot(v, v)))
        pw, nw = _chain_back(ops, p, nn, time[i:i + 1])
        point[i], normal[i], front[i] = pw[0], nw[0], bool(np.all(fr))
    res.update(point=point, normal=normal, uv=uv, front=front, kind=kind_w, radius=radius, uvscale=uvscale,
               origin_inf=np.abs(o).max(1))
    return res


def included(ref, m):
    """(comparable, tie): rays whose reference answer a rounded implementation must reproduce, and the
    excluded rays that are ties (a second candidate within the gap rule): `hit` and `t` still hold there.
    Excluded, by the reference alone: the gap to the second candidate <= m max(t, 1); the winner's margin
    or conditioning below m; a borderline loser at or before the winner; t within m of an interval end."""
    hit = ref["hit"]
    t = np.where(hit, ref["t"], 0)
    with np.errstate(invalid="ignore"):
        tie = hit & (ref["gap"] <= m * np.maximum(t, 1))
        weak = hit & ((ref["margin"] < m) | (ref["c"] < m))
        ends = hit & ((t - ref["tmin"] <= m) | (ref["tmax"] - t <= m))
    excluded = tie | weak | ref["border"] | ends
    return ~excluded, tie & ~(weak | ref["border"] | ends)
