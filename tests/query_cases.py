"""TEST TOOLING shared by tests/test_query_host.py and tests/test_query_gpu.py: the scenes and rays of
the ray-query tests, their cached references (tests/query_ref.py) and the bars.

Rays: 512 per scene, default_rng(11), origins uniform in the scene's bounding box inflated by a quarter
of its extent, each aimed at a uniform point of the box (`demo1_moving`: at a point of a moving sphere's
swept box), directions left un-normalised.  Times are multiples of 2^-24, which the kernel keeps exactly.

Included rays (query_ref.included, margin m = 1e-6 binary64, 1e-3 FP32).  Excluded shares measured with
this evaluator (at most 5 % allowed):
    scene            m = 1e-6   m = 1e-3
    cornell_box       3.1 %      3.7 %    (exact ties: the boxes stand on the floor)
    box_gallery       1.2 %      1.6 %
    demo1             0          0.2 %
    bunny_cornell     0          0.6 %
    pawn_instances    0          0.2 %
    demo1_moving      0          0.4 %

Bars on included rays, eps the precision's machine epsilon, S = |o|inf + (largest |coordinate| of the
scene's bounding box) + |t_ref|, c the winner's conditioning, K the constant tests/test_device_probe.py
asserts for the leaf kind's intersection function (plane shapes 8, spheres 1024):
    t       |t - t_ref| <= 2 K eps S / c                     (the "t bar")
    point   within the t bar + 4 eps S (largest component)
    normal  | |n|^2 - 1 | <= 8 eps; plane shapes within 16 eps of the reference's facing normal;
            spheres within (t bar) / r + 4 eps
    uv      plane shapes only, within (t bar) / min(|u|, |v|) + 8 eps
"""
import functools
import math
import os

import numpy as np

import query_ref as QR
import raytrace_amd as R
from raytrace_amd import scenes
from raytrace_amd.query import make_rays
from raytrace_amd.scene import flatten

N_RAYS = 512
SCENES = ["cornell_box", "box_gallery", "demo1", "bunny_cornell", "pawn_instances", "demo1_moving"]
MARGIN = {"f64": 1e-6, "f32": 1e-3}
K_PLANE, K_SPHERE = 8.0, 1024.0  # tests/test_device_probe.py: test_plane_test_random_cases, test_sphere_test_random_cases
RT_VAR_BASE, RT_VAR_INST = 3, 64
MOVING = [((-3.0 + 1.5 * k, 0.45 + 0.1 * (k % 3), 2.0 + 0.7 * (k % 4)), 0.3 + 0.02 * k) for k in range(12)]


def pawn_instances():
    """Three rigid placements of ONE pawn mesh (each an rt_instance: the mesh has far more than
    scene.INSTANCE_MIN_LEAVES leaves), one with a material over the placement, on a floor."""
    mesh = R.transformVertices(R.scale(100), scenes.load_mesh("pawn.obj"))
    pawn = R.lambertian(R.constantTexture(R.V3(0.8, 0.6, 0.3))) << R.triangleMesh(mesh)
    return R.group([
        R.lambertian(R.constantTexture(0.5)) << R.parallelogram((-12, 0, -12), (24, 0, 0), (0, 0, 24)),
        R.transform(R.translate(R.V3(-4, 0, -1)) @ R.rotateY(R.degrees(35)), pawn),
        R.metal(0.1, R.constantTexture(0.9)) << R.transform(R.translate(R.V3(0, 0.5, 2)) @ R.rotateX(R.degrees(20)), pawn),
        R.transform(R.translate(R.V3(4, 0, -2)) @ R.rotateY(R.degrees(-100)), pawn),
    ])


def demo1_moving():
    """demo1's world (which has no `moving` geometry of its own) with twelve moving spheres and a
    moving triangle above it: the motion path of the generic-leaf BVH class."""
    world = scenes.demo1()[1]
    mat = R.lambertian(R.constantTexture(R.V3(0.7, 0.3, 0.1)))
    movers = [mat << R.moving((0, 0, 0), (0.4 * (k % 3), 0.5, -0.2 * k), R.sphere(c, r)) for k, (c, r) in enumerate(MOVING)]
    movers.append(mat << R.moving((0, 0.3, 0), (1.0, 0, 0),
                                  R.triangle(((-1, 2, 1), (0, 0)), ((1, 2, 1), (1, 0)), ((0, 3.5, 1.5), (0.5, 1)))))
    return R.group([world] + movers)


@functools.lru_cache(None)
def world_of(name):
    if name == "pawn_instances":
        return pawn_instances()
    if name == "demo1_moving":
        return demo1_moving()
    return getattr(scenes, name)()[1]


@functools.lru_cache(None)
def flat_of(name):
    return flatten(world_of(name))


@functools.lru_cache(None)
def leaves_of(name):
    return QR.Leaves(world_of(name))


@functools.lru_cache(None)
def rays_of(name, n=N_RAYS):
    """(origins, directions, tmin, tmax, time) of the scene's test rays."""
    L = leaves_of(name)
    lo, hi = L.box
    ext = hi - lo
    rng = np.random.default_rng(11)
    o = rng.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (n, 3))
    tgt = rng.uniform(lo, hi, (n, 3))
    time = np.zeros(n)
    if name in ("demo1", "demo1_moving"):
        time = rng.integers(0, 2 ** 24, n) / 2.0 ** 24
    if name == "demo1_moving":  # from near the spheres, at a point of a mover's swept box
        k = rng.integers(0, len(MOVING), n)
        c = np.array([m[0] for m in MOVING])[k]
        o = c + rng.uniform(-6, 6, (n, 3)) + [0, 4, 0]
        tgt = c + rng.uniform(-0.3, 0.3, (n, 3)) + rng.uniform(0, 1, (n, 1)) * np.stack([0.4 * (k % 3), 0.5 + 0 * k, -0.2 * k], 1)
    return o, tgt - o, 1e-4, np.inf, time


def ray_records(name, n=N_RAYS):
    return make_rays(*rays_of(name, n))


@functools.lru_cache(None)
def reference(name, precision):
    """(ref, included, tie) of the scene's test rays at the precision's margin."""
    m = MARGIN[precision]
    ref = QR.evaluate(leaves_of(name), *rays_of(name), m)
    inc, tie = QR.included(ref, m)
    return ref, inc, tie


def expected_leaf(name, ref, variant):
    """rt_hit.leaf of the reference's winner: its depth-first order; a flat scene's key order is the
    leaf's rank among the surface leaves in that order (rt_internal.h DevFlatSet)."""
    leaf = ref["leaf"].copy()
    if (variant & RT_VAR_BASE) == 0:
        orders = np.sort(leaves_of(name).order)
        leaf = np.where(ref["hit"], np.searchsorted(orders, np.maximum(leaf, 0)), -1)
    return leaf


def expected_instance(name, ref):
    """The placement the scene tree puts the winner's leaf in (-1: none): flatten's instances own the
    orders [order, order + leaves of the object)."""
    flat = flat_of(name)
    inst = np.full(len(ref["leaf"]), -1)
    for k, rec in enumerate(flat.instances):
        n_obj = int(np.sum(flat.prims["set"] == -1 - rec["blas"]))
        inst[(ref["leaf"] >= rec["order"]) & (ref["leaf"] < rec["order"] + n_obj)] = k
    return inst


def check_against_ref(hits, name, precision, variant, report=None):
    """Assert the bars of this module's docstring on rt_hit records of the scene's test rays."""
    ref, inc, tie = reference(name, precision)
    L, flat = leaves_of(name), flat_of(name)
    eps = float(np.finfo(np.float64 if precision == "f64" else np.float32).eps)
    excluded = 1.0 - float(inc.mean())
    print(f"{name} {precision}: excluded {100 * excluded:.2f} %, ties {100 * float(tie.mean()):.2f} %, "
          f"hits {100 * float(ref['hit'].mean()):.1f} %")
    assert excluded <= 0.05, excluded
    got_hit = hits["hit"] == 1
    assert (hits["hit"] >= 0).all()
    use = inc | tie
    assert (got_hit == ref["hit"])[use].all(), np.flatnonzero((got_hit != ref["hit"]) & use)[:8]
    h = inc & ref["hit"]
    ht = use & ref["hit"]
    S = ref["origin_inf"] + L.extent + np.abs(np.where(ref["hit"], ref["t"], 0))
    K = np.where(ref["kind"] == QR.SPHERE, K_SPHERE, K_PLANE)
    with np.errstate(all="ignore"):
        tbar = 2 * K * eps * S / ref["c"]
    with np.errstate(invalid="ignore"):
        t_err = np.abs(hits["t"].astype(QR.LD) - ref["t"])
    fig = {"t": float((t_err[ht] / tbar[ht]).max())}
    assert (t_err[ht] <= tbar[ht]).all(), fig
    assert (hits["leaf"] == expected_leaf(name, ref, variant))[h].all()
    assert ((hits["front"] != 0) == ref["front"])[h].all()
    assert (hits["instance"] == expected_instance(name, ref))[h].all()
    for i in np.flatnonzero(h):
        want = L.material[ref["index"][i]]
        got = flat.material_objects[hits["material"][i]]
        assert got.key() == want.key(), (i, got, want)
    p_err = np.abs(hits["point"].astype(QR.LD) - ref["point"]).max(1)
    p_bar = tbar + 4 * eps * S
    fig["point"] = float((p_err[h] / p_bar[h]).max())
    assert (p_err[h] <= p_bar[h]).all(), fig
    n2 = np.abs((hits["normal"].astype(QR.LD) ** 2).sum(1) - 1)
    fig["n2"] = float(n2[h].max() / eps)
    assert (n2[h] <= 8 * eps).all(), fig
    n_err = np.abs(hits["normal"].astype(QR.LD) - ref["normal"]).max(1)
    sph = h & (ref["kind"] == QR.SPHERE)
    pl = h & (ref["kind"] != QR.SPHERE)
    if pl.any():
        fig["n_plane"] = float(n_err[pl].max() / eps)
        assert (n_err[pl] <= 16 * eps).all(), fig
        uv_err = np.abs(hits["uv"].astype(QR.LD) - ref["uv"]).max(1)
        uv_bar = tbar / ref["uvscale"] + 8 * eps
        fig["uv"] = float((uv_err[pl] / uv_bar[pl]).max())
        assert (uv_err[pl] <= uv_bar[pl]).all(), fig
    if sph.any():
        n_bar = tbar / ref["radius"] + 4 * eps
        fig["n_sphere"] = float((n_err[sph] / n_bar[sph]).max())
        assert (n_err[sph] <= n_bar[sph]).all(), fig
    print("  worst error / bar:", {k: round(v, 4) for k, v in fig.items()})
    if report is not None:
        report[(name, precision)] = dict(fig, excluded=excluded)
    return fig


def deep_scene():
    """A BVH more than 20 levels deep (spheres 8^k apart along the view axis), as tests/test_gpu.py
    test_deep_bvh_against_oracle builds one."""
    objs = [R.lambertian(R.constantTexture(0.5)) << R.sphere((0, -1000.5, -1), 1000)]
    for k in range(40):
        objs.append(R.lambertian(R.constantTexture((0.8, 0.3, 0.2))) << R.sphere((0.3 * (k % 3 - 1), 0.0, -2.0 - 8.0 ** k), 0.2))
    return R.group(objs)


def deep_rays(n=256):
    """Rays into deep_scene: half from the camera side at random (some hit), half parallel to the view
    axis through the gap between the spheres (x = 0.15, y = 0.19: inside every node's box, outside
    every sphere), which push one far child per BVH level."""
    rng = np.random.default_rng(3)
    o = np.array([0, 0.3, 1.0]) + rng.uniform(-0.2, 0.2, (n, 3))
    d = np.array([0, 0, -1.0]) + rng.uniform(-0.12, 0.12, (n, 3))
    o[n // 2:] = np.array([0.15, 0.19, 1.0]) + rng.uniform(-0.01, 0.01, (n - n // 2, 3))
    d[n // 2:] = (0, 0, -1.0)
    return make_rays(o, d)
