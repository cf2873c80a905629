"""TEST TOOLING: one small scene per dispatchable render-kernel class (rt_kernel_class.h).

A class is written (base, tex, media, mats, leaf, deep): base "flat" / "bvh" / "inst", tex 0 / 1 / 2,
media 0 / 1 (query chain) / 2 (events in the shading phase), mats and deep (the 512-lane twin) as
booleans, leaf 0 / 1 (triangles) / 2 (spheres).  `scene_of(cls)` builds its scene from the public
constructors alone and sets no RT_AMD_* knob: the class follows from the scene, as for a caller.  The
levers, read from rt_build.cpp and rt_bvh.cpp:

  flat    every set has at most RT_FLAT_MAX = 32 leaves and the scene at most RT_LDS_PRIMS_MAX = 256
          primitives, no prefix (at most 48 surface leaves), no instance: 12 items, a moving sphere, a
          cuboid and a floor quad
  bvh     more than RT_FLAT_MAX + RT_PREFIX_MAX = 48 surface leaves: a grid of 64 items
  leaf    all-static triangles 1 (the floor is two triangles, whether the prefix takes them or not),
          all-static spheres 2 (a ground sphere of radius 100), spheres and triangles alternating 0 (a
          floor quad, which the prefix takes)
  tex     1: two checker textures (on a sphere and a triangle where the leaf class has both: both uv
          maps); 2: one checker, a noise and a marble item
  mats    a metal and a dielectric item; and the medium's material: isotropic with mats, a lightSource
          (a glowing fog) without, because any other medium material sets RT_VAR_MATS
  media 2 a fog sphere: a one-leaf boundary (rt_host_media_late).  Flat scenes: media 1 whatever the boundary
  media 1 the boundary is a box of 48 triangles (more than RT_FLAT_MAX leaves, so it has a BVH of its own)
          that aliases nothing
  inst    an object of 64 leaves or more (scene.INSTANCE_MIN_LEAVES) under two rigid transforms, one of them
          with a material over the placement; a floor quad and the emitter outside it
  deep    stack depth + 1 > RT_WIDE_STACK_ROWS = 23: 41 items 8^k apart along the view axis, one BVH level
          each.  A prefix would take 16 of them as outliers (RT_PREFIX_SHRINK), so a deep BVH scene has
          exactly 48 surface leaves: more than RT_FLAT_MAX, a BVH, and no prefix.  For an instanced class
          the chain is inside the object

Every scene is lit by the sky and one emitter item (a redirect target points at it), has each enabled
feature in the front row of the grid, and shows the ground below a horizon: hits and misses.
"""
import functools

import raytrace_amd as R

WIDTH, HEIGHT, SPP = 48, 32, 4
LMAX = 2.0  # the emitter item (and the glowing fog) against the sky's 1
COLS = 8
CHAIN_N, CHAIN_RATIO = 41, 8.0
FRONT = [3, 4, 2, 5, 1, 6, 0, 7]  # front-row slots from the image centre outwards

RT_VAR_FLAT, RT_VAR_BVH = 0, 2
BASES = ("flat", "bvh", "inst")


def from_fields(fields):
    """(base, tex, media, mats, leaf, deep) of rt_class_of's seven fields (emu.class_of)."""
    var, tex, media, mats, inst, leaf, narrow = fields
    assert var in (RT_VAR_FLAT, RT_VAR_BVH), fields
    return ("flat" if var == RT_VAR_FLAT else "inst" if inst else "bvh", tex, media, bool(mats), leaf, bool(narrow))


def to_fields(cls):
    base, tex, media, mats, leaf, deep = cls
    return (RT_VAR_FLAT if base == "flat" else RT_VAR_BVH, tex, media, int(mats), int(base == "inst"), leaf, int(deep))


def class_id(cls):
    base, tex, media, mats, leaf, deep = cls
    return f"{base}-t{tex}-m{media}-{'mats' if mats else 'diff'}-l{leaf}{'-deep' if deep else ''}"


def need32(cls):
    """The FP32 per-pixel bar of tests/test_gpu.py for the kind of scene: 0.97 with glass or metal in
    view, 0.98 for the deep chains, 0.99 otherwise."""
    return 0.97 if cls[3] else 0.98 if cls[5] else 0.99


def _grey(k):
    return R.lambertian(R.constantTexture((0.25 + 0.07 * (k % 9), 0.45 + 0.05 * (k % 7), 0.8 - 0.06 * (k % 10))))


def _sphere_at(x, y, z, r=0.16):
    return R.sphere((x, y + r + 0.02, z), r)


def _triangle_at(x, y, z, r=0.17):
    return R.triangle(((x - r, y + 0.02, z), (0.0, 0.0)), ((x + r, y + 0.02, z), (1.0, 0.0)),
                      ((x, y + 0.02 + 2 * r, z + 0.05), (0.5, 1.0)))


def _shape(kind, x, y, z, r=0.16):
    return _sphere_at(x, y, z, r) if kind == 2 else _triangle_at(x, y, z, r + 0.01)


def _kind(leaf, k):
    return leaf if leaf else 2 - (k + k // COLS) % 2


def _specials(tex, mats):
    """The materials of the front row: the emitter, then one or two items per enabled feature."""
    out = [R.lightSource(R.constantTexture((LMAX, 0.9 * LMAX, 0.7 * LMAX)))]
    if tex >= 1:
        out += [R.lambertian(R.checkerTexture(6, 4, (0.9, 0.2, 0.1), (0.1, 0.2, 0.9)))]
    if tex == 1:
        out += [R.lambertian(R.checkerTexture(5, 5, 0.15, 0.85))]
    if tex == 2:
        out += [R.lambertian(R.noiseTexture(2, 6.0, (3, 0, 0), 0.05, 0.95)), R.lambertian(R.marbleTexture((0, 1, 0.5), 9.0, 0.3))]
    if mats:
        out += [R.metal(0.1, R.constantTexture((0.8, 0.8, 0.9))), R.dielectric(1.5)]
    return out


def _grid(n, leaf, tex, mats, x0=-1.4, dx=0.4, z0=-0.6, dz=-0.45, y=0.0, r=0.16, back=None):
    """n items in rows of COLS from the front row back; the front row holds the special materials, on
    alternating shapes where the leaf class allows."""
    special = dict(zip(FRONT, _specials(tex, mats)))
    items = []
    for k in range(n):
        row, col = divmod(k, COLS)
        mat = special.get(k, _grey(k)) if row == 0 else _grey(k)
        kind = back if back and row > 0 and k % 5 else _kind(leaf, k)
        items.append(mat << _shape(kind, x0 + dx * col + 0.05 * (row % 2), y, z0 + dz * row, r))
    return items


def _chain(n, leaf, scale=1.0, z0=-4.0):
    """n items 8^k apart along -z (tests/query_cases.py deep_scene): one BVH level each."""
    return [_grey(k) << _shape(_kind(leaf, k), scale * 0.3 * (k % 3 - 1), 0.0, scale * (z0 - CHAIN_RATIO ** k), scale * 0.2)
            for k in range(n)]


def _ground(leaf):
    m = R.lambertian(R.constantTexture(0.5))
    if leaf == 1:  # two triangles, 40 x 40
        return [m << R.triangle(((-20, 0, -30), (0, 0)), ((20, 0, -30), (1, 0)), ((-20, 0, 10), (0, 1))),
                m << R.triangle(((20, 0, 10), (1, 1)), ((-20, 0, 10), (0, 1)), ((20, 0, -30), (1, 0)))]
    if leaf == 2:
        return [m << R.sphere((0, -100, 0), 100)]
    # (a quad where the class allows one: FP32 places a hit on a 1000-unit sphere only within 1e-4,
    # which decides grazing second segments under the small items differently from binary64)
    return [m << R.parallelogram((-20, 0, 10), (40, 0, 0), (0, 0, -40))]


def triangle_box(lo, hi, n=2):
    """The six faces of a box as 12 n^2 triangles (n = 2: 48 leaves, more than RT_FLAT_MAX)."""
    tris = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (lo[axis], hi[axis]):
            for i in range(n):
                for j in range(n):
                    def p(s, t):
                        q = [0.0, 0.0, 0.0]
                        q[axis] = side
                        q[a] = lo[a] + (hi[a] - lo[a]) * s / n
                        q[b] = lo[b] + (hi[b] - lo[b]) * t / n
                        return tuple(q)
                    c = [p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)]
                    tris.append(R.triangle((c[0], (0, 0)), (c[1], (1, 0)), (c[2], (1, 1))))
                    tris.append(R.triangle((c[0], (0, 0)), (c[2], (1, 1)), (c[3], (0, 1))))
    return R.group(tris)


def _medium(base, media, mats):
    if not media:
        return []
    mat = R.isotropic(R.constantTexture((0.9, 0.8, 0.7))) if mats else R.lightSource(R.constantTexture((0.6, 0.9, 1.4)))
    if media == 2 or base == "flat":
        return [mat << R.constantMedium(2.5, R.sphere((0.45, 0.42, 0.3), 0.36))]
    return [mat << R.constantMedium(2.5, triangle_box((-0.8, 0.05, 0.1), (-0.2, 0.65, 0.7)))]


def _object(leaf_mix, tex, mats, deep):
    """The instanced object: a grid of small items in object space around the origin, the special
    materials on its front row, and for a deep class the chain (scaled to the object)."""
    n = 24 if deep else 64
    items = _grid(n, leaf_mix, tex, mats, x0=-0.7, dx=0.2, z0=0.65, dz=-0.19, y=0.0, r=0.075, back=1)
    if deep:
        items += _chain(CHAIN_N, leaf_mix, scale=0.3, z0=-2.0)
    return R.group(items)


@functools.lru_cache(maxsize=None)
def scene_of(cls):
    """(settings, world, seed, lmax) of a class (base, tex, media, mats, leaf, deep)."""
    base, tex, media, mats, leaf, deep = cls
    assert base in BASES and tex in (0, 1, 2) and media in (0, 1, 2) and leaf in (0, 1, 2), cls
    if base == "flat":
        assert leaf == 0 and not deep and media != 2, cls
        objs = _grid(12, 0, tex, mats)
        objs.append(_grey(20) << R.moving((0, 0, 0), (0.25, 0.1, 0), R.sphere((-1.1, 0.5, -1.6), 0.2)))
        objs.append(_grey(21) << R.cuboid(R.fromCorners((0.9, 0.0, -1.9), (1.4, 0.55, -1.5))))
        floor = R.lambertian(R.checkerTexture(16, 16, 0.3, 0.7)) if tex else R.lambertian(R.constantTexture(0.5))
        objs.append(floor << R.parallelogram((-20, 0, 10), (40, 0, 0), (0, 0, -40)))
    elif base == "bvh":
        if deep:  # 1 + 6 + 41 = 48 surface leaves: a BVH (more than RT_FLAT_MAX) and no prefix to take the chain's far end
            big = R.triangle(((-60, 0, 10), (0, 0)), ((60, 0, 10), (1, 0)), ((0, 0, -100), (0.5, 1)))
            ground = [R.lambertian(R.constantTexture(0.5)) << big] if leaf == 1 else _ground(leaf)
            objs = ground + _grid(6, leaf, tex, mats, x0=-1.0) + _chain(CHAIN_N, leaf)
        else:
            objs = _ground(leaf) + _grid(64, leaf, tex, mats)
    else:
        assert leaf == 0, cls
        obj = _object(0, tex, mats, deep)
        objs = _ground(0) + [
            R.transform(R.translate((-0.65, 0.05, -0.9)) @ R.rotateY(R.degrees(18)), obj),
            (R.metal(0.05, R.constantTexture(0.85)) if mats else R.lambertian(R.constantTexture((0.8, 0.5, 0.2))))
            << R.transform(R.translate((0.7, 0.35, -1.4)) @ R.rotateY(R.degrees(-30)) @ R.rotateX(R.degrees(25)), obj),
            R.lightSource(R.constantTexture((LMAX, 0.9 * LMAX, 0.7 * LMAX))) << R.sphere((0.0, 0.9, -1.6), 0.2),
        ]
    objs += _medium(base, media, mats)
    target = (0.15, (-0.3, 0.0, -0.8), (0.6, 0.0, 0.0), (0.0, 0.5, 0.0))  # around the emitter item
    if base == "inst":
        target = (0.15, (-0.25, 0.65, -1.6), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0))
    cs = R.defaultCameraSettings(cs_imageWidth=WIDTH, cs_aspectRatio=WIDTH / HEIGHT, cs_samplesPerPixel=SPP,
                                 cs_maxRecursionDepth=12, cs_background=R.sky, cs_vfov=R.degrees(30),
                                 cs_center=(0.0, 0.9, 2.2), cs_lookAt=(0.0, 0.3, -0.8), cs_redirectTargets=[target])
    return cs, R.group(objs), R.mkStdGen(SEEDS.get(cls, 7)), LMAX


# seeds chosen per class where the default's FP32 host render sat within a percent of its bar
SEEDS = {("bvh", tex, 0, False, 2, False): 2 for tex in (0, 1, 2)}  # (seed 7: one or two of 1536 pixels off)


# ---- the argument space of the scalar rt_host_variant, and the classes it reaches
DEEP_STACK, SHALLOW_STACK = 30, 6


def enumerate_variants():
    """Every argument tuple of rt_host_variant a scene can produce: flat x media x {tex 0, 1, noise} x
    mats x inst x leaf kind x media_late x {shallow, deep}; a flat scene has no instance, leaf class,
    late media or deep stack; late needs a medium."""
    out = []
    for flat in (0, 1):
        for n_media in (0, 1):
            for tex, noise in ((0, 0), (1, 0), (0, 1), (1, 1)):
                for mats in (0, 1):
                    for inst in (0, 1):
                        for leaf_kind in (0, 1, 2):
                            for late in (0, 1):
                                for deep in (0, 1):
                                    if flat and (inst or leaf_kind or late or deep):
                                        continue
                                    if late and not n_media:
                                        continue
                                    out.append((flat, n_media, noise, mats, tex, inst, leaf_kind, late,
                                                DEEP_STACK if deep else SHALLOW_STACK))
    return out


@functools.lru_cache(maxsize=None)
def enumerated_classes(precision):
    """The distinct classes (sorted) the variants of enumerate_variants dispatch to in one precision,
    as {cls: (fields, block, compiled)}."""
    import emu
    found = {}
    for args in enumerate_variants():
        fields, block, compiled = emu.class_of(precision, emu.variant_of(*args))
        found[from_fields(fields)] = (fields, block, compiled)
    return dict(sorted(found.items(), key=lambda kv: (BASES.index(kv[0][0]),) + kv[0][1:]))


# classes no scene can produce, with the reason read from the builder (expected to stay empty)
UNREACHABLE = {}


def all_cases():
    """[(cls, precision)] of every dispatchable class, for parametrised tests."""
    return [(c, p) for p in ("f64", "f32") for c in enumerated_classes(p) if (c, p) not in UNREACHABLE]
