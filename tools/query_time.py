"""What a batched ray query costs: Mrays/s of rt_scene_cast_async on resident buffers.

    python tools/query_time.py [--rays 1048576] [--reps 7] [--scenes cornell_box,bunny_cornell,instance_gallery]
                               [--out query_time.json]

Per scene (cornell_box: the flat class; bunny_cornell: the triangle BVH; instance_gallery: instancing),
precision (binary64, FP32) and query (closest hit with uv, any hit), two ray sets of --rays rays:
  coherent    a pinhole grid from the scene's camera centre (its look-at and field of view, square),
              row-major: a wave's 64 rays are 64 neighbouring pixels of a row
  incoherent  the tests' random rays: origins uniform in the scene's bounding box inflated by a
              quarter of its extent, each aimed at a uniform point of the box, default_rng(11)
The kernel traces rays in the caller's order (one lane per ray, no sorting): the two sets are the two
ends of what a caller's coherence does to the rate.  HIP events on one stream around the call alone
(the rays and hits stay on the device), 2 warm-up calls, the median, minimum and maximum of --reps.

For scale, `features`: rt_denoise_features(n_feat = 1) of a square film of the same number of pixels
from the same camera — the feature pass's primary rays per second, a query plus a texture lookup and
64-bit atomic adds (its memset included), timed in the same session the same way.

Prints one JSON line; nothing is asserted.
"""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def unit(v):
    import numpy as np
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="cornell_box,bunny_cornell,instance_gallery")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytrace_amd as R
    from raytrace_amd import query, scenes

    side = int(math.isqrt(args.rays))
    n = side * side
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def timed(fn):
        for _ in range(2):
            fn()
        stream.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))

    def rate(t):  # Mrays/s at the median, and the run-to-run range
        return dict(mrays=n / t["median"] / 1e3, lo=n / t["max"] / 1e3, hi=n / t["min"] / 1e3, ms=t["median"])

    rec = dict(rays=n, reps=args.reps, scenes={})
    for name in args.scenes.split(","):
        cs, world, seed = getattr(scenes, name)()
        scene = R.DeviceScene(world)
        # coherent: a pinhole grid
        c = np.array(cs.cs_center, float)
        w = unit(np.array(cs.cs_lookAt, float) - c)
        u = unit(np.cross(w, np.array(cs.cs_up, float)))
        v = np.cross(u, w)
        half = math.tan(0.5 * float(cs.cs_vfov))
        g = (np.arange(side) + 0.5) / side * 2 - 1
        d = w[None, None] + half * g[None, :, None] * u[None, None] - half * g[:, None, None] * v[None, None]
        sets = {"coherent": query.make_rays(c, d.reshape(-1, 3))}
        # incoherent: the tests' random rays
        lo = np.array([b[0] for b in world.bbox])
        hi = np.array([b[1] for b in world.bbox])
        rng = np.random.default_rng(11)
        o = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3))
        sets["incoherent"] = query.make_rays(o, rng.uniform(lo, hi, (n, 3)) - o)
        d_hits = torch.zeros(n * query.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        out = {}
        for kind, rays in sets.items():
            d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
            for precision in ("f64", "f32"):
                for any_hit in (False, True):
                    t = timed(lambda: scene.cast_async(d_rays.data_ptr(), d_hits.data_ptr(), n, sp, precision=precision,
                                                       any_hit=any_hit))
                    hits = d_hits.cpu().numpy().view(query.HIT_DTYPE)
                    out[f"{kind}_{precision}_{'any' if any_hit else 'closest'}"] = dict(rate(t), hit_share=float((hits["hit"] == 1).mean()))
        # the feature pass's primary rays on the same camera, one sample per pixel
        fcs = cs.replace(cs_imageWidth=side, cs_aspectRatio=1.0, cs_samplesPerPixel=1)
        for precision in ("f64", "f32"):
            film = R.Film(scene, fcs, seed, precision=precision)
            L = film._lib
            t = timed(lambda: R._lib.check(L.rt_denoise_features(film.handle, 1, ctypes.c_void_p(sp))))
            out[f"features_{precision}"] = rate(t)
            film.close()
        assert not scene.cast_overflowed()
        rec["scenes"][name] = out
        print(name, {k: round(v["mrays"], 1) for k, v in out.items()}, file=sys.stderr, flush=True)
        scene.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
