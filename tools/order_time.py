"""What ordering a ray batch buys: the ordered queries (rt_scene_cast_ordered_async,
rt_scene_radiance_ordered_async) and the order call (rt_scene_ray_order_async) against the unordered
calls on incoherent rays, HIP events on one stream, warm.

    python tools/order_time.py [--reps 7] [--samples 16] [--scenes bunny_cornell,instance_gallery,pawn_fog]
                               [--unordered-only] [--keys-dir DIR] [--out order_time.json]

Per scene, ray sets of 1024 x 1024 rays for the casts:
  incoherent  tools/query_time.py's random rays (origins in the inflated bounding box, aimed at the box)
  shuffled    a pinhole grid from the scene's camera in a random order
and for the radiance queries (--samples samples) the scene's own camera rays at 400 pixels wide,
shuffled.  Casts: closest hit with uv / any hit, binary64 / FP32.  Rows per case, each the median
(minimum .. maximum) of --reps timed calls after two warm-up calls, in ms:
  a  the unordered call on the set
  b  the order call alone (key, sort; the same for every precision and query of a set)
  c  the ordered call with a ready order
  d  b + c
  e  the unordered call on the same rays in their coherent order (the pinhole grid / the camera rays
     row-major; the incoherent set has none)
--unordered-only times rows a and e alone, through calls that a library without the ordered entry
points has too (the parent's side of an A/B run).  `sort`: the radix sort alone
(rt_order_sort_keys_async) on 2^20 and 2^16 random 30-bit keys; --keys-dir writes those key sets as
keys_<n>.bin for tools/rocprim_sort_time.hip.  Prints one JSON line per row; profiles/order/README.md
holds a recorded run.  Nothing here is asserted by a test.
"""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--scenes", default="bunny_cornell,instance_gallery,pawn_fog")
    ap.add_argument("--unordered-only", action="store_true")
    ap.add_argument("--keys-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytrace_amd as R
    from raytrace_amd import _lib, query, scenes
    from raytrace_amd import radiance as rad

    st = torch.cuda.Stream()
    sp = st.cuda_stream
    P = ctypes.c_void_p

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def timed(calls):
        """{name: fn} -> {name: dict(ms, min, max)}, the calls alternating"""
        ms = {k: [] for k in calls}
        for rep in range(args.reps + 2):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    fn()
                    e1.record(st)
                st.synchronize()
                if rep >= 2:
                    ms[k].append(e0.elapsed_time(e1))
        return {k: dict(ms=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in ms.items()}

    def unit(v):
        v = np.asarray(v, float)
        return v / np.linalg.norm(v)

    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    side = args.side
    n = side * side
    for name in [s for s in args.scenes.split(",") if s]:
        cs, world, seed = getattr(scenes, name)()
        scene = R.DeviceScene(world)
        # ---- casts
        c = np.array(cs.cs_center, float)
        w = unit(np.array(cs.cs_lookAt, float) - c)
        u = unit(np.cross(w, np.array(cs.cs_up, float)))
        v = np.cross(u, w)
        half = math.tan(0.5 * float(cs.cs_vfov))
        g = (np.arange(side) + 0.5) / side * 2 - 1
        d = w[None, None] + half * g[None, :, None] * u[None, None] - half * g[:, None, None] * v[None, None]
        grid = query.make_rays(c, d.reshape(-1, 3))
        lo = np.array([b[0] for b in world.bbox])
        hi = np.array([b[1] for b in world.bbox])
        rng = np.random.default_rng(11)
        o = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3))
        sets = {"incoherent": (query.make_rays(o, rng.uniform(lo, hi, (n, 3)) - o), None),
                "shuffled": (grid[np.random.default_rng(1).permutation(n)], grid)}
        d_hits = torch.zeros(n * query.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        for set_name, (rays, coherent) in sets.items():
            d_rays = dev(rays)
            d_coh = dev(coherent) if coherent is not None else None
            b_row = None
            if not args.unordered_only:
                d_order = torch.zeros(n, dtype=torch.int32, device="cuda")
                d_ws = torch.zeros(scene.ray_order_workspace_bytes(n), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                b_row = timed({"b": lambda: scene.ray_order_async(d_rays.data_ptr(), n, d_order.data_ptr(), d_ws.data_ptr(), sp)})["b"]
            for precision in ("f64", "f32"):
                for any_hit in (False, True):
                    kw = dict(precision=precision, any_hit=any_hit)
                    calls = {"a": lambda: scene.cast_async(d_rays.data_ptr(), d_hits.data_ptr(), n, sp, **kw)}
                    if d_coh is not None:
                        calls["e"] = lambda: scene.cast_async(d_coh.data_ptr(), d_hits.data_ptr(), n, sp, **kw)
                    if not args.unordered_only:
                        calls["c"] = lambda: scene.cast_async(d_rays.data_ptr(), d_hits.data_ptr(), n, sp,
                                                              order_ptr=d_order.data_ptr(), **kw)
                    row = dict(kind="cast", scene=name, set=set_name, precision=precision, query="any" if any_hit else "closest",
                               rays=n, **timed(calls))
                    if b_row:
                        row["b"] = b_row
                        row["d"] = dict(ms=round(b_row["ms"] + row["c"]["ms"], 4))
                    emit(row)
        assert not scene.cast_overflowed()
        # ---- radiance queries on the scene's camera rays, 400 wide
        rcs = cs.replace(cs_imageWidth=400, cs_samplesPerPixel=1)
        for precision in ("f64", "f32"):
            cam = scene.camera_rays(rcs, seed, 0, precision)
            m = len(cam)
            d_cam, d_shuf = dev(cam), dev(cam[np.random.default_rng(1).permutation(m)])
            d_out = torch.zeros(m * rad.RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_work = torch.zeros(rad.workspace_bytes(m, precision), dtype=torch.uint8, device="cuda")
            kw = dict(unit_dir=True, precision=precision)

            def run(d_r, **more):
                scene.radiance_async(d_r.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), m, args.samples, rcs, seed, sp, **kw, **more)

            calls = {"a": lambda: run(d_shuf), "e": lambda: run(d_cam)}
            if not args.unordered_only:
                d_order = torch.zeros(m, dtype=torch.int32, device="cuda")
                d_ws = torch.zeros(scene.ray_order_workspace_bytes(m), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                calls["b"] = lambda: scene.ray_order_async(d_shuf.data_ptr(), m, d_order.data_ptr(), d_ws.data_ptr(), sp, path_rays=True)
                calls["c"] = lambda: run(d_shuf, order_ptr=d_order.data_ptr())
            torch.cuda.synchronize()
            row = dict(kind="radiance", scene=name, set="shuffled", precision=precision, rays=m, samples=args.samples, **timed(calls))
            if "c" in row:
                row["d"] = dict(ms=round(row["b"]["ms"] + row["c"]["ms"], 4))
            emit(row)
        assert not scene.radiance_overflowed()
        scene.close()
    # ---- the sort alone
    if not args.unordered_only:
        L = _lib.load()
        for bits in (20, 16):
            k = 1 << bits
            keys = np.random.default_rng(bits).integers(0, 1 << 30, k).astype(np.uint32)
            if args.keys_dir:
                os.makedirs(args.keys_dir, exist_ok=True)
                keys.tofile(os.path.join(args.keys_dir, f"keys_{k}.bin"))
            d_keys = dev(keys)
            d_order = torch.zeros(k, dtype=torch.int32, device="cuda")
            d_ws = torch.zeros(int(L.rt_ray_order_workspace_bytes(k)), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t = timed({"sort": lambda: _lib.check(L.rt_order_sort_keys_async(0, P(d_keys.data_ptr()), k, P(d_order.data_ptr()),
                                                                              P(d_ws.data_ptr()), P(sp)))})
            assert (d_order.cpu().numpy().view(np.uint32) == np.argsort(keys, kind="stable")).all()
            emit(dict(kind="sort", pairs=k, **t))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
