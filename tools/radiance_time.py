"""What a radiance query costs: rt_scene_radiance_async on a scene's own camera rays against
Film.add at the same count, HIP events on one stream, warm.

    python tools/radiance_time.py [--samples 16] [--reps 7] [--out radiance_time.json]

Per scene (the Cornell box 600 x 600, bunny-Cornell and pawn+fog at 400 wide) and precision:
  film      Film.add(samples): the render kernels' pass and its merge
  rows      radiance_async(samples) on camera_rays(sample 0) in row order (workspace memset, path
            kernel, resolve): every sample of a ray starts from that one ray
  shuffled  the same rays in a random order (no coherence inside a wave)
each the median (minimum .. maximum) of --reps timed calls after two warm-up calls, alternating, in
ms and Msamples/s, and the two query rates as fractions of the film's.  Prints one JSON line per row;
profiles/radiance/README.md holds a recorded run.  Nothing here is asserted by a test.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytrace_amd as R
    from raytrace_amd import radiance as rad
    from raytrace_amd import scenes

    cases = {"cornell": lambda: scenes.cornell_box(width=600, spp=1),
             "bunny_cornell": lambda: scenes.bunny_cornell(width=400, spp=1),
             "pawn_fog": lambda: scenes.pawn_fog(width=400, spp=1)}
    st = torch.cuda.Stream()

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        with torch.cuda.stream(st):
            ev[0].record(st)
            fn()
            ev[1].record(st)
        st.synchronize()
        return ev[0].elapsed_time(ev[1])

    rows = []
    for name, make in cases.items():
        cs, world, seed = make()
        scene = R.DeviceScene(world)
        for precision in ("f64", "f32"):
            rays = scene.camera_rays(cs, seed, 0, precision)
            n = len(rays)
            perm = np.random.default_rng(1).permutation(n)
            d_rays = {k: torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).reshape(-1).copy()).cuda()
                      for k, r in (("rows", rays), ("shuffled", rays[perm]))}
            d_out = torch.zeros(n * rad.RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_work = torch.zeros(rad.workspace_bytes(n, precision), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with R.Film(scene, cs, seed, precision=precision) as f:
                calls = {"film": lambda: f.add(args.samples, st.cuda_stream)}
                for k in d_rays:
                    calls[k] = (lambda k=k: scene.radiance_async(d_rays[k].data_ptr(), d_out.data_ptr(), d_work.data_ptr(), n,
                                                                args.samples, cs, seed, st.cuda_stream, unit_dir=True,
                                                                precision=precision))
                ms = {k: [] for k in calls}
                for rep in range(args.reps + 2):
                    for k, fn in calls.items():
                        t = timed(fn)
                        if rep >= 2:
                            ms[k].append(t)
                    f.reset()
            row = dict(scene=name, precision=precision, rays=n, samples=args.samples)
            for k, v in ms.items():
                med = float(np.median(v))
                row[k] = dict(ms=round(med, 4), min=round(min(v), 4), max=round(max(v), 4),
                              msamples_s=round(n * args.samples / med / 1e3, 1))
            for k in d_rays:
                row[k]["of_film"] = round(row[k]["msamples_s"] / row["film"]["msamples_s"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
        scene.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
