"""What adaptive film passes buy and cost (profiles/adaptive/README.md).

    python tools/adaptive_measure.py [--out bench_out/adaptive_measure.json]

cost     Cornell box 600 x 600, both precisions, a film after add(8), add(8): HIP events around
         Film.add_where(16, t) alone for thresholds whose selections are about 1, 3, 10, 20, 50 and
         100 % of the pixels (t: the value the film holds whose selection is nearest the share; ties
         move it), against Film.add(16) timed the same way in the same session; the state is restored
         before every call, 2 warm-up calls, the median of 7.  At 10 and 100 % also with the list
         kernel's chunk fixed (RT_AMD_LIST_CHUNK = 1, 2, 4, 16).
quality  Cornell box 96 px and bunny-Cornell 80 px in binary64 against `raytrace` at 4096 spp:
         `uniform_passes` uniform passes of `batch`, then add_where(batch, t, 1024) until a pass selects
         nothing, for t = 0.2, 0.1, 0.05; the RMSE of that frame over the RMSE of a uniform frame at the
         same mean sample count (the two neighbouring integer counts, interpolated in 1 / spp).

Prints one JSON line per row and writes them all to --out; nothing is asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import raytrace_amd as R  # noqa: E402
from raytrace_amd import film, scenes  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

OUT = os.path.join(ROOT, "bench_out", "adaptive_measure.json")
res = {"quality": [], "cost": []}


def dump():
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def rel_rmse(a, b):
    """RMS over the pixels of the luminance error relative to max(reference, 3 / 256): the selection's own measure"""
    d = (a.astype(np.float64) - b.astype(np.float64)).sum(-1) / np.maximum(b.astype(np.float64).sum(-1), 3.0 / 256.0)
    return float(np.sqrt(np.mean(d * d)))


def quality(name, fn, width, thresholds, batch=8, max_spp=1024, warm=2):
    cs, world, seed = fn(width=width, spp=1)
    flat = flatten(world)
    t0 = time.time()
    ref = R.raytrace(cs.replace(cs_samplesPerPixel=4096), flat, seed, precision="f64")
    print(name, "reference 4096 spp", round(time.time() - t0, 2), "s", flush=True)
    for t in thresholds:
        with R.Film(flat, cs, seed) as f:
            for _ in range(warm):
                f.add(batch)
            sel = []
            while True:
                f.add_where(batch, t, max_spp)
                k = f.adaptive_info()["selected"]
                if not k:
                    break
                sel.append(k)
            img = f.image()
            n = f.sample_map()
            info = f.adaptive_info()
        mean = float(n.mean())
        rows, rel_rows = {}, {}
        for spp in sorted({int(np.floor(mean)), int(np.ceil(mean))}):
            with R.Film(flat, cs, seed) as u:
                uimg = u.add(spp).image()
                rows[spp] = rmse(uimg, ref)
                rel_rows[spp] = rel_rmse(uimg, ref)
        # the uniform RMSE at the adaptive frame's mean count, interpolated in 1 / spp between the neighbours
        lo, hi = min(rows), max(rows)
        if lo == hi:
            uni = rows[lo]
        else:
            w = (1.0 / mean - 1.0 / hi) / (1.0 / lo - 1.0 / hi)
            uni = float(np.sqrt(w * rows[lo] ** 2 + (1 - w) * rows[hi] ** 2))
        rec = dict(scene=name, width=width, threshold=t, batch=batch, uniform_passes=warm, max_spp=max_spp, adaptive_passes=len(sel),
                   spp_min=int(n.min()), spp_mean=mean, spp_max=int(n.max()), total_samples=info["total_samples"],
                   rmse_adaptive=rmse(img, ref), rmse_uniform_floor_ceil={str(k): v for k, v in rows.items()},
                   rmse_uniform_at_mean=uni, ratio=rmse(img, ref) / uni,
                   rel_rmse_adaptive=rel_rmse(img, ref), rel_rmse_uniform_floor_ceil={str(k): v for k, v in rel_rows.items()})
        print(json.dumps(rec), flush=True)
        res["quality"].append(rec)
        dump()


def cost(precision, width=600, n=16, reps=7):
    cs, world, seed = scenes.cornell_box(width=width, spp=1)
    flat = flatten(world)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with R.Film(flat, cs, seed, precision=precision) as f:
        f.add(8).add(8)
        base = f.state().copy()
        st = film.unpack_state(base)
        r = film.noise_from_counts(st["sums"], st["q"], np.broadcast_to(np.array((16, 2), np.uint32), st["q"].shape + (2,)))
        pixels = r.size

        def timed(call):
            ms = []
            for i in range(reps + 2):  # two warm-up rounds
                f.restore(base)
                torch.cuda.synchronize()
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
            return ms

        ms = timed(lambda: f.add(n))
        rec = dict(precision=precision, width=width, what="Film.add", n=n, selected=pixels, share=1.0, ms=ms,
                   median_ms=statistics.median(ms), msamples_per_s=pixels * n / statistics.median(ms) / 1e3)
        print(json.dumps(rec), flush=True)
        res["cost"].append(rec)
        vals = np.unique(r)
        above = r.size - np.searchsorted(np.sort(r.ravel()), vals, side="right")  # pixels with r > vals[i]
        for share in (0.01, 0.03, 0.1, 0.2, 0.5, 1.0):
            for chunk in ((0,) if share not in (0.1, 1.0) else (0, 1, 2, 4, 16)):
                if chunk:
                    os.environ["RT_AMD_EXPERIMENTS"] = "1"
                    os.environ["RT_AMD_LIST_CHUNK"] = str(chunk)
                else:
                    os.environ.pop("RT_AMD_EXPERIMENTS", None)
                    os.environ.pop("RT_AMD_LIST_CHUNK", None)
                # the threshold (a value the film holds) whose selection is nearest the share
                t = -1.0 if share == 1.0 else float(vals[np.argmin(np.abs(above - share * r.size))])
                ms = timed(lambda: f.add_where(n, t))
                k = f.adaptive_info()["selected"]
                rec = dict(precision=precision, width=width, what="Film.add_where", n=n, threshold=t, selected=k,
                           share=k / pixels, chunk_knob=chunk, ms=ms, median_ms=statistics.median(ms),
                           msamples_per_s=k * n / statistics.median(ms) / 1e3)
                print(json.dumps(rec), flush=True)
                res["cost"].append(rec)
                dump()
        os.environ.pop("RT_AMD_EXPERIMENTS", None)
        os.environ.pop("RT_AMD_LIST_CHUNK", None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    OUT = ap.parse_args().out
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    for p in ("f64", "f32"):
        cost(p)
    for batch, warm in ((8, 2), (32, 2), (8, 8)):
        quality("cornell", scenes.cornell_box, 96, (0.2, 0.1, 0.05), batch=batch, warm=warm)
        quality("bunny_cornell", scenes.bunny_cornell, 80, (0.2, 0.1, 0.05), batch=batch, warm=warm)
    dump()
    print("done")
