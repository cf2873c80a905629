"""What the film's feature pass and denoiser cost: Cornell 600x600, HIP events on one stream, warm.

    python tools/denoise_time.py [--reps 20] [--precision f64] [--out denoise_time.json]

Times (median, min, max over --reps, alternating so every figure sees the same machine):
  add8        film.add(8): one pass of 8 samples and its merge
  frame200    one rt_render_async of 200 samples planned to run alone (RT_EXEC_SOLO)
  features8   rt_denoise_features(8): the first-hit pass (its memset included)
  albedo64    rt_denoise_albedo(64): the same pass over 64 samples, the remodulation albedo (once per film)
  denoise[L]  rt_denoise_film at levels = 1..5 into a device buffer: prepare + L levels + finish, so
              level i alone is denoise[i + 1] - denoise[i]
and prints one JSON line with them, features8 and denoise[5] as fractions of add8 and frame200, and
the bytes each denoise kernel moves per launch if every tap came from memory once per pixel
(prepare: sums, q and both feature buffers read, 15 planes written; a level: 4 planes + flags read once
for the LDS kernels' tiles, 8 guide planes read, 4 planes written — the taps' re-reads are cache
hits; finish: 6 planes + flags read, the image written), to set against HBM / L2 rates.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ctypes

    import numpy as np
    import torch

    import raytrace_amd as R
    from raytrace_amd import denoise, scenes

    cs, world, seed = scenes.cornell_box(spp=200, width=args.width)
    h, w = R.image_height(cs), args.width
    dt = torch.float64 if args.precision == "f64" else torch.float32
    dev = R.DeviceScene(world)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    out = torch.zeros(h * w * 3, dtype=dt, device="cuda")
    film = R.Film(dev, cs, seed, precision=args.precision)
    L = film._lib
    film.add(4, sp), film.add(4, sp)
    params = {n: denoise.params_struct(levels=n) for n in range(1, 6)}

    def add8():
        film.add(8, sp)

    def frame200():
        dev.render_async(cs, seed, out.data_ptr(), sp, precision=args.precision, solo=True)

    def features8():
        R._lib.check(L.rt_denoise_features(film.handle, 8, ctypes.c_void_p(sp)))

    def albedo64():
        R._lib.check(L.rt_denoise_albedo(film.handle, 64, ctypes.c_void_p(sp)))

    def dn(n):
        return lambda: R._lib.check(L.rt_denoise_film(film.handle, ctypes.byref(params[n]), out.data_ptr(), ctypes.c_void_p(sp)))

    jobs = dict(add8=add8, frame200=frame200, features8=features8, albedo64=albedo64, **{f"denoise{n}": dn(n) for n in range(1, 6)})

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    features8()
    albedo64()
    for _ in range(3):  # warm-up: code objects, the lazily allocated buffers
        for fn in jobs.values():
            timed(fn)
    t = {k: [] for k in jobs}
    for _ in range(args.reps):
        if film.spp > (1 << 23):
            film.reset(), film.add(4, sp), film.add(4, sp)
        for k, fn in jobs.items():
            t[k].append(timed(fn))
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))  # noqa: E731
    med = {k: float(np.median(v)) for k, v in t.items()}
    n = h * w
    words = 6 if args.precision == "f64" else 3
    fw = 16 if args.precision == "f64" else 8
    rec = dict(workload=f"cornell {w}x{h} {args.precision}", reps=args.reps, ms={k: stat(v) for k, v in t.items()},
               level_ms=[med["denoise1"]] + [med[f"denoise{i + 1}"] - med[f"denoise{i}"] for i in range(1, 5)],
               features8_over_add8=med["features8"] / med["add8"], features8_over_frame200=med["features8"] / med["frame200"],
               albedo64_over_add8=med["albedo64"] / med["add8"], albedo64_over_frame200=med["albedo64"] / med["frame200"],
               denoise5_over_add8=med["denoise5"] / med["add8"], denoise5_over_frame200=med["denoise5"] / med["frame200"],
               bytes=dict(prepare=n * (8 * words + 8 + 2 * 8 * fw + 15 * 8), level=n * (4 * 8 + 4 + 8 * 8 + 4 * 8),
                          finish=n * (6 * 8 + 4 + 3 * out.element_size())))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    film.close()
    dev.close()


if __name__ == "__main__":
    main()
