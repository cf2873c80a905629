"""What progressive passes cost against one launch: Cornell 600x600 in binary64, 8 film passes of
25 samples (render + merge each, then one resolve) against one rt_render_async of 200 samples
planned to run alone (RT_EXEC_SOLO), both on one stream and timed with HIP events.

    python tools/film_overhead.py [--reps 20] [--out overhead.json]            # the timings
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/film_overhead.py --reps 3 --noise
                                                                                 # kernel times

Prints one JSON line (and writes it to --out): ms per frame of both ways (median, min, max over
--reps), their ratio, and the bytes each HBM-bound kernel moves per launch (merge: the pass sums
and flag read, the totals, flags and q read and written; noise: high words, flag and q read;
resolve: sums and flag read, the image written), to set a trace's kernel times against.  The
images of the two ways are compared bit for bit.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--batch", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--noise", action="store_true", help="also run the noise kernel once per frame (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytrace_amd as R
    from raytrace_amd import scenes

    spp = args.passes * args.batch
    cs, world, seed = scenes.cornell_box(spp=spp, width=args.width)
    h, w = R.image_height(cs), args.width
    dt = torch.float64 if args.precision == "f64" else torch.float32
    dev = R.DeviceScene(world)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    out_one = torch.zeros(h * w * 3, dtype=dt, device="cuda")
    out_film = torch.zeros(h * w * 3, dtype=dt, device="cuda")
    film = R.Film(dev, cs, seed, precision=args.precision)

    def one_shot():
        dev.render_async(cs, seed, out_one.data_ptr(), sp, precision=args.precision, solo=True)

    def progressive():
        for _ in range(args.passes):
            film.add(args.batch, sp)
        R._lib.check(film._lib.rt_film_resolve(film.handle, out_film.data_ptr(), sp))

    def timed(fn):
        if fn is progressive:
            film.reset()  # (synchronous: outside the timed window)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    for fn in (one_shot, progressive) * 3:  # warm-up: code objects, the precision's upload
        timed(fn)
    a, b = [], []
    for _ in range(args.reps):  # alternating, so both see the same machine
        a.append(timed(one_shot))
        b.append(timed(progressive))
        if args.noise:
            film.noise()
    same = bool(torch.equal(out_one, out_film))
    n = h * w
    words = 6 if args.precision == "f64" else 3
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))  # noqa: E731
    rec = dict(workload=f"cornell {w}x{h} {args.precision}, {args.passes} passes of {args.batch} against one launch of {spp} (solo)",
               reps=args.reps, one_shot_ms=stat(a), film_ms=stat(b), ratio=float(np.median(b) / np.median(a)),
               extra_ms_per_pass=float((np.median(b) - np.median(a)) / args.passes), images_equal=same,
               bytes=dict(merge=n * (3 * 8 * words + 3 * 4 + 2 * 8), noise=n * (3 * 8 + 4 + 8),
                          resolve=n * (8 * words + 4 + 3 * out_one.element_size())))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    film.close()
    dev.close()
    assert same, "the film's image differs from the one-shot render"


if __name__ == "__main__":
    main()
