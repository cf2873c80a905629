"""What a pass of a multi-device film costs against a plain film's: Cornell 600x600, passes of 16
samples, in binary64 and FP32.

    python tools/multi_film_overhead.py [--runs 7] [--passes 8] [--out overhead.json]

Configurations: (a) Film.add(16) — the yardstick —, (b) MultiFilm([0]), (c) MultiFilm([0, 0]) — two
shards sharing one GPU: a functional figure only — and, where the machine has more GPUs, (d)
MultiFilm([0, 1, ...]).  A run is --passes passes enqueued back to back and one wait for all of
them (a host clock around both: Film on a stream of its own that is then synchronised, MultiFilm by
rt_multi_film_frame), after a reset outside the timed window; runs of the configurations alternate,
so all see the same machine.  Prints one JSON line per precision (and writes them to --out): ms per
pass of every configuration (median, min, max over --runs, after two warm-up runs) and the bytes a
merge moves.  The images of all configurations are compared bit for bit.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytrace_amd as R
    from raytrace_amd import scenes
    from raytrace_amd.scene import flatten

    cs, world, seed = scenes.cornell_box(spp=args.batch, width=args.width)
    flat = flatten(world)
    h, w = R.image_height(cs), args.width
    n_gpus = torch.cuda.device_count()
    stream = torch.cuda.Stream()
    lines = []
    for precision in ("f64", "f32"):
        films = {"a_film": R.Film(flat, cs, seed, precision=precision),
                 "b_multi_0": R.MultiFilm(flat, cs, seed, devices=[0], precision=precision),
                 "c_multi_0_0": R.MultiFilm(flat, cs, seed, devices=[0, 0], precision=precision)}
        if n_gpus > 1:
            films[f"d_multi_{n_gpus}_gpus"] = R.MultiFilm(flat, cs, seed, devices=list(range(n_gpus)), precision=precision)

        def run(f):
            f.reset()  # (synchronous: outside the timed window)
            t0 = time.perf_counter()
            if isinstance(f, R.MultiFilm):
                for _ in range(args.passes):
                    f.add(args.batch)
                f._frame()
            else:
                for _ in range(args.passes):
                    f.add(args.batch, stream.cuda_stream)
                stream.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.passes

        ms = {k: [] for k in films}
        for i in range(2 + args.runs):
            for k, f in films.items():
                t = run(f)
                if i >= 2:
                    ms[k].append(t)
        images = {k: f.image() for k, f in films.items()}
        same = all(np.array_equal(images["a_film"], v, equal_nan=True) for v in images.values())
        for f in films.values():
            f.close()
        words = 6 if precision == "f64" else 3
        stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))  # noqa: E731
        rec = dict(workload=f"cornell {w}x{h} {precision}, passes of {args.batch} samples, {args.passes} per run",
                   runs=args.runs, gpus=n_gpus, ms_per_pass={k: stat(v) for k, v in ms.items()},
                   b_over_a=float(np.median(ms["b_multi_0"]) / np.median(ms["a_film"])), images_equal=same,
                   merge_bytes=h * w * (3 * 8 * words + 3 * 4 + 2 * 8))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        assert same, "a multi-device film's image differs from the plain film's"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
