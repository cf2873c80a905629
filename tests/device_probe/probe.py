"""Front end of the element-wise probes of rt_trace.h (TEST TOOLING): one calling convention for
the host emulator (backend "emu": tests/kernel_emu's rt_emu_probe_*, numpy arrays) and the device
(backend "gpu": tests/device_probe/rt_probe.hip's rt_probe_*, torch tensors' data_ptr()).

    call(backend, precision, name, *inputs) -> tuple of numpy outputs

`inputs` are the probe's scalar and input-array arguments in the order of probe_body.h; the
element count is that of the first input array; outputs come back as numpy arrays."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "librt_probe.so")
_lib = None

# argument kinds: ("int" | "u32") scalars, ("in", dtype, per-element width), ("out", dtype, width);
# dtype "real" is the precision's float type.  ("rec", name): one Dev* record per element as raw bytes,
# per-element width sizeof(record) in the chosen precision (tests/kernel_emu/emu.py record_dtypes(precision)
# [name]; a structured array of that dtype or its bytes).  ("table", dtype): an array of any length shared
# by all elements (dtype "bytes": records' raw bytes).  ("kp",): the call's KernelParams by value, from a
# dict: mats (DevMaterial records, one per element), med_mat, key0, key1, targets (DevTarget records),
# cfg (rem_prob, bg_kind, bg0, bg1) -- built on the host by probe_body.h pb_shade_params
SIGS = {
    "math1": [("int",), ("in", "real", 1), ("out", "real", 1)],
    "uniform": [("int",), ("in", np.uint32, 1), ("out", "real", 1)],
    "sincos": [("in", np.uint32, 1), ("out", "real", 1), ("out", "real", 1)],
    "unit_vector": [("in", np.uint32, 1), ("in", np.uint32, 1), ("out", "real", 3)],
    "philox": [("in", np.uint32, 4), ("u32",), ("u32",), ("out", np.uint32, 4)],
    "acc": [("in", "real", 1), ("out", np.int64, 1), ("out", np.uint64, 1), ("out", np.int32, 1)],
    "isect": [("int",), ("in", "real", 16), ("in", "real", 3), ("in", "real", 3), ("in", "real", 1),
              ("in", np.int32, 1), ("out", "real", 1), ("out", "real", 1), ("out", np.int32, 1)],
    "target": [("in", "real", 12), ("in", "real", 3), ("in", "real", 3), ("out", np.int32, 1), ("out", "real", 1),
               ("out", "real", 1)],
    "texture": [("rec", "texs"), ("table", "real"), ("table", np.int32), ("table", "real"), ("in", "real", 2),
                ("in", "real", 3), ("out", "real", 3)],
    "noise": [("int",), ("table", np.int32), ("table", "real"), ("in", "real", 3), ("out", "real", 1)],
    "surface": [("int",), ("in", "real", 16), ("in", "real", 6), ("table", "real"), ("in", "real", 3), ("in", "real", 3),
                ("in", "real", 1), ("out", "real", 3), ("out", "real", 3), ("out", np.int32, 1), ("out", "real", 2),
                ("out", np.int32, 1)],
    "box": [("int",), ("table", "bytes"), ("in", "real", 3), ("in", "real", 3), ("in", "real", 1), ("in", np.int32, 1),
            ("out", "real", 1), ("out", np.int32, 1), ("out", np.int32, 1)],
    "medium": [("in", np.int32, 1), ("in", np.uint32, 4), ("in", "real", 1), ("in", "real", 2), ("in", "real", 1),
               ("out", "real", 1), ("out", np.int32, 1)],
    "shade": [("int",), ("kp",), ("in", "real", 16), ("in", np.int32, 1), ("in", "real", 7), ("in", np.uint32, 3),
              ("in", "real", 6), ("out", np.int32, 1), ("out", "real", 3), ("out", "real", 3), ("out", "real", 3),
              ("out", "real", 3), ("out", np.int32, 1)],
    "node": [("in", "real", 3), ("in", "real", 3), ("in", np.float32, 6), ("in", "real", 2), ("out", np.int32, 1)],
}


def build():
    subprocess.run(["make", "-C", HERE, "-s"], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
    return _lib


def _emu_lib():
    kd = os.path.join(os.path.dirname(HERE), "kernel_emu")
    if kd not in sys.path:
        sys.path.insert(0, kd)
    import emu
    return emu.lib()


def record_size(precision, name):
    _emu_lib()
    import emu
    return emu.record_dtypes(precision)[name].itemsize


def sincos_table():
    """The (sin, cos) table of rt_sincos_table.h as the compiler reads it: (128, 2) float64."""
    out = np.zeros(4096, np.float64)
    n = _emu_lib().rt_emu_probe_sincos_table(out.ctypes.data_as(ctypes.c_void_p))
    return out[:2 * n].reshape(n, 2)


def _kernel_params(precision, kp, mats_address):
    """The KernelParams of a shade probe call as a ctypes structure to pass by value (its bytes come
    from the host builder in the emulator library; `mats_address`: where the call's material records
    are, host or device)."""
    f = getattr(_emu_lib(), f"rt_emu_probe_shade_params_{precision}")
    f.restype = ctypes.c_longlong
    targets = np.ascontiguousarray(kp.get("targets", np.zeros(0, np.uint8))).reshape(-1).view(np.uint8).copy()
    n_targets = targets.size // record_size(precision, "targets")
    assert targets.size == n_targets * record_size(precision, "targets")
    cfg = np.ascontiguousarray(kp["cfg"], np.float64)
    assert cfg.size == 8
    tg = np.concatenate([targets, np.zeros(16, np.uint8)])
    def build(out, cap):
        return f(out, ctypes.c_longlong(cap), ctypes.c_void_p(mats_address), ctypes.c_int(int(kp.get("med_mat", 0))),
                 ctypes.c_uint32(int(kp["key0"])), ctypes.c_uint32(int(kp["key1"])), ctypes.c_int(n_targets),
                 tg.ctypes.data_as(ctypes.c_void_p), cfg.ctypes.data_as(ctypes.c_void_p))
    size = build(None, 0)
    assert size > 0 and size % 8 == 0, size

    class KernelParams(ctypes.Structure):
        _fields_ = [("words", ctypes.c_uint64 * (size // 8))]
    P = KernelParams()
    assert build(ctypes.byref(P), size) == size
    return P


def call(backend, precision, name, *inputs):
    real = np.float64 if precision == "f64" else np.float32
    sig = SIGS[name]
    inputs = list(inputs)
    n = None
    plan = []  # ("scalar", ctypes value) | ("in", numpy array) | ("out", dtype, shape)
    for a in sig:
        if a[0] in ("int", "u32"):
            v = inputs.pop(0)
            plan.append(("scalar", ctypes.c_int(int(v)) if a[0] == "int" else ctypes.c_uint32(int(v))))
            continue
        if a[0] == "kp":
            plan.append(("kp", inputs.pop(0)))
            continue
        if a[0] in ("rec", "table"):
            x = np.ascontiguousarray(inputs.pop(0))
            if a[0] == "rec" or a[1] == "bytes":
                x = x.reshape(-1).view(np.uint8).copy()
            else:
                x = np.require(x, real if a[1] == "real" else a[1], ["C", "W"]).reshape(-1)
            if a[0] == "rec":
                w = record_size(precision, a[1])
                assert x.size % w == 0, (name, x.size, w)
                if n is None:
                    n = x.size // w
                assert x.size == n * w, (name, x.size, n, w)
            if x.size == 0:  # an empty table: never read, but a valid address
                x = np.zeros(16, x.dtype)
            plan.append(("in", x))
            continue
        dt = real if a[1] == "real" else a[1]
        if a[0] == "in":
            x = np.require(inputs.pop(0), dt, ["C", "W"])  # (torch wants writable memory)
            assert x.size % a[2] == 0, (name, x.shape, a)
            if n is None:
                n = x.size // a[2]
            assert x.size == n * a[2], (name, x.shape, n, a)
            plan.append(("in", x))
        else:
            plan.append(("out", dt, (n,) if a[2] == 1 else (n, a[2])))
    assert not inputs and n is not None and n < 2 ** 31, name
    if backend == "emu":
        f = getattr(_emu_lib(), f"rt_emu_probe_{name}_{precision}")
        keep, args, outs = [], [ctypes.c_int(n)], []
        for p in plan:
            if p[0] == "scalar":
                args.append(p[1])
            elif p[0] == "kp":
                mats = np.ascontiguousarray(p[1]["mats"]).reshape(-1).view(np.uint8).copy()
                keep.append(mats)
                args.append(_kernel_params(precision, p[1], mats.ctypes.data))
            elif p[0] == "in":
                keep.append(p[1])
                args.append(p[1].ctypes.data_as(ctypes.c_void_p))
            else:
                o = np.zeros(p[2], p[1])
                outs.append(o)
                args.append(o.ctypes.data_as(ctypes.c_void_p))
        rc = f(*args)
        assert rc == 0, (name, rc)
        return tuple(outs)
    assert backend == "gpu", backend
    import torch
    f = getattr(lib(), f"rt_probe_{name}_{precision}")
    # uint32 / uint64 words travel as the signed torch types of the same width (bit patterns)
    as_signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    keep, args, outs = [], [ctypes.c_int(n)], []
    for p in plan:
        if p[0] == "scalar":
            args.append(p[1])
        elif p[0] == "kp":
            t = torch.from_numpy(np.ascontiguousarray(p[1]["mats"]).reshape(-1).view(np.uint8).copy()).cuda()
            keep.append(t)
            args.append(_kernel_params(precision, p[1], t.data_ptr()))
        elif p[0] == "in":
            x = p[1]
            t = torch.from_numpy(x.view(as_signed.get(x.dtype, x.dtype))).cuda()
            keep.append(t)
            args.append(ctypes.c_void_p(t.data_ptr()))
        else:
            dt = np.dtype(p[1])
            t = torch.zeros(p[2], dtype=getattr(torch, np.dtype(as_signed.get(dt, dt)).name), device="cuda")
            outs.append((t, dt))
            args.append(ctypes.c_void_p(t.data_ptr()))
    args.append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = f(*args)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(dt) for t, dt in outs)
