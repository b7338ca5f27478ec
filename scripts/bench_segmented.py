#!/usr/bin/env python3
"""Benchmark of the segmented sort (sortKeysSegmented / sortPairsSegmented).

Three contestants on the same inputs, resident in HBM and fresh per step:
  thrs     the segmented call of this library;
  hipcub   hipcub::DeviceSegmentedRadixSort (libthrs_vendor.so);
  loop     the only way before the segmented call existed: one sortKeys /
           sortPairs per segment -- run only for shapes of <= 4096 segments.

Timing: after `--warmup` untimed steps, device events around a batch of
`--steps` steps, each step on its own copy of the input (copies are filled
before the first event).  `loop` is dominated by host-side launches, so its
batch is closed by a device synchronise and timed by the host clock as well.

One JSON line per shape.  `hbm_fraction` is the bytes the sort must move (one
read and one write of every key and value of every segment) over the thrs
call's time, as a fraction of the 8 TB/s HBM peak: the rate of the whole call
(classify + the three class kernels), not of one kernel.  The uniform shapes
fall into one size class each, so there the call's rate is that class
kernel's, launch gaps included; `classes` shows which.

    python scripts/bench_segmented.py [--steps 5] [--warmup 1] [--shapes NAME,...]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes/s, MI355X HBM3E specification
LOOP_MAX_SEGMENTS = 4096

# name -> (key type name, value bytes, segment sizes factory)
SHAPES = {
    "1Mx32_u32": ("u32", 0, lambda np: np.full(1 << 20, 32, np.int64)),
    "64Kx1024_u32_u32": ("u32", 4, lambda np: np.full(65536, 1024, np.int64)),
    "4Kx16K_u64_u32": ("u64", 4, lambda np: np.full(4096, 16384, np.int64)),
    "512x256K_f32": ("f32", 0, lambda np: np.full(512, 1 << 18, np.int64)),
    "ragged100K_lognormal300_u32_u32": ("u32", 4, lambda np: np.maximum(
        0, np.exp(np.random.default_rng(300).normal(np.log(300.0), 1.0, 100000))).astype(np.int64)),
}
KEYS = {"u32": (0, 4), "u64": (1, 8), "f32": (2, 4), "f64": (3, 8)}


def vendor_lib():
    path = os.path.join(ROOT, "tinyhipradixsort_amd", "libthrs_vendor.so")
    if not os.path.exists(path):
        return None
    L = ctypes.CDLL(path)
    if not hasattr(L, "thrsv_segmented_sort"):
        return None
    vp = ctypes.c_void_p
    L.thrsv_segmented_sort.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_uint32, vp,
                                       ctypes.c_uint32, vp, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_int), vp]
    return L


def master_keys(torch, kname, n):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    if kname == "f32":
        return torch.randn(n, generator=g, device="cuda", dtype=torch.float32).view(torch.uint8)
    if kname == "f64":
        return torch.randn(n, generator=g, device="cuda", dtype=torch.float64).view(torch.uint8)
    words = n * (KEYS[kname][1] // 4)
    return torch.randint(-(1 << 31), 1 << 31, (words,), generator=g, device="cuda", dtype=torch.int64).to(
        torch.int32).view(torch.uint8)


def timed_batch(torch, stream, steps, body):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(stream)
    for j in range(steps):
        body(j)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, (time.perf_counter() - t0) * 1e3 / steps


def bench_shape(torch, T, V, name, steps, warmup):
    import numpy as np
    kname, vb, make = SHAPES[name]
    kt, kb = KEYS[kname]
    sizes = make(np)
    ns = int(sizes.shape[0])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offs[-1])
    assert n < (1 << 31)
    stream = torch.cuda.current_stream()
    od = torch.from_numpy(offs.astype(np.int64)).to("cuda").to(torch.int32)
    mk = master_keys(torch, kname, n)
    mv = torch.arange(n, device="cuda", dtype=torch.int32).view(torch.uint8) if vb else None
    keys = [torch.empty_like(mk) for _ in range(steps)]
    vals = [torch.empty_like(mv) for _ in range(steps)] if vb else [None] * steps

    def refill():
        for j in range(steps):
            keys[j].copy_(mk)
            if vb:
                vals[j].copy_(mv)

    cfg = T.RadixSort.Config()
    cfg.keyType = T.KeyType(kt)
    cfg.valueType = {0: T.ValueType.U32, 4: T.ValueType.U32, 8: T.ValueType.U64, 16: T.ValueType.U128}[vb]
    rs = T.RadixSort([], cfg)
    moved = 2 * n * (kb + vb)
    row = {"shape": name, "key": kname, "value_bytes": vb, "segments": ns, "keys": n, "steps": steps,
           "warmup": warmup, "bytes_moved_min": moved}

    # ---- thrs
    tmp = torch.empty(rs.getSegmentedTemporaryBufferBytes(n, ns, bool(vb)), dtype=torch.uint8, device="cuda")

    def thrs_step(j):
        if vb:
            rs.sortPairsSegmented(keys[j], vals[j], n, od, ns, tmp, 0, kb * 8, stream=stream)
        else:
            rs.sortKeysSegmented(keys[j], n, od, ns, tmp, 0, kb * 8, stream=stream)

    refill()
    for _ in range(warmup):
        thrs_step(0)
    refill()
    ms, _ = timed_batch(torch, stream, steps, thrs_step)
    rs.checkDeviceError(tmp, stream=stream)
    row["classes"] = dict(zip(("trivial", "wave", "workgroup", "streaming"), T.debug_segment_classes(tmp, stream)))
    row["thrs_ms"] = round(ms, 4)
    row["thrs_gkeys_s"] = round(n / ms / 1e6, 3)
    row["hbm_fraction"] = round(moved / (ms * 1e-3) / HBM_PEAK, 4)
    ours_k = keys[0].clone()
    ours_v = vals[0].clone() if vb else None

    # ---- hipcub
    row["hipcub_ms"] = "not run"
    if V is not None:
        tb = ctypes.c_uint64()
        sel = ctypes.c_int()
        rc = V.thrsv_segmented_sort(kt, vb, None, None, None, None, n, od.data_ptr(), ns, None, ctypes.byref(tb), None,
                                    None)
        if rc == 0:
            vtmp = torch.empty(max(1, tb.value), dtype=torch.uint8, device="cuda")
            kalt = torch.empty_like(mk)
            valt = torch.empty_like(mv) if vb else None

            def cub_step(j):
                r = V.thrsv_segmented_sort(kt, vb, keys[j].data_ptr(), kalt.data_ptr(),
                                           vals[j].data_ptr() if vb else None, valt.data_ptr() if vb else None, n,
                                           od.data_ptr(), ns, vtmp.data_ptr(), ctypes.byref(tb), ctypes.byref(sel),
                                           stream.cuda_stream)
                assert r == 0, r

            refill()
            for _ in range(warmup):
                cub_step(0)
            refill()
            cms, _ = timed_batch(torch, stream, steps, cub_step)
            row["hipcub_ms"] = round(cms, 4)
            row["thrs_over_hipcub_time"] = round(ms / cms, 3)
            ck = keys[steps - 1] if sel.value == 0 else kalt
            cv = (vals[steps - 1] if sel.value == 0 else valt) if vb else None
            same = bool(torch.equal(ck, ours_k)) and (not vb or bool(torch.equal(cv, ours_v)))
            row["agrees_with_hipcub"] = same
            del vtmp, kalt, valt

    # ---- loop of single sorts
    row["loop_ms"] = "not run"
    if ns <= LOOP_MAX_SEGMENTS:
        d = rs.getTemporaryBufferBytes(int(sizes.max()))
        ltmp = torch.empty(d.getTemporaryBufferBytesForSortPairs() if vb else d.getTemporaryBufferBytesForSortKeys(),
                           dtype=torch.uint8, device="cuda")
        lsteps = min(steps, 2)

        def loop_step(j):
            kp = keys[j].data_ptr()
            vp_ = vals[j].data_ptr() if vb else 0
            for s in range(ns):
                a, m = int(offs[s]), int(sizes[s])
                if vb:
                    rs.sortPairs(kp + a * kb, vp_ + a * vb, m, ltmp, 0, kb * 8, stream=stream)
                else:
                    rs.sortKeys(kp + a * kb, m, ltmp, 0, kb * 8, stream=stream)

        refill()
        loop_step(0)
        refill()
        lms, lwall = timed_batch(torch, stream, lsteps, loop_step)
        row["loop_ms"] = round(lms, 3)
        row["loop_wall_ms"] = round(lwall, 3)
        row["loop_agrees"] = bool(torch.equal(keys[0], ours_k)) and (not vb or bool(torch.equal(vals[0], ours_v)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_segmented.py needs a GPU: nothing is measured without one")
    import tinyhipradixsort_amd as T
    torch.cuda.set_device(0)
    V = vendor_lib()
    for name in a.shapes.split(","):
        row = bench_shape(torch, T, V, name, a.steps, a.warmup)
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
