#!/usr/bin/env python3
"""What hashing the windows of a whole library in ONE call buys: vdf_hash_windows_clips_u8_device of this build beside the parent
commit's way of getting the same hashes - one vdf_hash_windows_u8_device call per video - on the same device-resident buffer.

    python tools/bench_hash_windows_mixed.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows_mixed.txt]

Two sets, stride 1, random bytes generated on the device, videos packed one after the other on 64-byte boundaries, in random order:
  small   1000 videos of five sizes up to 96 x 96 (32 x 32, 48 x 36, 64 x 64, 80 x 60, 96 x 96) with 32 ... 96 frames
  large   24 videos of 640 x 360, 854 x 480, 1280 x 720 and 1920 x 1080 with 64 ... 256 frames
Legs:
  mixed      (a) vdf_hash_windows_clips_u8_device of this build: one call for the set
  per-video  (b) vdf_hash_windows_u8_device of the library built from the PARENT commit (--parent-lib; without it this build's own uniform call
             stands in and is labelled so): one call per video on the same buffer, rows at first[i] - exactly the same hashes
  uniform    (c) the same library's single uniform call on a set of ONE size and length with about as many frames (1000 x 64 x 64 x 64;
             24 x 1280 x 720 x 160): the ceiling, not the same hashes
The words of (a) and (b) must be equal.  The tool fails unless (a) beats (b) by 3x on the small set: (b) is bound by at least two launches per
video.  No ratio is demanded against (c), and none on the large set, which is bound by the frame reads either way.
Every leg runs in a fresh child process (one library per process), the legs take turns ROUNDS times, each turn is one warm-up and REPEATS timed
calls (12 timed calls per leg); host clock around calls that end in a device synchronise; min / median over all timed calls of a leg."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS, ROUNDS = 6, 2
STRIDE = 1
SETS = {
    "small": dict(n=1000, sizes=[(32, 32), (48, 36), (64, 64), (80, 60), (96, 96)], frames=(32, 96), uniform=(1000, 64, 64, 64)),
    "large": dict(n=24, sizes=[(640, 360), (854, 480), (1280, 720), (1920, 1080)], frames=(64, 256), uniform=(24, 1280, 720, 160)),
}
CLIP_DTYPE = np.dtype([("offset", "<u8"), ("frame_stride", "<u8"), ("w", "<u4"), ("h", "<u4"), ("crop", "<u4", (4,))])


def open_lib(path):
    lib = C.CDLL(path)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    return lib, ctx


def library(name):
    """The set's descriptors: (CLIP_DTYPE records, frame counts, first, buffer bytes) - the same in every process."""
    s = SETS[name]
    rng = np.random.default_rng(len(name) * 1000 + s["n"])
    recs = np.zeros(s["n"], CLIP_DTYPE)
    nf = rng.integers(s["frames"][0], s["frames"][1] + 1, size=s["n"]).astype(np.uint32)
    at = 0
    for i in range(s["n"]):
        w, h = s["sizes"][int(rng.integers(0, len(s["sizes"])))]
        recs[i]["offset"], recs[i]["frame_stride"], recs[i]["w"], recs[i]["h"] = at, w * h, w, h
        at += (int(nf[i]) * w * h + 63) & ~63
    first = np.concatenate([[0], np.cumsum((nf.astype(np.int64) - 16) // STRIDE + 1)]).astype(np.uint32)
    return recs, nf, first, at


def timed(run):
    out = []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        run()
        if r:
            out.append(time.perf_counter() - t0)
    return out


def digest(words):
    w = words.view(np.uint64).reshape(-1)
    return int(np.bitwise_xor.reduce(w * np.arange(1, w.size + 1, dtype=np.uint64)))


def child(args):
    import torch

    lib, ctx = open_lib(args.lib)
    uniform_args = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vdf_hash_windows_u8_device.argtypes = uniform_args
    if args.leg == "mixed":
        lib.vdf_hash_windows_clips_u8_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]
    res = {}
    for name, s in SETS.items():
        recs, nf, first, nbytes = library(name)
        if args.leg == "uniform":
            n, w, h, f = s["uniform"]
            nbytes, rows = n * f * w * h, n * ((f - 16) // STRIDE + 1)
        else:
            rows = int(first[-1])
        gen = torch.Generator(device="cuda")
        gen.manual_seed(len(name))
        d = torch.randint(0, 256, (nbytes,), generator=gen, device="cuda", dtype=torch.uint8)
        out = torch.zeros((rows, 16), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def run():
            if args.leg == "mixed":
                rc = lib.vdf_hash_windows_clips_u8_device(ctx, d.data_ptr(), nbytes, recs.ctypes.data, nf.ctypes.data, len(recs), STRIDE, out.data_ptr(), None, None)
            elif args.leg == "uniform":
                rc = lib.vdf_hash_windows_u8_device(ctx, d.data_ptr(), n, f, w, h, w * h, f * w * h, STRIDE, out.data_ptr(), None, None)
            else:
                rc = 0
                for i in range(len(recs)):
                    wi, hi, fi = int(recs[i]["w"]), int(recs[i]["h"]), int(nf[i])
                    rc = rc or lib.vdf_hash_windows_u8_device(ctx, d.data_ptr() + int(recs[i]["offset"]), 1, fi, wi, hi, wi * hi, fi * wi * hi, STRIDE,
                                                              out.data_ptr() + int(first[i]) * 128, None, None)
            assert rc == 0, (rc, lib.vdf_last_error(ctx))
            torch.cuda.synchronize()

        times = timed(run)
        res[name] = {"times": times, "digest": digest(out.cpu().numpy()), "rows": rows, "bytes": nbytes}
        del d, out
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def run_child(lib, leg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--leg", leg], capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_windows_mixed.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="mixed")
    args = ap.parse_args()
    if args.child:
        return child(args)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("mixed", args.lib), ("per-video", parent), ("uniform", parent)]
    times, info = {}, {}
    for _ in range(ROUNDS):
        for leg, lib in legs:
            for key, v in run_child(lib, leg).items():
                times.setdefault(key, {}).setdefault(leg, []).extend(v["times"])
                info.setdefault(key, {})[leg] = v
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's uniform call (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_hash_windows_mixed.py: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"mixed = vdf_hash_windows_clips_u8_device of this build, one call; per-video and uniform = vdf_hash_windows_u8_device of {whose}; stride {STRIDE}"]
    ok = True
    for name, s in SETS.items():
        same = info[name]["mixed"]["digest"] == info[name]["per-video"]["digest"]
        ok &= same
        n, w, h, f = s["uniform"]
        lines.append(f"\n{name}: {s['n']} videos of {', '.join(f'{a} x {b}' for a, b in s['sizes'])} with {s['frames'][0]} ... {s['frames'][1]} frames, device-resident: "
                     f"{info[name]['mixed']['bytes'] / 1e6:.1f} MB, {info[name]['mixed']['rows']} windows; words of mixed and per-video {'equal' if same else 'DIFFER'}")
        lines.append(f"  (uniform: {n} x {w} x {h} x {f} frames, {info[name]['uniform']['bytes'] / 1e6:.1f} MB, {info[name]['uniform']['rows']} windows)")
        lines.append(f"    {'leg':10s} {'min ms':>10s} {'median':>10s} {'max':>10s}   runs")
        for leg, _ in legs:
            ts = times[name][leg]
            lines.append(f"    {leg:10s} {min(ts) * 1e3:10.3f} {statistics.median(ts) * 1e3:10.3f} {max(ts) * 1e3:10.3f}   {len(ts)}")
        med = {leg: statistics.median(times[name][leg]) for leg, _ in legs}
        ratio = med["per-video"] / med["mixed"]
        verdict = ""
        if name == "small":
            verdict = "  - gate (at least 3x): " + ("HOLDS" if ratio >= 3 else "MISSED")
            ok &= ratio >= 3
        lines.append(f"    per-video / mixed, medians = {ratio:.2f}x{verdict}")
        lines.append(f"    mixed / uniform, medians = {med['mixed'] / med['uniform']:.2f}x at {info[name]['mixed']['bytes'] / info[name]['uniform']['bytes']:.2f}x the bytes (reported, not gated)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
