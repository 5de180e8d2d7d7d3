#!/usr/bin/env python3
"""What hashing the RETIMED windows of a whole library in ONE call buys: vdf_hash_windows_clips_u8_retimed_device of this build beside
the only route the parent commit offers for the same hashes - one vdf_hash_windows_u8_retimed_device call per video - on the same device-resident buffer.

    python tools/bench_hash_windows_mixed_retimed.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows_mixed_retimed.txt]

DESIGN.md 4.15's two sets, stride 1, random bytes generated on the device, videos packed one after the other on 64-byte boundaries, in random order, at the
rates 6/5 and 2/1:
  small   1000 videos of five sizes up to 96 x 96 (32 x 32, 48 x 36, 64 x 64, 80 x 60, 96 x 96) with 32 ... 96 frames
  large   24 videos of 640 x 360, 854 x 480, 1280 x 720 and 1920 x 1080 with 64 ... 256 frames
Legs:
  library    (a) vdf_hash_windows_clips_u8_retimed_device of this build: one call for the set
  per-video  (b) vdf_hash_windows_u8_retimed_device of the library built from the PARENT commit (--parent-lib; without it this build's own uniform retimed
             call stands in and is labelled so): one call per video on the same buffer, rows at first[i] - exactly the same hashes
  plain      (c) this build's vdf_hash_windows_clips_u8_device on the same buffer: the plain windows of the same frames in one call - the floor, not the
             same hashes, reported only
The words of (a) and (b) must be equal.  The tool fails unless, on the small set at both rates, (a) is no slower than (b) by the medians: (b) pays a launch
pair and an upload per video, so a one-call form that is not faster has failed its purpose.  The large set is reported, not gated; no further ratio is fixed.
Every leg runs in a fresh child process (one library per process); a leg is one warm-up and 12 timed calls per set and rate; host clock around calls that end
in a device synchronise; min / median / max over the timed calls.  Kernel-only times are not taken."""
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
REPEATS = 12
STRIDE = 1
RATES = [(6, 5), (2, 1)]
SETS = {
    "small": dict(n=1000, sizes=[(32, 32), (48, 36), (64, 64), (80, 60), (96, 96)], frames=(32, 96)),
    "large": dict(n=24, sizes=[(640, 360), (854, 480), (1280, 720), (1920, 1080)], frames=(64, 256)),
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


def span(rate):
    return (15 * rate[0]) // rate[1] + 1


def library(name):
    """The set's descriptors: (CLIP_DTYPE records, frame counts, buffer bytes) - the same in every process."""
    s = SETS[name]
    rng = np.random.default_rng(len(name) * 1000 + s["n"])
    recs = np.zeros(s["n"], CLIP_DTYPE)
    nf = rng.integers(s["frames"][0], s["frames"][1] + 1, size=s["n"]).astype(np.uint32)
    at = 0
    for i in range(s["n"]):
        w, h = s["sizes"][int(rng.integers(0, len(s["sizes"])))]
        recs[i]["offset"], recs[i]["frame_stride"], recs[i]["w"], recs[i]["h"] = at, w * h, w, h
        at += (int(nf[i]) * w * h + 63) & ~63
    return recs, nf, at


def first_of(nf, width):
    """prefix sums of the window counts of windows `width` frames wide (16: the plain ones)"""
    return np.concatenate([[0], np.cumsum((nf.astype(np.int64) - width) // STRIDE + 1)]).astype(np.uint32)


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
    lib.vdf_hash_windows_u8_retimed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32,
                                                       C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    if args.leg == "library":
        lib.vdf_hash_windows_clips_u8_retimed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    if args.leg == "plain":
        lib.vdf_hash_windows_clips_u8_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]
    res = {}
    for name in SETS:
        recs, nf, nbytes = library(name)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(len(name))
        d = torch.randint(0, 256, (nbytes,), generator=gen, device="cuda", dtype=torch.uint8)
        for rate in RATES:
            first = first_of(nf, 16 if args.leg == "plain" else span(rate))
            rows = int(first[-1])
            out = torch.zeros((rows, 16), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()

            def run():
                if args.leg == "library":
                    rc = lib.vdf_hash_windows_clips_u8_retimed_device(ctx, d.data_ptr(), nbytes, recs.ctypes.data, nf.ctypes.data, len(recs), STRIDE, rate[0], rate[1],
                                                                      out.data_ptr(), None, None)
                elif args.leg == "plain":
                    rc = lib.vdf_hash_windows_clips_u8_device(ctx, d.data_ptr(), nbytes, recs.ctypes.data, nf.ctypes.data, len(recs), STRIDE, out.data_ptr(), None, None)
                else:
                    rc = 0
                    for i in range(len(recs)):
                        wi, hi, fi = int(recs[i]["w"]), int(recs[i]["h"]), int(nf[i])
                        rc = rc or lib.vdf_hash_windows_u8_retimed_device(ctx, d.data_ptr() + int(recs[i]["offset"]), 1, fi, wi, hi, wi * hi, fi * wi * hi, STRIDE,
                                                                          rate[0], rate[1], out.data_ptr() + int(first[i]) * 128, None, None)
                assert rc == 0, (rc, lib.vdf_last_error(ctx))
                torch.cuda.synchronize()

            times = timed(run)
            res[f"{name} {rate[0]}/{rate[1]}"] = {"times": times, "digest": digest(out.cpu().numpy()), "rows": rows, "bytes": nbytes}
            del out
        del d
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_windows_mixed_retimed.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="library")
    args = ap.parse_args()
    if args.child:
        return child(args)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("library", args.lib), ("per-video", parent), ("plain", args.lib)]
    info = {leg: run_child(lib, leg) for leg, lib in legs}
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's uniform retimed call (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_hash_windows_mixed_retimed.py: one warm-up and {REPEATS} timed calls per leg, set and rate; fresh process per leg; stride {STRIDE}; host clock, "
             "kernel-only times not taken",
             f"library = vdf_hash_windows_clips_u8_retimed_device of this build, one call; per-video = vdf_hash_windows_u8_retimed_device of {whose}, one call per video;",
             "plain = vdf_hash_windows_clips_u8_device of this build on the same buffer (the plain windows: the floor, other hashes)"]
    ok = True
    for name, s in SETS.items():
        for rate in RATES:
            key = f"{name} {rate[0]}/{rate[1]}"
            same = info["library"][key]["digest"] == info["per-video"][key]["digest"]
            ok &= same
            lines.append(f"\n{key}: {s['n']} videos of {', '.join(f'{a} x {b}' for a, b in s['sizes'])} with {s['frames'][0]} ... {s['frames'][1]} frames, device-resident: "
                         f"{info['library'][key]['bytes'] / 1e6:.1f} MB, {info['library'][key]['rows']} retimed windows ({info['plain'][key]['rows']} plain); "
                         f"words of library and per-video {'equal' if same else 'DIFFER'}")
            lines.append(f"    {'leg':10s} {'min ms':>10s} {'median':>10s} {'max':>10s}   runs")
            med = {}
            for leg, _ in legs:
                ts = info[leg][key]["times"]
                med[leg] = statistics.median(ts)
                lines.append(f"    {leg:10s} {min(ts) * 1e3:10.3f} {med[leg] * 1e3:10.3f} {max(ts) * 1e3:10.3f}   {len(ts)}")
            verdict = ""
            if name == "small":
                holds = med["library"] <= med["per-video"]
                verdict = "  - gate (library <= per-video): " + ("HOLDS" if holds else "MISSED")
                ok &= holds
            lines.append(f"    per-video / library, medians = {med['per-video'] / med['library']:.2f}x{verdict}")
            lines.append(f"    library / plain, medians = {med['library'] / med['plain']:.2f}x (reported, not gated)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
