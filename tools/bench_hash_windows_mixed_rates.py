#!/usr/bin/env python3
"""What hashing the retimed windows of a whole library at SEVERAL rates in ONE call buys: vdf_hash_windows_clips_u8_rates_device of this
build beside the only one-call-per-rate route the parent commit offers for the same hashes - one vdf_hash_windows_clips_u8_retimed_device call per rate - on
the same device-resident buffer.

    python tools/bench_hash_windows_mixed_rates.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows_mixed_rates.txt]

DESIGN.md 4.15's two sets, stride 1, random bytes generated on the device, videos packed one after the other on 64-byte boundaries, in random order:
  small   1000 videos of five sizes up to 96 x 96 (32 x 32, 48 x 36, 64 x 64, 80 x 60, 96 x 96) with 32 ... 96 frames
  large   24 videos of 640 x 360, 854 x 480, 1280 x 720 and 1920 x 1080 with 64 ... 256 frames
Legs (a timed unit ends in one device synchronise):
  five-calls   (a) vdf_hash_windows_clips_u8_retimed_device of the library built from the PARENT commit (--parent-lib; without it this build's own call
               stands in and is labelled so): five calls, one per rate 1/1, 6/5, 5/4, 3/2, 2/1, back to back, into the blocks of the rate-major layout
  rates        (b) vdf_hash_windows_clips_u8_rates_device of this build at the five rates: one call
  one-new      (c) the new call with the list [3/2]
  one-parent   (c) the parent's single call at 3/2 - beside it, what the generality of the new kernel costs when there is one rate
Words and don't-care counts of every block of (b) must equal (a)'s, and (c)'s two legs must agree.  Gate (exit status 1): on BOTH sets, median (b) <= median
(a) + (max - min of (a)'s timed units) - the new call does strictly less work than (a), so the baseline's own run-to-run spread is all the margin it gets.
The ratio (b) / (a) is reported, not gated.  Every leg runs in a fresh child process (one library per process); a leg is one warm-up and 12 timed units per
set; host clock around units that end in a device synchronise; min / median / max over the timed units.  Kernel-only times are not taken."""
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
FIVE = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
ONE = [(3, 2)]
SETS = {
    "small": dict(n=1000, sizes=[(32, 32), (48, 36), (64, 64), (80, 60), (96, 96)], frames=(32, 96)),
    "large": dict(n=24, sizes=[(640, 360), (854, 480), (1280, 720), (1920, 1080)], frames=(64, 256)),
}
LEGS = {"five-calls": FIVE, "rates": FIVE, "one-new": ONE, "one-parent": ONE}
CLIP_DTYPE = np.dtype([("offset", "<u8"), ("frame_stride", "<u8"), ("w", "<u4"), ("h", "<u4"), ("crop", "<u4", (4,))])


class Job(C.Structure):  # include/vdf.h: vdf_windows_clips_rates_job
    _fields_ = [("buf", C.c_void_p), ("buf_bytes", C.c_size_t), ("clips", C.c_void_p), ("n_frames", C.c_void_p), ("n_videos", C.c_size_t),
                ("window_stride", C.c_uint32), ("n_rates", C.c_uint32), ("rate_num", C.c_void_p), ("rate_den", C.c_void_p),
                ("out_hashes", C.c_void_p), ("out_dontcare", C.c_void_p), ("stream", C.c_void_p)]


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


def rate_first_of(nf, rates):
    """rows of the blocks in front of each rate, the last entry the total (stride 1)"""
    return np.concatenate([[0], np.cumsum([int(((nf.astype(np.int64) - span(r)) // STRIDE + 1).sum()) for r in rates])]).astype(np.int64)


def timed(run):
    out = []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        run()
        if r:
            out.append(time.perf_counter() - t0)
    return out


def digest(a, width):
    w = np.ascontiguousarray(a).view(width).reshape(-1).astype(np.uint64)
    return int(np.bitwise_xor.reduce(w * np.arange(1, w.size + 1, dtype=np.uint64))) if w.size else 0


def child(args):
    import torch

    lib, ctx = open_lib(args.lib)
    rates = LEGS[args.leg]
    single = args.leg in ("five-calls", "one-parent")
    if single:
        lib.vdf_hash_windows_clips_u8_retimed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    else:
        lib.vdf_hash_windows_clips_u8_rates_device.argtypes = [C.c_void_p, C.POINTER(Job)]
    num, den = np.array([r[0] for r in rates], np.uint32), np.array([r[1] for r in rates], np.uint32)
    res = {}
    for name in SETS:
        recs, nf, nbytes = library(name)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(len(name))
        d = torch.randint(0, 256, (nbytes,), generator=gen, device="cuda", dtype=torch.uint8)
        rate_first = rate_first_of(nf, rates)
        rows = int(rate_first[-1])
        out = torch.zeros((rows, 16), dtype=torch.int64, device="cuda")
        dc = torch.zeros((rows,), dtype=torch.int32, device="cuda")
        job = Job(d.data_ptr(), nbytes, recs.ctypes.data, nf.ctypes.data, len(recs), STRIDE, len(rates), num.ctypes.data, den.ctypes.data, out.data_ptr(),
                  dc.data_ptr(), None)
        torch.cuda.synchronize()

        def run():
            if single:
                rc = 0
                for r, rate in enumerate(rates):
                    rc = rc or lib.vdf_hash_windows_clips_u8_retimed_device(ctx, d.data_ptr(), nbytes, recs.ctypes.data, nf.ctypes.data, len(recs), STRIDE, rate[0],
                                                                            rate[1], out.data_ptr() + int(rate_first[r]) * 128, dc.data_ptr() + int(rate_first[r]) * 4,
                                                                            None)
            else:
                rc = lib.vdf_hash_windows_clips_u8_rates_device(ctx, C.byref(job))
            assert rc == 0, (rc, lib.vdf_last_error(ctx))
            torch.cuda.synchronize()

        times = timed(run)
        words, counts = out.cpu().numpy(), dc.cpu().numpy()
        blocks = [(digest(words[rate_first[r]:rate_first[r + 1]], np.uint64), digest(counts[rate_first[r]:rate_first[r + 1]], np.uint32)) for r in range(len(rates))]
        res[name] = {"times": times, "blocks": blocks, "rows": rows, "bytes": nbytes}
        del out, dc, d
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_windows_mixed_rates.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="rates")
    args = ap.parse_args()
    if args.child:
        return child(args)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("five-calls", parent), ("rates", args.lib), ("one-new", args.lib), ("one-parent", parent)]
    info = {leg: run_child(lib, leg) for leg, lib in legs}
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's single-rate call (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_hash_windows_mixed_rates.py: one warm-up and {REPEATS} timed units per leg and set; fresh process per leg; stride {STRIDE}; device-resident "
             "frames; host clock, kernel-only times not taken",
             f"five-calls = vdf_hash_windows_clips_u8_retimed_device of {whose}, one call per rate {', '.join('%d/%d' % r for r in FIVE)}, back to back, one synchronise;",
             "rates = vdf_hash_windows_clips_u8_rates_device of this build at the five rates, one call; one-new = the same call with the list [3/2]; one-parent = the "
             "single call at 3/2"]
    ok = True
    for name, s in SETS.items():
        same = info["rates"][name]["blocks"] == info["five-calls"][name]["blocks"]
        same_one = info["one-new"][name]["blocks"] == info["one-parent"][name]["blocks"] and info["one-new"][name]["blocks"][0] == info["five-calls"][name]["blocks"][3]
        ok &= same and same_one
        lines.append(f"\n{name}: {s['n']} videos of {', '.join(f'{a} x {b}' for a, b in s['sizes'])} with {s['frames'][0]} ... {s['frames'][1]} frames, device-resident: "
                     f"{info['rates'][name]['bytes'] / 1e6:.1f} MB, {info['rates'][name]['rows']} rows at five rates ({info['one-new'][name]['rows']} at 3/2); words and "
                     f"counts of every block of rates and five-calls {'equal' if same else 'DIFFER'}; of one-new and one-parent {'equal' if same_one else 'DIFFER'}")
        lines.append(f"    {'leg':10s} {'min ms':>10s} {'median':>10s} {'max':>10s}   units")
        med = {}
        for leg, _ in legs:
            ts = info[leg][name]["times"]
            med[leg] = statistics.median(ts)
            lines.append(f"    {leg:10s} {min(ts) * 1e3:10.3f} {med[leg] * 1e3:10.3f} {max(ts) * 1e3:10.3f}   {len(ts)}")
        spread = max(info["five-calls"][name]["times"]) - min(info["five-calls"][name]["times"])
        holds = med["rates"] <= med["five-calls"] + spread
        ok &= holds
        lines.append(f"    rates / five-calls, medians = {med['rates'] / med['five-calls']:.2f}x; five-calls' spread (max - min) = {spread * 1e3:.3f} ms"
                     f"  - gate (rates <= five-calls + spread): {'HOLDS' if holds else 'MISSED'}")
        lines.append(f"    rates / one-parent, medians = {med['rates'] / med['one-parent']:.2f} single calls (reported, not gated)")
        lines.append(f"    one-new / one-parent, medians = {med['one-new'] / med['one-parent']:.2f}x (what the generality costs at one rate; reported, not gated)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
