#!/usr/bin/env python3
"""What hashing the retimed windows at several rates in ONE call saves: vdf_hash_windows_u8_rates_device of this build beside one
vdf_hash_windows_u8_retimed_device call per rate of the PARENT commit's library, on the same device-resident frames.

    python tools/bench_hash_windows_rates.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows_rates.txt]

Input (random bytes generated on the device from a seed): one clip of 1920 x 1080 x 256 frames, and 1000 clips of 64 x 64 x 64 frames; stride 1; the
rates 1/1, 6/5, 5/4, 3/2, 2/1.
Legs (device-resident frames and outputs):
  (a) five calls    the parent library: one vdf_hash_windows_u8_retimed_device call per rate, back to back on the context's stream, then ONE device
                    synchronise - the sum of the five calls with the least host time between them
  (b) one call      this build: vdf_hash_windows_u8_rates_device at the five rates, then a device synchronise
  (c) one rate      this build's call with the list [3/2] beside the parent's single call at 3/2: what the generality costs
and at 1920 x 1080 the HOST forms as well (pageable host memory): five vdf_hash_windows_u8_retimed calls of the parent - five uploads - beside one
vdf_hash_windows_u8_rates call - one upload.
Gate (exit status 1 if it fails): at both shapes median (b) <= median (a) + (max - min of (a)'s timed calls) - the new call does strictly less
work, so the run-to-run spread of the baseline is all the margin it gets - and every block of (b), (c) and the host form equals the parent's words
and don't-care counts (a digest over both).
Every leg runs in a fresh child process (one library per process): one warm-up, then REPEATS timed units, host clock around units that end in a
device synchronise; median / min / max over the timed units.  Without --parent-lib this build's own single-rate call stands in and is labelled so."""
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
SHAPES = [(1920, 1080, 1, 256), (64, 64, 1000, 64)]  # w, h, clips, frames per clip
RATES = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
ONE = (3, 2)
STRIDE = 1
REPEATS, HOST_REPEATS = 12, 6
HASH_ARGS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t]


class Job(C.Structure):  # include/vdf.h: vdf_windows_rates_job
    _fields_ = [("frames", C.c_void_p), ("n_clips", C.c_size_t), ("frames_per_clip", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("frame_stride", C.c_size_t), ("clip_stride", C.c_size_t), ("window_stride", C.c_uint32), ("n_rates", C.c_uint32),
                ("rate_num", C.c_void_p), ("rate_den", C.c_void_p), ("out_hashes", C.c_void_p), ("out_dontcare", C.c_void_p), ("stream", C.c_void_p)]


def open_lib(path):
    lib = C.CDLL(path)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    return lib, ctx


def timed(run, repeats):
    out = []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        run()
        if r:
            out.append(time.perf_counter() - t0)
    return out


def digest(words, counts):
    w = np.concatenate([np.ascontiguousarray(words).view(np.uint64).reshape(-1), np.ascontiguousarray(counts).astype(np.uint64).reshape(-1)])
    return int(np.bitwise_xor.reduce(w * np.arange(1, w.size + 1, dtype=np.uint64)))


def n_windows(nf, rate):
    span = (15 * rate[0]) // rate[1] + 1
    return (nf - span) // STRIDE + 1


def child(args):
    import torch

    lib, ctx = open_lib(args.lib)
    new = args.leg == "new"
    if new:
        lib.vdf_hash_windows_u8_rates_device.argtypes = lib.vdf_hash_windows_u8_rates.argtypes = [C.c_void_p, C.POINTER(Job)]
    else:
        lib.vdf_hash_windows_u8_retimed_device.argtypes = HASH_ARGS + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.vdf_hash_windows_u8_retimed.argtypes = HASH_ARGS + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    check = lambda rc: rc == 0 or sys.exit(f"rc {rc}: {lib.vdf_last_error(ctx)}")
    res = {}
    for w, h, n, nf in SHAPES:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(w * 7 + h)
        d = torch.randint(0, 256, (n * nf * w * h,), generator=gen, device="cuda", dtype=torch.uint8)
        fs = w * h
        key = f"{w}x{h}"

        def device_leg(rates, repeats=REPEATS):
            rows = [n * n_windows(nf, r) for r in rates]
            first = np.concatenate([[0], np.cumsum(rows)])
            out = torch.zeros((int(first[-1]), 16), dtype=torch.int64, device="cuda")
            dc = torch.zeros((int(first[-1]),), dtype=torch.int32, device="cuda")
            num, den = np.array([r[0] for r in rates], np.uint32), np.array([r[1] for r in rates], np.uint32)
            job = Job(d.data_ptr(), n, nf, w, h, fs, nf * fs, STRIDE, len(rates), num.ctypes.data, den.ctypes.data, out.data_ptr(), dc.data_ptr(), None)
            torch.cuda.synchronize()

            def run():
                if new:
                    check(lib.vdf_hash_windows_u8_rates_device(ctx, C.byref(job)))
                else:
                    for i, (a, b) in enumerate(rates):
                        check(lib.vdf_hash_windows_u8_retimed_device(ctx, d.data_ptr(), n, nf, w, h, fs, nf * fs, STRIDE, a, b, out.data_ptr() + int(first[i]) * 128,
                                                                     dc.data_ptr() + int(first[i]) * 4, None))
                torch.cuda.synchronize()

            times = timed(run, repeats)
            words, counts = out.cpu().numpy(), dc.cpu().numpy()
            return {"times": times, "digests": [digest(words[first[i]:first[i + 1]], counts[first[i]:first[i + 1]]) for i in range(len(rates))], "rows": int(first[-1])}

        res[key + "/five"] = device_leg(RATES)
        res[key + "/one"] = device_leg([ONE])
        if n == 1:  # the host forms: pageable host memory, the call returns when the results are down
            host = d.cpu().numpy()
            rows = [n * n_windows(nf, r) for r in RATES]
            first = np.concatenate([[0], np.cumsum(rows)])
            words, counts = np.zeros((int(first[-1]), 16), np.uint64), np.zeros(int(first[-1]), np.uint32)
            num, den = np.array([r[0] for r in RATES], np.uint32), np.array([r[1] for r in RATES], np.uint32)
            job = Job(host.ctypes.data, n, nf, w, h, fs, nf * fs, STRIDE, len(RATES), num.ctypes.data, den.ctypes.data, words.ctypes.data, counts.ctypes.data, None)

            def run_host():
                if new:
                    check(lib.vdf_hash_windows_u8_rates(ctx, C.byref(job)))
                else:
                    for i, (a, b) in enumerate(RATES):
                        check(lib.vdf_hash_windows_u8_retimed(ctx, host.ctypes.data, n, nf, w, h, fs, nf * fs, STRIDE, a, b, words.ctypes.data + int(first[i]) * 128,
                                                              counts.ctypes.data + int(first[i]) * 4))

            res[key + "/host"] = {"times": timed(run_host, HOST_REPEATS),
                                  "digests": [digest(words[first[i]:first[i + 1]], counts[first[i]:first[i + 1]]) for i in range(len(RATES))], "rows": int(first[-1])}
            del host
        del d
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def run_child(lib, leg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--leg", leg], capture_output=True, text=True, timeout=1100)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    print(f"[{leg}: done]", file=sys.stderr, flush=True)
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_windows_rates.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="new")
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    old = run_child(os.path.abspath(args.parent_lib) if args.parent_lib else args.lib, "parent")
    new = run_child(args.lib, "new")
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's single-rate call (no --parent-lib: not the parent commit)"
    ms = lambda ts: f"{statistics.median(ts) * 1e3:9.3f} {min(ts) * 1e3:9.3f} {max(ts) * 1e3:9.3f}   {len(ts)}"
    lines = [f"tools/bench_hash_windows_rates.py: fresh process per leg, one warm-up, then {REPEATS} timed units per device leg ({HOST_REPEATS} per host leg); host clock around",
             f"units that end in a device synchronise.  five calls / single call = vdf_hash_windows_u8_retimed[_device] of {whose};",
             f"one call = vdf_hash_windows_u8_rates[_device] of this build.  stride {STRIDE}; rates {', '.join('%d/%d' % r for r in RATES)}; the single rate is {ONE[0]}/{ONE[1]}",
             "gate: median (b) <= median (a) + (max - min of (a)); all words and don't-care counts equal"]
    ok = True
    for w, h, n, nf in SHAPES:
        key = f"{w}x{h}"
        lines.append(f"\n{n} clip(s) of {w} x {h} x {nf} frames, device-resident: {new[key + '/five']['rows']} windows at the five rates, {new[key + '/one']['rows']} at {ONE[0]}/{ONE[1]}")
        lines.append(f"    {'leg':34s} {'median ms':>9s} {'min':>9s} {'max':>9s}   units")
        a, b = old[key + "/five"]["times"], new[key + "/five"]["times"]
        a1, b1 = old[key + "/one"]["times"], new[key + "/one"]["times"]
        lines.append(f"    {'(a) five calls, one per rate':34s} {ms(a)}")
        lines.append(f"    {'(b) one call, five rates':34s} {ms(b)}")
        lines.append(f"    {'(c) single call at one rate':34s} {ms(a1)}")
        lines.append(f"    {'(c) one call, that one rate':34s} {ms(b1)}")
        same = old[key + "/five"]["digests"] == new[key + "/five"]["digests"] and old[key + "/one"]["digests"] == new[key + "/one"]["digests"]
        spread = max(a) - min(a)
        gate = statistics.median(b) <= statistics.median(a) + spread
        ok &= same and gate
        lines.append(f"    (b) / (a), medians = {statistics.median(b) / statistics.median(a):.3f}x   (b) / single call = {statistics.median(b) / statistics.median(a1):.3f}x   "
                     f"(c) one-rate list / single call = {statistics.median(b1) / statistics.median(a1):.3f}x")
        lines.append(f"    spread of (a) = {spread * 1e3:.3f} ms; gate (b) <= (a) + spread: {'holds' if gate else 'FAILS'}; words and counts of every block {'equal' if same else 'DIFFER'}")
        if key + "/host" in new:
            ha, hb = old[key + "/host"]["times"], new[key + "/host"]["times"]
            hsame = old[key + "/host"]["digests"] == new[key + "/host"]["digests"] == new[key + "/five"]["digests"]
            ok &= hsame
            lines.append(f"  host forms (pageable host memory; the frames are {n * nf * w * h / 2**20:.0f} MiB):")
            lines.append(f"    {'five host calls: five uploads':34s} {ms(ha)}")
            lines.append(f"    {'one host call: one upload':34s} {ms(hb)}")
            lines.append(f"    one / five, medians = {statistics.median(hb) / statistics.median(ha):.3f}x; words and counts {'equal' if hsame else 'DIFFER'}")
    lines.append(f"\ngate: {'PASS' if ok else 'FAIL'}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
