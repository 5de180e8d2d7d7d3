#!/usr/bin/env python3
"""What hashing every window from one read of the frames buys: vdf_hash_windows_u8_device of this build beside the parent
commit's way of getting the same hashes - the plain call with clip_stride = stride * frame_stride - on the same device-resident frames.

    python tools/bench_hash_windows.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows.txt]

Input (random bytes generated on the device): one clip of 1920 x 1080 x 256 frames, and 1000 clips of 64 x 64 x 64 frames; strides 1, 4, 16.
Legs:
  windows       vdf_hash_windows_u8_device of this build: one call
  parent        vdf_hash_frames_u8_device of the library built from the PARENT commit (--parent-lib; without it this build's own plain
                call stands in and is labelled so): one call per clip, n_win overlapping 16-frame stacks each - exactly the same hashes
  parent-1call  the same library, ONE call over the packed buffer as one long sequence: a superset (it also hashes the stacks that
                straddle two clips), without the per-clip launches; only where there is more than one clip
The claim under test: at stride 1 the windows call is faster than the parent's form (the faster of its two legs) at both sizes.  The tool
prints the ratio and reports a miss as a miss.  At stride 16 on 64 x 64 the plain call runs its fused persistent kernel and is expected to
win: that is why the plain call stays the route for disjoint stacks.
Every leg runs in a fresh child process (one library per process), the legs take turns ROUNDS times, each turn is one warm-up and REPEATS
timed calls; host clock around calls that end in a device synchronise; min / median over all timed calls of a leg.  The windows leg's and
the parent leg's words must be equal.

    python tools/bench_hash_windows.py --planes --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows_planes.txt]

What the zero planes of the windows cost.  Same shapes, strides 1 and 4, same protocol (median of 12 per leg).  Legs:
  planes          vdf_hash_windows_u8_planes_device of this build
  windows         vdf_hash_windows_u8_device of this build
  parent-windows  vdf_hash_windows_u8_device of the library built from the PARENT commit
Gate, at 1920 x 1080 stride 1: this build's plain call and the planes call may each be slower than the parent's by no more than the max / min
spread of the parent's own 12 runs (the frame read dominates there; the plane adds 128 B per window).  At 64 x 64 the planes call doubles the
bytes written per window: the ratio is reported, not gated.  The hash words of all three legs must be equal."""
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
STRIDES = (1, 4, 16)
PLANES_STRIDES = (1, 4)
REPEATS, ROUNDS = 6, 2
HASH_ARGS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t]


def open_lib(path):
    lib = C.CDLL(path)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    return lib, ctx


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
    lib.vdf_hash_frames_u8_device.argtypes = HASH_ARGS + [C.c_void_p, C.c_void_p, C.c_void_p]
    if args.leg == "windows":
        lib.vdf_hash_windows_u8_device.argtypes = HASH_ARGS + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    if args.leg == "planes":
        lib.vdf_hash_windows_u8_planes_device.argtypes = HASH_ARGS + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    res = {}
    for w, h, n, nf in SHAPES:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(w * 7 + h)
        d = torch.randint(0, 256, (n * nf * w * h,), generator=gen, device="cuda", dtype=torch.uint8)
        fs = w * h
        for stride in (PLANES_STRIDES if args.planes else STRIDES):
            n_win = (nf - 16) // stride + 1
            n_seq = (n * nf - 16) // stride + 1  # stacks of the packed buffer taken as one sequence
            if args.leg == "parent-1call" and n == 1:
                continue
            out = torch.zeros((n_seq if args.leg == "parent-1call" else n * n_win, 16), dtype=torch.int64, device="cuda")
            zero = torch.zeros((n * n_win, 16), dtype=torch.int64, device="cuda") if args.leg == "planes" else None
            torch.cuda.synchronize()

            def run():
                if args.leg == "planes":
                    rc = lib.vdf_hash_windows_u8_planes_device(ctx, d.data_ptr(), n, nf, w, h, fs, nf * fs, stride, out.data_ptr(), None, zero.data_ptr(), None)
                elif args.leg == "windows":
                    rc = lib.vdf_hash_windows_u8_device(ctx, d.data_ptr(), n, nf, w, h, fs, nf * fs, stride, out.data_ptr(), None, None)
                elif args.leg == "parent-1call":
                    rc = lib.vdf_hash_frames_u8_device(ctx, d.data_ptr(), n_seq, 16, w, h, fs, stride * fs, out.data_ptr(), None, None)
                else:
                    rc = 0
                    for c in range(n):
                        rc = rc or lib.vdf_hash_frames_u8_device(ctx, d.data_ptr() + c * nf * fs, n_win, 16, w, h, fs, stride * fs,
                                                                 out.data_ptr() + c * n_win * 128, None, None)
                assert rc == 0, (rc, lib.vdf_last_error(ctx))
                torch.cuda.synchronize()

            times = timed(run)
            words = out.cpu().numpy()
            if args.leg == "parent-1call":  # the stacks that are windows of a clip, in the windows call's order
                assert nf % stride == 0
                words = words[(np.arange(n)[:, None] * (nf // stride) + np.arange(n_win)[None, :]).reshape(-1)]
            res[f"{w}x{h}/{stride}"] = {"times": times, "digest": digest(words)}
            if zero is not None:  # H & Z == 0 and no bit above 999, for every window
                z = zero.cpu().numpy()
                assert not np.any(z & words) and not np.any(z[:, 15].view(np.uint64) >> np.uint64(40))
            del out, zero
        del d
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def run_child(lib, leg, planes=False):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--leg", leg] + (["--planes"] if planes else []),
                         capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads(line[-1][7:])


def planes_main(args):
    if not args.parent_lib:
        raise SystemExit("--planes compares against the parent commit's library: --parent-lib is required")
    legs = [("planes", "planes", args.lib), ("windows", "windows", args.lib), ("parent-windows", "windows", os.path.abspath(args.parent_lib))]
    times, digests = {}, {}
    for _ in range(ROUNDS):
        for name, leg, lib in legs:
            for key, v in run_child(lib, leg, planes=True).items():
                times.setdefault(key, {}).setdefault(name, []).extend(v["times"])
                digests.setdefault(key, {})[name] = v["digest"]
    lines = [f"tools/bench_hash_windows.py --planes: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             "planes = vdf_hash_windows_u8_planes_device, windows = vdf_hash_windows_u8_device of this build; parent-windows = the PARENT commit's library"]
    ok = True
    for w, h, n, nf in SHAPES:
        lines.append(f"\n{n} clip(s) of {w} x {h} x {nf} frames, device-resident")
        for stride in PLANES_STRIDES:
            key = f"{w}x{h}/{stride}"
            n_win = (nf - 16) // stride + 1
            same = len(set(digests[key].values())) == 1
            ok &= same
            lines.append(f"  stride {stride}: {n * n_win} windows; hash words of all legs {'equal' if same else 'DIFFER'}; bytes written per window: 128 plain, 256 with the plane")
            lines.append(f"    {'leg':15s} {'min ms':>9s} {'median':>9s} {'max':>9s}   runs")
            for name, _, _ in legs:
                ts = times[key][name]
                lines.append(f"    {name:15s} {min(ts) * 1e3:9.3f} {statistics.median(ts) * 1e3:9.3f} {max(ts) * 1e3:9.3f}   {len(ts)}")
            parent = times[key]["parent-windows"]
            spread = max(parent) / min(parent)
            for name in ("windows", "planes"):
                ratio = statistics.median(times[key][name]) / statistics.median(parent)
                verdict = ""
                if (w, stride) == (1920, 1):
                    verdict = f"  - gate (at most the parent's own max / min spread, {spread:.3f}x): " + ("HOLDS" if ratio <= spread else "MISSED")
                    ok &= ratio <= spread
                lines.append(f"    {name} / parent-windows, medians = {ratio:.3f}x{verdict}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--planes", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="windows")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "hash_windows_planes.txt" if args.planes else "hash_windows.txt")
    if args.planes:
        return planes_main(args)
    plain_lib = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("windows", args.lib), ("parent", plain_lib), ("parent-1call", plain_lib)]
    times, digests = {}, {}
    for _ in range(ROUNDS):
        for leg, lib in legs:
            for key, v in run_child(lib, leg).items():
                times.setdefault(key, {}).setdefault(leg, []).extend(v["times"])
                digests.setdefault(key, {})[leg] = v["digest"]
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's plain call (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_hash_windows.py: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"parent legs: vdf_hash_frames_u8_device of {whose} with clip_stride = stride * frame_stride"]
    ok = True
    for w, h, n, nf in SHAPES:
        lines.append(f"\n{n} clip(s) of {w} x {h} x {nf} frames, device-resident")
        for stride in STRIDES:
            key = f"{w}x{h}/{stride}"
            n_win = (nf - 16) // stride + 1
            same = len(set(digests[key].values())) == 1
            ok &= same
            read_new, read_old = n * nf * w * h, n * n_win * 16 * w * h
            lines.append(f"  stride {stride}: {n * n_win} windows; hash words of all legs {'equal' if same else 'DIFFER'}; frame bytes read: windows {read_new / 1e6:.1f} MB, "
                         f"parent {read_old / 1e6:.1f} MB")
            lines.append(f"    {'leg':13s} {'min ms':>9s} {'median':>9s}   runs")
            for leg, _ in legs:
                if leg in times[key]:
                    ts = times[key][leg]
                    lines.append(f"    {leg:13s} {min(ts) * 1e3:9.3f} {statistics.median(ts) * 1e3:9.3f}   {len(ts)}")
            best = min(statistics.median(times[key][leg]) for leg in ("parent", "parent-1call") if leg in times[key])
            ratio = best / statistics.median(times[key]["windows"])
            verdict = ""
            if stride == 1:
                verdict = "  - claim (windows faster at stride 1): " + ("HOLDS" if ratio > 1 else "MISSED")
                ok &= ratio > 1
            lines.append(f"    parent's faster leg / windows, medians = {ratio:.3f}x{verdict}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
