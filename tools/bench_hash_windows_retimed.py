#!/usr/bin/env python3
"""What the retimed windows call costs: vdf_hash_windows_u8_retimed_device of this build beside the two things it can be held against,
on the same device-resident frames.

    python tools/bench_hash_windows_retimed.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_windows_retimed.txt]

Input (random bytes generated on the device): one clip of 1920 x 1080 x 256 frames, and 1000 clips of 64 x 64 x 64 frames; stride 1; rates 6/5 and 2/1.
Legs:
  retimed   vdf_hash_windows_u8_retimed_device of this build: one call
  gather    (a) the only route the PARENT commit's library (--parent-lib; without it this build's own plain call stands in and is labelled so) has to
            these words: the 16 frames of every window gathered into a stack on the device (torch index_select, timed with the call), then ONE
            vdf_hash_frames_u8_device call over the stacks (a device synchronise between the two: they run on different streams).  The words must equal the retimed leg's.
  windows   (b) vdf_hash_windows_u8_device of this build at the same F and stride: the same frame reads and resize stage, the plain kernel at three
            workgroups per CU instead of two, span - 16 more windows per clip (other words: not compared)
Nothing is gated: the ratios are reported.  Every leg runs in a fresh child process (one library per process), the legs take turns ROUNDS times, each turn
is one warm-up and REPEATS timed calls; host clock around calls that end in a device synchronise; min / median over all timed calls of a leg.
At 1920 x 1080 the gather leg is run in slabs of windows (its stacks are 16 x the frames) and the slabs' times are summed.

    python tools/bench_hash_windows_retimed.py --align [--out ...]     (appends to the same file)

align_retimed on 1000 x 49 retimed windows against 1000 x 49 plain windows at 6/5 (random hashes with planted copies) beside ONE plain `align` call on
the cells the composition walks (the windows of A against every fifth window of B): time and launches (calls of the C ABI) of each."""
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
RATES = [(6, 5), (2, 1)]
STRIDE = 1
REPEATS, ROUNDS = 6, 2
GATHER_SLAB_BYTES = 6 << 30
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
    if args.leg == "retimed":
        lib.vdf_hash_windows_u8_retimed_device.argtypes = HASH_ARGS + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    res = {}
    for w, h, n, nf in SHAPES:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(w * 7 + h)
        d = torch.randint(0, 256, (n * nf * w * h,), generator=gen, device="cuda", dtype=torch.uint8)
        fs = w * h
        for num, den in RATES:
            taps = [(i * num) // den for i in range(16)]
            span = taps[15] + 1
            n_win = (nf - 16) // STRIDE + 1 if args.leg == "windows" else (nf - span) // STRIDE + 1
            out = torch.zeros((n * n_win, 16), dtype=torch.int64, device="cuda")
            if args.leg == "gather":  # frame index of (clip, window, tap) in the buffer, and the windows of one slab
                idx = (torch.arange(n, device="cuda")[:, None, None] * nf + torch.arange(n_win, device="cuda")[None, :, None] * STRIDE
                       + torch.tensor(taps, device="cuda")[None, None, :]).reshape(-1, 16)
                slab = max(1, min(n * n_win, GATHER_SLAB_BYTES // (16 * fs)))
                frames = d.view(n * nf, fs)
            torch.cuda.synchronize()

            def run():
                if args.leg == "retimed":
                    rc = lib.vdf_hash_windows_u8_retimed_device(ctx, d.data_ptr(), n, nf, w, h, fs, nf * fs, STRIDE, num, den, out.data_ptr(), None, None)
                elif args.leg == "windows":
                    rc = lib.vdf_hash_windows_u8_device(ctx, d.data_ptr(), n, nf, w, h, fs, nf * fs, STRIDE, out.data_ptr(), None, None)
                else:
                    rc = 0
                    for k0 in range(0, n * n_win, slab):
                        k1 = min(k0 + slab, n * n_win)
                        stacks = frames.index_select(0, idx[k0:k1].reshape(-1))
                        torch.cuda.synchronize()  # the gather runs on torch's stream, the hash call on the context's: nothing else orders them
                        rc = rc or lib.vdf_hash_frames_u8_device(ctx, stacks.data_ptr(), k1 - k0, 16, w, h, fs, 16 * fs, out.data_ptr() + k0 * 128, None, None)
                        torch.cuda.synchronize()
                        del stacks
                assert rc == 0, (rc, lib.vdf_last_error(ctx))
                torch.cuda.synchronize()

            times = timed(run)
            res[f"{w}x{h}/{num}_{den}"] = {"times": times, "digest": digest(out.cpu().numpy()), "n_win": n * n_win}
            del out
        del d
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def align_child(args):
    sys.path.insert(0, ROOT)
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(5)
    n_videos, n_win, rate = 1000, 49, (6, 5)

    def library():
        words = rng.integers(0, 2**64, size=(n_videos, n_win, 16), dtype=np.uint64)
        words[:, :, 15] &= np.uint64((1 << 40) - 1)
        return words

    wa, wb = library(), library()
    for v in range(0, n_videos, 10):  # every tenth video of B is a copy of the same video of A at 6/5, from A's frame 7: B window 5 m = A window 7 + 6 m
        for m in range(7):
            wb[v, 5 * m] = wa[v, 7 + 6 * m]
    mk = lambda words, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10) for w in ws] for i, ws in enumerate(words)]
    va, vb = mk(wa, "a"), mk(wb, "b")
    eng = vdf.Engine(0)
    calls = {"n": 0}
    for name in ("align_windows", "align_windows_pairs", "align_seed_pairs"):
        def counted(*a, _f=getattr(eng, name), **kw):
            calls["n"] += 1
            return _f(*a, **kw)
        setattr(eng, name, counted)
    res = {}
    for leg, run in (("align_retimed", lambda: vdf.align_retimed(va, vb, rate, 0.35, min_run=2, engine=eng)),
                     ("align_retimed seeded", lambda: vdf.align_retimed(va, vb, rate, 0.35, min_run=2, engine=eng, seed=True)),
                     ("align, same cells", lambda: vdf.align(va, [ws[0::5] for ws in vb], 0.35, min_run=2, engine=eng))):
        calls["n"] = 0
        found = len(run())
        per_call = calls["n"]
        res[leg] = {"times": timed(run), "records": found, "abi_calls": per_call}
    eng.close()
    print("RESULT " + json.dumps(res))


def run_child(lib, leg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--leg", leg], capture_output=True, text=True, timeout=1100)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    print(f"[{leg}: done]", file=sys.stderr, flush=True)
    return json.loads(line[-1][7:])


def align_main(args):
    res = run_child(args.lib, "align")
    lines = ["", f"tools/bench_hash_windows_retimed.py --align: 1000 videos x 49 retimed windows against 1000 videos x 49 plain windows, rate 6/5, tolerance 0.35, min_run 2;",
             f"one warm-up and {REPEATS} timed calls per leg, host clock around the whole Python call (CSR build, C ABI calls, record mapping)",
             "align, same cells = ONE align call of the windows of A against every fifth window of B: the cells the six sub-calls walk between them",
             f"  {'leg':22s} {'min ms':>9s} {'median':>9s}   records   C ABI calls per call"]
    for leg, v in res.items():
        lines.append(f"  {leg:22s} {min(v['times']) * 1e3:9.1f} {statistics.median(v['times']) * 1e3:9.1f}   {v['records']:7d}   {v['abi_calls']}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "a") as f:
        f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_windows_retimed.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="retimed")
    args = ap.parse_args()
    if args.child:
        return align_child(args) if args.leg == "align" else child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if args.align:
        return align_main(args)
    plain_lib = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("retimed", args.lib), ("gather", plain_lib), ("windows", args.lib)]
    times, digests, counts = {}, {}, {}
    for _ in range(ROUNDS):
        for leg, lib in legs:
            for key, v in run_child(lib, leg).items():
                times.setdefault(key, {}).setdefault(leg, []).extend(v["times"])
                digests.setdefault(key, {})[leg] = v["digest"]
                counts.setdefault(key, {})[leg] = v["n_win"]
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's plain call (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_hash_windows_retimed.py: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"retimed = vdf_hash_windows_u8_retimed_device, windows = vdf_hash_windows_u8_device of this build; gather = device gather + vdf_hash_frames_u8_device of {whose}",
             f"stride {STRIDE}; nothing gated"]
    ok = True
    for w, h, n, nf in SHAPES:
        lines.append(f"\n{n} clip(s) of {w} x {h} x {nf} frames, device-resident")
        for num, den in RATES:
            key = f"{w}x{h}/{num}_{den}"
            same = digests[key]["retimed"] == digests[key]["gather"]
            ok &= same
            lines.append(f"  rate {num}/{den}: {counts[key]['retimed']} retimed windows ({counts[key]['windows']} plain); words of retimed and gather {'equal' if same else 'DIFFER'}")
            lines.append(f"    {'leg':9s} {'min ms':>9s} {'median':>9s} {'max':>9s}   runs")
            for leg, _ in legs:
                ts = times[key][leg]
                lines.append(f"    {leg:9s} {min(ts) * 1e3:9.3f} {statistics.median(ts) * 1e3:9.3f} {max(ts) * 1e3:9.3f}   {len(ts)}")
            med = {leg: statistics.median(times[key][leg]) for leg, _ in legs}
            lines.append(f"    (a) gather / retimed, medians = {med['gather'] / med['retimed']:.3f}x      (b) retimed / windows, medians = {med['retimed'] / med['windows']:.3f}x")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
