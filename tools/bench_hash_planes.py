#!/usr/bin/env python3
"""What the zero plane costs: the planes call beside the plain call on the same device-resident clips, and the search over
the flipped hashes beside one reference search of the same shape.

    python tools/bench_hash_planes.py --parent-lib tools/_libvdf_parent.so [--out profiles/hash_planes.txt]

Hashing, at 64 x 64 x 100 000 clips and at 1920 x 1080 x 1000 clips (random bytes generated on the device):
  parent   vdf_hash_frames_u8_device of the library built from the PARENT commit (--parent-lib; without it the leg is left out and no
           verdict is given)
  plain    vdf_hash_frames_u8_device of this build
  planes   vdf_hash_frames_u8_planes_device of this build
The planes call writes 128 B more per clip against at least 4 KB read, so it is held against the parent's plain call on the same machine:
it may be slower by no more than the max / min spread of the parent's own runs; the plain call of this build gets the same bound (it shows
that the existing instantiations did not move).  Both verdicts are printed as measured - a miss is reported, the bound is not tuned.
Search: vdf_search_variants_device with 1 and with 3 variants beside one vdf_search_refs_device of the same shape (n references against
the same n candidates).
Every leg runs in a fresh child process (one library per process), the legs take turns ROUNDS times, each turn is one warm-up and REPEATS
timed calls; host clock around calls that end in a device synchronise; min / median / max over all timed calls of a leg.  The hash legs
must produce the same words."""
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
SHAPES = [(64, 64, 100_000), (1920, 1080, 1000)]  # w, h, clips
SEARCH_N = 200_000
REPEATS, ROUNDS = 5, 2
HASH_ARGS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]


class Groups(C.Structure):
    _fields_ = [("n_groups", C.c_uint64), ("offsets", C.c_void_p), ("members", C.c_void_p), ("ref_index", C.c_void_p)]


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


def child_hash(args):
    import torch

    lib, ctx = open_lib(args.lib)
    lib.vdf_hash_frames_u8_device.argtypes = HASH_ARGS + [C.c_void_p]
    if args.leg == "planes":
        lib.vdf_hash_frames_u8_planes_device.argtypes = HASH_ARGS + [C.c_void_p, C.c_void_p]
    res = {}
    for w, h, n in SHAPES:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(w * 7 + h)
        d = torch.empty(n * 16 * w * h, dtype=torch.uint8, device="cuda")
        step = 1 << 30
        for o in range(0, d.numel(), step):  # (in pieces: randint makes an int64 temporary)
            m = min(step, d.numel() - o)
            d[o:o + m] = torch.randint(0, 256, (m,), generator=gen, device="cuda", dtype=torch.uint8)
        out = torch.zeros((n, 16), dtype=torch.int64, device="cuda")
        zero = torch.zeros((n, 16), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def run():
            if args.leg == "planes":
                rc = lib.vdf_hash_frames_u8_planes_device(ctx, d.data_ptr(), n, 16, w, h, w * h, 16 * w * h, out.data_ptr(), None, zero.data_ptr(), None)
            else:
                rc = lib.vdf_hash_frames_u8_device(ctx, d.data_ptr(), n, 16, w, h, w * h, 16 * w * h, out.data_ptr(), None, None)
            assert rc == 0, (rc, lib.vdf_last_error(ctx))
            torch.cuda.synchronize()

        times = timed(run)
        words = out.cpu().numpy()
        res[f"{w}x{h}"] = {"times": times, "digest": int(np.bitwise_xor.reduce(words.view(np.uint64).reshape(-1) * np.arange(1, words.size + 1, dtype=np.uint64))),
                           "zero_bits": int(np.unpackbits(zero.cpu().numpy().view(np.uint8)).sum())}
        del d, out, zero
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def child_search(args):
    import torch

    lib, ctx = open_lib(args.lib)
    n = SEARCH_N
    rng = np.random.default_rng(5)
    h = rng.integers(0, 2**64, size=(n, 16), dtype=np.uint64)
    h[:, 15] &= np.uint64((1 << 40) - 1)
    zb = (rng.random((n, 1024)) < 0.01).astype(np.uint8)
    zb[:, 1000:] = 0
    z = np.packbits(zb, axis=1, bitorder="little").view(np.uint64).copy()
    h &= ~z
    for k in range(0, n - 1, 1000):  # a mirrored near-duplicate every 1000 entries: the searches have something to report
        i = np.arange(1000)
        m = np.zeros(1024, np.uint8)
        m[:1000] = ((i // 10) % 10) & 1
        h[k + 1] = ((h[k] ^ np.packbits(m, bitorder="little").view(np.uint64)) & ~z[k]) & ~z[k + 1]
    d = np.sort(rng.integers(10, 7200, size=n).astype(np.uint32))
    dh, dz, dd = (torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda() for a in (h, z, d))
    cap = 1 << 22
    hits = np.zeros((cap, 2), np.uint32)
    n_hits = C.c_uint64(0)
    lib.vdf_search_refs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    lib.vdf_search_variants_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(Groups), C.c_void_p]
    lib.vdf_groups_free.argtypes = [C.POINTER(Groups)]
    torch.cuda.synchronize()
    found = {}

    def refs():
        rc = lib.vdf_search_refs_device(ctx, dh.data_ptr(), dd.data_ptr(), n, dh.data_ptr(), dd.data_ptr(), n, 350, 0, hits.ctypes.data, cap, C.byref(n_hits), None)
        assert rc == 0, (rc, lib.vdf_last_error(ctx))
        found["refs"] = int(n_hits.value)

    def variants(mask, name):
        def run():
            g = (Groups * 8)()
            rc = lib.vdf_search_variants_device(ctx, dh.data_ptr(), dz.data_ptr(), dd.data_ptr(), n, 350, mask, g, None)
            assert rc == 0, (rc, lib.vdf_last_error(ctx))
            found[name] = [int(g[v].n_groups) for v in range(8)]
            for v in range(8):
                lib.vdf_groups_free(C.byref(g[v]))
        return run

    res = {"refs": timed(refs), "variants1": timed(variants(2, "variants1")), "variants3": timed(variants(2 | 4 | 8, "variants3")), "found": found}
    print("RESULT " + json.dumps(res))


def run_child(lib, leg, what):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--lib", lib, "--leg", leg], capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child {what} / {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads(line[-1][7:])


def stats(ts):
    return min(ts), statistics.median(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_planes.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="plain")
    args = ap.parse_args()
    if args.child == "hash":
        return child_hash(args)
    if args.child == "search":
        return child_search(args)
    legs = ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else []) + [("plain", args.lib), ("planes", args.lib)]
    times = {leg: {f"{w}x{h}": [] for w, h, _ in SHAPES} for leg, _ in legs}
    digests = {}
    lines = [f"tools/bench_hash_planes.py: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn"]
    for _ in range(ROUNDS):
        for leg, lib in legs:
            r = run_child(lib, leg, "hash")
            for shape, v in r.items():
                times[leg][shape] += v["times"]
                digests.setdefault(shape, {})[leg] = (v["digest"], v["zero_bits"])
    ok = True
    for w, h, n in SHAPES:
        shape = f"{w}x{h}"
        same = len({d[0] for d in digests[shape].values()}) == 1
        ok &= same
        gb = n * 16 * w * h / 1e9
        lines.append(f"\n{w} x {h} x {n} clips ({gb:.2f} GB of frames), device-resident; hash words of all legs {'equal' if same else 'DIFFER'}; "
                     f"zero-plane bits set: {digests[shape]['planes'][1]}")
        lines.append(f"  {'leg':8s} {'min ms':>9s} {'median':>9s} {'max':>9s}   TB/s at the median")
        for leg, _ in legs:
            lo, med, hi = stats(times[leg][shape])
            lines.append(f"  {leg:8s} {lo * 1e3:9.3f} {med * 1e3:9.3f} {hi * 1e3:9.3f}   {gb / med / 1e3:.2f}")
        if args.parent_lib:
            plo, pmed, phi = stats(times["parent"][shape])
            spread = phi / plo
            lines.append(f"  parent's own spread max / min = {spread:.4f}: the bound for the medians below")
            for leg in ("plain", "planes"):
                ratio = stats(times[leg][shape])[1] / pmed
                verdict = "within the bound" if ratio <= spread else "MISSES the bound"
                ok &= ratio <= spread
                lines.append(f"  {leg:8s} median / parent median = {ratio:.4f}: {verdict}")
        else:
            lines.append("  no --parent-lib: no verdict")
    s = run_child(args.lib, "plain", "search")
    lines.append(f"\nsearch, {SEARCH_N} hashes against themselves (tolerance 350, a mirrored near-duplicate every 1000 entries), device-resident")
    lines.append(f"  {'call':34s} {'min ms':>9s} {'median':>9s} {'max':>9s}")
    for key, name in (("refs", "vdf_search_refs_device (n x n)"), ("variants1", "vdf_search_variants_device, 1 variant"), ("variants3", "vdf_search_variants_device, 3 variants")):
        lo, med, hi = stats(s[key])
        lines.append(f"  {name:34s} {lo * 1e3:9.3f} {med * 1e3:9.3f} {hi * 1e3:9.3f}")
    lines.append(f"  found: {s['found']}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
