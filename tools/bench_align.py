#!/usr/bin/env python3
"""What aligning videos on the device buys: vdf_align_windows_device of this build beside the only way to get the same
answer from the parent commit - its reference search of all A windows against all B windows with every duration 0, the hit list brought
down, and the runs aggregated in numpy - on the same device-resident window hashes.

    python tools/bench_align.py --parent-lib tools/_libvdf_parent.so [--out profiles/align_windows.txt]

Shapes: 1000 videos x 49 windows against each other (self mode); 2 videos x 7185 windows (self mode: one pair, 225 bands); 64 x 64 videos x
1000 windows.  Corpora: `plain` - random hashes with planted shifted copies (0 .. 40 flipped bits per window); `static` - the same with a
stretch of 10 % of every video's windows replaced by ONE static hash, so that every pair of videos shares static cells; `static+skip`
(align only) - the static windows flagged in the skip bytes.
Legs, each in a fresh child process, taking turns ROUNDS times, each turn one warm-up and REPEATS timed calls per (shape, corpus); host
clock around calls that end in a device synchronise:
  align    vdf_align_windows_device, capacity = all pairs
  parent   vdf_search_refs_device of the library built from the PARENT commit (--parent-lib; without it this build's own search stands in
           and is labelled so) with a 2^24-entry hit buffer, then the aggregation; on an overflow the call is timed as far as it got and
           the answer is reported as not available
The records of both legs must be equal wherever the parent leg has an answer.  The one claim under test: the align call's time on the
static corpus is that of the plain corpus within the run-to-run spread of the 12 calls.  cells/s is printed beside the VALU search
backend's measured 7.5e11 pairs/s (README): the yardstick of this inner loop, not a gate.

    python tools/bench_align.py --variants [--out profiles/align_variants.txt]

What alignment against the variants costs, on the 1000 x 49 self shape, plain corpus, with random zero planes (5 % of the
bits): vdf_align_windows_variants_device with 1 and with 3 variants beside ONE vdf_align_windows_device call and one
vdf_window_variants_device call, all of this build, same protocol.  Expected: plain x variants + derive x variants.  Reported; nothing is
gated.

    python tools/bench_align.py --stretches --parent-lib tools/_libvdf_parent.so [--out profiles/align_stretches.txt]

What reporting every stretch of a pair costs, on the 1000 x 49 self shape, device-resident input, max_stretches 4, guard 2.
Leg (a): the shape's random hashes WITHOUT planted copies - no pair has a record, so no second round is launched and the call runs the plain
kernel once, as vdf_align_windows_device does: vdf_align_windows_stretches_device of this build beside vdf_align_windows_device of the parent
commit's library (without --parent-lib this build's stands in and is labelled so).  GATE: the new call's median is at most the parent's
median times the parent's own max / min over its 12 calls.  Leg (b): the same hashes with 0.99 % of the pairs (90 groups of 11 videos) sharing
two planted stretches of 12 windows on two different diagonals: the time, the rounds and the surviving pairs per round, beside leg (a) - no
gate.

    python tools/bench_align.py --seeded --parent-lib tools/_libvdf_parent.so [--out profiles/align_seeded.txt]

What seeding the candidate pairs buys, same protocol.  The seeded path on device arrays is vdf_align_seed_pairs_device and
then, if there is a candidate, vdf_align_windows_pairs_device on the candidates.  Leg (a): the no-copies corpus of --stretches (1000 x 49 self,
device-resident; no candidate), min_run 2 and 4, beside vdf_align_windows_device of the parent commit's library.  GATE: the seeded median is
below the parent's median divided by the parent's own max / min over its 12 calls - faster by more than the parent's noise - at both min_run.
Leg (b): the planted corpus of --stretches (0.99 % of the pairs share stretches), min_run 2: the seeded path beside this build's all-pairs
call; the records must be equal.  Leg (c): 8000 videos x 49 windows, self mode, host lists through api.align (three blocks of videos):
seed=True beside seed=False, equal lists.  Leg (d): leg (a) at min_run 1, where every window is a seed and the filter saves no distance
work.  Only leg (a) is gated.

    python tools/bench_align.py --seeded-variants --parent-lib tools/_libvdf_parent.so [--out profiles/align_seeded_variants.txt]

The candidates of the flipped alignment from ONE pass over the seeds (vdf_align_seed_pairs_variants_device) beside what the
parent commit's library offers for the same question - per requested variant vdf_window_variants_device, then vdf_align_seed_pairs_device on the
derived set - for 1, 3 and 7 variants, min_run 2 and 4, on the 1000 x 49 corpus with zero planes, without and with related pairs; the candidate
lists must be equal.  GATE: at 7 variants the one-pass median is below the composition's median divided by the composition's own max / min over
its 12 calls.  End to end: the parent's vdf_align_windows_variants_device beside seed + vdf_align_windows_variants_pairs_device, records equal."""
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
TOL, MIN_RUN = 350, 2
HIT_CAPACITY = 1 << 24
VALU_PAIRS_PER_S = 7.5e11
SHAPES = {"1000x49 self": (1000, 49, None), "2x7185 self": (2, 7185, None), "64x64x1000": (64, 1000, 64)}
ALIGN_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("offset", "<i4"), ("start_a", "<u4"), ("n_windows", "<u4"), ("dist_sum", "<u4")])


def random_hashes(rng, n):
    w = rng.integers(0, 2**64, size=(n, 16), dtype=np.uint64)
    w[:, 15] &= np.uint64((1 << 40) - 1)
    return w


def flip_bits(rng, rows):
    """0 .. 40 flipped bits per row"""
    out = rows.copy()
    for r in out:
        for pos in rng.choice(1000, size=int(rng.integers(0, 41)), replace=False):
            r[pos >> 6] ^= np.uint64(1) << np.uint64(pos & 63)
    return out


def corpus(shape, static):
    """-> a_hashes, a_first, b_hashes | None, b_first | None, a_skip, b_skip (the static windows)"""
    n_a, n_win, n_b = SHAPES[shape]
    rng = np.random.default_rng([11, n_a, n_win])
    a, fa = random_hashes(rng, n_a * n_win), np.arange(n_a + 1, dtype=np.uint32) * n_win
    b, fb = (None, None) if n_b is None else (random_hashes(rng, n_b * n_win), np.arange(n_b + 1, dtype=np.uint32) * n_win)
    length = n_win // 2
    if n_b is None:  # every tenth video holds a shifted copy of half of its predecessor
        for v in range(1, n_a, 10 if n_a > 2 else 1):
            s, t = int(rng.integers(0, n_win - length + 1)), int(rng.integers(0, n_win - length + 1))
            a[v * n_win + s:v * n_win + s + length] = flip_bits(rng, a[(v - 1) * n_win + t:(v - 1) * n_win + t + length])
    else:
        for v in range(0, n_b, 4):
            s, t = int(rng.integers(0, n_win - length + 1)), int(rng.integers(0, n_win - length + 1))
            b[v * n_win + s:v * n_win + s + length] = flip_bits(rng, a[v * n_win + t:v * n_win + t + length])
    ska, skb = np.zeros(len(a), np.uint8), None if b is None else np.zeros(len(b), np.uint8)
    if static:
        one = random_hashes(rng, 1)[0]
        k = max(1, n_win // 10)
        for h, sk, n in ((a, ska, n_a),) + (() if b is None else ((b, skb, n_b),)):
            for v in range(n):
                s = int(rng.integers(0, n_win - k + 1))
                h[v * n_win + s:v * n_win + s + k] = one
                sk[v * n_win + s:v * n_win + s + k] = 1
    return a, fa, b, fb, ska, skb


POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def aggregate(hits, a, fa, b, fb, self_mode):
    """the runs of a (row = window of A, col = window of B) hit list, the best per pair of videos: the definition of include/vdf.h in numpy"""
    ra, cb = hits[:, 0].astype(np.int64), hits[:, 1].astype(np.int64)
    va, vb = np.searchsorted(fa, ra, side="right") - 1, np.searchsorted(fb, cb, side="right") - 1
    if self_mode:
        keep = va < vb
        ra, cb, va, vb = ra[keep], cb[keep], va[keep], vb[keep]
    ka, kb = ra - fa[va], cb - fb[vb]
    dist = np.zeros(len(ra), np.int64)
    for i in range(0, len(ra), 1 << 18):
        dist[i:i + (1 << 18)] = POP8[(a[ra[i:i + (1 << 18)]] ^ b[cb[i:i + (1 << 18)]]).view(np.uint8)].sum(axis=1)
    off = kb - ka
    order = np.lexsort((ka, off, vb, va))
    va, vb, off, ka, dist = va[order], vb[order], off[order], ka[order], dist[order]
    if len(va) == 0:
        return np.zeros(0, ALIGN_DTYPE)
    new = np.ones(len(va), bool)
    new[1:] = (va[1:] != va[:-1]) | (vb[1:] != vb[:-1]) | (off[1:] != off[:-1]) | (ka[1:] != ka[:-1] + 1)
    first = np.flatnonzero(new)
    n = np.diff(np.append(first, len(va)))
    s = np.add.reduceat(dist, first)
    ok = n >= MIN_RUN
    first, n, s = first[ok], n[ok], s[ok]
    score = n * (TOL + 1) - s
    pick = np.lexsort((ka[first], off[first], -score, vb[first], va[first]))
    first, n, s = first[pick], n[pick], s[pick]
    lead = np.ones(len(first), bool)
    lead[1:] = (va[first][1:] != va[first][:-1]) | (vb[first][1:] != vb[first][:-1])
    first, n, s = first[lead], n[lead], s[lead]
    out = np.zeros(len(first), ALIGN_DTYPE)
    out["a"], out["b"], out["offset"], out["start_a"], out["n_windows"], out["dist_sum"] = va[first], vb[first], off[first], ka[first], n, s
    return out


def digest(rec):
    w = np.ascontiguousarray(rec).view(np.uint32).astype(np.uint64).reshape(-1)
    return int(np.bitwise_xor.reduce(w * np.arange(1, w.size + 1, dtype=np.uint64))) if w.size else 0


def child(args):
    import torch

    lib = C.CDLL(args.lib)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    if args.leg == "align":
        lib.vdf_align_windows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    else:
        lib.vdf_search_refs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    dev = lambda x, t: None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(t)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    res = {}
    for shape, (n_a, n_win, n_b) in SHAPES.items():
        self_mode = n_b is None
        pairs = n_a * (n_a - 1) // 2 if self_mode else n_a * n_b
        for kind in ("plain", "static", "static+skip") if args.leg == "align" else ("plain", "static"):
            a, fa, b, fb, ska, skb = corpus(shape, kind != "plain")
            d_a, d_fa, d_b, d_fb = dev(a, np.int64), dev(fa, np.int32), dev(b, np.int64), dev(fb, np.int32)
            d_ska, d_skb = (dev(ska, np.uint8), dev(skb, np.uint8)) if kind == "static+skip" else (None, None)
            torch.cuda.synchronize()
            key = f"{shape}/{kind}"
            if args.leg == "align":
                out = np.zeros(pairs, ALIGN_DTYPE)
                n_out = C.c_size_t(0)

                def run():
                    rc = lib.vdf_align_windows_device(ctx, ptr(d_a), ptr(d_fa), n_a, ptr(d_ska), ptr(d_b), ptr(d_fb), 0 if self_mode else n_b, ptr(d_skb), TOL, MIN_RUN,
                                                      out.ctypes.data, pairs, C.byref(n_out), None)
                    assert rc == 0, (rc, lib.vdf_last_error(ctx))
                times = []
                for r in range(REPEATS + 1):
                    t0 = time.perf_counter()
                    run()
                    if r:
                        times.append(time.perf_counter() - t0)
                res[key] = {"times": times, "records": int(n_out.value), "digest": digest(out[:n_out.value]), "overflow": False}
            else:
                bb, fbb, d_bb = (a, fa, d_a) if self_mode else (b, fb, d_b)
                zeros_a, zeros_b = torch.zeros(len(a), dtype=torch.int32, device="cuda"), torch.zeros(len(bb), dtype=torch.int32, device="cuda")
                hits = np.zeros((HIT_CAPACITY, 2), np.uint32)
                n_hits = C.c_uint64(0)
                torch.cuda.synchronize()
                times, search_times, rec, overflow = [], [], None, False
                for r in range(REPEATS + 1):
                    t0 = time.perf_counter()
                    rc = lib.vdf_search_refs_device(ctx, ptr(d_bb), zeros_b.data_ptr(), len(bb), ptr(d_a), zeros_a.data_ptr(), len(a), TOL, 0, hits.ctypes.data,
                                                    HIT_CAPACITY, C.byref(n_hits), None)
                    t1 = time.perf_counter()
                    overflow = rc == -6 or n_hits.value > HIT_CAPACITY
                    assert rc == 0 or overflow, (rc, lib.vdf_last_error(ctx))
                    rec = None if overflow else aggregate(hits[:n_hits.value], a, fa.astype(np.int64), bb, fbb.astype(np.int64), self_mode)
                    if r:
                        times.append(time.perf_counter() - t0)
                        search_times.append(t1 - t0)
                res[key] = {"times": times, "search_times": search_times, "hits": int(n_hits.value), "overflow": bool(overflow),
                            "records": None if rec is None else len(rec), "digest": None if rec is None else digest(rec)}
            del d_a, d_b
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


VARIANTS_SHAPE = "1000x49 self"
VARIANT_MASKS = {"variants-1": 1 << 1, "variants-3": (1 << 1) | (1 << 4) | (1 << 5)}
ALIGN_VARIANT_DTYPE = np.dtype(ALIGN_DTYPE.descr + [("variant", "<u4")])


def variants_child(args):
    """one leg of --variants: align | derive | variants-1 | variants-3"""
    import torch

    lib = C.CDLL(args.lib)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    P = C.c_void_p
    lib.vdf_align_windows_device.argtypes = [P, P, P, C.c_size_t, P, P, P, C.c_size_t, P, C.c_uint32, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t), P]
    lib.vdf_window_variants_device.argtypes = [P, P, P, P, C.c_size_t, P, C.c_uint32, P, P, P]
    lib.vdf_align_windows_variants_device.argtypes = [P, P, P, P, C.c_size_t, P, P, P, P, C.c_size_t, P, C.c_uint32, C.c_uint32, C.c_uint32, P, C.c_size_t,
                                                      C.POINTER(C.c_size_t), P]
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    pairs = n_a * (n_a - 1) // 2
    a, fa, _, _, _, _ = corpus(VARIANTS_SHAPE, False)
    rng = np.random.default_rng(12)
    zero = np.zeros_like(a)
    for pos in range(1000):
        zero[rng.random(len(a)) < 0.05, pos >> 6] |= np.uint64(1) << np.uint64(pos & 63)
    a &= ~zero
    d_a, d_z, d_fa = (torch.from_numpy(x.view(t)).cuda() for x, t in ((a, np.int64), (zero, np.int64), (fa, np.int32)))
    d_out = torch.zeros_like(d_a)
    torch.cuda.synchronize()
    n_out = C.c_size_t(0)
    if args.leg == "align":
        out = np.zeros(pairs, ALIGN_DTYPE)

        def run():
            return lib.vdf_align_windows_device(ctx, d_a.data_ptr(), d_fa.data_ptr(), n_a, None, None, None, 0, None, TOL, MIN_RUN, out.ctypes.data, pairs, C.byref(n_out), None)
    elif args.leg == "derive":
        out = np.zeros(0, ALIGN_DTYPE)

        def run():
            rc = lib.vdf_window_variants_device(ctx, d_a.data_ptr(), d_z.data_ptr(), d_fa.data_ptr(), n_a, None, 5, d_out.data_ptr(), None, None)
            torch.cuda.synchronize()
            return rc
    else:
        mask = VARIANT_MASKS[args.leg]
        out = np.zeros(pairs * bin(mask).count("1"), ALIGN_VARIANT_DTYPE)

        def run():
            return lib.vdf_align_windows_variants_device(ctx, d_a.data_ptr(), d_z.data_ptr(), d_fa.data_ptr(), n_a, None, None, None, None, 0, None, TOL, MIN_RUN, mask,
                                                         out.ctypes.data, len(out), C.byref(n_out), None)
    times = []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = run()
        if r:
            times.append(time.perf_counter() - t0)
        assert rc == 0, (rc, lib.vdf_last_error(ctx))
    print("RESULT " + json.dumps({"times": times, "records": int(n_out.value)}))


def variants_main(args):
    legs = ["align", "derive"] + list(VARIANT_MASKS)
    got = {leg: {"times": []} for leg in legs}
    for _ in range(ROUNDS):
        for leg in legs:
            v = run_child(args.lib, leg, variants=True)
            got[leg]["times"] += v["times"]
            got[leg]["records"] = v["records"]
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    pairs = n_a * (n_a - 1) // 2
    med = {leg: statistics.median(got[leg]["times"]) for leg in legs}
    ms = lambda ts: f"min {min(ts) * 1e3:9.3f}  median {statistics.median(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f} ms ({len(ts)} calls)"
    lines = [f"tools/bench_align.py --variants: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"{VARIANTS_SHAPE}: {pairs} pairs of videos, {n_a * n_win} windows, zero planes with 5 % of the bits; tolerance {TOL}, min_run {MIN_RUN}; all legs of this build",
             f"  align       {ms(got['align']['times'])}  {got['align']['records']} records   (one vdf_align_windows_device call)",
             f"  derive      {ms(got['derive']['times'])}   (one vdf_window_variants_device call and the wait for it)"]
    for leg, mask in VARIANT_MASKS.items():
        k = bin(mask).count("1")
        expected = k * (med["align"] + med["derive"])
        lines.append(f"  {leg:11s} {ms(got[leg]['times'])}  {got[leg]['records']} records; expected {k} x (align + derive) = {expected * 1e3:.3f} ms: measured / expected = "
                     f"{med[leg] / expected:.3f}x")
    lines.append("nothing is gated")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


STRETCH_DTYPE = np.dtype(ALIGN_DTYPE.descr + [("rank", "<u4")])
STRETCH_MAX, STRETCH_GUARD, STRETCH_GROUP, STRETCH_LEN = 4, 2, 11, 12


def stretches_corpus(planted):
    """the 1000 x 49 self shape: random hashes; planted: in every group of 11 consecutive videos (90 groups) all videos hold the same two
    stretches of 12 windows, video i of a group at windows i and 35 - i - so the pair (i, j) shares them on the diagonals j - i and i - j"""
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    rng = np.random.default_rng([13, n_a, n_win])
    a, fa = random_hashes(rng, n_a * n_win), np.arange(n_a + 1, dtype=np.uint32) * n_win
    pairs = 0
    if planted:
        for g in range(n_a // STRETCH_GROUP):
            one, two = random_hashes(rng, STRETCH_LEN), random_hashes(rng, STRETCH_LEN)
            for i in range(STRETCH_GROUP):
                v = (g * STRETCH_GROUP + i) * n_win
                a[v + i:v + i + STRETCH_LEN] = flip_bits(rng, one)
                a[v + 35 - i:v + 35 - i + STRETCH_LEN] = flip_bits(rng, two)
            pairs += STRETCH_GROUP * (STRETCH_GROUP - 1) // 2
    return a, fa, pairs


def stretches_child(args):
    """one leg of --stretches: parent-align (vdf_align_windows_device of args.lib) | stretches-a | stretches-b"""
    import torch

    lib = C.CDLL(args.lib)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    P = C.c_void_p
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    pairs = n_a * (n_a - 1) // 2
    a, fa, _ = stretches_corpus(args.leg == "stretches-b")
    d_a, d_fa = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(fa.view(np.int32)).cuda()
    torch.cuda.synchronize()
    n_out = C.c_size_t(0)
    if args.leg == "parent-align":
        lib.vdf_align_windows_device.argtypes = [P, P, P, C.c_size_t, P, P, P, C.c_size_t, P, C.c_uint32, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t), P]
        out = np.zeros(pairs, ALIGN_DTYPE)

        def run():
            return lib.vdf_align_windows_device(ctx, d_a.data_ptr(), d_fa.data_ptr(), n_a, None, None, None, 0, None, TOL, MIN_RUN, out.ctypes.data, len(out), C.byref(n_out), None)
    else:
        lib.vdf_align_windows_stretches_device.argtypes = [P, P, P, C.c_size_t, P, P, P, C.c_size_t, P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P, C.c_size_t,
                                                           C.POINTER(C.c_size_t), P]
        out = np.zeros(pairs, STRETCH_DTYPE)  # room for one record per pair: the planted legs find far fewer

        def run():
            return lib.vdf_align_windows_stretches_device(ctx, d_a.data_ptr(), d_fa.data_ptr(), n_a, None, None, None, 0, None, TOL, MIN_RUN, STRETCH_MAX, STRETCH_GUARD,
                                                          out.ctypes.data, len(out), C.byref(n_out), None)
    times = []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = run()
        if r:
            times.append(time.perf_counter() - t0)
        assert rc == 0, (rc, lib.vdf_last_error(ctx))
    res = {"times": times, "records": int(n_out.value)}
    if args.leg != "parent-align":
        rec = out[:n_out.value]
        res["per_rank"] = [int((rec["rank"] == r).sum()) for r in range(STRETCH_MAX)]
    print("RESULT " + json.dumps(res))


def stretches_main(args):
    parent_lib = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("parent-align", parent_lib), ("stretches-a", args.lib), ("stretches-b", args.lib)]
    got = {leg: {"times": []} for leg, _ in legs}
    for _ in range(ROUNDS):
        for leg, lib in legs:
            v = run_child(lib, leg, mode="--stretches")
            got[leg]["times"] += v["times"]
            got[leg].update({k: v[k] for k in v if k != "times"})
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    pairs = n_a * (n_a - 1) // 2
    _, _, planted = stretches_corpus(True)
    med = {leg: statistics.median(got[leg]["times"]) for leg, _ in legs}
    ms = lambda ts: f"min {min(ts) * 1e3:9.3f}  median {statistics.median(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f} ms ({len(ts)} calls)"
    pt = got["parent-align"]["times"]
    spread = max(pt) / min(pt)
    bound = med["parent-align"] * spread
    held = med["stretches-a"] <= bound
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"

    def rounds(per_rank):
        """round 0 always runs; round r runs on the pairs that had a record of rank r - 1, while r < max_stretches"""
        out = [f"round 0: {pairs} pairs"]
        for r in range(1, STRETCH_MAX):
            if per_rank[r - 1] == 0:
                break
            out.append(f"round {r}: {per_rank[r - 1]} surviving pairs")
        return len(out), ", ".join(out)
    ra, rb = rounds(got["stretches-a"]["per_rank"]), rounds(got["stretches-b"]["per_rank"])
    lines = [f"tools/bench_align.py --stretches: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"{VARIANTS_SHAPE}: {pairs} pairs of videos, {n_a * n_win} windows, device-resident; tolerance {TOL}, min_run {MIN_RUN}, max_stretches {STRETCH_MAX}, guard {STRETCH_GUARD}",
             "leg (a): random hashes without planted copies - no pair has a record",
             f"  parent align   {ms(pt)}  {got['parent-align']['records']} records   (vdf_align_windows_device of {whose})",
             f"  stretches (a)  {ms(got['stretches-a']['times'])}  {got['stretches-a']['records']} records; {ra[0]} round(s): {ra[1]}",
             f"  GATE: median {med['stretches-a'] * 1e3:.3f} ms <= parent median {med['parent-align'] * 1e3:.3f} ms x parent max / min {spread:.3f} = {bound * 1e3:.3f} ms: "
             f"{'HOLDS' if held else 'MISSED'}   (stretches / parent, medians = {med['stretches-a'] / med['parent-align']:.3f}x)",
             f"leg (b): {planted} pairs ({100.0 * planted / pairs:.2f} %) share two planted stretches of {STRETCH_LEN} windows on two diagonals",
             f"  stretches (b)  {ms(got['stretches-b']['times'])}  {got['stretches-b']['records']} records, per rank {got['stretches-b']['per_rank']}; {rb[0]} round(s): {rb[1]}",
             f"  (b) - (a), medians = {(med['stretches-b'] - med['stretches-a']) * 1e3:.3f} ms for {rb[0] - 1} more round(s); no gate"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if held else 1


SEEDED_API_VIDEOS = 8000


def seeded_child(args):
    """one leg of --seeded: parent-a (vdf_align_windows_device of args.lib at min_run 1, 2, 4) | seeded-a | b | api-plain | api-seeded"""
    import torch

    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    if args.leg.startswith("api-"):
        sys.path.insert(0, ROOT)
        import vid_dup_finder_lib_amd as vdf

        rng = np.random.default_rng([14, SEEDED_API_VIDEOS, n_win])
        words = random_hashes(rng, SEEDED_API_VIDEOS * n_win)
        for v in range(1, SEEDED_API_VIDEOS, 100):  # every hundredth video holds 24 windows of its predecessor, shifted
            words[v * n_win + 5:v * n_win + 29] = flip_bits(rng, words[(v - 1) * n_win + 11:(v - 1) * n_win + 35])
        wins = [[vdf.VideoHash(words[v * n_win + k], f"/v/{v}.mp4", 1) for k in range(n_win)] for v in range(SEEDED_API_VIDEOS)]
        eng = vdf.Engine(0)
        times, got = [], None
        for r in range(REPEATS + 1):
            t0 = time.perf_counter()
            got = vdf.align(wins, min_run=MIN_RUN, engine=eng, seed=args.leg == "api-seeded")
            if r:
                times.append(time.perf_counter() - t0)
        rec = np.array([(g.a, g.b, g.offset_frames, g.first_frame_a, g.n_windows, round(g.mean_distance * g.n_windows)) for g in got], ALIGN_DTYPE)
        eng.close()
        print("RESULT " + json.dumps({"api": {"times": times, "records": len(got), "digest": digest(rec)}}))
        return
    lib = C.CDLL(args.lib)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    P = C.c_void_p
    sides = [P, P, P, C.c_size_t, P, P, P, C.c_size_t, P]
    lib.vdf_align_windows_device.argtypes = sides + [C.c_uint32, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t), P]
    if args.leg != "parent-a":
        lib.vdf_align_seed_pairs_device.argtypes = sides + [C.c_uint32, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t), P]
        lib.vdf_align_windows_pairs_device.argtypes = sides + [P, C.c_size_t, C.c_uint32, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t), P]
    pairs = n_a * (n_a - 1) // 2
    a, fa, _ = stretches_corpus(args.leg == "b")
    d_a, d_fa = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(fa.view(np.int32)).cuda()
    torch.cuda.synchronize()
    out, cand = np.zeros(pairs, ALIGN_DTYPE), np.zeros(pairs, np.dtype([("a", "<u4"), ("b", "<u4")]))
    n_out, n_cand = C.c_size_t(0), C.c_size_t(0)
    dev = (ctx, d_a.data_ptr(), d_fa.data_ptr(), n_a, None, None, None, 0, None)

    def all_pairs(min_run):
        return lib.vdf_align_windows_device(*dev, TOL, min_run, out.ctypes.data, len(out), C.byref(n_out), None)

    def seeded(min_run):
        rc = lib.vdf_align_seed_pairs_device(*dev, TOL, min_run, cand.ctypes.data, len(cand), C.byref(n_cand), None)
        n_out.value = 0
        if rc == 0 and n_cand.value:
            rc = lib.vdf_align_windows_pairs_device(*dev, cand.ctypes.data, n_cand.value, TOL, min_run, out.ctypes.data, len(out), C.byref(n_out), None)
        return rc
    runs = {"parent-a": [("align", m, all_pairs) for m in (1, 2, 4)], "seeded-a": [("seeded", m, seeded) for m in (1, 2, 4)],
            "b": [("align", MIN_RUN, all_pairs), ("seeded", MIN_RUN, seeded)]}[args.leg]
    res = {}
    for name, min_run, run in runs:
        times = []
        for r in range(REPEATS + 1):
            t0 = time.perf_counter()
            rc = run(min_run)
            if r:
                times.append(time.perf_counter() - t0)
            assert rc == 0, (rc, lib.vdf_last_error(ctx))
        res[f"{name}-m{min_run}"] = {"times": times, "records": int(n_out.value), "digest": digest(out[:n_out.value]),
                                     "candidates": int(n_cand.value) if name == "seeded" else None}
    print("RESULT " + json.dumps(res))


def seeded_main(args):
    parent_lib = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("parent-a", parent_lib), ("seeded-a", args.lib), ("b", args.lib), ("api-plain", args.lib), ("api-seeded", args.lib)]
    got = {}
    for _ in range(ROUNDS):
        for leg, lib in legs:
            for key, v in run_child(lib, leg, mode="--seeded").items():
                e = got.setdefault(f"{leg}/{key}", {"times": []})
                e["times"] += v["times"]
                e.update({k: v[k] for k in v if k != "times"})
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    pairs = n_a * (n_a - 1) // 2
    _, _, planted = stretches_corpus(True)
    med = lambda key: statistics.median(got[key]["times"])
    ms = lambda ts: f"min {min(ts) * 1e3:9.3f}  median {statistics.median(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f} ms ({len(ts)} calls)"
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_align.py --seeded: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"{VARIANTS_SHAPE}: {pairs} pairs of videos, {n_a * n_win} windows, device-resident; tolerance {TOL}",
             "seeded = vdf_align_seed_pairs_device, then vdf_align_windows_pairs_device on the candidates if there is one",
             f"leg (a): random hashes without planted copies - no pair is a candidate; all-pairs = vdf_align_windows_device of {whose}"]
    held = True
    for m in (2, 4):
        pt, st = got[f"parent-a/align-m{m}"]["times"], got[f"seeded-a/seeded-m{m}"]
        spread = max(pt) / min(pt)
        bound = statistics.median(pt) / spread
        ok = statistics.median(st["times"]) < bound
        held &= ok
        lines += [f"  min_run {m}  all-pairs  {ms(pt)}  {got[f'parent-a/align-m{m}']['records']} records",
                  f"  min_run {m}  seeded     {ms(st['times'])}  {st['candidates']} candidates, {st['records']} records",
                  f"  GATE min_run {m}: seeded median {statistics.median(st['times']) * 1e3:.3f} ms < parent median {statistics.median(pt) * 1e3:.3f} ms / parent max / min "
                  f"{spread:.3f} = {bound * 1e3:.3f} ms: {'HOLDS' if ok else 'MISSED'}   (all-pairs / seeded, medians = {statistics.median(pt) / statistics.median(st['times']):.2f}x)"]
    al, se = got[f"b/align-m{MIN_RUN}"], got[f"b/seeded-m{MIN_RUN}"]
    same = al["digest"] == se["digest"] and al["records"] == se["records"]
    lines += [f"leg (b): {planted} pairs ({100.0 * planted / pairs:.2f} %) share planted stretches; min_run {MIN_RUN}; both legs of this build",
              f"  all-pairs  {ms(al['times'])}  {al['records']} records",
              f"  seeded     {ms(se['times'])}  {se['candidates']} candidates, {se['records']} records: records of both legs {'equal' if same else 'DIFFER'}; "
              f"all-pairs / seeded, medians = {med(f'b/align-m{MIN_RUN}') / med(f'b/seeded-m{MIN_RUN}'):.2f}x"]
    ap_, as_ = got["api-plain/api"], got["api-seeded/api"]
    same_c = ap_["digest"] == as_["digest"] and ap_["records"] == as_["records"]
    lines += [f"leg (c): {SEEDED_API_VIDEOS} videos x {n_win} windows, self mode, host lists through api.align (three blocks of videos), min_run {MIN_RUN}; host clock around the call",
              f"  seed=False {ms(ap_['times'])}  {ap_['records']} alignments",
              f"  seed=True  {ms(as_['times'])}  {as_['records']} alignments: lists {'equal' if same_c else 'DIFFER'}; seed=False / seed=True, medians = "
              f"{med('api-plain/api') / med('api-seeded/api'):.2f}x   (both legs build the same arrays from the lists and upload them)"]
    p1, s1 = got["parent-a/align-m1"], got["seeded-a/seeded-m1"]
    lines += ["leg (d): leg (a) at min_run 1 - every window is a seed: the seed pass computes every distance the all-pairs call computes, and saves only the walk",
              f"  all-pairs  {ms(p1['times'])}  {p1['records']} records",
              f"  seeded     {ms(s1['times'])}  {s1['candidates']} candidates, {s1['records']} records; all-pairs / seeded, medians = {med('parent-a/align-m1') / med('seeded-a/seeded-m1'):.2f}x",
              "only leg (a) is gated"]
    ok = held and same and same_c
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


SV_MASKS = {"1 variant": 0b00000010, "3 variants": 0b00110010, "7 variants": 0b11111110}
PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4")])
TRIPLE_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("variant", "<u4")])


def seeded_variants_corpus(related):
    """the 1000 x 49 self shape with zero planes of 5 % of the bits; related: every fifth video (index % 5 == 4) is a SOURCE and is left as it
    is; every other video a holds, at windows 9 k ... 9 k + 8 (k < 5), what the variant-v set of the k-th source behind it shows at derived
    rows 5 ... 13, v = (1, 4, 5)[source % 3], with 0 ... 40 bits changed.  All holders of a source use one variant and no source is a holder,
    so nothing chains: 3960 of the 499 500 pairs (0.79 %) share a stretch, each under one of the variants 1, 4, 5."""
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    rng = np.random.default_rng([15, n_a, n_win])
    a, fa = random_hashes(rng, n_a * n_win), np.arange(n_a + 1, dtype=np.uint32) * n_win
    zero = np.zeros_like(a)
    for pos in range(1000):
        zero[rng.random(len(a)) < 0.05, pos >> 6] |= np.uint64(1) << np.uint64(pos & 63)
    a &= ~zero
    planted = 0
    if related:
        masks = {}
        for v in (1, 4, 5):
            m = np.zeros(16, np.uint64)
            for i in range(1000):
                kt, kx, ky = i // 100, (i // 10) % 10, i % 10
                if ((v & 1) * kx + (v >> 1 & 1) * ky + (v >> 2 & 1) * kt) & 1:
                    m[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
            masks[v] = m
        for va in range(n_a):
            if va % 5 == 4:
                continue
            for k in range(5):
                vb = va // 5 * 5 + 4 + 5 * k
                if vb >= n_a:
                    continue
                v = (1, 4, 5)[vb % 3]
                src = np.arange(5, 14)
                if v & 4:
                    src = n_win - 1 - src
                rows = vb * n_win + src
                a[va * n_win + 9 * k:va * n_win + 9 * k + 9] = flip_bits(rng, (a[rows] ^ masks[v]) & ~zero[rows])
                planted += 1
    seeded_variants_corpus.planted = planted
    return a, zero, fa


def seeded_variants_child(args):
    """one leg of --seeded-variants: parent-comp (per variant vdf_window_variants_device + vdf_align_seed_pairs_device of args.lib on the derived
    set) | new (vdf_align_seed_pairs_variants_device) | parent-e2e (vdf_align_windows_variants_device of args.lib) | new-e2e (seed + list call)"""
    import torch

    lib = C.CDLL(args.lib)
    lib.vdf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vdf_last_error.restype = C.c_char_p
    lib.vdf_last_error.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert lib.vdf_ctx_create(0, C.byref(ctx)) == 0, lib.vdf_last_error(None)
    P, S = C.c_void_p, C.c_size_t
    sides, vsides = [P, P, P, S, P, P, P, S, P], [P, P, P, P, S, P, P, P, P, S, P]
    lib.vdf_window_variants_device.argtypes = [P, P, P, P, S, P, C.c_uint32, P, P, P]
    lib.vdf_align_seed_pairs_device.argtypes = sides + [C.c_uint32, C.c_uint32, P, S, C.POINTER(S), P]
    lib.vdf_align_windows_variants_device.argtypes = vsides + [C.c_uint32, C.c_uint32, C.c_uint32, P, S, C.POINTER(S), P]
    if args.leg.startswith("new"):
        lib.vdf_align_seed_pairs_variants_device.argtypes = vsides + [C.c_uint32, C.c_uint32, C.c_uint32, P, S, C.POINTER(S), P]
        lib.vdf_align_windows_variants_pairs_device.argtypes = vsides + [P, S, C.c_uint32, C.c_uint32, P, S, C.POINTER(S), P]
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    res = {}
    for corpus_name in ("unrelated", "related"):
        a, zero, fa = seeded_variants_corpus(corpus_name == "related")
        d_a, d_z, d_fa = (torch.from_numpy(x.view(t)).cuda() for x, t in ((a, np.int64), (zero, np.int64), (fa, np.int32)))
        d_var = torch.zeros_like(d_a)
        torch.cuda.synchronize()
        vdev = (ctx, d_a.data_ptr(), d_z.data_ptr(), d_fa.data_ptr(), n_a, None, None, None, None, 0, None)
        cap = 1 << 22
        pair_buf, triple_buf, rec_buf = np.zeros(cap, PAIR_DTYPE), np.zeros(cap, TRIPLE_DTYPE), np.zeros(cap, ALIGN_VARIANT_DTYPE)
        n_out, n_cand = S(0), S(0)
        state = {}

        def composition(min_run, mask):  # what the parent offers: per variant the derived set, then the plain seed call on (A, derived A) - the whole square
            found = []
            for v in range(1, 8):
                if not mask >> v & 1:
                    continue
                rc = lib.vdf_window_variants_device(ctx, d_a.data_ptr(), d_z.data_ptr(), d_fa.data_ptr(), n_a, None, v, d_var.data_ptr(), None, None)
                if rc:
                    return rc
                rc = lib.vdf_align_seed_pairs_device(ctx, d_a.data_ptr(), d_fa.data_ptr(), n_a, None, d_var.data_ptr(), d_fa.data_ptr(), n_a, None, TOL, min_run,
                                                     pair_buf.ctypes.data, cap, C.byref(n_cand), None)
                if rc:
                    return rc
                p = pair_buf[:n_cand.value]
                p = p[p["a"] < p["b"]]  # the self-mode rule
                t = np.zeros(len(p), TRIPLE_DTYPE)
                t["a"], t["b"], t["variant"] = p["a"], p["b"], v
                found.append(t)
            state["triples"] = np.concatenate(found) if found else np.zeros(0, TRIPLE_DTYPE)
            return 0

        def one_pass(min_run, mask):
            rc = lib.vdf_align_seed_pairs_variants_device(*vdev, TOL, min_run, mask, triple_buf.ctypes.data, cap, C.byref(n_cand), None)
            state["triples"] = triple_buf[:n_cand.value]
            return rc

        def e2e_parent(min_run, mask):
            rc = lib.vdf_align_windows_variants_device(*vdev, TOL, min_run, mask, rec_buf.ctypes.data, cap, C.byref(n_out), None)
            state["records"] = rec_buf[:n_out.value]
            return rc

        def e2e_new(min_run, mask):
            rc = one_pass(min_run, mask)
            n_out.value = 0
            if rc == 0 and n_cand.value:
                rc = lib.vdf_align_windows_variants_pairs_device(*vdev, triple_buf.ctypes.data, n_cand.value, TOL, min_run, rec_buf.ctypes.data, cap, C.byref(n_out), None)
            state["records"] = rec_buf[:n_out.value]
            return rc
        if args.leg in ("parent-comp", "new"):
            run = composition if args.leg == "parent-comp" else one_pass
            runs = [(f"{name}/m{m}", m, mask, run) for m in ((2, 4) if corpus_name == "unrelated" else (2,)) for name, mask in SV_MASKS.items()]
        else:
            if corpus_name == "unrelated":
                continue
            runs = [("e2e/m2", 2, SV_MASKS["7 variants"], e2e_parent if args.leg == "parent-e2e" else e2e_new)]
        for key, min_run, mask, run in runs:
            times = []
            for r in range(REPEATS + 1):
                t0 = time.perf_counter()
                rc = run(min_run, mask)
                if r:
                    times.append(time.perf_counter() - t0)
                assert rc == 0, (rc, lib.vdf_last_error(ctx))
            out = state["records" if key.startswith("e2e") else "triples"]
            res[f"{corpus_name}/{key}"] = {"times": times, "n": int(len(out)), "digest": digest(out)}
    print("RESULT " + json.dumps(res))


def seeded_variants_main(args):
    parent_lib = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    legs = [("parent-comp", parent_lib), ("new", args.lib), ("parent-e2e", parent_lib), ("new-e2e", args.lib)]
    got = {}
    for _ in range(ROUNDS):
        for leg, lib in legs:
            for key, v in run_child(lib, leg, mode="--seeded-variants").items():
                e = got.setdefault(f"{leg}:{key}", {"times": []})
                e["times"] += v["times"]
                e.update({k: v[k] for k in v if k != "times"})
    n_a, n_win, _ = SHAPES[VARIANTS_SHAPE]
    pairs = n_a * (n_a - 1) // 2
    seeded_variants_corpus(True)
    n_planted = seeded_variants_corpus.planted
    med = lambda e: statistics.median(e["times"])
    ms = lambda ts: f"min {min(ts) * 1e3:9.3f}  median {statistics.median(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f} ms ({len(ts)} calls)"
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_align.py --seeded-variants: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"{VARIANTS_SHAPE}: {pairs} pairs of videos, {n_a * n_win} windows, zero planes with 5 % of the bits, device-resident; tolerance {TOL}; host clock around calls that wait",
             f"composition = per requested variant vdf_window_variants_device, then vdf_align_seed_pairs_device on (A, the derived A) of {whose}: the parent has no self",
             "mode against a derived set, so it compares the whole square of videos and the pairs a < b are kept on the host; one pass = vdf_align_seed_pairs_variants_device"]
    ok = True
    for corpus_name, runs in (("unrelated", (2, 4)), ("related", (2,))):
        lines.append(f"corpus '{corpus_name}':" + ("  no pair shares anything" if corpus_name == "unrelated" else f"  {n_planted} pairs ({100.0 * n_planted / pairs:.2f} %) share a stretch planted under variant 1, 4 or 5"))
        for m in runs:
            for name in SV_MASKS:
                pc, nw = got[f"parent-comp:{corpus_name}/{name}/m{m}"], got[f"new:{corpus_name}/{name}/m{m}"]
                same = pc["digest"] == nw["digest"] and pc["n"] == nw["n"]
                ok &= same
                spread = max(pc["times"]) / min(pc["times"])
                lines += [f"  min_run {m}  {name:10s}  composition  {ms(pc['times'])}  {pc['n']} candidates",
                          f"  min_run {m}  {name:10s}  one pass     {ms(nw['times'])}  {nw['n']} candidates: lists {'equal' if same else 'DIFFER'}; composition / one pass, medians = "
                          f"{med(pc) / med(nw):.2f}x  (composition's own max / min {spread:.3f})"]
                if name == "7 variants":
                    bound = med(pc) / spread
                    held = med(nw) < bound
                    ok &= held
                    lines.append(f"  GATE min_run {m}, 7 variants, '{corpus_name}': one-pass median {med(nw) * 1e3:.3f} ms < composition median {med(pc) * 1e3:.3f} ms / its max / min "
                                 f"{spread:.3f} = {bound * 1e3:.3f} ms: {'HOLDS' if held else 'MISSED'}")
    pe, ne = got["parent-e2e:related/e2e/m2"], got["new-e2e:related/e2e/m2"]
    same = pe["digest"] == ne["digest"] and pe["n"] == ne["n"]
    ok &= same
    lines += ["end to end, corpus 'related', 7 variants, min_run 2:",
              f"  vdf_align_windows_variants_device of {whose}  {ms(pe['times'])}  {pe['n']} records",
              f"  seed + vdf_align_windows_variants_pairs_device       {ms(ne['times'])}  {ne['n']} records: records {'equal' if same else 'DIFFER'}; all-pairs / seeded, medians = "
              f"{med(pe) / med(ne):.2f}x",
              "the 1- and 3-variant ratios and the end-to-end leg are reported, not gated; kernel times apart from call times: not measured"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


def run_child(lib, leg, variants=False, mode=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--leg", leg] + (["--variants"] if variants else []) + ([mode] if mode else []),
                         capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"child {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--stretches", action="store_true")
    ap.add_argument("--seeded", action="store_true")
    ap.add_argument("--seeded-variants", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="align")
    args = ap.parse_args()
    if args.child and args.seeded_variants:
        return seeded_variants_child(args)
    if args.child:
        return seeded_child(args) if args.seeded else stretches_child(args) if args.stretches else variants_child(args) if args.variants else child(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "align_seeded_variants.txt" if args.seeded_variants else "align_seeded.txt" if args.seeded else "align_stretches.txt" if args.stretches else "align_variants.txt" if args.variants
                                else "align_windows.txt")
    if args.seeded_variants:
        return seeded_variants_main(args)
    if args.seeded:
        return seeded_main(args)
    if args.stretches:
        return stretches_main(args)
    if args.variants:
        return variants_main(args)
    search_lib = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    got = {}
    for _ in range(ROUNDS):
        for leg, lib in (("align", args.lib), ("parent", search_lib)):
            for key, v in run_child(lib, leg).items():
                e = got.setdefault(key, {}).setdefault(leg, {"times": [], "search_times": []})
                e["times"] += v["times"]
                e["search_times"] += v.get("search_times", [])
                e.update({k: v[k] for k in v if k not in ("times", "search_times")})
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's search (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_align.py: {ROUNDS} rounds x {REPEATS} timed calls per leg (one warm-up per round), fresh process per leg and round, legs in turn",
             f"tolerance {TOL}, min_run {MIN_RUN}; parent leg: vdf_search_refs_device of {whose}, durations 0, {HIT_CAPACITY} hit slots, + numpy aggregation",
             f"cells/s beside the VALU search backend's measured {VALU_PAIRS_PER_S:.2e} pairs/s (README): a yardstick, not a gate"]
    ok = True
    ms = lambda ts: f"min {min(ts) * 1e3:9.3f}  median {statistics.median(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f} ms ({len(ts)} calls)"
    for shape, (n_a, n_win, n_b) in SHAPES.items():
        pairs = n_a * (n_a - 1) // 2 if n_b is None else n_a * n_b
        cells = pairs * n_win * n_win
        lines.append(f"\n{shape}: {pairs} pairs of videos, {cells:.3e} cells")
        for kind in ("plain", "static", "static+skip"):
            e = got[f"{shape}/{kind}"]
            al = e["align"]
            med = statistics.median(al["times"])
            lines.append(f"  {kind:12s} align   {ms(al['times'])}  {al['records']} records  {cells / med:.3e} cells/s = {cells / med / VALU_PAIRS_PER_S:.2f} of the VALU yardstick")
            if "parent" in e:
                pa = e["parent"]
                lines.append(f"  {kind:12s} parent  {ms(pa['times'])}  of which search {statistics.median(pa['search_times']) * 1e3:.3f} ms median; {pa['hits']} hits, "
                             f"hit buffer {'OVERFLOWED: no answer' if pa['overflow'] else 'held them'}")
                if not pa["overflow"]:
                    same = pa["digest"] == al["digest"] and pa["records"] == al["records"]
                    ok &= same
                    lines.append(f"  {kind:12s} records of both legs {'equal' if same else 'DIFFER'}; parent / align, medians = {statistics.median(pa['times']) / med:.2f}x")
        p, s = got[f"{shape}/plain"]["align"]["times"], got[f"{shape}/static"]["align"]["times"]
        spread = max(max(p) - min(p), max(s) - min(s))
        diff = abs(statistics.median(s) - statistics.median(p))
        held = diff <= spread
        ok &= held
        lines.append(f"  claim (align on the static corpus takes what it takes on the plain one, within the spread of the 12 calls): medians differ by {diff * 1e3:.3f} ms, "
                     f"spread (max - min, the wider of the two) {spread * 1e3:.3f} ms: {'HOLDS' if held else 'MISSED'}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
