#!/usr/bin/env python3
"""What reporting EVERY stretch of a retimed pair costs: vdf_align_windows_rates_stretches_device of this build beside the parent
commit's vdf_align_windows_rates_device, on the same resident arrays.

    python tools/bench_align_rates_stretches.py --parent-lib tools/_libvdf_parent.so [--out profiles/align_rates_stretches.txt]

Input (the shape of DESIGN.md 4.23's measurement): 1000 videos x 49 windows per side and per rate (random hashes), rates 1/1, 6/5, 5/4, 3/2 and 2/1;
every tenth video of B is a copy of the same video of A at one of the rates, from A's window 7 (100 planted pairs, 20 per rate); tolerance 0.35,
min_run 2; guard 2.  The CUT library: the same, but every copy leaves out max(1, 4 // num) sub-sampled windows of A in its middle (at 6/5 a video of 49
windows has seven cells on a line: a longer cut would leave no second stretch) - two stretches per planted pair.
Legs, all with seed = 1 on device-resident arrays:
  parent    (a) vdf_align_windows_rates_device on the library built from the PARENT commit (--parent-lib; without it this build's library stands in
            and is labelled so).
  one       (b) the new device call with max_stretches = 1.
  four      (c) the new device call with max_stretches = 4 on the plain library: no planted pair has a second stretch, so round 1 walks the 100 triples
            of round 0's records, finds nothing, and no further round runs.
  cut       (d) the new device call with max_stretches = 4 on the CUT library, with the number of rounds read from the ranks.
Gates: median (b) and median (c) are not above the slowest of (a)'s own timed runs; the records of (a), (b) and (c) are equal (rank 0 added); the
records of (d) equal vdf_align_windows_rates_stretches_host's on the candidate triples and hold two stretches for every planted pair.  (d) has no time
gate.  The tool writes its report either way and fails if a gate does.  Every leg runs in a fresh child process under its own time limit, one
warm-up and 12 timed calls, host clock around calls that wait for their own work; medians with (min ... max).
Not measured here: other shapes, the host-array C form, kernel-only times."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VIDEOS, N_WIN = 1000, 49
RATES = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
TOLERANCE, MIN_RUN, GUARD = 0.35, 2, 2
REPEATS = 12
LEGS = ("parent", "one", "four", "cut")
CHILD_LIMIT_S = 300


def library(cut):
    """({rate: words of A}, words of B) [videos, windows, 16] u64: random; video 10 k of B holds windows 0, den, ... of video 10 k of A at rate
    RATES[k % 5], from A's window 7; cut: the second half of the copy comes from max(1, 4 // num) sub-sampled windows further on in A"""
    rng = np.random.default_rng([5, 24])

    def words():
        w = rng.integers(0, 2**64, size=(N_VIDEOS, N_WIN, 16), dtype=np.uint64)
        w[:, :, 15] &= np.uint64((1 << 40) - 1)
        return w

    wa, wb = {rate: words() for rate in RATES}, words()
    for v in range(0, N_VIDEOS, 10):
        num, den = rate = RATES[(v // 10) % len(RATES)]
        cells = 0
        while 7 + num * cells < N_WIN and den * cells < N_WIN:
            cells += 1
        gap = max(1, 4 // num) if cut else 0  # sub-sampled windows of A left out in the middle of the copy
        half = (cells - gap) // 2 if cut else cells
        for m in range(cells - gap):  # B window den m = A window 7 + num (m, or m + gap behind the cut)
            wb[v, den * m] = wa[rate][v, 7 + num * (m if m < half else m + gap)]
    return wa, wb


def timed(run):
    out = []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        run()
        if r:
            out.append(time.perf_counter() - t0)
    return out


def child(args):
    sys.path.insert(0, ROOT)
    import torch  # before any libvdf_hip.so is mapped: one HIP runtime per process (_capi.load)

    from vid_dup_finder_lib_amd import _capi

    if os.path.abspath(args.lib) != os.path.abspath(_capi.LIB_PATH):  # the parent's library: everything it exports is bound, the rest must be this feature's
        import ctypes

        _capi.LIB_PATH = os.path.abspath(args.lib)
        probe = ctypes.CDLL(_capi.LIB_PATH)
        missing = [n for n in _capi.SIGNATURES if not hasattr(probe, n)]
        assert all(n.startswith("vdf_align_windows_rates_stretches") for n in missing), missing
        for n in missing:
            del _capi.SIGNATURES[n]
    import vid_dup_finder_lib_amd as vdf

    eng = vdf.Engine(0)
    tol_int = vdf.engine.tolerance_int(TOLERANCE)
    wa, wb = library(args.leg == "cut")
    dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x).view(t).copy()).cuda()
    first = np.arange(N_VIDEOS + 1, dtype=np.uint32) * N_WIN
    a_words = np.concatenate([wa[rate].reshape(-1, 16) for rate in RATES])
    d_a, d_b = dev(a_words, np.int64), dev(wb, np.int64)
    d_fa, d_fb = dev(np.tile(first, len(RATES)), np.int32), dev(first, np.int32)
    rate_first = np.arange(len(RATES) + 1, dtype=np.int64) * (N_VIDEOS * N_WIN)
    torch.cuda.synchronize()
    sides = (d_a.data_ptr(), d_fa.data_ptr(), N_VIDEOS, d_b.data_ptr(), d_fb.data_ptr(), N_VIDEOS)
    fields = ("rate", "a", "b", "first_a", "first_b", "n_windows", "dist_sum", "n_frames_b")
    host = None
    if args.leg == "parent":
        def run():
            rec, n = eng.align_windows_rates_device(*sides, RATES, tol_int=tol_int, min_run=MIN_RUN, a_rate_first=rate_first, seed=True, capacity=1 << 12)
            assert n == len(rec)
            return [[int(x[k]) for k in fields] + [0] for x in rec]
    else:
        most = 1 if args.leg == "one" else 4

        def run():
            rec, n = eng.align_windows_rates_stretches_device(*sides, RATES, tol_int=tol_int, min_run=MIN_RUN, max_stretches=most, guard=GUARD,
                                                              a_rate_first=rate_first, seed=True, capacity=1 << 12)
            assert n == len(rec)
            return [[int(x[k]) for k in fields + ("rank",)] for x in rec]
        if args.leg == "cut":  # the plain C++ definition on the candidate triples (the whole library is hours of CPU time)
            t, n = eng.align_seed_pairs_rates_device(*sides, RATES, tol_int=tol_int, min_run=MIN_RUN, a_rate_first=rate_first, capacity=1 << 16)
            assert n == len(t)
            rec, n = vdf.align_windows_rates_stretches_host(a_words, np.tile(first, (len(RATES), 1)), wb.reshape(-1, 16), first, RATES, tol_int=tol_int, min_run=MIN_RUN,
                                                            max_stretches=most, guard=GUARD, a_rate_first=rate_first, triples=t, capacity=1 << 12)
            assert n == len(rec)
            host = [[int(x[k]) for k in fields + ("rank",)] for x in rec]
    res = {"times": timed(run), "records": run(), "host": host}
    eng.close()
    print("RESULT " + json.dumps(res))


def run_child(lib, leg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--leg", leg], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:  # a leg that failed ends the run: nothing more is started on the GPU
        raise SystemExit(f"child {leg} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    print(f"[{leg}: done]", file=sys.stderr, flush=True)
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_rates_stretches.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="four", choices=LEGS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    res = {leg: run_child(parent if leg == "parent" else args.lib, leg) for leg in LEGS}
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"
    same = res["one"]["records"] == res["parent"]["records"] and res["four"]["records"] == res["parent"]["records"]
    cut = res["cut"]["records"]
    per_triple = {}
    for r in cut:
        per_triple.setdefault(tuple(r[:3]), []).append(r[8])
    planted = [((v // 10) % len(RATES), v, v) for v in range(0, N_VIDEOS, 10)]
    cut_ok = cut == res["cut"]["host"] and all(per_triple.get(t, [])[:2] == [0, 1] for t in planted)
    rounds = 1 + max(r[8] for r in cut) + (1 if max(len(v) for v in per_triple.values()) < 4 else 0)   # the round that found nothing included
    med = {leg: statistics.median(res[leg]["times"]) for leg in LEGS}
    slowest = max(res["parent"]["times"])
    gates = {"(b) <= the slowest run of (a)": med["one"] <= slowest, "(c) <= the slowest run of (a)": med["four"] <= slowest}
    passed = same and cut_ok and all(gates.values())
    lines = [f"tools/bench_align_rates_stretches.py: {N_VIDEOS} videos x {N_WIN} windows per side and rate, rates {', '.join(f'{n}/{d}' for n, d in RATES)}, 100 planted "
             f"pairs, tolerance {TOLERANCE}, min_run {MIN_RUN}, guard {GUARD}; seed = 1, device-resident arrays",
             f"one warm-up and {REPEATS} timed calls per leg, fresh process per leg, host clock around the C-ABI call; leg (a) on {whose}",
             "",
             f"records of (a), (b), (c): {len(res['parent']['records'])}, {'equal' if same else 'DIFFERENT'} (rank 0 added to (a)'s)",
             f"records of (d): {len(cut)} in {len(per_triple)} triples, {rounds} rounds; {'equal to' if cut == res['cut']['host'] else 'DIFFERENT from'} "
             f"vdf_align_windows_rates_stretches_host's on the candidate triples; every planted pair has ranks 0 and 1: {all(per_triple.get(t, [])[:2] == [0, 1] for t in planted)}",
             f"  {'leg':78s} {'min ms':>9s} {'median':>9s} {'max':>9s}"]
    label = {"parent": "(a) vdf_align_windows_rates_device, seed = 1", "one": "(b) vdf_align_windows_rates_stretches_device, max_stretches = 1",
             "four": "(c) vdf_align_windows_rates_stretches_device, max_stretches = 4, no second stretch", "cut": "(d) the same on the cut library: two stretches per planted pair"}
    for leg in LEGS:
        ts = res[leg]["times"]
        lines.append(f"  {label[leg]:78s} {min(ts) * 1e3:9.2f} {statistics.median(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
    lines.append(f"  (b) / (a) = {med['one'] / med['parent']:.3f}      (c) / (a) = {med['four'] / med['parent']:.3f}      (d) / (a) = {med['cut'] / med['parent']:.3f}")
    for name, ok in gates.items():
        lines.append(f"  gate {name}: {'holds' if ok else 'FAILS'}")
    lines.append("not measured: other shapes, the host-array C form, kernel-only times")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if passed else 1


if __name__ == "__main__":
    sys.exit(main())
