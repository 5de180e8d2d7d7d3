#!/usr/bin/env python3
"""What aligning retimed windows at every rate in ONE call costs: vdf_align_windows_rates* of this build beside the routes to the
same records that the parent commit has, on the same arrays.

    python tools/bench_align_rates.py --parent-lib tools/_libvdf_parent.so [--out profiles/align_rates.txt]

Input (the shape of DESIGN.md 4.22's measurement): 1000 videos x 49 windows per side and per rate (random hashes), rates 1/1, 6/5, 5/4, 3/2 and 2/1;
every tenth video of B is a copy of the same video of A at one of the rates, from A's window 7 (100 planted pairs, 20 per rate); tolerance 0.35,
min_run 2.
Legs:
  one_pass  (a) align_rates(seed=True, native=True, one_pass=True): one seed call for all rates, then one list call per rate that has candidates, each
            with its own upload of A's block and of B.  On the library built from the PARENT commit (--parent-lib; without it this build's library
            stands in and is labelled so): the leg uses only entry points the parent has.
  one_call  (b) align_rates(seed=True, one_call=True) of this build: ONE vdf_align_windows_rates call, A and B uploaded once.
  device    (c) vdf_align_windows_rates_device with seed = 1 alone, on device-resident arrays.
  sequence  (d) the parent's resident sequence for the same records: one vdf_align_seed_pairs_rates_device, the triples split by rate on the host,
            one vdf_align_windows_retimed_pairs_device per rate.  On the parent's library.
  all       (e) the seed = 0 all-triples call of this build: 5 x 10^6 triples, the same cells as ...
  five      ... five vdf_align_windows_retimed_device calls, one per rate.  On the parent's library.
Gates: median (b) <= median (a); median (c) <= median (d); median (e) <= the slowest of the parent's own timed runs of its five calls (inside its
run-to-run spread, or below it); and the records of all legs equal.  The tool writes its report either way and fails if a gate does.  Every leg runs
in a fresh child process under its own time limit, one warm-up and 12 timed calls, host clock around calls that wait for their own work; medians
with (min ... max)."""
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
TOLERANCE, MIN_RUN = 0.35, 2
REPEATS = 12
LEGS = ("one_pass", "one_call", "device", "sequence", "all", "five")
PARENT_LEGS = ("one_pass", "sequence", "five")
CHILD_LIMIT_S = 420


def library():
    """({rate: words of A}, words of B) [videos, windows, 16] u64: random; video 10 k of B holds windows 0, den, ... of video 10 k of A at rate
    RATES[k % 5], from A's window 7"""
    rng = np.random.default_rng([5, 23])

    def words():
        w = rng.integers(0, 2**64, size=(N_VIDEOS, N_WIN, 16), dtype=np.uint64)
        w[:, :, 15] &= np.uint64((1 << 40) - 1)
        return w

    wa, wb = {rate: words() for rate in RATES}, words()
    for v in range(0, N_VIDEOS, 10):
        num, den = rate = RATES[(v // 10) % len(RATES)]
        m = 0
        while 7 + num * m < N_WIN and den * m < N_WIN:  # B window den m = A window 7 + num m
            wb[v, den * m] = wa[rate][v, 7 + num * m]
            m += 1
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
        assert all(n.startswith("vdf_align_windows_rates") for n in missing), missing
        for n in missing:
            del _capi.SIGNATURES[n]
    import vid_dup_finder_lib_amd as vdf

    eng = vdf.Engine(0)
    tol_int = vdf.engine.tolerance_int(TOLERANCE)
    wa, wb = library()
    # every leg's records as [rate index, a, b, first_a, first_b, n_windows, dist_sum], in (rate, a, b) order
    if args.leg in ("one_pass", "one_call"):
        mk = lambda words, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10) for w in ws] for i, ws in enumerate(words)]
        va, vb = {rate: mk(wa[rate], "a") for rate in RATES}, mk(wb, "b")
        kw = dict(one_pass=True, native=True) if args.leg == "one_pass" else dict(one_call=True)
        run = lambda: [[i, r.a, r.b, r.first_frame_a, r.first_frame_b, r.n_windows, round(r.mean_distance * r.n_windows)]
                       for i, (rate, rs) in enumerate(vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, engine=eng, seed=True, **kw).items()) for r in rs]
    else:
        dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x).view(t).copy()).cuda()
        first = np.arange(N_VIDEOS + 1, dtype=np.uint32) * N_WIN
        block = N_VIDEOS * N_WIN
        d_a = dev(np.concatenate([wa[rate].reshape(-1, 16) for rate in RATES]), np.int64)
        d_b, d_fa, d_fb = dev(wb, np.int64), dev(np.tile(first, len(RATES)), np.int32), dev(first, np.int32)
        rate_first = np.arange(len(RATES) + 1, dtype=np.int64) * block
        torch.cuda.synchronize()
        sides = (d_a.data_ptr(), d_fa.data_ptr(), N_VIDEOS, d_b.data_ptr(), d_fb.data_ptr(), N_VIDEOS)
        of_rate = lambda r, rec: [[r, int(x["a"]), int(x["b"]), int(x["first_a"]), int(x["first_b"]), int(x["n_windows"]), int(x["dist_sum"])] for x in rec]
        a_of = lambda r: d_a.data_ptr() + r * block * 128   # block r of A: 128 bytes per window

        def rates_call(seed):
            rec, n = eng.align_windows_rates_device(*sides, RATES, tol_int=tol_int, min_run=MIN_RUN, a_rate_first=rate_first, seed=seed, capacity=1 << 12)
            assert n == len(rec)
            return [[int(x[k]) for k in ("rate", "a", "b", "first_a", "first_b", "n_windows", "dist_sum")] for x in rec]

        def sequence():
            t, n = eng.align_seed_pairs_rates_device(*sides, RATES, tol_int=tol_int, min_run=MIN_RUN, a_rate_first=rate_first, capacity=1 << 16)
            assert n == len(t)
            out = []
            for r, rate in enumerate(RATES):
                pairs = np.zeros(int(np.count_nonzero(t["rate"] == r)), vdf.VIDEO_PAIR_DTYPE)
                pairs["a"], pairs["b"] = t["a"][t["rate"] == r], t["b"][t["rate"] == r]
                if not len(pairs):
                    continue
                rec, n = eng.align_windows_retimed_pairs_device(a_of(r), d_fa.data_ptr(), N_VIDEOS, pairs, d_b.data_ptr(), d_fb.data_ptr(), N_VIDEOS, rate,
                                                                tol_int=tol_int, min_run=MIN_RUN, capacity=1 << 12)
                assert n == len(rec)
                out += of_rate(r, rec)
            return out

        def five():
            out = []
            for r, rate in enumerate(RATES):
                rec, n = eng.align_windows_retimed_device(a_of(r), d_fa.data_ptr(), N_VIDEOS, d_b.data_ptr(), d_fb.data_ptr(), N_VIDEOS, rate, tol_int=tol_int,
                                                          min_run=MIN_RUN, capacity=1 << 12)
                assert n == len(rec)
                out += of_rate(r, rec)
            return out

        run = {"device": lambda: rates_call(True), "all": lambda: rates_call(False), "sequence": sequence, "five": five}[args.leg]
    res = {"times": timed(run), "records": run()}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_rates.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="one_call", choices=LEGS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    res = {leg: run_child(parent if leg in PARENT_LEGS else args.lib, leg) for leg in LEGS}
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"
    same = all(res[leg]["records"] == res[LEGS[0]]["records"] for leg in LEGS)
    med = {leg: statistics.median(res[leg]["times"]) for leg in LEGS}
    gates = {"(b) <= (a)": med["one_call"] <= med["one_pass"], "(c) <= (d)": med["device"] <= med["sequence"],
             "(e) one call <= the slowest run of the five calls": med["all"] <= max(res["five"]["times"])}
    passed = same and all(gates.values())
    per_rate = [sum(1 for r in res[LEGS[0]]["records"] if r[0] == i) for i in range(len(RATES))]
    lines = [f"tools/bench_align_rates.py: {N_VIDEOS} videos x {N_WIN} windows per side and rate, rates {', '.join(f'{n}/{d}' for n, d in RATES)}, 100 planted pairs, "
             f"tolerance {TOLERANCE}, min_run {MIN_RUN}",
             f"one warm-up and {REPEATS} timed calls per leg, fresh process per leg; legs (a), (d) and the five calls of (e) on {whose}",
             "(a) / (b): host clock around the whole Python route from VideoHash lists to the dict; the others: around the C-ABI calls on resident arrays",
             "",
             f"records per rate: {per_rate}; the records of the six legs are {'equal' if same else 'DIFFERENT'}",
             f"  {'leg':64s} {'min ms':>9s} {'median':>9s} {'max':>9s}"]
    label = {"one_pass": "(a) align_rates(seed, one_pass): seed call + a list call per rate", "one_call": "(b) align_rates(seed, one_call): one call",
             "device": "(c) vdf_align_windows_rates_device, seed = 1", "sequence": "(d) seed_pairs_rates_device + split + 5 retimed_pairs_device",
             "all": "(e) vdf_align_windows_rates_device, seed = 0: 5 x 10^6 triples", "five": "    five vdf_align_windows_retimed_device calls"}
    for leg in LEGS:
        ts = res[leg]["times"]
        lines.append(f"  {label[leg]:64s} {min(ts) * 1e3:9.2f} {statistics.median(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
    lines.append(f"  (b) / (a) = {med['one_call'] / med['one_pass']:.3f}      (c) / (d) = {med['device'] / med['sequence']:.3f}      "
                 f"(e) / five = {med['all'] / med['five']:.3f}")
    for name, ok in gates.items():
        lines.append(f"  gate {name}: {'holds' if ok else 'FAILS'}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if passed else 1


if __name__ == "__main__":
    sys.exit(main())
