#!/usr/bin/env python3
"""What aligning retimed windows in ONE call costs: api.align_retimed(native=True) of this build beside the composition it replaces,
the C-ABI call alone and its floor, on the same arrays.

    python tools/bench_align_retimed.py --parent-lib tools/_libvdf_parent.so [--out profiles/align_retimed_native.txt]

Input: 1000 videos x 49 retimed windows against 1000 videos x 49 plain windows (random hashes), every tenth video of B a copy of the same video of
A at the rate from A's frame 7 (100 planted pairs); rates 6/5 and 2/1; tolerance 0.35, min_run 2; unseeded and seed=True.
Legs:
  composition  (a) api.align_retimed(native=False) - `num` sliced CSRs, uploads and align calls, merged on the host - on the library built from the
               PARENT commit (--parent-lib; without it this build's library stands in and is labelled so).  The Python of the composition is the
               parent's, unchanged; the six entry points the parent's library does not export are left unbound for this leg.
  native       (b) api.align_retimed(native=True) of this build: one CSR, one vdf_align_windows_retimed[_pairs] call.  Records must equal (a)'s.
  device       (c) vdf_align_windows_retimed_device alone, on device-resident arrays (seeded: the _pairs_device form on the candidate list, which is
               made once, outside the timing).  Records must equal (a)'s.
  plain        (d) ONE vdf_align_windows_device call of A against every den-th window of B, resident: the same number of cells on diagonals
               instead of `num` phases - other records, the floor (seeded: vdf_align_windows_pairs_device on the same list).
Gate: the tool fails only if (b)'s median is above (a)'s - one call is not slower than `num` calls on equal cells - or if records differ.
(b) / (a) and (c) / (d) are reported.  Every leg runs in a fresh child process under its own time limit, one warm-up and 12 timed calls per
measurement, host clock around calls that wait for their own work; medians."""
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
RATES = [(6, 5), (2, 1)]
TOLERANCE, MIN_RUN = 0.35, 2
REPEATS = 12
LEGS = ("composition", "native", "device", "plain")
CHILD_LIMIT_S = 420


def library(rate):
    """(words of A, words of B) [videos, windows, 16] u64: random, every tenth video of B a copy of A's at the rate from A's frame 7"""
    num, den = rate
    rng = np.random.default_rng([5, num, den])

    def words():
        w = rng.integers(0, 2**64, size=(N_VIDEOS, N_WIN, 16), dtype=np.uint64)
        w[:, :, 15] &= np.uint64((1 << 40) - 1)
        return w

    wa, wb = words(), words()
    for v in range(0, N_VIDEOS, 10):
        m = 0
        while 7 + num * m < N_WIN and den * m < N_WIN:  # B window den m = A window 7 + num m
            wb[v, den * m] = wa[v, 7 + num * m]
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
        assert all(n.startswith("vdf_align_windows_retimed") for n in missing), missing
        for n in missing:
            del _capi.SIGNATURES[n]
    import vid_dup_finder_lib_amd as vdf

    eng = vdf.Engine(0)
    tol_int = vdf.engine.tolerance_int(TOLERANCE)
    res = {}
    for rate in RATES:
        num, den = rate
        wa, wb = library(rate)
        mk = lambda words, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10) for w in ws] for i, ws in enumerate(words)]
        va, vb = mk(wa, "a"), mk(wb, "b")
        first = np.arange(N_VIDEOS + 1, dtype=np.uint32) * N_WIN
        sub_b = np.ascontiguousarray(wb[:, 0::den])
        first_sub = np.arange(N_VIDEOS + 1, dtype=np.uint32) * sub_b.shape[1]
        dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x).view(t).copy()).cuda()
        d_a, d_b, d_sub = dev(wa, np.int64), dev(wb, np.int64), dev(sub_b, np.int64)
        d_first, d_first_sub = dev(first, np.int32), dev(first_sub, np.int32)
        torch.cuda.synchronize()
        for seed in (False, True):
            key = f"{num}_{den}/{'seeded' if seed else 'all pairs'}"
            cand = None
            if seed and args.leg in ("device", "plain"):  # the candidate list of native=True, seed=True: made once, outside the timing
                pairs = set()
                for p in range(num):
                    pairs.update(vdf.candidate_pairs([ws[p::num] for ws in va], [ws[0::den] for ws in vb], TOLERANCE, min_run=MIN_RUN, engine=eng))
                cand = vdf.engine.video_pairs(np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2))
            as_records = lambda rs: [[r.a, r.b, r.first_frame_a, r.first_frame_b, r.n_windows, round(r.mean_distance * r.n_windows)] for r in rs]
            if args.leg == "composition":
                run = lambda: as_records(vdf.align_retimed(va, vb, rate, TOLERANCE, min_run=MIN_RUN, engine=eng, seed=seed))
            elif args.leg == "native":
                run = lambda: as_records(vdf.align_retimed(va, vb, rate, TOLERANCE, min_run=MIN_RUN, engine=eng, seed=seed, native=True))
            elif args.leg == "device":
                def run():
                    kw = dict(tol_int=tol_int, min_run=MIN_RUN, capacity=1 << 16)
                    if cand is not None:
                        rec, n = eng.align_windows_retimed_pairs_device(d_a.data_ptr(), d_first.data_ptr(), N_VIDEOS, cand, d_b.data_ptr(), d_first.data_ptr(),
                                                                        N_VIDEOS, rate, **kw)
                    else:
                        rec, n = eng.align_windows_retimed_device(d_a.data_ptr(), d_first.data_ptr(), N_VIDEOS, d_b.data_ptr(), d_first.data_ptr(), N_VIDEOS, rate, **kw)
                    assert n == len(rec)
                    return [[int(r[k]) for k in ("a", "b", "first_a", "first_b", "n_windows", "dist_sum")] for r in rec]
            else:
                def run():
                    kw = dict(d_b_hashes=d_sub.data_ptr(), d_b_first=d_first_sub.data_ptr(), n_b=N_VIDEOS, tol_int=tol_int, min_run=MIN_RUN, capacity=1 << 16)
                    if cand is not None:
                        rec, n = eng.align_windows_pairs_device(d_a.data_ptr(), d_first.data_ptr(), N_VIDEOS, cand, **kw)
                    else:
                        rec, n = eng.align_windows_device(d_a.data_ptr(), d_first.data_ptr(), N_VIDEOS, **kw)
                    assert n == len(rec)
                    return None  # other records: diagonals of the whole matrix, not phases
            records = run()
            res[key] = {"times": timed(run), "records": records, "listed": None if cand is None else int(len(cand))}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_retimed_native.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="native", choices=LEGS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    res = {leg: run_child(parent if leg == "composition" else args.lib, leg) for leg in LEGS}
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"
    lines = [f"tools/bench_align_retimed.py: {N_VIDEOS} videos x {N_WIN} retimed windows against {N_VIDEOS} x {N_WIN} plain windows, 100 planted pairs, tolerance {TOLERANCE}, "
             f"min_run {MIN_RUN}",
             f"one warm-up and {REPEATS} timed calls per measurement, fresh process per leg; composition on {whose}",
             "composition / native: host clock around the whole Python call (CSR, C ABI calls, record mapping); device / plain: around the C-ABI call on resident arrays",
             "gate: median of native <= median of composition, records equal"]
    ok = True
    for key in res["native"]:
        med = {leg: statistics.median(res[leg][key]["times"]) for leg in LEGS}
        same = res["native"][key]["records"] == res["composition"][key]["records"] == res["device"][key]["records"]
        passed = same and med["native"] <= med["composition"]
        ok &= passed
        listed = res["device"][key]["listed"]
        lines.append(f"\nrate {key}: {len(res['native'][key]['records'])} records" + (f", {listed} candidate pairs" if listed is not None else "")
                     + f"; records of composition, native and device {'equal' if same else 'DIFFER'}")
        lines.append(f"  {'leg':12s} {'min ms':>9s} {'median':>9s} {'max':>9s}")
        for leg in LEGS:
            ts = res[leg][key]["times"]
            lines.append(f"  {leg:12s} {min(ts) * 1e3:9.2f} {statistics.median(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
        lines.append(f"  (b) / (a) native / composition = {med['native'] / med['composition']:.3f}      (c) / (d) device / plain = {med['device'] / med['plain']:.3f}"
                     f"      gate: {'passed' if passed else 'FAILED'}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
