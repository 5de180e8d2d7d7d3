#!/usr/bin/env python3
"""What seeding the retimed alignment at every rate in ONE call costs: api.candidate_pairs_rates of this build beside the route
align_rates(seed=True, native=True) takes to the same candidates today, the C-ABI call alone and its floor, on the same arrays.

    python tools/bench_align_seed_rates.py --parent-lib tools/_libvdf_parent.so [--out profiles/align_seed_rates.txt]

Input (the profile shape of DESIGN.md 4.17): 1000 videos x 49 windows per side and per rate (random hashes), rates 1/1, 6/5, 5/4, 3/2 and 2/1; every tenth
video of B is a copy of the same video of A at one of the rates, from A's frame 7 (100 planted pairs, 20 per rate); tolerance 0.35, min_run 2.
Legs:
  today   (a) the candidates as align_rates(seed=True, native=True) gets them today: per rate the CSR of both sides, `num` sub-sampled copies of A and
          one of B cut out with numpy, `num` vdf_align_seed_pairs calls on uploaded copies, the union on the host - 17 seed calls.  On the library built
          from the PARENT commit (--parent-lib; without it this build's library stands in and is labelled so): the leg uses only entry points the
          parent has.  The same process also times the parent's align_rates(seed=True, native=True) end to end.
  rates   (b) api.candidate_pairs_rates of this build: the CSR of B once and of each rate's A once, ONE vdf_align_seed_pairs_rates call.  The same
          process also times align_rates(seed=True, native=True, one_pass=True) end to end.
  device  (c) vdf_align_seed_pairs_rates_device alone, on device-resident arrays.
  floor   (d) the 17 vdf_align_seed_pairs_device calls on pre-sub-sampled resident arrays: the same cells without any host work.
Gate: the tool fails only if (b)'s median is above (a)'s - the two walk the same cells, and (b) drops 16 launches' worth of fixed cost and all the
sub-sampling - or if the candidate lists (or the end-to-end dicts) differ.  (c) / (d) and the end-to-end ratio are reported.  Every leg runs in a
fresh child process under its own time limit, one warm-up and 12 timed calls per measurement, host clock around calls that wait for their own work;
medians."""
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
LEGS = ("today", "rates", "device", "floor")
CHILD_LIMIT_S = 420


def library():
    """({rate: words of A}, words of B) [videos, windows, 16] u64: random; video 10 k of B holds windows 0, den, ... of video 10 k of A at rate
    RATES[k % 5], from A's window 7"""
    rng = np.random.default_rng([5, 22])

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


def candidates_today(vdf, va, vb, eng, tol_int):
    """what api._align_retimed_native(seed=True) does per block before its align call, rate by rate (one block: 1000 x 1000 pairs)"""
    from vid_dup_finder_lib_amd import api

    out = {}
    for rate in RATES:
        num, den = rate
        wa, fa, ka, _ = api._align_csr(va[rate], None)
        wb, fb, kb, _ = api._align_csr(vb, None)

        def sub(side, p, step):
            words, first, skip = side
            counts = np.diff(first.astype(np.int64))
            video = np.repeat(np.arange(len(counts)), counts)
            keep = (np.arange(len(words)) - first[:-1].astype(np.int64)[video]) % step == p
            sub_first = np.zeros(len(first), np.uint32)
            sub_first[1:] = np.cumsum(np.bincount(video[keep], minlength=len(counts)))
            return words[keep], sub_first, None if skip is None else skip[keep]

        key = lambda p: (p["a"].astype(np.uint64) << np.uint64(32)) | p["b"].astype(np.uint64)
        B0 = sub((wb, fb, kb), 0, den)
        keys = np.unique(np.concatenate([key(api._seed_call(eng, sub((wa, fa, ka), p, num), B0, tol_int, MIN_RUN)) for p in range(num)]))
        out[f"{num}/{den}"] = [[int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF))] for k in keys]
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
        assert all(n.startswith("vdf_align_seed_pairs_rates") for n in missing), missing
        for n in missing:
            del _capi.SIGNATURES[n]
    import vid_dup_finder_lib_amd as vdf

    eng = vdf.Engine(0)
    tol_int = vdf.engine.tolerance_int(TOLERANCE)
    wa, wb = library()
    name = lambda rate: f"{rate[0]}/{rate[1]}"
    as_records = lambda d: {name(rate): [[r.a, r.b, r.first_frame_a, r.first_frame_b, r.n_windows, round(r.mean_distance * r.n_windows)] for r in rs]
                            for rate, rs in d.items()}
    res = {}
    if args.leg in ("today", "rates"):
        mk = lambda words, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10) for w in ws] for i, ws in enumerate(words)]
        va, vb = {rate: mk(wa[rate], "a") for rate in RATES}, mk(wb, "b")
        if args.leg == "today":
            cand = lambda: candidates_today(vdf, va, vb, eng, tol_int)
            e2e = lambda: as_records(vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, engine=eng, native=True, seed=True))
        else:
            cand = lambda: {name(rate): [list(p) for p in ps] for rate, ps in vdf.candidate_pairs_rates(va, vb, TOLERANCE, MIN_RUN, engine=eng).items()}
            e2e = lambda: as_records(vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, engine=eng, native=True, seed=True, one_pass=True))
        res["candidates"] = {"times": timed(cand), "lists": cand()}
        res["end to end"] = {"times": timed(e2e), "lists": e2e()}
    else:
        dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x).view(t).copy()).cuda()
        first = np.arange(N_VIDEOS + 1, dtype=np.uint32) * N_WIN
        if args.leg == "device":
            d_a = dev(np.concatenate([wa[rate].reshape(-1, 16) for rate in RATES]), np.int64)
            d_b, d_fa, d_fb = dev(wb, np.int64), dev(np.tile(first, len(RATES)), np.int32), dev(first, np.int32)
            rate_first = np.arange(len(RATES) + 1, dtype=np.int64) * (N_VIDEOS * N_WIN)
            torch.cuda.synchronize()

            def cand():
                t, n = eng.align_seed_pairs_rates_device(d_a.data_ptr(), d_fa.data_ptr(), N_VIDEOS, d_b.data_ptr(), d_fb.data_ptr(), N_VIDEOS, RATES, tol_int=tol_int,
                                                         min_run=MIN_RUN, a_rate_first=rate_first, capacity=1 << 16)
                assert n == len(t)
                return {name(rate): [[int(x["a"]), int(x["b"])] for x in t[t["rate"] == r]] for r, rate in enumerate(RATES)}
        else:
            subs = []
            for num, den in RATES:
                sb = np.ascontiguousarray(wb[:, 0::den])
                d_sb, d_fsb = dev(sb, np.int64), dev(np.arange(N_VIDEOS + 1, dtype=np.uint32) * sb.shape[1], np.int32)
                for p in range(num):
                    sa = np.ascontiguousarray(wa[(num, den)][:, p::num])
                    subs.append((name((num, den)), dev(sa, np.int64), dev(np.arange(N_VIDEOS + 1, dtype=np.uint32) * sa.shape[1], np.int32), d_sb, d_fsb))
            assert len(subs) == sum(r[0] for r in RATES) == 17
            torch.cuda.synchronize()

            def cand():
                out = {name(rate): set() for rate in RATES}
                for key, sa, fsa, sb, fsb in subs:
                    p, n = eng.align_seed_pairs_device(sa.data_ptr(), fsa.data_ptr(), N_VIDEOS, d_b_hashes=sb.data_ptr(), d_b_first=fsb.data_ptr(), n_b=N_VIDEOS,
                                                       tol_int=tol_int, min_run=MIN_RUN, capacity=1 << 16)
                    assert n == len(p)
                    out[key].update((int(x["a"]), int(x["b"])) for x in p)
                return {k: [list(ab) for ab in sorted(v)] for k, v in out.items()}
        res["candidates"] = {"times": timed(cand), "lists": cand()}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_seed_rates.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vid_dup_finder_lib_amd", "libvdf_hip.so"))
    ap.add_argument("--leg", default="rates", choices=LEGS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else args.lib
    res = {leg: run_child(parent if leg == "today" else args.lib, leg) for leg in LEGS}
    whose = "the PARENT commit's library" if args.parent_lib else "THIS build's library (no --parent-lib: not the parent commit)"
    lists = [res[leg]["candidates"]["lists"] for leg in LEGS]
    same = all(x == lists[0] for x in lists)
    same_e2e = res["today"]["end to end"]["lists"] == res["rates"]["end to end"]["lists"]
    med = {leg: statistics.median(res[leg]["candidates"]["times"]) for leg in LEGS}
    med_e2e = {leg: statistics.median(res[leg]["end to end"]["times"]) for leg in ("today", "rates")}
    passed = same and same_e2e and med["rates"] <= med["today"]
    lines = [f"tools/bench_align_seed_rates.py: {N_VIDEOS} videos x {N_WIN} windows per side and rate, rates {', '.join(f'{n}/{d}' for n, d in RATES)}, 100 planted pairs, "
             f"tolerance {TOLERANCE}, min_run {MIN_RUN}",
             f"one warm-up and {REPEATS} timed calls per measurement, fresh process per leg; leg (a) on {whose}",
             "(a) / (b): host clock around the whole Python route from VideoHash lists to the candidate lists; (c) / (d): around the C-ABI calls on resident arrays",
             "gate: median of (b) <= median of (a), candidate lists and end-to-end dicts equal",
             "",
             "candidates per rate: " + ", ".join(f"{k}: {len(v)}" for k, v in lists[0].items()) + f"; the lists of the four legs are {'equal' if same else 'DIFFERENT'}",
             f"  {'leg':44s} {'min ms':>9s} {'median':>9s} {'max':>9s}"]
    label = {"today": "(a) today: 17 seed calls, sub-sampled uploads", "rates": "(b) candidate_pairs_rates: one call", "device": "(c) vdf_align_seed_pairs_rates_device",
             "floor": "(d) 17 vdf_align_seed_pairs_device calls"}
    for leg in LEGS:
        ts = res[leg]["candidates"]["times"]
        lines.append(f"  {label[leg]:44s} {min(ts) * 1e3:9.2f} {statistics.median(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
    lines.append(f"  (b) / (a) = {med['rates'] / med['today']:.3f}      (c) / (d) = {med['device'] / med['floor']:.3f}      gate: {'passed' if passed else 'FAILED'}")
    lines.append("")
    lines.append(f"end to end, align_rates(seed=True, native=True): {sum(len(v) for v in res['rates']['end to end']['lists'].values())} records; the dicts are "
                 f"{'equal' if same_e2e else 'DIFFERENT'}")
    for leg, what in (("today", "one call per rate (parent)"), ("rates", "one_pass=True")):
        ts = res[leg]["end to end"]["times"]
        lines.append(f"  {what:44s} {min(ts) * 1e3:9.2f} {statistics.median(ts) * 1e3:9.2f} {max(ts) * 1e3:9.2f}")
    lines.append(f"  one_pass / today = {med_e2e['rates'] / med_e2e['today']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if passed else 1


if __name__ == "__main__":
    sys.exit(main())
