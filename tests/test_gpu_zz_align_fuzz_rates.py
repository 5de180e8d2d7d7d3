"""Randomised differential tests of the rate-list align kernels (csrc/align.hip: align_seed_rates_kernel<2, 14|22|26|32> with align_seed_count_kernel
and align_seed_variants_scatter_kernel on the identity slot table; align_bands_kernel<AlignTripleUnits, false|true>, align_reduce_rates_kernel,
align_scan_kernel, align_scatter_kernel<vdf_alignment_rate>, on the rounds of align_rates_stretch_plan.h) at the sizes where their structure is
exercised: the seeded problems of tests/ratefuzz.py through vdf_align_seed_pairs_rates*, vdf_align_windows_rates* and
vdf_align_windows_rates_stretches* - the _device form on torch device arrays of exactly the problem's size (skip pointers 0 where absent) and the
host-array form - against the plain C++ definitions the library ships as vdf_align_*_rates*_host, which tests/test_align_fuzz_rates_host.py pins to
the independent numpy twins on the same generator.  Records and `found` are compared for equality.

The profiles (ratefuzz's docstring has the details and the constant behind every size):
  bands      2 - 5 videos per side, 4 - 8 rates, window counts around the 64 and 128 edges of the SUB-matrix: three and more bands of kAlignBand = 64
             diagonals per phase, reloads and lane wraps inside a band, empty phases and videos, the four waves of a workgroup on units of
             different rates, phases and bands, masked rectangles across band boundaries;
  tiles      B of 1040 - 1480 windows: two tiles of kSeedTileRows = 512 gathered rows in the class of den 2, a single tile with padding-only waves
             in the class of den 4, videos across every tile edge; more than kSeedChunk = 256 seeds in the two slots of one class, chunk 0 across
             the slot boundary; a hit behind tile 0 and chunk 0;
  many_tiny  60 - 130 videos per side of 0 - 4 windows, 4 - 8 rates: tens of thousands of triples - several 256-item blocks of the reduction, the scan
             and the scatter, in round 0 and (dense content) in the later rounds - and a rate-slotted bitmap of thousands of words with n_a n_b no
             multiple of 32.

Per (profile, seed): align_seed_pairs_rates; align_windows_rates over every triple, with seed = 1, on the seed call's own output and on a drawn
sublist (triples of empty videos in it); align_windows_rates_stretches in the same four modes at the drawn max_stretches and guard.  Every call
again with a drawn capacity below `found` (0 among them): the same `found` and the prefix.  Relations between device results, which need no
reference and localise a failure: the rank-0 stretches are align_windows_rates' records; max_stretches = 1 is align_windows_rates' call; seed = 1
equals seed = 0; the list call on the whole seed output equals the all-triples call; a one-rate job on block r equals align_windows_retimed at
that rate, field mapped; the two slots of an un-reduced duplicate (3/2 and 6/4 on equal blocks) give the same records up to the rate index.

ONE Engine for the whole file with the profiles INTERLEAVED, on purpose: problems of very different sizes one after the other on one context are
also the test for bitmap words, scratch and band records left over from the call before.  A failure names profile, seed, entry point, form and
the first record that differs, and prints ratefuzz.describe(seed, profile): one failing seed is a complete report.

VDF_FUZZ_SEEDS=N widens the seed range for a soak run (default: 16 seeds per profile).  The file's name sorts it behind the other rate-list files,
for the reason test_gpu_zz_align_seed_rates.py gives."""
import os

import numpy as np
import pytest

import ratefuzz as rf

pytestmark = pytest.mark.gpu
_SOAK = int(os.environ.get("VDF_FUZZ_SEEDS", "0"))
SEEDS = max(16, _SOAK)
CAP = 1 << 21  # above every record count of these problems (135 000 triples x 8 ranks, of which tiny matrices leave a fraction)

_DEVICE_NAMES = {"a_hashes": ("d_a_hashes", np.int64), "a_first": ("d_a_first", np.int32), "a_skip": ("d_a_skip", np.uint8),
                 "b_hashes": ("d_b_hashes", np.int64), "b_first": ("d_b_first", np.int32), "b_skip": ("d_b_skip", np.uint8)}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


class Run:
    """one (profile, seed): the problem, its arrays on the device (uploaded once), the _host results and the device forms' tables (computed once)"""

    def __init__(self, eng, profile, seed):
        import vid_dup_finder_lib_amd as vdf

        self.eng, self.vdf, self.profile, self.seed = eng, vdf, profile, seed
        self.fp = rf.problem(seed, profile)
        self.caps = np.random.default_rng([rf.FUZZ, 1, seed])
        self.n_calls = 0
        self._dev, self._want, self.got = {}, {}, {}
        self.calls = {c.entry: c for c in rf.calls(self.fp)}

    def ptr(self, x, dtype) -> int:
        import torch

        if x is None:
            return 0
        if id(x) not in self._dev:
            assert len(x), "an empty array has no device address: the generator draws none"
            self._dev[id(x)] = (x, torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).cuda())
            torch.cuda.synchronize()
        return self._dev[id(x)][1].data_ptr()

    def device_kw(self, kw: dict) -> dict:
        out = {_DEVICE_NAMES[k][0] if k in _DEVICE_NAMES else k: self.ptr(v, _DEVICE_NAMES[k][1]) if k in _DEVICE_NAMES else v for k, v in kw.items()}
        out["n_a"] = kw["a_first"].shape[1] - 1
        out["n_b"] = len(kw["b_first"]) - 1
        return out

    def want(self, call):
        if call.entry not in self._want:
            self._want[call.entry] = rf.host_form(self.vdf, call, CAP)
            assert self._want[call.entry][1] <= CAP
        return self._want[call.entry]

    def fail(self, entry, form, text):
        pytest.fail(f"{self.profile} seed {self.seed}, {entry}, {form}: {text}\n{rf.describe(self.seed, self.profile)}", pytrace=False)

    def check(self, call) -> np.ndarray:
        """both forms of one call against its _host form, and again under a drawn capacity below `found`; -> the device form's table"""
        if call.entry in self.got:
            return self.got[call.entry]
        want, found = self.want(call)
        self.n_calls += 1
        cap = 0 if (self.seed + self.n_calls) % 4 == 0 or found == 0 else int(self.caps.integers(0, found))
        forms = (("device form", getattr(self.eng, call.name + "_device"), self.device_kw(call.kw)), ("host-array form", getattr(self.eng, call.name), call.kw))
        for form, fn, kw in forms:
            rec, n = fn(capacity=found + 16, **kw)
            got = rf.table(rec, call.fields)
            diff = rf.first_difference(got, want, call.fields)
            if diff or n != found:
                self.fail(call.entry, form, f"found {n}, the host form {found}; {diff}")
            if found:
                rec, n = fn(capacity=cap, **kw)
                diff = rf.first_difference(rf.table(rec, call.fields), want[:cap], call.fields)
                if diff or n != found:
                    self.fail(call.entry, form, f"capacity {cap}: found {n}, the host form {found}; {diff}")
            if form == "device form":
                device_table = got
        self.got[call.entry] = device_table
        return device_table

    def seed_list(self) -> np.ndarray:
        """the seed call's own output (device form) as the list the align calls take"""
        return rf.as_list(self.check(self.calls["align_seed_pairs_rates"]))

    def list_calls(self) -> dict:
        return {c.entry: c for c in rf.list_calls(self.fp, self.seed_list())}

    def relation(self, what, got, want, fields):
        diff = rf.first_difference(got, want, fields)
        if diff:
            self.fail(what, "device forms", diff)


# the profiles interleaved: bands-0, tiles-0, many_tiny-0, bands-1 ...
@pytest.fixture(scope="module", params=[(p, s) for s in range(SEEDS) for p in rf.PROFILES], ids=lambda c: f"{c[0]}-{c[1]}")
def run(request, eng):
    return Run(eng, *request.param)


def test_seed_call_and_align_in_four_modes(run):
    c = run.calls
    run.check(c["align_seed_pairs_rates"])
    align = run.check(c["align_windows_rates"])
    seeded = run.check(c["align_windows_rates[seed=1]"])
    run.relation("align_windows_rates with seed = 1 against seed = 0", seeded, align, rf.RATE_FIELDS)
    lists = run.list_calls()
    on_seeds = run.check(lists["align_windows_rates[seeds]"])
    run.check(lists["align_windows_rates[sublist]"])
    run.relation("align_windows_rates on the whole seed list against the call over every triple", on_seeds, align, rf.RATE_FIELDS)


def test_stretches_in_four_modes(run):
    c, fp = run.calls, run.fp
    align = run.check(c["align_windows_rates"])
    stretches = run.check(c["align_windows_rates_stretches"])
    run.relation("the rank-0 records of align_windows_rates_stretches against align_windows_rates", stretches[stretches[:, 8] == 0][:, :8], align, rf.RATE_FIELDS)
    seeded = run.check(c["align_windows_rates_stretches[seed=1]"])
    run.relation("align_windows_rates_stretches with seed = 1 against seed = 0", seeded, stretches, rf.RATE_STRETCH_FIELDS)
    lists = run.list_calls()
    on_seeds = run.check(lists["align_windows_rates_stretches[seeds]"])
    run.check(lists["align_windows_rates_stretches[sublist]"])
    run.relation("align_windows_rates_stretches on the whole seed list against the call over every triple", on_seeds, stretches, rf.RATE_STRETCH_FIELDS)
    once = dict(run.device_kw(c["align_windows_rates_stretches"].kw), max_stretches=1)
    rec, n = run.eng.align_windows_rates_stretches_device(capacity=len(align) + 16, **once)
    ranked = np.concatenate([align, np.zeros((len(align), 1), np.int64)], axis=1)
    run.relation("align_windows_rates_stretches with max_stretches = 1 against align_windows_rates", rf.table(rec, rf.RATE_STRETCH_FIELDS), ranked, rf.RATE_STRETCH_FIELDS)
    assert n == len(align)
    assert fp.max_stretches > 1 or np.array_equal(stretches, ranked)


def test_one_rate_job_and_duplicate_slots(run):
    fp, eng = run.fp, run.eng
    p = fp.p
    n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
    # block r alone, as a one-rate job and through align_windows_retimed: the same arrays, addressed from the block's first row
    r = run.seed % len(p.rates)
    lo = int(p.a_rate_first[r])
    d_ah, d_af, d_ak = run.ptr(p.a_hashes, np.int64) + lo * 128, run.ptr(p.a_first, np.int32) + r * (n_a + 1) * 4, run.ptr(p.a_skip, np.uint8)
    d_ak = d_ak + lo if d_ak else 0
    sides = (d_ah, d_af, n_a, run.ptr(p.b_hashes, np.int64), run.ptr(p.b_first, np.int32), n_b)
    common = dict(tol_int=p.tol, min_run=p.min_run, d_a_skip=d_ak, d_b_skip=run.ptr(p.b_skip, np.uint8), capacity=n_a * n_b + 16)
    one, n_one = eng.align_windows_rates_device(*sides, [p.rates[r]], a_rate_first=[0], **common)
    ret, n_ret = eng.align_windows_retimed_device(*sides, p.rates[r], **common)
    one = rf.table(one, rf.RATE_FIELDS)
    assert n_one == len(one) and n_ret == len(ret) and not one[:, 2].any()
    run.relation(f"a one-rate job on block {r} ({p.rates[r]}) against align_windows_retimed", one[:, [0, 1, 3, 4, 5, 6]], rf.table(ret, rf.RETIMED_FIELDS), rf.RETIMED_FIELDS)
    den = rf.lowest(p.rates[r])[1]
    assert np.array_equal(one[:, 7], (one[:, 5] - 1) * den + 16), "n_frames_b = (n_windows - 1) den + 16"
    if not p.exclude_same:   # and it is block r of the whole job
        whole = run.check(run.calls["align_windows_rates"])
        mine = whole[whole[:, 2] == r].copy()
        mine[:, 2] = 0
        run.relation(f"a one-rate job on block {r} against slot {r} of the whole job", one, mine, rf.RATE_FIELDS)
    # 3/2 and 6/4 on equal blocks: two slots, the same records up to the rate index
    if fp.params["dup_equal"]:
        x, y = (p.rates.index(rate) for rate in rf.CLASS_PAIRS[2])
        for entry, fields in (("align_seed_pairs_rates", rf.TRIPLE_FIELDS), ("align_windows_rates", rf.RATE_FIELDS), ("align_windows_rates_stretches", rf.RATE_STRETCH_FIELDS)):
            t = run.check(run.calls[entry])
            tx, ty = t[t[:, 2] == x].copy(), t[t[:, 2] == y].copy()
            tx[:, 2] = ty[:, 2] = 0
            run.relation(f"{entry}: slot {x} (3/2) against slot {y} (6/4) on equal blocks", tx, ty, fields)
