"""Randomised differential tests of the align kernels (csrc/align.hip) at the sizes where their structure is exercised: the seeded problems of
tests/alignfuzz.py through EVERY align entry point - the _device form on torch device arrays of exactly the problem's size (skip and zero
pointers 0 where absent) and the host-array form - against the plain C++ definitions the library ships as vdf_align_*_host, which
tests/test_align_fuzz_host.py pins to the independent numpy twins on the same generator.  Records and `found` are compared for equality.

The profiles (alignfuzz's docstring has the details and the constant behind every size):
  bands      2 - 5 videos per side of up to 260 windows: 1 - 8 bands of kAlignBand = 64 diagonals per pair, reloads and lane wraps inside a band,
             both orientations, empty videos - align_bands_kernel, its masked and its retimed form;
  tiles      B of 520 - 1100 windows: 2 - 3 tiles of kSeedTileRows = 512 rows, 3 - 5 of kSeedVariantsTileRows = 256, videos across every edge, a
             padded last tile; A with more than one chunk of kSeedChunk = 256 seeds - both seed kernels, the class layout;
  many_tiny  60 - 130 videos per side of 0 - 4 windows: thousands of pairs - more than kAlignWaves = 4 units per workgroup, more than one
             256-pair block of the reductions, the scan and the scatter, pair bitmaps of several hundred words with n_b no multiple of 32.

Per (profile, seed): align_windows, align_windows_stretches, align_seed_pairs, align_windows_pairs and align_windows_stretches_pairs on the seed
call's own output and on a drawn sublist (pairs of empty videos in it), window_variants for every variant of the mask and the class layout of
seeds and rows word for word, align_windows_variants, align_seed_pairs_variants, align_windows_variants_pairs on the seed triples and a drawn
sublist, align_windows_retimed and align_windows_retimed_pairs.  Relations between calls, which need no reference and localise a failure: the
rank-0 stretches are align_windows' records; the pairs call on the whole seed list is align_windows; the retimed call at rate 1 / 1 is
align_windows, field mapped; every call again with a drawn capacity below `found` (0 among them) returns the same `found` and the prefix.

ONE Engine for the whole file, on purpose: problems of very different sizes one after the other on one context are also the test for bitmap
words, scratch and band records left over from the call before.  A failure names profile, seed, entry point, form and the first record that
differs, and prints alignfuzz.describe(seed, profile): one failing seed is a complete report.

VDF_FUZZ_SEEDS=N widens the seed range for a soak run (default: 16 seeds per profile)."""
import os

import numpy as np
import pytest

import alignfuzz as fz

pytestmark = pytest.mark.gpu
# VDF_FUZZ_SEEDS=N widens every case list for a soak run (default sizes keep the suite fast)
_SOAK = int(os.environ.get("VDF_FUZZ_SEEDS", "0"))
SEEDS = max(16, _SOAK)
CAP = 1 << 18  # above every record count of these problems (16 900 pairs x 8 ranks)

_DEVICE_NAMES = {"a_hashes": ("d_a_hashes", np.int64), "a_first": ("d_a_first", np.int32), "a_skip": ("d_a_skip", np.uint8), "a_zero": ("d_a_zero", np.int64),
                 "b_hashes": ("d_b_hashes", np.int64), "b_first": ("d_b_first", np.int32), "b_skip": ("d_b_skip", np.uint8), "b_zero": ("d_b_zero", np.int64)}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


class Run:
    """one (profile, seed): the problem, its arrays on the device (uploaded once), the _host results (computed once)"""

    def __init__(self, eng, profile, seed):
        import vid_dup_finder_lib_amd as vdf

        self.eng, self.vdf, self.profile, self.seed = eng, vdf, profile, seed
        self.fp = fz.problem(seed, profile)
        self.caps = np.random.default_rng([fz.FUZZ, 1, seed])
        self.n_calls = 0
        self._dev, self._want, self.got = {}, {}, {}

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
        out["n_a"] = len(kw["a_first"]) - 1
        out["n_b"] = 0 if kw["b_first"] is None else len(kw["b_first"]) - 1
        return out

    def want(self, call):
        if call.entry not in self._want:
            self._want[call.entry] = fz.host_form(self.vdf, call, CAP)
            assert self._want[call.entry][1] <= CAP
        return self._want[call.entry]

    def fail(self, entry, form, text):
        pytest.fail(f"{self.profile} seed {self.seed}, {entry}, {form}: {text}\n{fz.describe(self.seed, self.profile)}", pytrace=False)

    def check(self, call) -> np.ndarray:
        """both forms of one call against its _host form, and again under a drawn capacity below `found`; -> the device form's table"""
        want, found = self.want(call)
        self.n_calls += 1
        cap = 0 if (self.seed + self.n_calls) % 4 == 0 or found == 0 else int(self.caps.integers(0, found))
        forms = (("device form", getattr(self.eng, call.name + "_device"), self.device_kw(call.kw)), ("host-array form", getattr(self.eng, call.name), call.kw))
        for form, fn, kw in forms:
            rec, n = fn(capacity=found + 16, **kw)
            got = fz.table(rec, call.fields)
            diff = fz.first_difference(got, want, call.fields)
            if diff or n != found:
                self.fail(call.entry, form, f"found {n}, the host form {found}; {diff}")
            if found:
                rec, n = fn(capacity=cap, **kw)
                diff = fz.first_difference(fz.table(rec, call.fields), want[:cap], call.fields)
                if diff or n != found:
                    self.fail(call.entry, form, f"capacity {cap}: found {n}, the host form {found}; {diff}")
            if form == "device form":
                self.got[call.entry] = got
        return self.got[call.entry]

    def relation(self, what, got, want, fields):
        diff = fz.first_difference(got, want, fields)
        if diff:
            self.fail(what, "device forms", diff)


@pytest.fixture(scope="module", params=[(p, s) for p in fz.PROFILES for s in range(SEEDS)], ids=lambda c: f"{c[0]}-{c[1]}")
def run(request, eng):
    return Run(eng, *request.param)


def test_plain_stretches_seeds_and_lists(run):
    c = {x.entry: x for x in fz.calls(run.fp)}
    align = run.check(c["align_windows"])
    stretches = run.check(c["align_windows_stretches"])
    run.relation("the rank-0 records of align_windows_stretches against align_windows", stretches[stretches[:, 6] == 0][:, :6], align, fz.ALIGN_FIELDS)
    seed_pairs = run.check(c["align_seed_pairs"])
    for call in fz.list_calls(run.fp, seed_pairs, np.zeros((0, 3), np.int64)):
        if "variants" not in call.name:
            run.check(call)
    run.relation("align_windows_pairs on the whole seed list against align_windows", run.got["align_windows_pairs[seeds]"], align, fz.ALIGN_FIELDS)


def test_variant_sets_class_layout_and_variant_calls(run):
    import torch

    fp, eng, vdf = run.fp, run.eng, run.vdf
    p = fp.p
    bh, bz, bf, bs = (p.a_hashes, fp.a_zero, p.a_first, p.a_skip) if fp.self_mode else (p.b_hashes, fp.b_zero, p.b_first, p.b_skip)
    d_h, d_z, d_f, d_s = run.ptr(bh, np.int64), run.ptr(bz, np.int64), run.ptr(bf, np.int32), run.ptr(bs, np.uint8)
    n = len(bh)
    for v in range(1, 8):
        if not fp.mask >> v & 1:
            continue
        out = torch.full((n, 16), -1, dtype=torch.int64, device="cuda")
        out_k = torch.full((n,), 255, dtype=torch.uint8, device="cuda") if bs is not None else None
        torch.cuda.synchronize()
        eng.window_variants(d_h, d_z, d_f, len(bf) - 1, v, out.data_ptr(), d_s, 0 if out_k is None else out_k.data_ptr())
        torch.cuda.synchronize()
        want = vdf.window_variants_host(bh, bz, bf, v, bs)
        want_h, want_k = want if bs is not None else (want, None)
        got = out.cpu().numpy().view(np.uint64)
        if not np.array_equal(got, want_h):
            row = int(np.flatnonzero((got != want_h).any(axis=1))[0])
            run.fail("window_variants", "device form", f"variant {v}, row {row}: got {got[row].tolist()}, want {want_h[row].tolist()}")
        if bs is not None and not np.array_equal(out_k.cpu().numpy(), want_k):
            run.fail("window_variants", "device form", f"variant {v}: skip byte {int(np.flatnonzero(out_k.cpu().numpy() != want_k)[0])} differs")
    layouts = (("seeds", p.a_hashes, p.a_first, None, p.a_skip, p.min_run), ("rows", bh, bf, bz, bs, 1), ("rows of A", p.a_hashes, p.a_first, fp.a_zero, p.a_skip, 1))
    for what, h, f, z, s, min_run in layouts:
        want = vdf.window_class_layout_host(h, f, z, s, min_run)
        out = torch.full((len(h), want.shape[1]), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rows = eng.window_class_layout_device(run.ptr(h, np.int64), run.ptr(f, np.int32), len(f) - 1, out.data_ptr(), len(h), run.ptr(z, np.int64), run.ptr(s, np.uint8), min_run)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)[:rows]
        if rows != len(want) or not np.array_equal(got, want):
            row = int(np.flatnonzero((got[:len(want)] != want[:rows]).any(axis=1))[0]) if rows == len(want) else -1
            run.fail("window_class_layout_device", what, f"{rows} rows for {len(want)}" + (f"; row {row}: got {got[row].tolist()}, want {want[row].tolist()}" if row >= 0 else ""))

    c = {x.entry: x for x in fz.calls(fp)}
    run.check(c["align_windows_variants"])
    seed_triples = run.check(c["align_seed_pairs_variants"])
    for call in fz.list_calls(fp, np.zeros((0, 2), np.int64), seed_triples):
        if "variants" in call.name:
            run.check(call)


def test_retimed_calls(run):
    fp = run.fp
    c = {x.entry: x for x in fz.calls(fp)}
    run.check(c["align_windows_retimed"])
    run.check(c["align_windows_retimed_pairs[sublist]"])
    two = fz.plain_args(fp.two)
    align = run.check(fz.Call("align_windows[two-sided]", "align_windows", two, fz.ALIGN_FIELDS))
    unit = run.check(fz.Call("align_windows_retimed[1/1]", "align_windows_retimed", dict(two, rate=(1, 1)), fz.RETIMED_FIELDS))
    mapped = np.stack([align[:, 0], align[:, 1], align[:, 3], align[:, 3] + align[:, 2], align[:, 4], align[:, 5]], axis=1).reshape(-1, 6)
    run.relation("align_windows_retimed at rate 1 / 1 against align_windows (first_a = start_a, first_b = start_a + offset)", unit, mapped, fz.RETIMED_FIELDS)
