"""vdf_align_seed_pairs_variants_host and vdf_align_windows_variants_pairs_host (the definitions in plain C++) against the numpy
twin of tests/seedvariantgen.py, triples and records equal, on the problems the GPU tests give the kernels and on 200 random ones; the superset
property and the independence of the reversal asserted directly; the pairs that are candidates under one variant only; the hashes on and one over
the tolerance under a variant; align_flipped(seed=True) and align_flipped(pairs=...) equal to the plain call, also across a forced split into
blocks; the list checks with their messages and their order; the C++ mirror.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import aligngen
import hashgen
import planegen
import seedgen
import seedvariantgen as svg
import variantgen

import vid_dup_finder_lib_amd as vdf
from vid_dup_finder_lib_amd import Flip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seed_host(vp, mask=None, capacity=1 << 16, min_run=None):
    kw = svg.call_args(vp, mask)
    if min_run is not None:
        kw["min_run"] = min_run
    a_hashes, a_first = kw.pop("a_hashes"), kw.pop("a_first")
    got, found = vdf.align_seed_pairs_variants_host(a_hashes, a_first, capacity=capacity, **kw)
    return svg.triples_of(got), found


def pairs_host(vp, triples, capacity=1 << 16):
    kw = svg.list_args(vp)
    a_hashes, a_first = kw.pop("a_hashes"), kw.pop("a_first")
    t = np.array([(a, b, v) for v, a, b in triples], vdf.VIDEO_PAIR_VARIANT_DTYPE)
    rec, found = vdf.align_windows_variants_pairs_host(a_hashes, a_first, t, capacity=capacity, **kw)
    return variantgen.records(rec), found


@pytest.mark.parametrize("name", sorted(svg.BUILDERS))
def test_host_forms_match_the_twin(name):
    vp, want = svg.case(name), list(svg.expected(name))
    got, found = seed_host(vp)
    print(f"{name}: mask {vp.mask:#010b}, {len(want)} candidate triples, host form found {found}")
    assert found == len(want) and got == want
    recs = list(svg.expected_records(name))
    assert {r[:3] for r in recs} <= set(want)                       # the superset, on every problem
    assert pairs_host(vp, want) == (recs, len(recs))                # the listed call on the candidates: the all-pairs records
    sub = want[::2]
    assert pairs_host(vp, sub)[0] == svg.records_twin(vp, sub)


def test_host_forms_on_random_problems():
    rng = np.random.default_rng(1414)
    candidates = records = 0
    for _ in range(200):
        vp = svg.random_problem(rng)
        want = svg.seed_twin(vp)
        assert seed_host(vp) == (want, len(want))
        recs = variantgen.twin(vp)
        assert {r[:3] for r in recs} <= set(want)
        assert pairs_host(vp, want)[0] == recs
        every = svg.all_triples(vp)
        assert pairs_host(vp, every)[0] == recs
        candidates += len(want)
        records += len(recs)
    assert candidates > 200 and records > 100


@pytest.mark.parametrize("name", ["tile_edges", "tile_edges_self", "variant_self_mode_all", "variant_all_variants_order"])
def test_every_record_is_a_candidate_at_min_run_1_to_6(name):
    vp = svg.case(name)
    for m in range(1, 7):
        q = vp._replace(p=vp.p._replace(min_run=m))
        cand = set(svg.seed_twin(q))
        recs = variantgen.twin(q)
        assert {r[:3] for r in recs} <= cand, m
        assert set(seed_host(q)[0]) == cand


@pytest.mark.parametrize("name", ["tile_edges", "tile_edges_self", "only_under_5"])
def test_the_reversal_does_not_enter_the_candidate_set(name):
    """bit 2 of v reorders b's rows: the candidates under v are those of the set made with M_v and Z in the ORIGINAL row order"""
    vp = svg.case(name)
    p = vp.p._replace(a_skip=None, b_skip=None)
    self_mode = p.b_hashes is None
    bh, bz = (p.a_hashes, vp.a_zero) if self_mode else (p.b_hashes, vp.b_zero)
    vq = vp._replace(p=p, mask=svg.ALL)
    got = svg.seed_twin(vq)
    for v in (4, 5, 6, 7):
        unordered = (bh ^ planegen.variant_mask(v)) & ~bz
        q = p._replace(b_hashes=unordered, b_first=p.a_first if self_mode else p.b_first)
        want = [(v, a, b) for a, b in seedgen.seed_twin(q) if not self_mode or a < b]
        assert [t for t in got if t[0] == v] == want
    assert seed_host(vq)[0] == got


def test_candidate_under_one_variant_only():
    got5 = seed_host(svg.case("only_under_5"))[0]
    assert (5, 0, 1) in got5 and not {(1, 0, 1), (4, 0, 1)} & set(got5)
    for v in (1, 4):
        got = seed_host(svg.case(f"only_under_{v}"))[0]
        assert (v, 0, 1) in got and (5, 0, 1) not in got and (5 - v, 0, 1) not in got


@pytest.mark.parametrize("name,tol", [("on_the_tolerance", 350), ("on_the_tolerance_100", 100)])
def test_on_and_one_over_the_tolerance_under_a_variant(name, tol):
    vp = svg.case(name)
    got = set(seed_host(vp)[0])
    n = len(vp.p.a_first) - 1
    assert n == 84
    for i in range(n):
        v = 1 + i // 12
        assert ((v, i, i) in got) == (i % 2 == 0), (i, v)   # even: exactly tol under v; odd: tol + 1
    assert got == set(svg.expected(name))


def test_capacity_protocol_of_the_host_forms():
    vp, want = svg.case("tile_edges"), list(svg.expected("tile_edges"))
    recs = list(svg.expected_records("tile_edges"))
    assert len(want) > 5 and len(recs) > 5
    for cap in (5, 0, len(want)):
        assert seed_host(vp, capacity=cap) == (want[:cap], len(want))
    for cap in (5, 0, len(recs)):
        assert pairs_host(vp, want, capacity=cap) == (recs[:cap], len(recs))


def _windows(hashes, zero, first, name):
    return [[vdf.VideoHash(hashes[k], name, 1, None if zero is None else zero[k]) for k in range(int(first[i]), int(first[i + 1]))] for i in range(len(first) - 1)]


@pytest.mark.parametrize("name", ["variant_all_variants_order_all", "variant_self_mode_all", "variant_static_skipped", "tile_edges"])
def test_align_flipped_seeded_and_listed_equals_the_plain_call(name, monkeypatch):
    vp = svg.case(name)
    p = vp.p
    self_mode = p.b_hashes is None
    cells = len(p.a_hashes) * len(p.a_hashes if self_mode else p.b_hashes)
    assert cells * 7 <= vdf.api.ALIGN_HOST_CELLS or name.startswith("tile"), "the host forms are what runs here"
    if name.startswith("tile"):
        monkeypatch.setattr(vdf.api, "ALIGN_HOST_CELLS", 1 << 40)
    wa = _windows(p.a_hashes, vp.a_zero, p.a_first, "a")
    wb = None if self_mode else _windows(p.b_hashes, vp.b_zero, p.b_first, "b")
    flips = [Flip(v) for v in variantgen.ALL_VARIANTS if vp.mask >> v & 1]
    static = lambda skip, first: None if skip is None else [skip[int(first[i]):int(first[i + 1])] for i in range(len(first) - 1)]
    kw = dict(tolerance=p.tol / 1000, min_run=p.min_run, stride=2, flips=flips, static_a=static(p.a_skip, p.a_first),
              static_b=None if self_mode else static(p.b_skip, p.b_first))
    assert vdf.api.tolerance_int(kw["tolerance"]) == p.tol
    plain = vdf.align_flipped(wa, wb, **kw)
    assert sum(map(len, plain.values())) == len(svg.expected_records(name)) and (plain != {f: [] for f in flips} or name == "variant_static_skipped")
    seeded = vdf.align_flipped(wa, wb, seed=True, **kw)
    assert seeded == plain
    cand = vdf.candidate_pairs_flipped(wa, wb, **{k: v for k, v in kw.items() if k != "stride"})
    assert all({(g.a, g.b) for g in plain[f]} <= set(cand[f]) for f in flips)
    assert vdf.align_flipped(wa, wb, pairs=cand, **kw) == plain
    some = {f: cand[f][::2] for f in flips}
    want = {f: [g for g in plain[f] if (g.a, g.b) in set(some[f])] for f in flips}
    assert vdf.align_flipped(wa, wb, pairs=some, **kw) == want
    assert vdf.align_flipped(wa, wb, pairs=some, seed=True, **kw) == want
    one_list = sorted(set().union(*[set(c) for c in cand.values()]))
    assert vdf.align_flipped(wa, wb, pairs=one_list, **kw) == plain
    # a forced split: blocks of 2 x 2 videos
    monkeypatch.setattr(vdf.api, "ALIGN_MAX_PAIRS", 4)
    assert vdf.align_flipped(wa, wb, **kw) == plain
    assert vdf.align_flipped(wa, wb, seed=True, **kw) == plain
    assert vdf.align_flipped(wa, wb, pairs=some, seed=True, **kw) == want
    assert vdf.candidate_pairs_flipped(wa, wb, **{k: v for k, v in kw.items() if k != "stride"}) == cand
    with pytest.raises(ValueError, match="strictly increasing"):
        vdf.align_flipped(wa, wb, pairs=[(0, 1), (0, 1)], **kw)


def test_list_checks_with_their_messages_and_their_order():
    vp = svg.case("variant_mirrored")      # 2 x 2 videos
    self_vp = svg.case("variant_self_mode")  # 5 videos
    T = lambda *t: [(v, a, b) for v, a, b in t]

    def refused(vp, triples, match, **over):
        kw = svg.list_args(vp)
        kw.update(over)
        a_hashes, a_first = kw.pop("a_hashes"), kw.pop("a_first")
        with pytest.raises(vdf.VdfError, match=match) as ei:
            vdf.align_windows_variants_pairs_host(a_hashes, a_first, np.array(triples, np.int64).reshape(-1, 3), **kw)
        assert ei.value.code == -5

    refused(vp, T((1, 0, 1), (1, 0, 1)), "not strictly increasing in \\(variant, a, b\\) at entry 1")
    refused(vp, T((2, 0, 0), (1, 0, 1)), "not strictly increasing in \\(variant, a, b\\) at entry 1")
    refused(vp, T((1, 1, 0), (1, 0, 1)), "not strictly increasing in \\(variant, a, b\\) at entry 1")
    refused(vp, T((1, 0, 0), (8, 0, 5)), "triple 1 of the list has a variant outside 1 ... 7")       # (and a video that does not exist)
    refused(vp, T((0, 0, 0)), "triple 0 of the list has a variant outside 1 ... 7")
    refused(vp, T((1, 0, 0), (1, 0, 2)), "triple 1 of the list names a video that does not exist")
    refused(vp, T((1, 2, 0)), "triple 0 of the list names a video that does not exist")
    refused(self_vp, T((1, 0, 1), (3, 2, 2)), "triple 1 of the list has a >= b in self mode")
    refused(self_vp, T((1, 0, 1), (3, 4, 9)), "triple 1 of the list names a video that does not exist")   # (and a >= b is not said)
    refused(vp, T((1, 0, 1)), "bad argument", min_run=0)
    refused(vp, T((1, 0, 1)), "bad argument", b_zero=None)                                                # the zero plane, behind a good list
    refused(vp, T((1, 0, 1), (1, 0, 0)), "not strictly increasing", b_zero=None)                          # ... and behind a bad one
    # the seed form: the mask, then the zero plane
    kw = svg.call_args(vp)
    a_hashes, a_first = kw.pop("a_hashes"), kw.pop("a_first")
    for bad in (dict(variant_mask=1), dict(variant_mask=0x102), dict(b_zero=None), dict(min_run=0)):
        with pytest.raises(vdf.VdfError):
            vdf.align_seed_pairs_variants_host(a_hashes, a_first, **{**kw, **bad})
    got, found = vdf.align_seed_pairs_variants_host(a_hashes, a_first, **{**kw, "variant_mask": 0})
    assert found == 0 and len(got) == 0
    rec, found = vdf.align_windows_variants_pairs_host(a_hashes, a_first, [], **{k: v for k, v in svg.list_args(vp).items() if k not in ("a_hashes", "a_first")})
    assert found == 0 and len(rec) == 0


@pytest.mark.parametrize("min_run", [1, 3, 300])
def test_class_layout_host_form_against_the_numpy_twin(min_run):
    """vdf_window_class_layout_host (the host twin of align_class_layout_kernel, both from csrc/window_class_layout.h) against the layout written
    from the header's text in numpy: seeds and rows, word for word; and the rows give the distance to every variant by the identity"""
    hashes, zero, first, skip = svg.layout_problem()
    for sk in (None, skip):
        seeds = vdf.window_class_layout_host(hashes, first, skip=sk, min_run=min_run)
        assert seeds.shape == (sum(-(-(int(first[v + 1]) - int(first[v])) // min_run) for v in range(len(first) - 1)), 36)
        assert np.array_equal(seeds, svg.class_layout_twin(hashes, first, None, sk, min_run))
        rows = vdf.window_class_layout_host(hashes, first, zero=zero, skip=sk, min_run=min_run)
        assert rows.shape == (772, 72) and np.array_equal(rows, svg.class_layout_twin(hashes, first, zero, sk))
    assert len(vdf.window_class_layout_host(hashes[:0], [0], min_run=1)) == 0
    with pytest.raises(vdf.VdfError):
        vdf.window_class_layout_host(hashes, [5, 3], min_run=1)
    # the identity on the rows: seed s against row r under variant v
    pc = lambda x: np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).sum(-1).astype(np.int64)
    seeds, rows = vdf.window_class_layout_host(hashes, first, min_run=1)[:40], vdf.window_class_layout_host(hashes, first, zero=zero)[:60]
    t = seeds[:, None, :33] & rows[None, :, 36:69]
    u = t ^ rows[None, :, :33]
    cls = np.array([0] * 5 + [c for c in range(1, 8) for _ in range(4)])
    acc = np.stack([pc(u[:, :, cls == c]) for c in range(8)], axis=-1)
    live = np.stack([np.zeros(len(rows), np.int64)] + [(rows[:, 33 + (c - 1) // 4].astype(np.int64) >> (8 * ((c - 1) % 4))) & 0xFF for c in range(1, 8)], axis=-1)
    for v in variantgen.ALL_VARIANTS:
        d = seeds[:, 33].astype(np.int64)[:, None] - pc(t) + acc[:, :, 0]
        for c in range(1, 8):
            d = d + (live[None, :, c] - acc[:, :, c] if bin(v & c).count("1") & 1 else acc[:, :, c])
        derived = (hashes[5:65] ^ planegen.variant_mask(v)) & ~zero[5:65]
        assert np.array_equal(d, hashgen.all_distances(hashes[5:45], derived))


def test_the_python_copy_of_the_list_messages_is_the_library_s_text():
    """engine.triple_list_problem names the list's problem for the host forms, which have no context to keep a message in: every message it can
    give stands word for word in csrc/api.cpp, so the copy cannot drift from the library's text unnoticed"""
    import re

    src = open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc", "api.cpp")).read()
    t = lambda *x: np.array([(a, b, v) for v, a, b in x], vdf.VIDEO_PAIR_VARIANT_DTYPE)
    cases = [(t((1, 0, 1), (1, 0, 1)), 2, 2, False), (t((9, 0, 1)), 2, 2, False), (t((1, 0, 5)), 2, 2, False), (t((1, 1, 1)), 2, 2, True)]
    for lst, n_a, n_b, self_mode in cases:
        msg = vdf.engine.triple_list_problem(lst, n_a, n_b, self_mode)
        head, _, tail = msg.partition(str(len(lst) - 1))
        assert head and ('"' + head in src) and (not tail or tail + '"' in src), msg
    assert vdf.engine.triple_list_problem(t((1, 0, 1), (2, 0, 1)), 2, 2, False) is None


def test_cpp_mirror_seeds_and_aligns_the_flipped_candidates_on_the_cpu():
    lib = os.path.join(ROOT, "vid_dup_finder_lib_amd")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_seed_variants_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(lib, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_seed_variants_mirror_main.cpp"),
                           "-L" + lib, "-lvdf_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "align seed variants mirror ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
