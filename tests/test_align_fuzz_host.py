"""The random align problems of tests/alignfuzz.py on the CPU: what makes tests/test_gpu_align_fuzz.py worth its GPU time.

(a) The _host definitions against the numpy twins.  For the first TWIN_SEEDS seeds of every profile (the GPU file's default range), at the REDUCED size the twins can walk cell
    by cell (alignfuzz.problem(..., reduced=True): bands - at most 3 videos per side of at most 140 windows, the edges at 64 and 128 kept; tiles -
    B 520 - 600 windows over the 512-row tile edge, A just over the 256 seeds of a chunk; many_tiny - 60 - 95 videos per side), every _host form
    against its twin, records field for field and `found`: align_windows, align_windows_stretches, align_seed_pairs, align_windows_pairs,
    align_windows_stretches_pairs, align_windows_variants, align_seed_pairs_variants, align_windows_variants_pairs, align_windows_retimed,
    align_windows_retimed_pairs, window_variants and window_class_layout.  The twins of the list forms are the all-pairs twins filtered by
    the list (seedgen.pairs_twin, seedvariantgen.records_twin say so); the filter is applied here, to one walk.  This is what makes the _host
    forms a reference for the GPU file on problems of this kind.
(b) The generator is not vacuous: over the GPU file's default seeds (GPU_SEEDS per profile) at FULL size, by the _host forms alone - the
    conditions are asserted, the counts printed (profiles/align_fuzz.txt keeps them).  A record's band is (offset + Na - 1) // 64 (align_plan.h:
    align_band_d0); its run crosses a reload where its rows of B pass a multiple of 64 - the lane that held row kb takes row kb + 64 and the run
    state wraps from lane 63 to lane 0 (align_row_lane, align_rotate_source).
(c) alignfuzz.check_words - where the tolerance list has its edges - against align_seed_check_words itself, through a three-line C++ program.

Measured: 27 s for the file with TWIN_SEEDS = 16 - (a) 48 problems 23 s, at most 3 s each; (b) 48 problems at full size 3 s - with numpy's matrix
products spread over the cores: 3 minutes of CPU time in all, which is what a single core would take."""
import functools
import os
import subprocess

import numpy as np
import pytest

import alignfuzz as fz
import aligngen
import hashgen
import retimedaligngen as rag
import seedgen
import seedvariantgen as svg
import stretchgen
import variantgen as vg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN_SEEDS = 16    # per profile, reduced size, every form against its twin: the GPU file's default seeds
GPU_SEEDS = 16     # per profile: the default of tests/test_gpu_align_fuzz.py
CAP = 1 << 18      # above every record count of these problems (16 900 pairs x 8 ranks)


def _vdf():
    import vid_dup_finder_lib_amd as vdf

    return vdf


def _same(entry, fp, got, want, fields):
    got_t, found = got
    want_t = fz.table(want, fields)
    diff = fz.first_difference(got_t, want_t, fields)
    q = fp.params
    assert not diff and found == len(want_t), f"{q['profile']} seed {q['seed']} (reduced) {entry}: found {found}, twin {len(want_t)}; {diff}"


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(TWIN_SEEDS))
@pytest.mark.parametrize("profile", fz.PROFILES)
def test_host_forms_equal_their_twins(profile, seed):
    vdf = _vdf()
    fp = fz.problem(seed, profile, reduced=True)
    p, self_mode = fp.p, fp.self_mode
    host = {c.entry: fz.host_form(vdf, c, CAP) for c in fz.calls(fp)}
    seed_pairs, seed_triples = host["align_seed_pairs"][0], host["align_seed_pairs_variants"][0]
    host.update({c.entry: fz.host_form(vdf, c, CAP) for c in fz.list_calls(fp, seed_pairs, seed_triples)})

    align = aligngen.align_twin(p)
    stretches = stretchgen.stretches_twin(p, fp.max_stretches, fp.guard)
    _same("align_windows", fp, host["align_windows"], align, fz.ALIGN_FIELDS)
    _same("align_windows_stretches", fp, host["align_windows_stretches"], stretches, fz.STRETCH_FIELDS)
    _same("align_seed_pairs", fp, host["align_seed_pairs"], seedgen.seed_twin(p), fz.PAIR_FIELDS)
    vp = vg.VariantProblem(p, fp.a_zero if self_mode else None, None if self_mode else fp.b_zero, fp.mask)
    all_variants = vg.twin(vp._replace(mask=svg.ALL))
    _same("align_windows_variants", fp, host["align_windows_variants"], [r for r in all_variants if fp.mask >> r[0] & 1], fz.VARIANT_FIELDS)
    _same("align_seed_pairs_variants", fp, host["align_seed_pairs_variants"], svg.seed_twin(vp), fz.TRIPLE_FIELDS)
    for which, pairs, triples in (("seeds", seed_pairs, seed_triples), ("sublist", fp.pairs, fp.triples)):
        want_p, want_t = set(map(tuple, pairs.tolist())), set(map(tuple, triples.tolist()))
        _same(f"align_windows_pairs[{which}]", fp, host[f"align_windows_pairs[{which}]"], [r for r in align if r[:2] in want_p], fz.ALIGN_FIELDS)
        _same(f"align_windows_stretches_pairs[{which}]", fp, host[f"align_windows_stretches_pairs[{which}]"], [r for r in stretches if r[:2] in want_p],
              fz.STRETCH_FIELDS)
        _same(f"align_windows_variants_pairs[{which}]", fp, host[f"align_windows_variants_pairs[{which}]"], [r for r in all_variants if r[:3] in want_t],
              fz.VARIANT_FIELDS)
    t = fp.two
    rp = rag.Problem(t.a_hashes, t.a_first, t.b_hashes, t.b_first, fp.rate, t.tol, t.min_run, t.a_skip, t.b_skip)
    _same("align_windows_retimed", fp, host["align_windows_retimed"], rag.align_retimed_twin(rp), fz.RETIMED_FIELDS)
    _same("align_windows_retimed_pairs[sublist]", fp, host["align_windows_retimed_pairs[sublist]"],
          rag.align_retimed_twin(rp, pairs=[tuple(x) for x in fp.pairs_two.tolist()]), fz.RETIMED_FIELDS)

    # the derived sets and the class-major rows, word for word
    bh, bz, bf, bs = (p.a_hashes, fp.a_zero, p.a_first, p.a_skip) if self_mode else (p.b_hashes, fp.b_zero, p.b_first, p.b_skip)
    for v in vg.ALL_VARIANTS:
        got, want = vdf.window_variants_host(bh, bz, bf, v, bs), vg.variant_twin(bh, bz, bf, v, bs)
        if bs is None:
            got, want = (got,), (want,)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"{profile} seed {seed} (reduced) window_variants, variant {v}"
    assert np.array_equal(vdf.window_class_layout_host(p.a_hashes, p.a_first, None, p.a_skip, p.min_run),
                          svg.class_layout_twin(p.a_hashes, p.a_first, None, p.a_skip, p.min_run)), f"{profile} seed {seed} (reduced) class layout, seeds"
    assert np.array_equal(vdf.window_class_layout_host(bh, bf, bz, bs), svg.class_layout_twin(bh, bf, bz, bs)), f"{profile} seed {seed} (reduced) class layout, rows"


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------
def _tied(fp, align) -> bool:
    """some pair with a record (the first 300 of them) has two runs of the best score: retimedaligngen's run finder on the pair's matrix"""
    p = fp.p
    bh, bf, bs = (p.a_hashes, p.a_first, p.a_skip) if fp.self_mode else (p.b_hashes, p.b_first, p.b_skip)
    dist = hashgen.all_distances(p.a_hashes, bh)
    ska = np.zeros(len(p.a_hashes), bool) if p.a_skip is None else np.asarray(p.a_skip) != 0
    skb = np.zeros(len(bh), bool) if bs is None else np.asarray(bs) != 0
    for a, b in align[:300, :2].tolist():
        a0, a1, b0, b1 = int(p.a_first[a]), int(p.a_first[a + 1]), int(bf[b]), int(bf[b + 1])
        scores = [r[0] for r in rag.diagonal_runs(dist[a0:a1, b0:b1], ~ska[a0:a1, None] & ~skb[None, b0:b1], min(p.tol, 1024), p.min_run)]
        if scores.count(max(scores)) > 1:
            return True
    return False


def _seed_hits_outside_the_first(fp, seed_pairs) -> tuple:
    """(a listed pair has a matching cell whose row of B lies behind tile 0, a listed pair has one whose seed lies behind chunk 0) - from the
    distance matrix, in numpy"""
    p = fp.p
    bh, bf, bs = (p.a_hashes, p.a_first, p.a_skip) if fp.self_mode else (p.b_hashes, p.b_first, p.b_skip)
    seeds = np.array([w for v in range(len(p.a_first) - 1) for w in range(int(p.a_first[v]), int(p.a_first[v + 1]), p.min_run)])
    vid_a = np.searchsorted(p.a_first.astype(np.int64), seeds, side="right") - 1
    vid_b = np.searchsorted(bf.astype(np.int64), np.arange(len(bh)), side="right") - 1
    hit = hashgen.all_distances(p.a_hashes[seeds], bh) <= min(p.tol, 1024)
    if p.a_skip is not None:
        hit &= (np.asarray(p.a_skip)[seeds] == 0)[:, None]
    if bs is not None:
        hit &= (np.asarray(bs) == 0)[None, :]
    if fp.self_mode:
        hit &= vid_a[:, None] < vid_b[None, :]
    listed = set(map(tuple, seed_pairs.tolist()))
    tile = {(int(vid_a[s]), int(vid_b[r + fz.SEED_TILE_ROWS])) for s, r in zip(*np.nonzero(hit[:, fz.SEED_TILE_ROWS:]))}
    chunk = {(int(vid_a[s + fz.SEED_CHUNK]), int(vid_b[r])) for s, r in zip(*np.nonzero(hit[fz.SEED_CHUNK:]))}
    return bool(tile & listed), bool(chunk & listed)


@functools.lru_cache(maxsize=None)
def _coverage():
    vdf = _vdf()
    rows = []
    for profile in fz.PROFILES:
        for seed in range(GPU_SEEDS):
            fp = fz.problem(seed, profile)
            c = {x.entry: x for x in fz.calls(fp)}
            align, found = fz.host_form(vdf, c["align_windows"], CAP)
            stretches, n_st = fz.host_form(vdf, c["align_windows_stretches"], CAP)
            assert found == len(align) and n_st == len(stretches), "CAP is too small"
            q = dict(profile=profile, seed=seed, has_record=found > 0, rank2=bool((stretches[:, 6] >= 2).any()), tied=found > 0 and _tied(fp, align),
                     check_words=fz.check_words(min(fp.p.tol, 1024)), rate=fp.rate, mask=fp.mask, max_stretches=fp.max_stretches,
                     content=fp.params["content"])
            if profile == "bands" and found:
                na = np.diff(fp.p.a_first.astype(np.int64))[align[:, 0]]
                start_b = align[:, 3] + align[:, 2]
                q["other_band"] = bool((((align[:, 2] + na - 1) // fz.ALIGN_BAND) != 0).any())
                q["reload"] = bool(((start_b // fz.ALIGN_BAND) != ((start_b + align[:, 4] - 1) // fz.ALIGN_BAND)).any())
            if profile == "tiles":
                q["other_tile"], q["other_chunk"] = _seed_hits_outside_the_first(fp, fz.host_form(vdf, c["align_seed_pairs"], CAP)[0])
            rows.append(q)
    return rows


def _share(rows, key):
    return sum(bool(r.get(key)) for r in rows), len(rows)


def test_the_generator_is_not_vacuous():
    rows = _coverage()
    bands, tiles = [r for r in rows if r["profile"] == "bands"], [r for r in rows if r["profile"] == "tiles"]
    report = {"problems": len(rows), "with an align record": _share(rows, "has_record"), "bands: a record outside band 0": _share(bands, "other_band"),
              "bands: a run across a 64-row reload": _share(bands, "reload"), "tiles: a seed hit behind tile 0": _share(tiles, "other_tile"),
              "tiles: a seed hit behind chunk 0": _share(tiles, "other_chunk"), "a stretch of rank >= 2": _share(rows, "rank2"),
              "tied best runs": _share(rows, "tied"),
              "check words": {w: sum(r["check_words"] == w for r in rows) for w in fz.CHECK_WORDS},
              "rates": {f"{n}/{d}": sum(r["rate"] == (n, d) for r in rows) for n, d in fz.RATES},
              "variant bits": {v: sum(r["mask"] >> v & 1 for r in rows) for v in range(1, 8)},
              "max_stretches": {m: sum(r["max_stretches"] == m for r in rows) for m in fz.MAX_STRETCHES},
              "content": {c: sum(r["content"] == c for r in rows) for c in fz.CONTENTS}}
    for k, v in report.items():
        print(f"{k}: {v}")
    assert len(rows) == len(fz.PROFILES) * GPU_SEEDS, "no problem is skipped"
    ok = lambda key, rs, share: _share(rs, key)[0] >= share * len(rs)
    assert ok("has_record", rows, 0.9), "at least 90 % of the problems have an align record"
    assert ok("other_band", bands, 1 / 3), "a third of the bands problems have a record outside band 0 of its pair"
    assert ok("reload", bands, 1 / 3), "a third of the bands problems have a record whose run crosses a 64-row reload"
    assert all(r["other_tile"] for r in tiles), [r["seed"] for r in tiles if not r["other_tile"]]
    assert all(r["other_chunk"] for r in tiles), [r["seed"] for r in tiles if not r["other_chunk"]]
    assert all(report["check words"].values()) and all(report["rates"].values()) and all(report["variant bits"].values()) and all(report["max_stretches"].values())
    assert ok("rank2", rows, 0.25), "a quarter of the problems produce a stretch of rank >= 2"
    assert ok("tied", rows, 0.25), "a quarter of the problems have tied best runs"


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------
def test_check_words_is_the_librarys():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_fuzz_check_words")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_fuzz_check_words_main.cpp")])
    theirs = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()]
    ours = [fz.check_words(t) for t in range(1025)]
    assert theirs == ours
    edges = [t for t in range(1024) if ours[t] != ours[t + 1]]
    assert edges == [179, 297, 357] and all(e in fz.TOLERANCES and e + 1 in fz.TOLERANCES for e in edges), edges
    assert sorted({fz.check_words(min(t, 1024)) for t in fz.TOLERANCES}) == list(fz.CHECK_WORDS)
