"""The random rate-list problems of tests/ratefuzz.py on the CPU: what makes tests/test_gpu_zz_align_fuzz_rates.py worth its GPU time.

(a) The _host definitions against the numpy twins.  For the GPU file's default seeds of every profile at the REDUCED size the twins can walk
    (ratefuzz.problem(..., reduced=True): at most 3 rates; bands - at most 3 videos per side, the sub-matrix edges at 64 and 128 kept; tiles - B
    520 - 600 windows over the 512-row tile edge of the class of den 1, a padded tile in the class of den 4, just over 256 seeds in two slots;
    many_tiny - 60 - 95 videos per side), every _host form in every mode against its twin, records field for field and `found`:
    align_seed_pairs_rates (seedrategen.seed_rates_twin), align_windows_rates (ratealigngen.twin) and align_windows_rates_stretches
    (ratestretchgen.twin) over every triple, with seed = 1, on the seed call's own output and on the drawn sublist.  The twins of the list modes are
    the all-triples twins filtered by the list; the twin of seed = 1 is the all-triples twin.  This is what makes the _host forms a reference for
    the GPU file on problems of this kind.
(b) The generator is not vacuous: over the GPU file's default seeds (GPU_SEEDS per profile) at FULL size, by the _host forms and numpy alone - the
    conditions are asserted, the counts printed (profiles/align_fuzz_rates.txt keeps them).  A record lies in phase first_a % num, at cell
    (i0, j0) = (first_a // num, first_b // den) of that phase's sub-matrix; its band is (j0 - i0 + rows - 1) // 64 with the phase's rows (align_plan.h:
    align_band_d0); its run crosses a reload where its columns pass a multiple of 64 (align_row_lane).  The seed kernel's view - the gathered rows of
    a class, its seeds in chunks of 256 - is rebuilt from align_seed_rates_plan.h's rules in ratefuzz.class_rows / class_seeds, and the candidate
    set that brute-force distances give on it must be the host form's: the seed definition once more, at full size.

Measured: 34 s for the file - (a) 48 problems 29 s, the slowest (many_tiny, 27 000 triples through the twins) 4 s; (b) 48 problems at full size
4 s - with numpy's matrix products spread over the cores."""
import functools

import numpy as np
import pytest

import alignfuzz as fz
import hashgen
import ratealigngen as gen
import ratefuzz as rf
import ratestretchgen as sg
import seedrategen as sgen

TWIN_SEEDS = 16    # per profile, reduced size, every form against its twin: the GPU file's default seeds
GPU_SEEDS = 16     # per profile: the default of tests/test_gpu_zz_align_fuzz_rates.py
CAP = 1 << 21      # above every record count of these problems


def _vdf():
    import vid_dup_finder_lib_amd as vdf

    return vdf


def _same(entry, fp, got, want, fields):
    got_t, found = got
    want_t = rf.table(want, fields)
    diff = rf.first_difference(got_t, want_t, fields)
    q = fp.params
    assert not diff and found == len(want_t), f"{q['profile']} seed {q['seed']} (reduced) {entry}: found {found}, twin {len(want_t)}; {diff}"


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(TWIN_SEEDS))
@pytest.mark.parametrize("profile", rf.PROFILES)
def test_host_forms_equal_their_twins(profile, seed):
    vdf = _vdf()
    fp = rf.problem(seed, profile, reduced=True)
    p = fp.p
    assert len(p.rates) <= 3
    host = {c.entry: rf.host_form(vdf, c, CAP) for c in rf.calls(fp)}
    seed_list = rf.as_list(host["align_seed_pairs_rates"][0])
    host.update({c.entry: rf.host_form(vdf, c, CAP) for c in rf.list_calls(fp, seed_list)})

    # one walk of every triple, self-named ones included; exclude_same and the lists are filters on it
    everything = p._replace(exclude_same=False)
    named = lambda r: not (p.exclude_same and r[0] == r[1])
    align_all = gen.twin(everything)
    align = [r for r in align_all if named(r)]
    stretches_all = sg.twin(everything, fp.max_stretches, fp.guard)
    stretches = [r for r in stretches_all if named(r)]
    _same("align_seed_pairs_rates", fp, host["align_seed_pairs_rates"], sgen.seed_rates_twin(p), rf.TRIPLE_FIELDS)
    for mode in ("", "[seed=1]"):
        _same("align_windows_rates" + mode, fp, host["align_windows_rates" + mode], align, rf.RATE_FIELDS)
        _same("align_windows_rates_stretches" + mode, fp, host["align_windows_rates_stretches" + mode], stretches, rf.RATE_STRETCH_FIELDS)
    for which, triples in (("seeds", seed_list), ("sublist", fp.triples)):
        listed = set(map(tuple, triples.tolist()))
        pick = lambda r: (r[2], r[0], r[1]) in listed
        _same(f"align_windows_rates[{which}]", fp, host[f"align_windows_rates[{which}]"], [r for r in align_all if pick(r)], rf.RATE_FIELDS)
        _same(f"align_windows_rates_stretches[{which}]", fp, host[f"align_windows_rates_stretches[{which}]"], [r for r in stretches_all if pick(r)],
              rf.RATE_STRETCH_FIELDS)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------
def _seed_view(fp, listed) -> dict:
    """the seed kernel's view of a problem, in numpy: per class the gathered rows and the seeds in the plan's order, their hits by brute force.
    -> other_tile (a candidate of a den >= 2 class all of whose hits lie behind the class's tile 0), other_chunk (a candidate of such a class with
    a hit whose seed lies behind its chunk 0), padding_wave (a class whose last tile has a wave of padding only beside live ones), split_chunk (a
    class of two slots whose chunk 0 holds seeds of both and is not the last), and the candidate set itself, which must be `listed`"""
    p = fp.p
    tol = min(p.tol, 1024)
    n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
    out = dict(other_tile=False, other_chunk=False, padding_wave=False, split_chunk=False)
    cand = set()
    for den, slots in rf.classes(p.rates):
        rows, seeds = rf.class_rows(rf.counts_b(p), den), rf.class_seeds(p, slots)
        if not rows:
            continue
        live = len(rows) - fz.SEED_TILE_ROWS * ((len(rows) - 1) // fz.SEED_TILE_ROWS)   # rows of the last tile
        out["padding_wave"] |= live <= fz.SEED_TILE_ROWS - rf.SEED_WAVE_ROWS
        if len(slots) >= 2 and len(seeds) > fz.SEED_CHUNK:
            out["split_chunk"] |= len({s[0] for s in seeds[:fz.SEED_CHUNK]}) >= 2
        if not seeds:
            continue
        s_slot, s_a, _ = (np.array(x) for x in zip(*seeds))
        r_b = np.array([b for b, _ in rows])
        s_row = np.array([rf._row_a(p, slot, a, ka) for slot, a, ka in seeds])
        r_row = np.array([int(p.b_first[b]) + kb for b, kb in rows])
        hit = hashgen.all_distances(p.a_hashes[s_row], p.b_hashes[r_row]) <= tol
        if p.a_skip is not None:
            hit &= (np.asarray(p.a_skip)[s_row] == 0)[:, None]
        if p.b_skip is not None:
            hit &= (np.asarray(p.b_skip)[r_row] == 0)[None, :]
        if p.exclude_same:
            hit &= s_a[:, None] != r_b[None, :]
        si, ri = np.nonzero(hit)
        if not len(si):
            continue
        key = (s_slot[si] * n_a + s_a[si]) * n_b + r_b[ri]
        uniq, inv = np.unique(key, return_inverse=True)
        cand |= {(int(k) // (n_a * n_b), int(k) // n_b % n_a, int(k) % n_b) for k in uniq}
        if den >= 2:
            first_row = np.full(len(uniq), len(rows))
            np.minimum.at(first_row, inv, ri)
            out["other_tile"] |= bool((first_row >= fz.SEED_TILE_ROWS).any())
            out["other_chunk"] |= bool((si >= fz.SEED_CHUNK).any())
    assert cand == listed, (fp.params["profile"], fp.params["seed"], sorted(cand ^ listed)[:5])
    return out


def _record_facts(fp, align) -> dict:
    """of the records of align_windows_rates (RATE_FIELDS): is one outside band 0 of its phase, across a 64-column reload, in a phase > 0"""
    p = fp.p
    out = dict(other_band=False, reload=False, later_phase=False)
    for a, b, r, first_a, first_b, n, _, _ in align.tolist():
        num, den = rf.lowest(p.rates[r])
        phase, i0, j0 = first_a % num, first_a // num, first_b // den
        rows = rf.sub_rows(rf.counts_a(p, r)[a], num, phase)
        out["other_band"] |= (j0 - i0 + rows - 1) // fz.ALIGN_BAND != 0
        out["reload"] |= j0 // fz.ALIGN_BAND != (j0 + n - 1) // fz.ALIGN_BAND
        out["later_phase"] |= phase > 0
    return out


@functools.lru_cache(maxsize=None)
def _coverage():
    vdf = _vdf()
    out = []
    for profile in rf.PROFILES:
        for seed in range(GPU_SEEDS):
            fp = rf.problem(seed, profile)
            p = fp.p
            c = {x.entry: x for x in rf.calls(fp)}
            seeds, n_seeds = rf.host_form(vdf, c["align_seed_pairs_rates"], CAP)
            align, found = rf.host_form(vdf, c["align_windows_rates"], CAP)
            stretches, n_st = rf.host_form(vdf, c["align_windows_rates_stretches"], CAP)
            assert n_seeds == len(seeds) and found == len(align) and n_st == len(stretches), "CAP is too small"
            n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
            q = dict(profile=profile, seed=seed, has_record=found > 0, rank2=bool((stretches[:, 8] >= 2).any()), tol=p.tol,
                     check_words=fz.check_words(min(p.tol, 1024)), rates=p.rates, max_stretches=fp.max_stretches, content=fp.params["content"],
                     exclude_same=p.exclude_same, dup_equal=fp.params["dup_equal"], n_rates=len(p.rates))
            if p.exclude_same:   # what exclude_same drops: candidates that name one video twice
                every, _ = rf.host_form(vdf, c["align_seed_pairs_rates"]._replace(kw=rf.rate_args(p, exclude_same=False)), CAP)
                q["self_named"] = int((every[:, 0] == every[:, 1]).sum())
                assert not (seeds[:, 0] == seeds[:, 1]).any() and len(every) == len(seeds) + q["self_named"]
            if profile == "bands":
                q["bands"] = max(rf.n_bands(rf.sub_rows(max(rf.counts_a(p, r)), rf.lowest(rate)[0]), rf.sub_cols(max(rf.counts_b(p)), rf.lowest(rate)[1]))
                                 for r, rate in enumerate(p.rates) if rf.lowest(rate)[0] >= 2)
                q.update(_record_facts(fp, align))
            if profile == "tiles":
                q.update(_seed_view(fp, set(map(tuple, rf.as_list(seeds).tolist()))))
            if profile == "many_tiny":
                live = [(rf.counts_a(p, r) > 0)[:, None] & (rf.counts_b(p) > 0)[None, :] for r in range(len(p.rates))]   # the triples with a unit
                q.update(units=sum(int(x.sum()) - (int(np.diagonal(x).sum()) if p.exclude_same else 0) for x in live), words=-(-len(p.rates) * n_a * n_b // 32),
                         off_word=(n_a * n_b) % 32 != 0, round1=int((stretches[:, 8] == 1).sum()))
            out.append(q)
    return out


def _share(rows, key):
    return sum(bool(r.get(key)) for r in rows), len(rows)


def test_the_generator_is_not_vacuous():
    rows = _coverage()
    by = {name: [r for r in rows if r["profile"] == name] for name in rf.PROFILES}
    bands, tiles, tiny = by["bands"], by["tiles"], by["many_tiny"]
    for r in tiny:
        r["round1_256"] = r["round1"] > fz.REDUCE_BLOCK
    drawn = {rate: sum(rate in r["rates"] for r in rows) for rate in rf.RATE_POOL}
    report = {"problems": len(rows), "with an align record": _share(rows, "has_record"), "a stretch of rank >= 2": _share(rows, "rank2"),
              "bands: bands of the longest phase (num >= 2)": sorted(r["bands"] for r in bands),
              "bands: a record outside band 0 of its phase": _share(bands, "other_band"), "bands: a run across a 64-column reload": _share(bands, "reload"),
              "bands: a record in a phase > 0": _share(bands, "later_phase"), "bands: rates per problem": sorted(r["n_rates"] for r in bands),
              "tiles: a candidate hit only behind tile 0 (den >= 2)": _share(tiles, "other_tile"), "tiles: a candidate's seed behind chunk 0 (den >= 2)": _share(tiles, "other_chunk"),
              "tiles: a class with a padding-only wave": _share(tiles, "padding_wave"), "tiles: chunk 0 of a two-slot class spans the slots": _share(tiles, "split_chunk"),
              "many_tiny: triples with a unit (min, max)": (min(r["units"] for r in tiny), max(r["units"] for r in tiny)),
              "many_tiny: bitmap words (min, max)": (min(r["words"] for r in tiny), max(r["words"] for r in tiny)),
              "many_tiny: more than 256 rank-1 records": _share(tiny, "round1_256"), "many_tiny: rank-1 records": sorted(r["round1"] for r in tiny),
              "check words": {w: sum(r["check_words"] == w for r in rows) for w in fz.CHECK_WORDS},
              "tolerances on the edges": {t: sum(r["tol"] == t for r in rows) for t in rf.EDGE_TOLERANCES},
              "rates": {f"{n}/{d}": k for (n, d), k in drawn.items()},
              "max_stretches": {m: sum(r["max_stretches"] == m for r in rows) for m in fz.MAX_STRETCHES},
              "content": {c: sum(r["content"] == c for r in rows) for c in fz.CONTENTS},
              "exclude_same": (sum(r["exclude_same"] for r in rows), "with self-named candidates", sum(r.get("self_named", 0) > 0 for r in rows)),
              "3/2 and 6/4 on equal blocks": _share(rows, "dup_equal")}
    for k, v in report.items():
        print(f"{k}: {v}")
    assert len(rows) == len(rf.PROFILES) * GPU_SEEDS, "no problem is skipped"
    # every problem of the profile
    assert all(r["bands"] >= 3 and r["n_rates"] >= 4 for r in bands), [r["seed"] for r in bands if r["bands"] < 3]
    for key in ("other_tile", "other_chunk", "padding_wave", "split_chunk"):
        assert all(r[key] for r in tiles), (key, [r["seed"] for r in tiles if not r[key]])
    assert all(r["units"] > fz.REDUCE_BLOCK and r["words"] > fz.REDUCE_BLOCK and r["off_word"] for r in tiny)
    # shares of the problems
    ok = lambda key, rs, share: _share(rs, key)[0] >= share * len(rs)
    assert ok("has_record", rows, 0.9), "at least 90 % of the problems have a record"
    assert ok("other_band", bands, 1 / 3), "a third of the bands problems have a record outside band 0 of its phase"
    assert ok("reload", bands, 1 / 3), "a third of the bands problems have a record whose run crosses a 64-row reload of the sub-matrix"
    assert ok("later_phase", bands, 1 / 3), "a third of the bands problems have a record in a phase > 0"
    assert ok("round1_256", tiny, 0.25), "a quarter of the many_tiny problems have more than 256 triples with a record in round 1"
    assert ok("rank2", rows, 0.25), "a quarter of the problems produce a stretch of rank >= 2"
    # the whole seed range
    assert all(report["check words"].values()) and all(report["tolerances on the edges"].values()) and all(report["max_stretches"].values())
    assert all(drawn.values()), drawn
    assert any(r.get("self_named", 0) > 0 for r in rows), "self-named triples under exclude_same are present"
