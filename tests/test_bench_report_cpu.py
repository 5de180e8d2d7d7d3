"""bench.py's reporting code executed on the CPU: a NameError or a key that moved must fail HERE, not 400 tests into a metered GPU call
(round 4 lost one to a leftover name).  Nothing below touches a GPU: the engine's per-step statistics are synthetic tuples."""
import builtins
import json
import os
import symtable
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

# (kernel_ms, n_launches, pairs, pairs_computed, n_hits, pairs_early_exit, early_exit_bits): the 1 M headline's figures
STEP = (106.1, 1, 499_999_500_000, 500_300_000_000, 3778, 500_200_000_000, 832)


def test_no_undefined_names_in_bench():
    """Every name a function of bench.py reads resolves to a local, an enclosing scope, a module-level name or a builtin."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    top = symtable.symtable(src, "bench.py", "exec")
    module_names = {s.get_name() for s in top.get_symbols() if s.is_assigned() or s.is_imported() or s.is_namespace()}
    known = module_names | set(dir(builtins)) | {"__file__", "__name__"}
    missing = []

    def walk(t):
        for s in t.get_symbols():
            if t.get_type() == "module":
                if s.is_referenced() and s.get_name() not in known:
                    missing.append((t.get_name(), s.get_name()))
            elif s.is_referenced() and s.is_global() and s.get_name() not in known:
                missing.append((t.get_name(), s.get_name()))
        for c in t.get_children():
            walk(c)

    walk(top)
    assert not missing, missing


@pytest.mark.parametrize("backend", ["mfma", "valu"])
def test_search_roofline_and_headline_assemble(backend, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "TRAFFIC_PATH", str(tmp_path / "none.json"))
    roofline, extra, dtype = bench.search_roofline(backend, [STEP, STEP])
    assert roofline["kernel"] == ("hamming_mfma2_kernel" if backend == "mfma" else "hamming_tile_kernel")
    assert roofline["traffic"] is None and "missing" in roofline["traffic_source"]
    assert abs(roofline["achieved"] / roofline["peak"] - roofline["frac"]) < 1e-12 and 0 < roofline["frac"]
    if backend == "mfma":
        # 8.1e14 executed FLOP in 106.1 ms of a 10 PF peak: the round-4 fraction
        assert 0.75 < roofline["frac"] < 0.82 and roofline["algorithmic_frac"] > roofline["frac"]
        assert extra["hbm_operand_stream_model"]["x_of_hbm_model"] > 50
    else:
        assert extra["valu"]["frac"] > 0
    out = bench.headline(4.7e12, 20, 5, 106.9, 1, dtype, 1_000_000, 1_000_000, 499_999_500_000, 350, "single GPU", roofline)
    assert list(out)[:13] == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                              "vs_baseline", "dtype", "data", "config"]
    assert out["vs_baseline"] is None and out["config"]["workload"].startswith("BASELINE configs[1]")
    out["cpu_baseline"] = {"value": 3.6e8, "unit": "pairs/s", "cores": 1, "kind": "port", "sample": "x"}
    out["c4_10m_sharded"] = dict(bench.c4_summary(10_000_000, 8, 1400.0), match_groups=100, planted_pairs=100,
                                 roofline={"bound": "mfma", "frac": 0.81, "kernel": "hamming_mfma2_kernel"})
    out["c5_end_to_end"] = {"workload": "x" * 200, "ms_per_step": 13.3, "ms_min": 13.0, "phases_ms": {"hash_ms": 11.2}}
    out["cache_ingest"] = {"entries": 10_000_000, "host_ms": 281.9, "search_cache_entries": {"search_ms": 271.4, "rank_ms": 214.9}}
    out["roofline"]["clock"] = {"sclk_mhz_median": 2150.0, "power_w_median": 1390.5, "samples": 400}
    lb = {"clips": 20000, "w": 64, "h": 64}
    for name, ms in (("no_bars", 0.2301), ("top_bottom_bars", 0.2604), ("side_bars", 0.2712)):
        lb[name] = {"ms_per_step": ms, "ms_min": ms, "frames_per_s_per_gpu": 1.3e9, "crop_of_clip_0": [0, 0, 7, 7], "box_GB_per_s": 5000.0}
    out["hash"] = {"value": 1.5e9, "unit": "frames/s", "clips_per_gpu": 100_000, "n_gpus": 1, "ms_per_step": 1.04,
                   "roofline": {"bound": "hbm", "kernel": "resize_dct_hash_persistent_kernel", "achieved": 6300.0, "peak": 8000.0,
                                "unit": "GB/s", "frac": 0.7875, "traffic": None, "traffic_source": "x",
                                "clock": {"sclk_mhz_median": 2390.0, "power_w_median": 900.1, "samples": 120}},
                   "letterbox_64x64": lb,
                   "host_queue_1080p": {"letterbox": {"clips_per_s": 1600, "link_GB_per_s": 53.1, "wrong": 0, "batch_call_link_GB_per_s": 56.0},
                                        "plain": {"error": "no compiler"}, "w": 1920, "h": 1080, "caller_threads": 32},
                   "full_hd": {"blah": "x" * 3000},
                   "cpu_baseline": {"value": 6e5, "unit": "frames/s", "cores": 256, "kind": "port",
                                    "sample": "oracle from_frames over a 256-thread pool, 24576 clips of 16x64x64 (single thread: 384 clips)"}}
    line = bench.finish_line(out)
    d = json.loads(line)
    # a reader of the line's TAIL gets, in one object of at most 1.5 KB: the second half of the metric, the north_star's 10 M leg and one
    # figure per widened leg (the driver keeps 2 - 8 KB of a line that is 11 KB: VERDICT r05 weak 6)
    assert list(d)[-1] == "summary" and "hash_summary" not in d
    sm = d["summary"]
    assert len(json.dumps(sm)) <= bench.SUMMARY_MAX_BYTES == 1536 and line.endswith(json.dumps(sm) + "}")
    assert set(sm) == {"hash_summary", "ten_million", "c5_end_to_end", "cache_ingest", "letterbox_64x64_ms", "host_queue_1080p_link_GB_per_s", "clock"}
    assert sm["host_queue_1080p_link_GB_per_s"] == {"letterbox": 53.1, "plain": "no compiler"}  # SURVEY 8f N2 through compiled callers (a child process)
    hs = sm["hash_summary"]
    assert hs["value"] == 1.5e9 and hs["roofline"]["frac"] == 0.7875 and hs["cpu_baseline"]["cores"] == 256 and hs["unit"] == "frames/s"
    assert hs["roofline"]["clock"]["sclk_mhz_median"] == 2390.0 and sm["clock"]["power_w_median"] == 1390.5
    assert sm["ten_million"] == {"n_hashes": 10_000_000, "n_gpus": 8, "ms": 1400.0, "pairs_per_s": d["c4_10m_sharded"]["pairs_per_s"],
                                 "roofline_frac": 0.81, "planted_found": 100, "planted": 100}
    assert sm["c5_end_to_end"] == {"ms_per_step": 13.3, "ms_min": 13.0} and sm["cache_ingest"] == {"entries": 10_000_000, "host_ms": 281.9, "search_ms": 271.4}
    assert sm["letterbox_64x64_ms"] == {"no_bars": 0.2301, "top_bottom_bars": 0.2604, "side_bars": 0.2712}
    c4 = d["c4_10m_sharded"]
    assert c4["scaling"] == "strong" and abs(c4["speedup_vs_n1_model"] - bench.C4_N1_REFERENCE_MS / 8 / 1400.0) < 1e-12
    # legs that did not run leave no key behind, and the summary of a headline-only line is still valid JSON at the tail
    bare = json.loads(bench.finish_line({"metric": "m", "roofline": {"frac": 0.8}}))
    assert list(bare)[-1] == "summary" and bare["summary"] == {}


def test_clock_sampler_reads_what_sysfs_offers(tmp_path, monkeypatch):
    """ClockSampler on a fake /sys tree: the '*' level of pp_dpm_sclk, hwmon's power in microwatts; and nothing at all without a card."""
    import glob as _glob

    card = tmp_path / "card1" / "device"
    (card / "hwmon" / "hwmon3").mkdir(parents=True)
    (card / "pp_dpm_sclk").write_text("0: 132Mhz\n1: 2150Mhz *\n2: 2400Mhz\n")
    (card / "hwmon" / "hwmon3" / "power1_average").write_text("1391000000\n")
    real_glob = _glob.glob
    monkeypatch.setattr(_glob, "glob", lambda pat: real_glob(pat.replace("/sys/class/drm", str(tmp_path))))
    real_exists = os.path.exists
    monkeypatch.setattr(os.path, "exists", lambda p: real_exists(p))
    s = bench.ClockSampler(0, period_s=0.001)
    assert s.card and s.card.endswith("card1")
    with s:
        import time

        time.sleep(0.02)
    r = s.result()
    assert r["sclk_mhz_median"] == 2150.0 and r["power_w_median"] == 1391.0 and r["samples"] >= 2
    monkeypatch.setattr(_glob, "glob", lambda pat: [])
    s = bench.ClockSampler(0)
    with s:
        pass
    assert s.result() == {"sclk_mhz_median": None, "power_w_median": None, "samples": 0}


def test_executed_pairs_and_medians():
    st = {"pairs_computed": 1000.0, "pairs_early_exit": 800.0, "early_exit_bits": 832}
    assert abs(bench.executed_pairs(st) - (1000.0 - 800.0 * (1 - 832 / 1024))) < 1e-9
    st["early_exit_bits"] = 0
    assert bench.executed_pairs(st) == 1000.0
    assert bench.med_min([16.3, 13.2, 13.3]) == (13.3, 13.2)  # one slow step moves the mean, not the median


def test_traffic_is_only_reported_for_the_library_it_was_measured_on(tmp_path, monkeypatch):
    lib = tmp_path / "libvdf_hip.so"
    lib.write_bytes(b"not really a library")
    monkeypatch.setattr(bench, "LIB_PATH", str(lib))
    monkeypatch.setattr(bench, "TRAFFIC_PATH", str(tmp_path / "pmc_traffic.json"))
    bench._lib_sha.clear()
    sha = bench.lib_sha256()
    assert sha and len(sha) == 64
    rec = {"lib_sha256": sha, "hamming_mfma2_kernel": {"hbm_bytes_per_launch": 8.2e10}}
    (tmp_path / "pmc_traffic.json").write_text(json.dumps(rec))
    v, src = bench.read_traffic("hamming_mfma2_kernel")
    assert v == 8.2e10 and sha[:12] in src
    assert bench.read_traffic("hamming_mfma2_kernel", 0.5)[0] == 4.1e10
    v, src = bench.read_traffic("no_such_kernel")
    assert v is None and "no entry" in src
    rec["lib_sha256"] = "0" * 64  # a profile of another build
    (tmp_path / "pmc_traffic.json").write_text(json.dumps(rec))
    v, src = bench.read_traffic("hamming_mfma2_kernel")
    assert v is None and "another libvdf_hip.so" in src
    del rec["lib_sha256"]  # a file from before the sha was recorded
    (tmp_path / "pmc_traffic.json").write_text(json.dumps(rec))
    assert bench.read_traffic("hamming_mfma2_kernel")[0] is None
    bench._lib_sha.clear()


def test_committed_traffic_file_names_live_kernels_only():
    """profiles/pmc_traffic.json: keyed to a library sha, no entry for a kernel that no longer exists."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    t = json.load(open(p))
    assert isinstance(t.get("lib_sha256"), str) and len(t["lib_sha256"]) == 64
    src = "".join(open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc", f)).read() for f in ("hamming.hip", "dct_hash.hip"))
    for k in t:
        if k in ("lib_sha256", "profiled_with"):
            continue
        assert k.split("@")[0] + "(" in src or k.split("@")[0] + "<" in src or ("void " + k.split("@")[0]) in src, k


def test_synthetic_cache_generator_round_trips():
    """bench.synth_cache (the cache_ingest leg's input): the app's wire format, decodable, paths plain and distinct."""
    import numpy as np

    from vid_dup_finder_lib_amd import cache as vc

    data, hashes, dur, blob, offs, planted = bench.synth_cache(5000, plant_every=100)
    c = vc.decode_cache(data, 1)
    assert c["n_entries"] == 5000 and c["n_err"] == 0 and c["n_key_differs"] == 0
    assert np.array_equal(c["hashes"], hashes) and np.array_equal(c["durations"], dur) and planted == 50
    assert c["paths"][0].startswith("/srv/media/lib_") and len(set(c["paths"])) == 5000
    assert all(int(np.unpackbits((hashes[i] ^ hashes[i + 1]).view(np.uint8)).sum()) <= 350 for i in range(0, 4900, 100))


def test_dump_outputs_writes_the_groups_as_csr_and_stays_under_its_bound(tmp_path, monkeypatch):
    """--dump-outputs: group g is members[offsets[g]:offsets[g + 1]], float64; past DUMP_MAX_BYTES a fixed every-k-th sample of whole groups."""
    import numpy as np

    groups = [[0, 5], [1, 2, 9], [3, 4], [6, 7, 8, 10]]
    bench.dump_outputs(str(tmp_path / "a"), groups)
    offsets, members = np.load(tmp_path / "a" / "groups_offsets.npy"), np.load(tmp_path / "a" / "groups_members.npy")
    assert offsets.dtype == members.dtype == np.float64
    assert [list(members[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])] == groups
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 8)
    bench.dump_outputs(str(tmp_path / "b"), groups)
    offsets, members = np.load(tmp_path / "b" / "groups_offsets.npy"), np.load(tmp_path / "b" / "groups_members.npy")
    assert 8 * (len(offsets) + len(members)) <= 8 * 8
    assert [list(members[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])] == [[0, 5], [3, 4]]
    bench.dump_outputs(str(tmp_path / "c"), [])
    assert list(np.load(tmp_path / "c" / "groups_offsets.npy")) == [0.0] and len(np.load(tmp_path / "c" / "groups_members.npy")) == 0
