"""Two ranks driving the REAL engine (both on GPU 0, collectives over gloo - RCCL refuses two ranks on one device):
  * `python bench.py --gpus 2` started plainly launches its own ranks, prints one JSON line, and finds the same
    MatchGroups as the 1-rank run over the same database;
  * search_self_sharded through the hit-buffer overflow protocol (consumption bitmap broadcast from rank 0, uploaded
    and consumed on torch's current stream) and search_refs_sharded, against the oracle."""
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bench(extra, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--full", "--hash-clips", "2000",
                          "--hash-hd-clips", "0", "--c4-hashes", "60000", "--c5-cands", "3000", "--c5-refs", "300", "--dup-heavy", "0", "--cache-entries", "0",
                          "--no-cpu-baseline", "--no-windowed", "--no-valu", "--no-refs"] + extra,
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_launches_its_own_ranks():
    n1 = 30000
    n2 = int(round(n1 * 2 ** 0.5))
    two = _bench(["--gpus", "2", "--n-hashes", str(n1)], {"VDF_DIST_BACKEND": "gloo"})
    one = _bench(["--gpus", "1", "--n-hashes", str(n2)])
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["config"]["n_hashes"] == n2 == one["config"]["n_hashes"]
    assert abs(two["config"]["hashes_per_gpu_shard"] * 2 - n2) <= 1
    assert two["match_groups"] == one["match_groups"] > 0
    assert two["config"]["pairs"] == one["config"]["pairs"] == n2 * (n2 - 1) // 2
    assert two["hash"]["n_gpus"] == 2 and two["value"] > 0 and two["summary"]["hash_summary"]["n_gpus"] == 2
    assert two["rccl_ranks_seen"] == 0 and two["dist_backend"] == "gloo"  # (two ranks on one GPU cannot use RCCL: this run says so)
    keys = list(two)
    assert keys.index("c4_10m_sharded") == min(keys.index(k) for k in keys if isinstance(two[k], dict) and k not in ("config", "roofline", "hbm_operand_stream_model"))
    # the named legs: BASELINE configs[3] sharded over the ranks (strong scaling) and configs[4] end to end
    for d in (one, two):
        c4 = d["c4_10m_sharded"]
        assert c4["n_hashes"] == 60000 and c4["pairs"] == 60000 * 59999 // 2 and c4["scaling"] == "strong"
        assert c4["n_gpus"] == d["n_gpus"] and c4["ms_per_step"] > 0 and c4["match_groups"] >= c4["planted_pairs"] - 1
        c5 = d["c5_end_to_end"]
        assert c5["n_candidates"] == 3000 and c5["n_references"] == 300 and c5["groups"] == c5["planted_references"] > 0
        assert c5["members"] == c5["groups"]  # every planted reference finds exactly its source
        assert set(c5["phases_ms"]) == {"hash_ms", "all_gather_ms", "sort_ms", "search_ms", "group_ms"} and c5["ms_per_step"] > 0
    assert "ten_million" in one and "ten_million" not in two
    # after the ranks, the C ABI's single-process form ran in a fresh child and is carried in the same line
    sp = two["single_process"]
    assert sp["rccl"] == "ok", sp
    assert sp["match_groups"] == two["match_groups"] and len(sp["per_device_kernel_ms"]) == 2 and sp["value"] > 0
    assert sp["devices"] == [0, 0] and "device-to-device" in sp["replication"]  # one GPU here: the device list wraps
    assert sp["c4_10m_sharded"]["n_hashes"] == 60000 and "single_process" not in one


def test_bench_with_eight_ranks_on_one_gpu():
    """`bench.py --gpus 8` before the driver's 8-GPU node runs it: eight children spawned before any GPU call, collectives over gloo (eight
    ranks share GPU 0; RCCL refuses that), every leg at a reduced size, and the single-process C-ABI form in a fresh child afterwards -
    the 8-way deal of row tiles, the 8-way hit gather / merge and the exchange of the replay filter are the code of the real run."""
    import time

    t0 = time.perf_counter()
    n1 = 70000
    n8 = int(round(n1 * 8 ** 0.5))
    d = _bench(["--gpus", "8", "--n-hashes", str(n1)], {"VDF_DIST_BACKEND": "gloo"})
    wall = time.perf_counter() - t0
    assert wall < 180, wall
    assert d["n_gpus"] == 8 and d["config"]["n_hashes"] == n8 and d["value"] > 0 and d["match_groups"] > 0
    assert d["rccl_ranks_seen"] == 0 and d["dist_backend"] == "gloo"
    assert abs(d["config"]["hashes_per_gpu_shard"] * 8 - n8) <= 8
    c4 = d["c4_10m_sharded"]
    assert c4["n_gpus"] == 8 and c4["n_hashes"] == 60000 and c4["scaling"] == "strong" and c4["match_groups"] >= c4["planted_pairs"] - 1
    assert "speedup_vs_n1_model" not in c4 or c4["speedup_vs_n1_model"] > 0  # (only quoted at the 10 M size)
    c5 = d["c5_end_to_end"]
    assert c5["n_gpus"] == 8 and c5["groups"] == c5["planted_references"] > 0 and c5["members"] == c5["groups"]
    assert d["hash"]["n_gpus"] == 8 and d["summary"]["hash_summary"]["n_gpus"] == 8 and d["summary"]["ten_million"]["n_gpus"] == 8
    sp = d["single_process"]  # the same library through ONE eight-slot context, in a fresh child
    assert sp["rccl"] == "ok" and sp["devices"] == [0] * 8 and len(sp["per_device_kernel_ms"]) == 8
    assert sp["match_groups"] == d["match_groups"] and sp["c4_10m_sharded"]["n_hashes"] == 60000
    one = _bench(["--gpus", "1", "--n-hashes", str(n8)])
    assert one["match_groups"] == d["match_groups"] and one["config"]["pairs"] == d["config"]["pairs"]


def _worker(rank, world, port, capacity, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    import hashgen as hg
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import distributed as vd

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = vdf.Engine(0)
    rng = np.random.default_rng(4242)
    words, dur = hg.planted_set(rng, 3000, n_clusters=40, max_copies=30, max_flips=150, durations="windowed")
    words[1000:1400] = words[1000]  # 400 identical hashes with equal durations: ~80 000 hits from one region
    dur[1000:1400] = dur[1000]
    w, d, _ = hg.sort_by_duration(words, dur)
    lo, hi = vd.split_range(len(d), rank, world)
    side = torch.cuda.Stream(device=dev)  # a non-default current stream: the library must order itself behind it
    with torch.cuda.stream(side):
        fw, fd = vd.all_gather_database(torch.from_numpy(w[lo:hi].view(np.int64)).to(dev),
                                        torch.from_numpy(d[lo:hi].view(np.int32)).to(dev))
        st = {}
        groups = vd.search_self_sharded(eng, fw, fd, 350, capacity=capacity, stats=st)
        calls_stream = eng.last_stats()["n_launches"]
    np.save(os.path.join(out_dir, f"filter_{rank}.npy"), np.array([st["filtered_launches"], st["hits_downloaded"], eng.last_timing()["hits_filtered"]]))
    # and once on torch's legacy default stream (handle 0)
    groups0 = vd.search_self_sharded(eng, fw, fd, 350, capacity=capacity)
    pick = np.random.default_rng(5).choice(len(d), size=301, replace=False)
    rw, rd = w[pick].copy(), d[pick].copy()
    a, b = vd.split_range(len(rd), rank, world)
    refs = vd.search_refs_sharded(eng, fw, fd, torch.from_numpy(rw[a:b].view(np.int64)).to(dev),
                                  torch.from_numpy(rd[a:b].view(np.int32)).to(dev), a, 300, capacity=capacity)
    if rank == 0:
        with open(os.path.join(out_dir, "res.pkl"), "wb") as f:
            pickle.dump({"groups": groups, "groups0": groups0, "refs": refs, "w": w, "d": d, "rw": rw, "rd": rd}, f)
    else:
        assert groups is None and refs is None
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


@pytest.mark.parametrize("capacity", [1 << 20, 500])
def test_two_ranks_real_engine_match_oracle(tmp_path, capacity):
    import torch.multiprocessing as mp

    from oracle import vdf_oracle as orc

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, capacity, str(tmp_path)), nprocs=2, join=True)
    res = pickle.load(open(tmp_path / "res.pkl", "rb"))
    want = orc.search_self_sorted(res["w"], res["d"], 350)
    assert res["groups"] == want and res["groups0"] == want
    # the 400 identical hashes alone are 79 800 thresholded pairs: with room for them the two ranks agree (gloo all-gather behind
    # vdf_shard_exchange's callbacks) to drop the rows that cannot become targets, and OR their bitmaps twice; with the small
    # buffer somebody overflows, nobody filters and the overflow protocol runs
    f = [np.load(tmp_path / f"filter_{r}.npy") for r in range(2)]
    if capacity > 100_000:
        assert all(x[0] == 1 and x[2] > 0 for x in f) and sum(int(x[1]) for x in f) < 3000
    else:
        assert all(x[0] == 0 for x in f)
    assert res["refs"] == orc.search_refs_sorted(res["w"], res["d"], res["rw"], res["rd"], 300)


def test_bench_single_process_multi_context():
    """`bench.py --gpus 2 --single-process`: the C ABI's multi-GPU context (device list wraps onto GPU 0 here) finds the
    same MatchGroups over the same database as the 1-GPU run; the two slots split the triangle evenly."""
    n1 = 30000
    n2 = int(round(n1 * 2 ** 0.5))
    two = _bench(["--gpus", "2", "--single-process", "--n-hashes", str(n1)])
    one = _bench(["--gpus", "1", "--n-hashes", str(n2)])
    assert two["n_gpus"] == 2 and "vdf_ctx_create_multi" in two["config"]["parallelism"]
    assert two["config"]["n_hashes"] == n2 and two["match_groups"] == one["match_groups"] > 0
    p = two["per_device_pairs"]
    assert sum(p) == two["config"]["pairs"] and abs(p[0] - p[1]) / sum(p) < 0.05
    assert two["hash"]["n_gpus"] == 2 and two["value"] > 0 and two["roofline"]["frac"] > 0
