"""ROUTE_CASES and CROP_CASES of tests/test_gpu_hash_saturating.py against the hash planner (csrc/resize_dispatch.cpp: plan_hash, plan_cropped),
on the CPU: every row lands on the route and instantiation it names, and together the rows reach every kernel.  tests/cpp/hash_route_main.cpp, compiled with g++
from resize_dispatch.cpp and resize_tables.cpp alone (no HIP, no GPU), is the planner's front end."""
import os
import subprocess

from test_gpu_hash_saturating import CROP_CASES, ROUTE_CASES, _boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _knobs(env):
    """The HashKnobs fields a context reads from these variables (csrc/api.cpp)."""
    known = {"VDF_RESIZE_MODE", "VDF_WAVESTREAM_NW", "VDF_NO_WAVESTREAM", "VDF_HASH_NO_PERSISTENT"}
    assert set(env) <= known, set(env) - known
    knob = -1 if "VDF_NO_WAVESTREAM" in env else int(env.get("VDF_WAVESTREAM_NW", 0))
    return int(env.get("VDF_RESIZE_MODE", 0)), knob, int(int(env.get("VDF_HASH_NO_PERSISTENT", "0")) != 0)


def _build():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "hash_route")
    src = [os.path.join(ROOT, "tests", "cpp", "hash_route_main.cpp"),
           os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc", "resize_dispatch.cpp"),
           os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc", "resize_tables.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror=switch", "-o", exe] + src)
    return exe


def test_crop_cases_reach_the_cropped_kernels_they_name():
    """CROP_CASES through plan_cropped: top / bottom bars = all clips on the ROWCROP launch of the width's per-wave kernel; a shared side-bar
    range = one per-wave box launch with all clips; unique ranges = all clips on the gather kernel (with the operand shift: boxes start off a
    dword); the same under VDF_RESIZE_MODE=4 = all clips on the whole-line cropped kernel; 96 x 128 = the small-frame kernel by default."""
    exe = _build()
    lines = ""
    for h, w, kind, mode in CROP_CASES:
        crops = _boxes(kind, h, w, 8)
        lines += "%d %d %d %d %s\n" % (w, h, mode, len(crops), " ".join(str(int(x)) for x in crops.reshape(-1)))
    out = subprocess.run([exe, "crop"], input=lines, capture_output=True, text=True, timeout=60)
    rows = out.stdout.splitlines()
    assert out.returncode == 0 and len(rows) == len(CROP_CASES), out.stdout[-2000:] + out.stderr[-2000:]
    for (h, w, kind, mode), row in zip(CROP_CASES, rows):
        print(f"{h:4d} x {w:4d} {kind:7s} mode {mode}  {row}")
        p = {k: (v if k in ("kind", "rows_route") else int(v)) for k, v in (f.split("=") for f in row.split())}
        assert (p["w"], p["h"]) == (w, h)
        if kind == "mixed":
            if mode == 0:
                assert p["kind"] == "kSmall", row
            else:
                assert p["kind"] == "kParts" and p["rest"] == 8 and not p["rest_gather"], row
            continue
        assert p["kind"] == "kParts", row
        if mode == 4:
            assert p["rows"] == 0 and p["groups"] == 0 and p["rest"] == 8 and not p["rest_gather"], row
        elif kind == "rows":
            assert p["rows_route"] == "kWaveStream" and p["rows_waves"] == 8 and p["rows"] == 8 and p["groups"] == 0 and p["rest"] == 0, row
        elif kind == "shared":
            assert p["groups"] == 1 and p["group_clips"] == 8 and p["group_waves"] == 8 and p["rows"] == 0 and p["rest"] == 0, row
        else:
            assert p["rest"] == 8 and p["rest_gather"] and p["gather_shift"] and p["rows"] == 0 and p["groups"] == 0, row


def test_route_cases_reach_every_hash_kernel():
    exe = _build()
    lines = "".join("%d %d %d %d %d\n" % ((w, h) + _knobs(env)) for _, h, w, _, env, _, _ in ROUTE_CASES)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = out.stdout.splitlines()
    all_routes, all_tiled = rows[0].split(), rows[1].split()
    assert all_routes[0] == "routes" and all_tiled[0] == "tiled" and len(rows) == 2 + len(ROUTE_CASES)
    plans = []
    for case, row in zip(ROUTE_CASES, rows[2:]):
        name, h, w, n_clips, env, route, detail = case
        plan = dict(f.split("=") for f in row.split())
        print(f"{name:32s} {h:4d} x {w:4d}  {n_clips:3d} clips  {row}")
        assert (int(plan["w"]), int(plan["h"])) == (w, h)
        # every row lands on the route it names, with the values it names
        assert plan["route"] == route, (name, row)
        for key, val in detail.items():
            assert int(plan[key]) == val, (name, key, row)
        # the persistent loops wrap: more clips than a launch has workgroups to give each one clip
        assert n_clips % 4 == 0 and n_clips >= (300 if route in ("kPersistentOneTile", "kTiled") else 8), name
        plans.append(plan)

    def hit(route, **kv):
        return any(p["route"] == route and all(int(p[k]) == v for k, v in kv.items()) for p in plans)

    # every HashRoute but kRefused (no kernel) and kDirect16 (no resize)
    for route in all_routes[1:]:
        assert route in ("kRefused", "kDirect16") or hit(route), f"no row takes {route}"
    # every instantiation: wave counts, <NKT, NRG> of the tiled kernel, <FULL> or not, the chunk form with shifted re-pitched rows, the
    # K-split form where the default dispatch picks it and where only the knob does
    for nw in (8, 6, 5, 4, 3):
        assert hit("kWaveStream", waves=nw), f"no row takes the per-wave form with {nw} waves"
    assert len(all_tiled) == 1 + 11
    for pair in all_tiled[1:]:
        nkt, nrg = (int(x) for x in pair.split(","))
        assert hit("kTiled", n_kt=nkt, tiled_nrg=nrg), f"no row takes resize_dct_hash_tiled_kernel<{nkt}, {nrg}>"
    assert hit("kPersistentOneTile", full_tile=1) and hit("kPersistentOneTile", full_tile=0)
    assert hit("kTiled", last_clip_apart=1) and hit("kTiled", last_clip_apart=0)
    assert any(p["route"] == "kChunkStream" and int(p["shift"]) == 1 and int(p["pitch"]) != int(p["w"]) for p in plans)
    assert any(p["route"] == "kChunkStream" and int(p["shift"]) == 0 and int(p["pitch"]) == int(p["w"]) for p in plans)
    ksplit_modes = {_knobs(c[4])[0] for c, p in zip(ROUTE_CASES, plans) if p["route"] == "kKsplit"}
    assert ksplit_modes == {0, 6}, ksplit_modes
    whole_line_modes = {_knobs(c[4])[0] for c, p in zip(ROUTE_CASES, plans) if p["route"] == "kWholeLine"}
    assert whole_line_modes == {0, 4}, whole_line_modes
