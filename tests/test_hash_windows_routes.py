"""Which resize kernel the windows calls give their pseudo-clip runs (csrc/resize_dispatch.cpp: plan_resize_only over csrc/windows_plan.h: windows_resize_runs),
on the CPU, for the rows and layouts of tests/test_gpu_hash_windows.py: tests/cpp/windows_route_main.cpp is the planner's front end (g++ alone, no HIP, no GPU).
The GPU test compares words, and every unfused route gives the same words - so that a row reaches the route it is named for is pinned here:
  - packed: the five unfused rows reach their own route on every run, the tail pseudo-clips included;
  - the three sizes the plain call hashes with the DCT fused in arrive at the whole-line kernel, in both layouts;
  - at an odd base address with padded strides the stream forms do not apply: whole-line (the scalar kernel where VDF_RESIZE_MODE=1 forces it);
  - no run is ever planned onto a kernel that fuses the DCT (the front end refuses)."""
import os
import subprocess

from test_gpu_hash_planes import ROWS
from test_hash_route_table import _knobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = ("kPersistentOneTile", "kTiled", "kPerClipFused")
CALLS = [(33, 1), (35, 2)]  # (F, clips) of the GPU test's two calls per row: 2 chunks + tail, one clip; 2 chunks + tail, two clips
LAYOUTS = {"packed": (0, 0, 0), "odd_base_padded": (1, 3, 5)}


def test_every_row_reaches_the_resize_route_it_is_named_for():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_route")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror=switch", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_route_main.cpp"),
                           os.path.join(csrc, "resize_dispatch.cpp"), os.path.join(csrc, "resize_tables.cpp")])
    cases = [(row, layout, call) for row in ROWS if row[0] != "kDirect16" for layout in LAYOUTS for call in CALLS]  # (16 x 16 is read in place: no resize stage)
    lines = ""
    for (route, h, w, env, _), layout, (nf, n) in cases:
        lines += "%d %d %d %d %d %d %d %d %d %d\n" % ((w, h) + _knobs(env) + LAYOUTS[layout] + (nf, n))
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=60)
    rows = out.stdout.splitlines()
    assert out.returncode == 0 and len(rows) == len(cases), out.stdout[-2000:] + out.stderr[-2000:]
    for ((route, h, w, env, _), layout, (nf, n)), row in zip(cases, rows):
        print(f"{route:20s} {h:4d} x {w:4d} {layout:16s} F={nf} clips={n}  {row}")
        p = dict(f.split("=") for f in row.split())
        got = p["routes"].split(",")
        assert len(got) == int(p["runs"]) == n + 1 and p["layout"] == "kByClip"  # one run per clip over its two chunks, one for the tails
        if route == "kScalar":
            want = "kScalar"
        elif route in FUSED or layout == "odd_base_padded":
            want = "kWholeLine"
        else:
            want = route
        assert got == [want] * len(got), (route, layout, row)
