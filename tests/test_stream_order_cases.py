"""The cases of tests/test_gpu_stream_order.py, on the CPU: that test can only fail where the expected result on `real` differs from the
one on `decoy` (the call ran ahead of its stream) and from the one on `decoy2` (it left work behind).  Here the references alone decide: every
case, every output, no exemptions.  And every _device call of include/vdf.h that takes a stream has a case: a new one without fails here."""
import os
import re

import numpy as np
import pytest

import streamcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream_calls():
    """every function of include/vdf.h with a `void *stream` parameter (the header parsed as tests/test_capi_symbols.py parses it)"""
    text = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf.h")).read(), flags=re.S))
    protos = re.findall(r"^[A-Za-z_][\w\s\*]*?\b(vdf_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.M | re.S)
    return sorted(name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args))


def test_every_device_call_with_a_stream_has_a_case():
    calls = _stream_calls()
    assert len(calls) >= 36 and all("_device" in c for c in calls), calls
    covered = {s for n in sc.names() for s in sc.symbols_of(n)}
    assert sorted(covered) == calls, {"without a case": sorted(set(calls) - covered), "not in the header": sorted(covered - set(calls))}
    # the hash family, one case per kernel route, and each of them also as the first call of its frame size on a fresh context
    routes = [n for n in sc.names() if sc.symbols_of(n) == ("vdf_hash_frames_u8_device",)]
    assert len(routes) == 6 and all(sc.is_cold(n) for n in routes)
    assert all(sc.is_cold(n) for n in sc.names() if any(s.startswith(("vdf_hash_frames", "vdf_hash_clips", "vdf_hash_windows", "vdf_cropdetect")) for s in sc.symbols_of(n)))


@pytest.mark.parametrize("name", sc.names())
def test_the_decoys_are_valid_and_give_other_results(name):
    c = sc.case(name)
    for s in c.sets:
        c.valid(s)
    for key in c.sets[0]:  # other frames, hashes, first arrays, skip bytes, planes, descriptors and lists: nothing is shared between the sets
        assert not any(np.array_equal(c.sets[i][key], c.sets[j][key]) for i, j in ((0, 1), (0, 2), (1, 2))), key
    real = sc.expected(name, 0)
    assert c.outputs or "host" in real
    for k in (1, 2):
        other = sc.expected(name, k)
        assert real.keys() == other.keys()
        for key in real:
            assert not sc.same(real[key], other[key]), f"{name}: the expected {key} on set {k} is the one on real - the case proves nothing"
    for key, (shape, dtype) in c.outputs.items():  # ... nor is any of them what the fill leaves behind
        assert not np.array_equal(real[key], sc.filled(shape, dtype))
