"""vdf_search_variants (include/vdf.h): for every requested variant v, the reference search with V_v = (H ^ M_v) & ~Z as the references and the
plain hashes as the candidates, minus the pairs (r, r) and the references left without a match.
(a) Synthetic (H, Z): tests/hashgen.py hashes with a sparse random zero plane (H &= ~Z), b = variant_v(a) planted with 0 - 40 flipped bits inside and outside a's
    duration window; expected = oracle.search_refs_sorted(H, d, V_v, d, tol), V_v restated here in numpy, with the (r, r) pairs and the emptied groups removed.
    Group order and member order must match.  n = 600 and n = vdf_row_tile_size() + 3 (a second, nearly empty row tile); host-array and device-resident form.
(b) End to end at 64 x 64: 40 clips, 8 of them mirrored copies of others with +-2 grey levels of noise: search() does not group them, search_flipped(.., (Flip.X,))
    at tolerance 0.3 returns exactly those pairs (from both sides), and a static clip - 50 bits from its own mirror - is not reported as its own duplicate."""
import numpy as np
import pytest

import hashgen
import planegen
from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu
_CACHE = {}


def _tile():
    from vid_dup_finder_lib_amd import _capi

    return int(_capi.load().vdf_row_tile_size())


def _variant_np(h, z, v):
    return (h ^ planegen.variant_mask(v)[None, :]) & ~z


def _database(n, variants):
    """(hashes, zero planes, durations) in sorted order with planted mirrors for every variant of `variants`."""
    key = (n, tuple(variants))
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(n * 31 + sum(variants))
    h = hashgen.random_hashes(rng, n)
    zbits = (rng.random((n, 1024)) < 0.02).astype(np.uint8)
    zbits[:, 1000:] = 0
    z = np.packbits(zbits, axis=1, bitorder="little").view(np.uint64).copy()
    h &= ~z
    d = np.sort(rng.integers(100, 600, size=n).astype(np.uint32))
    free = list(rng.permutation(n))
    for v in variants:
        for flips in (0, 1, 17, 40, 40, 33):
            a = free.pop()
            inside = flips != 33
            # b: a neighbour in sorted order with a duration inside a's +-5 % window, or an entry far outside it
            cands = [j for j in free if (abs(int(d[j]) - int(d[a])) * 40 <= int(d[a])) == inside and (inside or abs(int(d[j]) - int(d[a])) > int(d[a]) // 2)]
            b = cands[0]
            free.remove(b)
            hb = hashgen.hash_with_spatial_distance(_variant_np(h[a:a + 1], z[a:a + 1], v)[0], flips, rng)
            hb[15] &= np.uint64((1 << 40) - 1)
            h[b] = hb & ~z[b]
    for a in (h, z, d):
        a.setflags(write=False)
    _CACHE[key] = (h, z, d)
    return _CACHE[key]


def _expected(h, z, d, v, tol):
    res = orc.search_refs_sorted(h, d, _variant_np(h, z, v), d, tol)
    out = []
    for r, ms in res:
        ms = [m for m in ms if m != r]
        if ms:
            out.append((r, ms))
    return out


@pytest.mark.parametrize("variants", [(1,), (1, 2, 3), (7,)], ids=["x", "x_y_xy", "xyt"])
@pytest.mark.parametrize("tol", [350, 60])
@pytest.mark.parametrize("n", [600, "tile"])
def test_synthetic_planes_match_the_reference_search_of_the_variants(engine, n, tol, variants):
    import torch

    n = _tile() + 3 if n == "tile" else n
    h, z, d = _database(n, variants)
    mask = sum(1 << v for v in variants)
    want = {v: _expected(h, z, d, v, tol) for v in variants}
    planted = sum(len(ms) for v in variants for _, ms in want[v])
    print(f"n = {n}, tol = {tol}, variants {variants}: {[len(want[v]) for v in variants]} groups, {planted} members")
    assert all(len(want[v]) >= (4 if tol == 350 else 2) for v in variants), "the planted mirrors must show"
    got = engine.search_variants_sorted(h, z, d, tol, mask)
    assert sorted(got) == sorted(variants)
    for v in variants:
        assert got[v] == want[v], f"host form, variant {v}"
    dh, dz, dd = (torch.from_numpy(a.copy().view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda() for a in (h, z, d))
    torch.cuda.synchronize()
    got_d = engine.search_variants_device(dh.data_ptr(), dz.data_ptr(), dd.data_ptr(), n, tol, mask)
    for v in variants:
        assert got_d[v] == want[v], f"device form, variant {v}"


def test_bad_masks_and_unsorted_durations_are_refused(engine):
    import vid_dup_finder_lib_amd as vdf

    h, z, d = _database(600, (1,))
    for mask in (1, 3, 256, 0x1FE + 1):
        with pytest.raises(vdf.VdfError) as ei:
            engine.search_variants_sorted(h, z, d, 350, mask)
        assert ei.value.code == -5
    with pytest.raises(vdf.VdfError) as ei:
        engine.search_variants_sorted(h, z, d[::-1], 350, 2)
    assert ei.value.code == -5
    assert engine.search_variants_sorted(h, z, d, 350, 0) == {}
    assert engine.search_variants_sorted(h[:0], z[:0], d[:0], 350, 2) == {1: []}


def test_end_to_end_mirrored_copies_at_64x64(engine):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(4040)
    base = [planegen.clip("blocks_noise", rng, 64, 64) for _ in range(31)]
    base.insert(30, planegen.clip("static", rng, 64, 64))
    # (an x-symmetric clip is hashed apart, below: with half of its coefficients exactly zero it sits 272 bits from the static clip, whose
    # hash has 100 live bits - inside the tolerance of a plain search(), mirrors or not)
    clips, paths, pairs = list(base), [f"clip{i:02d}" for i in range(len(base))], {}
    for k in range(8):
        m = planegen.flip(base[k], 1).astype(np.int16) + rng.integers(-2, 3, size=base[k].shape)
        clips.append(np.clip(m, 0, 255).astype(np.uint8))
        paths.append(f"mirror{k:02d}")
        pairs[f"clip{k:02d}"] = f"mirror{k:02d}"
    assert len(clips) == 40
    hashes = vdf.hash_frame_stacks(np.stack(clips), paths, [100] * len(clips), engine=engine, zero_plane=True)
    assert vdf.search(hashes, 0.3, engine=engine) == [], "a mirrored copy is no duplicate for search()"
    static = hashes[30]
    d_self = static.hamming_distance(static.flipped(vdf.Flip.X))
    print("static clip against its own mirror:", d_self, "bits")
    assert 0 < d_self <= 300, "without the (r, r) rule the static clip would be its own mirrored duplicate"
    sym = vdf.hash_frame_stacks(planegen.clip("x_symmetric", rng, 64, 64)[None], ["sym"], [100], engine=engine, zero_plane=True)[0]
    assert sym.flipped(vdf.Flip.X) == sym  # an x-symmetric clip IS its own mirror
    got = vdf.search_flipped(hashes, 0.3, flips=(vdf.Flip.X,), engine=engine)
    assert list(got) == [vdf.Flip.X]
    found = {g.reference(): list(g.duplicates()) for g in got[vdf.Flip.X]}
    want = {a: [b] for a, b in pairs.items()}
    want.update({b: [a] for a, b in pairs.items()})
    assert found == want
    assert all(g.reference() not in list(g.duplicates()) for g in got[vdf.Flip.X])
    refs = [g.reference() for g in got[vdf.Flip.X]]
    assert refs == sorted(refs)  # Search::sort order of the references (equal durations: by path)
