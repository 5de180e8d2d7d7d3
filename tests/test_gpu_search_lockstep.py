"""The lock-step stream of hamming_mfma2_kernel (both row tiles of a wave on one LDS fragment, four accumulator sets, row terms in
one register per row tile) against the CPU oracle, at the smallest shapes at which each of its mechanisms can fail:

* row-term lanes: accumulator register r gets its row term from lane r of a 16-lane row.  Rows of very different popcounts sit side
  by side, so a term taken from the wrong lane moves a row's threshold by tens to hundreds of bits; a partner exactly AT the
  tolerance is planted for every one of the 64 row positions of a wave (a threshold raised by a wrong term loses it) next to one
  exactly one bit over it;
* set rotation and the two LDS buffers: partners in every (column sub-tile, stage parity, row tile of the wave), in the last,
  partial stage and in the first stage of the diagonal chunk, which starts mid-stage;
* the 256-row form (search_with_references) with narrow windows, live masks that differ inside a tile and a row permutation;
* a windowed self search whose column ranges begin and end mid-stage;

each at every instantiated early-exit step - the lock-step instances (8, 10, 11, 12) and both kept streams (6; 13, 14, 16) - and at
tolerances 120, 300 and 350.  Everything is == the oracle; that the oracle reports every planted pair at the tolerance and none
one bit over it is asserted on the CPU before the GPU is used."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu

N = 1537  # three 512-row tiles and a one-row fourth; thirteen 128-column stages, the last one holding a single column
STEPS = (6, 8, 10, 11, 12, 13, 14, 16)
TOLS = (120, 300, 350)


def _skewed_hashes(rng, n):
    """row i has bit density 0.1 + 0.8 ((37 i) mod 64) / 63: neighbouring rows' popcounts differ by hundreds, and each of the 64 row
    positions of a wave sees several densities (37 is odd: 64 consecutive rows take all 64 densities)"""
    dens = 0.1 + 0.8 * ((np.arange(n) * 37) % 64) / 63.0
    bits = (rng.random((n, 1024)) < dens[:, None]).astype(np.uint8)
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).copy()


def _flipped(h, d, rng):
    """h with exactly d of its 1024 bits flipped"""
    bits = np.unpackbits(h.view(np.uint8), bitorder="little")
    bits[rng.choice(1024, size=d, replace=False)] ^= 1
    return np.packbits(bits, bitorder="little").view(np.uint64)


def _plant(words, plants, tol, rng):
    """plants: (row, column of the partner at tol, column of the partner at tol + 1); the columns are overwritten"""
    rows = {r for r, _, _ in plants}
    cols = [c for _, a, b in plants for c in (a, b)]
    assert len(set(cols)) == len(cols) and not rows & set(cols) and all(r < a and r < b for r, a, b in plants)
    for r, a, b in plants:
        words[a] = _flipped(words[r], tol, rng)
        words[b] = _flipped(words[r], tol + 1, rng)


def _assert_oracle_reports(words, dur, plants, tol):
    """search_with_references outputs every hit: with the planted rows as references the oracle lists each partner at the tolerance
    and none of those one bit over it"""
    rows = sorted({r for r, _, _ in plants})
    res = dict(orc.search_refs_sorted(words, dur, words[rows], dur[rows], tol))
    for r, at, over in plants:
        members = res.get(rows.index(r), [])
        assert at in members and over not in members, (r, at, over)


@functools.lru_cache(maxsize=None)
def _row_term_case(tol):
    """a partner at the tolerance and one over it for each row position 0 .. 63 of wave 0 (rows 0 .. 63) and of wave 7 (rows
    448 .. 511) of row tile 0; partners in columns 1024 .. 1279"""
    rng = np.random.default_rng(4000 + tol)
    words = _skewed_hashes(rng, N)
    rows = list(range(0, 64)) + list(range(448, 512))
    plants = [(r, 1024 + 2 * k, 1025 + 2 * k) for k, r in enumerate(rows)]
    _plant(words, plants, tol, rng)
    dur = np.zeros(N, np.uint32)
    _assert_oracle_reports(words, dur, plants, tol)
    want = orc.search_self_sorted(words, dur, tol)
    if tol == 120:  # no two unrelated rows are that close (the sparsest pair sits near 180): every plant is a group of its own
        assert sorted(want) == sorted([at, r] for r, at, _ in plants)
    return words, dur, want


@functools.lru_cache(maxsize=None)
def _rotation_case(tol):
    """row tile 0 (columns from 1: its first stage starts mid-stage).  Partners in every (sub-tile s, stage parity q, row tile rt of the
    wave): rows 128 + 64 q + 32 rt + s (waves 2 and 3), columns 128 (4 + q) + 32 s + 2 rt (+ 1: the partner over the tolerance) -
    stages 4 and 5.  Column 1536, the only one of the last stage, partners row 200 at the tolerance.
    First stage of the diagonal chunk: rows 2 and 40 with partners in columns 100 .. 103; row tile 1 (columns from 513): row 517 with
    partners in columns 600 and 601."""
    rng = np.random.default_rng(5000 + tol)
    words = _skewed_hashes(rng, N)
    plants = [(128 + 64 * q + 32 * rt + s, 128 * (4 + q) + 32 * s + 2 * rt, 128 * (4 + q) + 32 * s + 2 * rt + 1)
              for s in range(4) for q in range(2) for rt in range(2)]
    plants += [(2, 100, 101), (40, 102, 103), (517, 600, 601)]
    _plant(words, plants, tol, rng)
    words[1536] = _flipped(words[200], tol, rng)
    dur = np.zeros(N, np.uint32)
    _assert_oracle_reports(words, dur, plants, tol)
    assert 1536 in dict(orc.search_refs_sorted(words, dur, words[[200]], dur[:1], tol)).get(0, [])
    return words, dur, orc.search_self_sorted(words, dur, tol)


@functools.lru_cache(maxsize=None)
def _windowed_case(tol):
    """the same skewed hashes under sorted log-uniform durations: a row sees the ~20 later entries within x 1.1, so the column range of a
    row tile begins and ends mid-stage.  Every 9th row gets a partner at the tolerance three entries on and one over it four on."""
    rng = np.random.default_rng(6000 + tol)
    words = _skewed_hashes(rng, N)
    dur = np.sort(np.floor(np.exp(rng.uniform(np.log(5), np.log(7200), size=N))).astype(np.uint32))
    for r in range(0, N - 4, 9):
        words[r + 3] = _flipped(words[r], tol, rng)
        words[r + 4] = _flipped(words[r], tol + 1, rng)
    want = orc.search_self_sorted(words, dur, tol)
    assert len(want) >= 100  # most of the 171 planted pairs are inside their row's window
    return words, dur, want


@functools.lru_cache(maxsize=None)
def _refs_case(tol):
    """300 references (two 256-row tiles, the second mostly padding) against 700 candidates, skewed densities, log-uniform durations
    (+-5 % windows: ~10 candidates a row, empty for some: the live masks differ inside a tile; the references are not sorted, so the
    row permutation is in play).  Reference r is candidate pick[r] at the tolerance (r even) or one bit over it (r odd), same duration."""
    rng = np.random.default_rng(7000 + tol)
    cw = _skewed_hashes(rng, 700)
    cd = np.sort(np.floor(np.exp(rng.uniform(np.log(5), np.log(7200), size=700))).astype(np.uint32))
    pick = rng.choice(700, size=300, replace=False)
    rw = np.stack([_flipped(cw[c], tol + (r & 1), rng) for r, c in enumerate(pick)])
    rd = cd[pick].copy()
    rd[::7] = 3  # no candidate is that short: rows with an empty window
    want = orc.search_refs_sorted(cw, cd, rw, rd, tol)
    res = dict(want)
    for r, c in enumerate(pick):
        assert (int(c) in res.get(r, [])) == (r % 2 == 0 and r % 7 != 0), (r, c)
    return cw, cd, rw, rd, want


@contextlib.contextmanager
def _engine(step, monkeypatch):
    import vid_dup_finder_lib_amd as vdf

    monkeypatch.setenv("VDF_SEARCH_BACKEND", "mfma")
    monkeypatch.setenv("VDF_MFMA_PRUNE_STEP", str(step))
    eng = vdf.Engine(0)  # created after the variable is set: the step is read once
    try:
        yield eng
    finally:
        eng.close()


def _expected_exit_bits(step):
    return 64 * (step + 1) if step < 15 else 0


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("step", STEPS)
def test_row_terms_reach_the_right_accumulator_registers(step, tol, monkeypatch):
    words, dur, want = _row_term_case(tol)
    with _engine(step, monkeypatch) as eng:
        assert eng.search_self_sorted(words, dur, tol) == want
        assert eng.last_stats()["early_exit_bits"] == _expected_exit_bits(step)  # the instance asked for is the one that ran


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("step", STEPS)
def test_every_set_of_the_rotation_and_both_lds_buffers(step, tol, monkeypatch):
    words, dur, want = _rotation_case(tol)
    with _engine(step, monkeypatch) as eng:
        assert eng.search_self_sorted(words, dur, tol) == want


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("step", STEPS)
def test_windowed_self_search_with_ranges_that_begin_and_end_mid_stage(step, tol, monkeypatch):
    words, dur, want = _windowed_case(tol)
    with _engine(step, monkeypatch) as eng:
        assert eng.search_self_sorted(words, dur, tol) == want


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("step", STEPS)
def test_256_row_form_with_narrow_windows_and_a_row_permutation(step, tol, monkeypatch):
    cw, cd, rw, rd, want = _refs_case(tol)
    with _engine(step, monkeypatch) as eng:
        assert eng.search_refs_sorted(cw, cd, rw, rd, tol) == want
