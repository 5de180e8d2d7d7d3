"""locate()'s bookkeeping (window index -> video and first frame, ascending, distances) on plain VideoHash lists, without a GPU: the engine is a stub whose
reference search is the oracle's."""
import numpy as np

from oracle import vdf_oracle as orc


class OracleEngine:
    calls = 0

    def search_refs_sorted(self, cand_hashes, cand_dur, ref_hashes, ref_dur, tol_int):
        OracleEngine.calls += 1
        assert not np.any(cand_dur) and not np.any(ref_dur)  # every duration 0: search_one's +-5 % window admits every entry
        return orc.search_refs_sorted(cand_hashes, cand_dur, ref_hashes, ref_dur, tol_int)


def test_locate_maps_windows_back_to_videos_and_frames():
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(7)
    stride = 3
    windows = [[vdf.VideoHash.random_hash(rng).with_src_path(f"v{v}").with_duration(10 + v) for _ in range(n)] for v, n in enumerate((4, 0, 6))]
    near = windows[0][2].hash_with_spatial_distance(40, rng)       # 40 bits from window 2 of video 0 ...
    windows[2][5] = near.hash_with_spatial_distance(25, rng)       # ... and window 5 of video 2 at 25 bits from it
    needles = [windows[2][1], near, vdf.VideoHash.random_hash(rng)]
    got = vdf.locate(needles, windows, 0.1, stride=stride, engine=OracleEngine())
    assert got[0] == [(2, 1 * stride, 0)]
    assert got[1] == [(0, 2 * stride, 40), (2, 5 * stride, 25)]  # ascending by (video, frame), each with its distance
    assert got[2] == []
    assert vdf.locate(needles, windows, 0.03, stride=stride, engine=OracleEngine())[1] == [(2, 5 * stride, 25)]
    before = OracleEngine.calls
    assert vdf.locate([], windows, 0.1, engine=OracleEngine()) == [] and vdf.locate(needles, [[], []], 0.1, engine=OracleEngine()) == [[], [], []]
    assert OracleEngine.calls == before  # nothing to search: no call
