"""What dct_hash_windows_kernel rests on, pinned on the CPU with the oracle's own functions: the 3-D DCT runs along y, x, then t
(raw_dct_ops.rs:118-132), the y and x passes of a frame touch no other frame, so the frame's 10 x 10 spatial coefficients can be computed ONCE and are the
same doubles in every window that holds the frame.  Per-frame coefficients, then one temporal DCT per window, equal oracle.hash_clip(window, want_coefs=True)
bit for bit as u64 - signs of zero included - on noisy, static and constant stretches.  Passes on the library as it stands, by design."""
import numpy as np

import windowgen
from oracle import vdf_oracle as orc


def _spatial(frame):
    """S[kx][ky] (16 x 16 kept; the hash reads 10 x 10) of one frame: resize, centre, DCT along y, then along x - the oracle's dct16 on each line."""
    small = orc.resize_frame(frame).astype(np.float64) - 128.0  # [y][x]
    m = small.T.copy()                                          # [x][y] (dct_3d.rs:40-44)
    for x in range(16):
        m[x, :] = orc.dct16(m[x, :])
    for y in range(16):
        m[:, y] = orc.dct16(m[:, y])
    return m


def test_per_frame_spatial_coefficients_then_a_temporal_dct_are_the_window_hash_bit_for_bit():
    rng = np.random.default_rng(20240914)
    frames = windowgen.video(rng, 40, 48, 64, lead=4)
    spatial = np.stack([_spatial(f) for f in frames])  # once per frame
    zeros = 0
    kinds = set()
    for s in range(len(frames) - 15):
        rc, _words, want = orc.hash_clip(frames[s:s + 16], want_coefs=True)
        assert rc == 0
        got = np.empty(1000, np.float64)
        for kx in range(10):
            for ky in range(10):
                got[np.arange(10) * 100 + 10 * kx + ky] = orc.dct16(spatial[s:s + 16, kx, ky])[:10]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"window {s}: {(got.view(np.uint64) != want.view(np.uint64)).sum()} coefficients differ"
        z = int((want == 0.0).sum())
        zeros += z
        kinds.add("static" if z == 900 else "constant" if z == 999 else "other")
    print(f"25 windows, {zeros} exact zeros, kinds {sorted(kinds)}")
    assert kinds == {"static", "constant", "other"} and zeros >= 2 * 900 + 999
