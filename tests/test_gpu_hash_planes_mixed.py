"""The zero plane from the mixed-size call (vdf_hash_clips_u8_planes[_device]; csrc/dct_hash.hip: resize_dct_hash_mixed_small_kernel<true>, dct_hash_indexed_kernel<true>
behind resize_mfma_mixed_kernel) against the CPU oracle: one call with clips of five small sizes in random order, some with crop boxes, every mixed part
(kSmall: w <= 256 and h <= 128; kLines: w < 192; kWideLines: w >= 192) taken by at least one clip.  The three assertions of tests/test_gpu_hash_planes.py, with
hash, plane and variants defined on the CROPPED clip; then the uniform shortcut (all clips of one size: the kernels of the uniform call, cropped and not)."""
import numpy as np
import pytest

import planegen

pytestmark = pytest.mark.gpu

SIZES = [(48, 36), (96, 96), (160, 90), (150, 140), (200, 136)]  # w x h: three small, one lines (w < 192, h > 128), one whole lines (w >= 192, h > 128)
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _expected(clips, crops):
    hs, zs, fl = [], [], {v: [] for v in range(1, 8)}
    for c, (l, r, t, b) in zip(clips, crops):
        h, w = c.shape[1:]
        box = np.ascontiguousarray(c[:, t:h - b, l:w - r])
        words, zero, _ = planegen.oracle_planes(box)
        hs.append(words)
        zs.append(zero)
        for v in fl:
            fl[v].append(planegen.oracle_variant(box, v))
    return np.stack(hs), np.stack(zs), {v: np.stack(x) for v, x in fl.items()}


def _corpus():
    if "mixed" not in _CACHE:
        rng = np.random.default_rng(909)
        kinds = planegen.KINDS
        clips, crops = [], []
        for i, (w, h) in enumerate(SIZES):
            for j in range(3):
                clips.append(planegen.clip(kinds[(3 * i + j) % len(kinds)], rng, h, w))
                crops.append(((w // 7, w // 9 + 1, 0, 0), (0, 0, h // 8, h // 6 + 1), (0, 0, 0, 0))[j])
        order = rng.permutation(len(clips))
        clips, crops = [clips[i] for i in order], np.array([crops[i] for i in order], np.uint32)
        _CACHE["mixed"] = (clips, crops) + _expected(clips, crops)
    return _CACHE["mixed"]


def _device(eng, clips, crops):
    import torch

    buf, recs, nf = eng._pack_stacks(clips)
    recs["crop"] = crops
    n = len(clips)
    d_buf = torch.from_numpy(buf).cuda()
    outs = [torch.full((n, 16), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    eng.hash_clips_device(d_buf.data_ptr(), buf.size, recs, outs[0].data_ptr())
    eng.hash_clips_planes_device(d_buf.data_ptr(), buf.size, recs, outs[1].data_ptr(), outs[2].data_ptr())
    torch.cuda.synchronize()
    var = {}
    for v in range(1, 8):
        o = torch.full((n, 16), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.hash_variants_device(outs[1].data_ptr(), outs[2].data_ptr(), n, v, o.data_ptr())
        torch.cuda.synchronize()
        var[v] = o.cpu().numpy().view(np.uint64)
    return [o.cpu().numpy().view(np.uint64) for o in outs], var


def _same(what, plain, got, zero, var, want_h, want_z, want_var):
    assert np.array_equal(got, plain), f"{what}: the planes call's hashes differ from the plain call's"
    assert np.array_equal(got, want_h), f"{what}: hashes differ from the oracle's"
    bad = np.nonzero((zero != want_z).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: zero planes of clips {bad} differ"
    for v in var:
        assert np.array_equal(var[v], want_var[v]), f"{what}: variant {v}"


def test_one_call_with_five_sizes_crop_boxes_and_every_mixed_part(eng):
    clips, crops, want_h, want_z, want_var = _corpus()
    boxes = [(c.shape[2] - int(l) - int(r), c.shape[1] - int(t) - int(b)) for c, (l, r, t, b) in zip(clips, crops)]
    assert any(w <= 256 and h <= 128 for w, h in boxes) and any(w < 192 and h > 128 for w, h in boxes) and any(w >= 192 and h > 128 for w, h in boxes)
    (plain, got, zero), var = _device(eng, clips, crops)
    _same("device", plain, got, zero, var, want_h, want_z, want_var)
    got_h, zero_h = eng.hash_clips_planes(clips, crops=crops)  # the host entry: clips repacked through the pinned staging
    assert np.array_equal(got_h, want_h) and np.array_equal(zero_h, want_z)


@pytest.mark.parametrize("cropped", [False, True])
def test_the_uniform_shortcut(eng, cropped):
    """All clips of one size, evenly spaced: the kernels of the uniform call (96 x 96: the tiled persistent kernel; with boxes resize_dct_hash_cropped_small_kernel)."""
    rng = np.random.default_rng(31 + cropped)
    clips = [planegen.clip(k, rng, 96, 96) for k in planegen.KINDS]
    crops = np.array([(i, 2 * i, 3 + i, 1) for i in range(len(clips))], np.uint32) if cropped else np.zeros((len(clips), 4), np.uint32)
    want_h, want_z, want_var = _expected(clips, crops)
    (plain, got, zero), var = _device(eng, clips, crops)
    _same("uniform", plain, got, zero, var, want_h, want_z, want_var)


def test_gen_hashes_letterbox_with_planes_flips_the_cropped_clip(eng):
    import vid_dup_finder_lib_amd as vdf
    from oracle import vdf_oracle as orc

    rng = np.random.default_rng(77)
    frames = np.stack([planegen.clip(k, rng, 64, 64) for k in ("blocks_noise", "ramp_noise", "static")])
    frames[:, :, :, :9] = 16
    frames[:, :, :, -5:] = 16
    vhs = vdf.gen_hashes(frames, ["a", "b", "c"], [5, 5, 5], engine=eng, zero_plane=True)
    plain = vdf.gen_hashes(frames, ["a", "b", "c"], [5, 5, 5], engine=eng)
    for i, v in enumerate(vhs):
        rc, want, _, crop = orc.hash_clip_letterbox(frames[i])
        assert rc == 0 and crop[0] > 0 and np.array_equal(v.hash, want) and np.array_equal(plain[i].hash, want) and plain[i].zero is None
        box = np.ascontiguousarray(frames[i][:, crop[2]:64 - crop[3], crop[0]:64 - crop[1]])
        assert np.array_equal(v.flipped(vdf.Flip.X).hash, planegen.oracle_variant(box, 1))
