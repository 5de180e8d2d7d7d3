"""The batching queue for clips of any frame size with Cropdetect::Letterbox (vdf_hash_queue_create_mixed_letterbox, vdf_hash_queue_mixed_submit_crop;
csrc/hash_queue_mixed.cpp): concurrent submitters share batched vdf_hash_clips_u8_letterbox calls; every caller gets the oracle's hash and box of its own clip
(the corpus of tests/letterbox_mixed_corpus.py without its 1080p clip)."""
import threading

import numpy as np
import pytest

import letterbox_mixed_corpus as lc

pytestmark = pytest.mark.gpu


def _without_1080p():
    names, clips, boxes, words, _ = lc.corpus()
    keep = [i for i, c in enumerate(clips) if c.shape[1:] != (1080, 1920)]
    return [names[i] for i in keep], [clips[i] for i in keep], boxes[keep], words[keep]


def test_24_threads_share_one_letterbox_queue(engine):
    from vid_dup_finder_lib_amd.engine import MixedHashQueue

    names, clips, boxes, words = _without_1080p()
    n = len(clips)
    order = np.random.default_rng(24).permutation(n)
    q = MixedHashQueue(engine, staging_bytes=64 << 20, max_batch=8, max_wait_us=20000, letterbox=True)
    got, errs = [None] * n, []

    def worker(t):
        try:
            for k in range(t, n, 24):
                i = int(order[k])
                got[i] = q.submit(clips[i])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(24)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errs, errs
    for i in range(n):
        assert got[i] is not None, names[i]
        h, crop = got[i]
        assert crop == tuple(int(x) for x in boxes[i]), (names[i], crop, boxes[i])
        assert np.array_equal(h, words[i]), names[i]
    n_batches, n_clips = q.stats()
    q.close()
    assert n_clips == n and (n + 7) // 8 <= n_batches <= n
    # a batch holds clips of ONE size only if there are at least as many batches as sizes: fewer batches means some batch held two
    n_sizes = len({c.shape[1:] for c in clips})
    print("batches", n_batches, "clips", n_clips, "sizes", n_sizes)
    assert n_batches < n_sizes, (n_batches, n_sizes)


def test_a_plain_queue_answers_submit_crop_with_zeros(engine):
    from oracle import vdf_oracle as orc
    from vid_dup_finder_lib_amd.engine import MixedHashQueue

    names, clips, boxes, _ = _without_1080p()
    i = next(k for k, c in enumerate(clips) if c.shape[1:] == (90, 160) and boxes[k].all())
    q = MixedHashQueue(engine, staging_bytes=1 << 20, max_batch=4, max_wait_us=0)
    h, crop = q.submit_crop(clips[i])
    assert crop == (0, 0, 0, 0) and np.array_equal(h, orc.hash_clips(clips[i][None])[0])  # the plain hash: the whole frame
    assert np.array_equal(q.submit(clips[i]), h)
    q.close()
