"""On-device random draws (restart list, down-sampling choice) against the numpy Philox restatement.

CPU: the restatement against the Random123 known-answer vectors of Philox4x32-10 (kat_vectors of the reference
implementation: all-zero, all-ones and the pi-digits case), and distribution sanity.
GPU: device == restatement bit for bit for the uniforms / choices / dropout masks, 1e-12 for the Box-Muller normals (device libm)."""
import math

import numpy as np
import pytest

from oracle import rng_np


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = rng_np.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], key[0], key[1])
        assert tuple(int(g[0]) for g in got) == want


def test_restart_distribution_and_choice_properties():
    ry, T, (u1, u2, u3) = rng_np.draw_restarts(12345, 64, 60, 10 * math.pi / 180, 10.0)
    assert ry.shape == (64, 60) and T.shape == (64, 60, 3)
    assert np.all(u1 > 0) and np.all(u1 <= 1) and np.all(T[..., :2] == 0) and np.all(np.abs(T[..., 2]) <= 10)
    assert abs(ry.mean()) < 0.01 and abs(ry.std() - 10 * math.pi / 180) < 0.01
    assert abs(T[..., 2].mean()) < 0.5 and abs(T[..., 2].std() - 10 / math.sqrt(3)) < 0.3
    idx = rng_np.random_choice(7, 0, 3, 5000, 1024)
    for b in range(3):
        assert len(set(idx[b].tolist())) == 1024 and idx[b].min() >= 0 and idx[b].max() < 5000
    assert not np.array_equal(idx[0], idx[1])
    assert np.array_equal(idx, rng_np.random_choice(7, 0, 3, 5000, 1024))                 # a pure function of its arguments
    assert not np.array_equal(idx, rng_np.random_choice(7, 1, 3, 5000, 1024))
    # every source index is equally likely: chi-square-ish check on the selection frequency over many frames
    many = rng_np.random_choice(99, 0, 200, 64, 16)
    freq = np.bincount(many.ravel(), minlength=64)
    assert abs(freq.mean() - 50) < 1e-9 and freq.std() < 12


@pytest.mark.gpu
def test_device_draws_match_restatement(dev):
    import torch
    from deepi2p_amd import prep
    from deepi2p_amd.registration import RegistrationPipeline
    pipe = RegistrationPipeline(160, 512, R=60)
    noise, Ts = pipe.draw_on_device(32, dev, seed=2**40 + 17)
    ry, T, _ = rng_np.draw_restarts(2**40 + 17, 32, 60, pipe.ry_sigma, pipe.amp)
    np.testing.assert_array_equal(Ts.cpu().numpy(), T)                                     # uniforms: exact integer arithmetic
    np.testing.assert_allclose(noise.cpu().numpy(), ry, rtol=0, atol=1e-12)
    n2, T2 = pipe.draw_on_device(32, dev, seed=2**40 + 17)
    assert torch.equal(n2, noise) and torch.equal(T2, Ts)
    for n_src, n_out in ((5000, 1024), (100000, 20480), (37, 37), (8192, 1)):
        got = prep.random_choice(5, 4, n_src, n_out, dev, stream_id=3).cpu().numpy()
        np.testing.assert_array_equal(got, rng_np.random_choice(5, 3, 4, n_src, n_out))


@pytest.mark.gpu
def test_device_downsample_and_node_sampling(dev):
    """downsample_np semantics (kitti_pc_img_pose_loader.py:158-171): a subset when the scan is long enough, otherwise every
    point floor(N/Nraw) times plus a random remainder; FPS nodes from on-device candidates are points of the cloud."""
    import torch
    from deepi2p_amd import prep
    g = torch.Generator().manual_seed(0)
    for Nraw, N in ((30000, 20480), (9000, 20480), (20480, 20480)):
        pc = torch.randn(2, 3, Nraw, generator=g).to(dev)
        inten = torch.rand(2, 1, Nraw, generator=g).to(dev)
        sn = torch.randn(2, 3, Nraw, generator=g).to(dev)
        p2, i2, s2, idx = prep.downsample(pc, inten, sn, N, seed=11)
        assert p2.shape == (2, 3, N) and i2.shape == (2, 1, N) and s2.shape == (2, 3, N)
        idc = idx.cpu().numpy()
        for b in range(2):
            counts = np.bincount(idc[b], minlength=Nraw)
            if Nraw >= N:
                assert counts.max() == 1 and counts.sum() == N
            else:
                assert counts.min() >= N // Nraw and counts.max() <= N // Nraw + 1 and counts.sum() == N
            assert torch.equal(p2[b], pc[b][:, idx[b].long()]) and torch.equal(i2[b], inten[b][:, idx[b].long()])
    nodes = prep.sample_nodes_device(p2, 128, seed=3, stream_id=1)
    assert nodes.shape == (2, 3, 128)
    d = (nodes[0].t().unsqueeze(1) - p2[0].t().unsqueeze(0)).abs().sum(-1).min(dim=1).values
    assert float(d.max()) == 0.0


# The dropout keep-mask.  A Philox word that is exactly 0 (kept at p = 0: the rule is word >= p * 2^32) comes once in 2^32 draws; this seed
# has one among its first 99457 elements on stream 5 (found by searching seeds from 2^40 upwards), so the boundary of the rule is tested.
DROPOUT_SEED, DROPOUT_STREAMS, DROPOUT_ZERO_AT = 2**40 + 75044, (5, 0), 16528
DROPOUT_N = (1, 2, 3, 4, 5, 1023, 1025, 99457)
DROPOUT_P = (0.0, 0.1, 0.5, float(np.nextafter(np.float32(1.0), np.float32(0.0))))


def test_dropout_mask_restatement_keep_rate_and_purity():
    n = 99457
    q = np.array([DROPOUT_ZERO_AT // 4], dtype=np.uint64)
    words = rng_np.philox4x32_10(q, q * np.uint64(0), q * np.uint64(0) + np.uint64(5), q * np.uint64(0) + np.uint64(3),
                                 DROPOUT_SEED & rng_np.MASK, DROPOUT_SEED >> 32)
    assert int(words[DROPOUT_ZERO_AT % 4][0]) == 0                       # the word behind element DROPOUT_ZERO_AT is 0 ...
    assert rng_np.dropout_mask(DROPOUT_SEED, 5, 0.0, n).all()             # ... and p = 0 keeps it, like every other element
    assert rng_np.dropout_mask(DROPOUT_SEED, 5, float(np.float32(2.0 ** -32)), n)[DROPOUT_ZERO_AT] == 0 and \
        rng_np.dropout_mask(DROPOUT_SEED, 5, float(np.float32(2.0 ** -32)), n).sum() == n - 1
    for p in DROPOUT_P:
        m = rng_np.dropout_mask(DROPOUT_SEED, 5, p, n)
        assert m.dtype == np.uint8 and m.shape == (n,) and set(np.unique(m)) <= {0, 1}
        keep = 1.0 - float(np.float32(p))
        assert abs(m.mean() - keep) <= 4.0 * math.sqrt(max(keep * (1.0 - keep), 1e-7) / n)            # four standard deviations of the mean
        assert np.array_equal(m, rng_np.dropout_mask(DROPOUT_SEED, 5, p, n))                            # a pure function of its arguments
        for shorter in (1, 2, 3, 4, 5, 1023):                                                           # element i does not depend on n
            assert np.array_equal(m[:shorter], rng_np.dropout_mask(DROPOUT_SEED, 5, p, shorter))
    half = rng_np.dropout_mask(DROPOUT_SEED, 5, 0.5, n)
    assert not np.array_equal(half, rng_np.dropout_mask(DROPOUT_SEED, 0, 0.5, n))                       # the stream id matters,
    assert not np.array_equal(half, rng_np.dropout_mask(DROPOUT_SEED + 1, 5, 0.5, n))                   # so does the low word of the seed
    assert not np.array_equal(half, rng_np.dropout_mask(DROPOUT_SEED + 2**32, 5, 0.5, n))               # and the high word


@pytest.mark.gpu
@pytest.mark.parametrize("n", DROPOUT_N)
def test_device_dropout_mask_matches_restatement(dev, n):
    """di2p_dropout_mask on raw pointers, the mask between NaN guard bands (n is mostly no multiple of 4: the last Philox block is cut)"""
    import torch
    from deepi2p_amd import _lib
    from tests.gpu_exact_harness import Guarded, twice
    for stream_id in DROPOUT_STREAMS:
        for p in DROPOUT_P:
            def run():
                out = Guarded(n, dev)
                _lib.call("di2p_dropout_mask", DROPOUT_SEED, stream_id, p, n, out.ptr, _lib.stream())
                return [out]
            got = twice(run)[0].cpu(torch.uint8).numpy()
            want = rng_np.dropout_mask(DROPOUT_SEED, stream_id, p, n)
            assert np.array_equal(got, want), "stream %d p %r: first differing element %d" % (stream_id, p, int(np.nonzero(got != want)[0][0]))
