"""CPU: the counter-based generator of the device RNG -- Philox4x32-10 known answers through the library's host entry and
through the numpy restatement the GPU tests measure the kernels against, and the packing of (step, rank, stream)."""
import itertools

import numpy as np
import pytest

import rng_restatement as rs

# Random123's known-answer vectors for Philox4x32-10: (counter, key, output)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers_library_and_restatement(counter, key, want):
    from denoising_diffusion_deep_fake_amd import ops
    assert ops.philox4x32_10(counter, key) == want
    assert tuple(int(v) for v in rs.philox4x32_10(counter, key)) == want


def test_library_and_restatement_agree_on_random_blocks():
    from denoising_diffusion_deep_fake_amd import ops
    words = np.random.default_rng(0).integers(0, 1 << 32, size=(64, 6), dtype=np.uint64)
    got = rs.philox4x32_10([words[:, i] for i in range(4)], (0, 0))  # vectorised over counters, one key
    for i, w in enumerate(words):
        assert ops.philox4x32_10(w[:4], (0, 0)) == tuple(int(v[i]) for v in got)
        assert ops.philox4x32_10(w[:4], w[4:]) == tuple(int(v) for v in rs.philox4x32_10(w[:4], w[4:]))


def test_restated_normals_begin_as_documented():
    """seed 0x5EED, offset 0, image 0: the first normals of the layout (Device RNG)"""
    z, r = rs.normals64(0x5EED, 0, 1, 8)
    want = [-0.34926039, 0.1513466, 0.43114642, 0.24097323, -0.24141967, -0.37667052]
    assert np.allclose(z[0, :6], want, rtol=0, atol=5e-8)
    assert np.allclose(z[0, 0] ** 2 + z[0, 1] ** 2, r[0, 0] ** 2)
    y = rs.y_uniform(0x5EED, 0, 4)
    assert y.dtype == np.float32 and ((0 <= y) & (y < 1)).all()


def test_offset_packing_is_injective_and_bounded():
    from denoising_diffusion_deep_fake_amd.rng import pack_offset
    steps = [0, 1, 2, 255, 256, (1 << 24) - 1, 1 << 24, (1 << 40) - 2, (1 << 40) - 1]
    ranks = [0, 1, 7, 255, 256, 65534, 65535]
    streams = [0, 1, 2, 254, 255]
    seen = {}
    for key in itertools.product(steps, ranks, streams):
        off = pack_offset(*key)
        assert 0 <= off < 1 << 64
        assert seen.setdefault(off, key) == key, (key, seen[off])
    assert len(seen) == len(steps) * len(ranks) * len(streams)
    assert pack_offset(3, 2, 1) == 3 << 24 | 2 << 8 | 1 and pack_offset(5) == 5 << 24
    for bad in ((1 << 40, 0, 0), (0, 65536, 0), (0, 0, 256), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        with pytest.raises(ValueError):
            pack_offset(*bad)


def test_graph_step_with_device_rng_is_refused():
    from denoising_diffusion_deep_fake_amd import rng
    with pytest.raises(ValueError, match="graph_step"):
        rng.refuse_graph_step({"device_rng": True, "graph_step": True})
    rng.refuse_graph_step({"device_rng": True})
    rng.refuse_graph_step({"graph_step": True})
