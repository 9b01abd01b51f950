"""CPU-only checks of tests/front_end_ref.py, the numpy references of test_gpu_front_end.py: against the C oracle
(strided-conv output sets) and torch (bf16 rounding).  No HIP code runs here."""
import numpy as np
import pytest
import torch

import front_end_ref as fr


@pytest.mark.parametrize("geom", fr.RULEBOOK_GEOMS)
@pytest.mark.parametrize("grid", [(2, 11, 21, 19), (2, 62, 9, 8), (1, 64, 8, 8)])
def test_down_set_matches_oracle_and_rows_are_a_permutation(geom, grid):
    from oracle import ops as oops

    ks, st, pd, subm = geom
    B, D, H, W = grid
    rng = np.random.default_rng(11)
    idx = fr.random_coords(rng, B, D, H, W, 0.1, force_z=(0, D - 1))
    o_idx, _, _, oshape = oops.rulebook(idx, (D, H, W), ks, st, pd, subm)
    if subm:
        want, osh = idx, (D, H, W)
    else:
        want, osh = fr.down_set(idx, (D, H, W), ks, st, pd), fr.out_shape((D, H, W), ks, st, pd)
    assert tuple(int(v) for v in oshape) == osh
    assert len(o_idx) == len(want) and set(map(tuple, o_idx)) == set(map(tuple, want))
    for coords, shape in ((idx, (D, H, W)), (want, osh)):
        rows = fr.index_rows(coords, B, *shape)
        assert rows.shape == coords.shape and set(map(tuple, rows)) == set(map(tuple, coords))
        key = fr.col_key(B, shape[1], shape[2], rows[:, 0], rows[:, 2], rows[:, 3]) * 128 + rows[:, 1]
        assert np.all(np.diff(key) > 0)  # strictly ascending (col_key, z): sorted and duplicate-free


def test_col_key_is_the_tiled_bijection():
    B, H, W = 2, 13, 22  # neither a multiple of 8
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    key = fr.col_key(B, H, W, b, y, x).ravel()
    assert len(np.unique(key)) == B * H * W and key.min() == 0 and key.max() < B * 2 * 3 * 64
    assert fr.col_key(B, H, W, 0, 0, 8) == 64 and fr.col_key(B, H, W, 0, 8, 0) == 3 * 64 and fr.col_key(B, H, W, 1, 0, 0) == 6 * 64
    assert fr.col_key(B, H, W, 0, 1, 0) == 8 and fr.col_key(B, H, W, 0, 0, 1) == 1


def test_bf16_rne_bits_matches_torch():
    """Bit for bit against torch.tensor(x).bfloat16() on 10 000 random floats, 1 000 exact ties (odd and even upper halves), +-inf,
    +-0 and the largest finite float.  The canonical quiet NaN (0x7fc00000) is compared with torch's scalar conversion
    (torch.tensor(nan, dtype=torch.bfloat16), c10's round_to_nearest_even: 0x7fc0): the vectorised CPU cast of a float32 tensor
    returns 0xffff for every NaN on some builds, another encoding of NaN than the scalar one of the same library, so for that
    one value the tensor cast is only required to give a NaN."""
    rng = np.random.default_rng(5)
    rand = rng.integers(0, 1 << 32, 10000, dtype=np.uint64).astype(np.uint32)
    exp = (rand >> 23) & 0xFF
    rand = rand[~((exp == 0xFF) & ((rand & 0x7FFFFF) != 0))]  # NaNs with arbitrary payloads are not part of the contract
    hi = rng.integers(0, 0x7F7F, 1000).astype(np.uint32)
    hi[::2] &= ~np.uint32(1)
    hi[1::2] |= np.uint32(1)
    hi[::3] |= np.uint32(0x8000)
    ties = (hi << 16) | np.uint32(0x8000)
    special = np.array([0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7F7FFFFF], np.uint32)
    probe = fr.bf16_probe_values(rng)
    probe = probe[~np.isnan(probe)].view(np.uint32)
    assert len(rand) > 9900
    for u in (rand, ties, special, probe):
        x = np.ascontiguousarray(u).view(np.float32)
        want = torch.tensor(x).bfloat16().view(torch.int16).numpy()
        assert np.array_equal(fr.bf16_rne_bits(x).view(np.int16), want)
    assert np.sum((ties >> 16) & 1 == 1) > 300 and np.sum((ties >> 16) & 1 == 0) > 300
    qnan = np.array([0x7FC00000], np.uint32).view(np.float32)
    assert torch.tensor(qnan).bfloat16().isnan().all()
    scalar = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item() & 0xFFFF
    assert scalar == 0x7FC0 and fr.bf16_rne_bits(qnan)[0] == scalar


def test_mean_seq_is_the_sequential_float32_sum():
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((50, 7, 4)) * 1e3).astype(np.float32)
    num = rng.integers(1, 8, 50).astype(np.int32)
    for i, n in enumerate(num):
        v[i, n:] = 0
    want = np.zeros((50, 4), np.float32)
    for i in range(50):
        for d in range(4):
            a = np.float32(0.0)
            for k in range(7):
                a = np.float32(a + v[i, k, d])
            want[i, d] = np.float32(a / np.float32(num[i]))
    assert np.array_equal(fr.mean_seq(v, num), want)
