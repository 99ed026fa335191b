"""The layer kernels map a workgroup to its tile with reciprocals the host
computes (tile_map / tile_of in csrc/vss_kernels.h) instead of dividing by the
grid's sizes at run time.  The library exports both halves host-only
(vss_tile_map, vss_tile_index), so the arithmetic is checked here without a
GPU: the quotient and remainder are exact, and the remapped index is the same
bijection on the grid as the division form it replaced."""
import numpy as np


def _divmod_by_reciprocal(T, d, r):
    """As tile_divmod: q = (T * r) >> 32, then one step on the remainder (T uint64 < 2^32)."""
    q = (T * np.uint64(r)) >> np.uint64(32)
    rem = T - q * np.uint64(d)
    fix = rem >= d
    return q + fix, rem - fix * np.uint64(d)


def test_reciprocal_division_is_exact(pkg):
    """T / d and T % d for every divisor 1..1024 and every T below 2^20."""
    chunks = np.arange(1 << 20, dtype=np.uint64).reshape(32, -1)  # (cache-sized pieces)
    for d in range(1, 1025):
        m = pkg.tile_map(d, 1, 1)
        assert m["gx"] == d and m["rx"] == min((1 << 32) // d, (1 << 32) - 1)
        for T in chunks:
            q, r = _divmod_by_reciprocal(T, d, m["rx"])
            # the quotient and remainder are the only pair with T = q d + r and 0 <= r < d
            assert int(r.max()) < d and np.array_equal(q * np.uint64(d) + r, T), d
        assert int(q[-1]) == ((1 << 20) - 1) // d
    # the reciprocal of gy is the same function of gy
    assert all(pkg.tile_map(1, d, 1)["ry"] == pkg.tile_map(d, 1, 1)["rx"] for d in (1, 2, 3, 7, 640, 1024))


def test_reciprocal_division_large_operands(pkg):
    """The estimate is off by at most one for every 32-bit T and any divisor: spot values up to 2^31."""
    rng = np.random.default_rng(5)
    T = np.concatenate([rng.integers(0, 1 << 31, 200000, dtype=np.uint64),
                        np.array([0, 1, (1 << 31) - 1, (1 << 31) - 2], np.uint64)])
    for d in [1, 2, 3, 5, 1023, 1025, 65535, 65537, (1 << 20) + 7, (1 << 30) - 1, (1 << 31) - 1]:
        q, r = _divmod_by_reciprocal(T, d, pkg.tile_map(d, 1, 1)["rx"])
        assert np.array_equal(q, T // np.uint64(d)) and np.array_equal(r, T % np.uint64(d)), d


def _remapped(n):
    """T of every linear workgroup index L < n, as the division form had it: L = 8 i + j below
    `full` = 8 (n >> 3) goes to j (n >> 3) + i — a transposition, so a permutation by
    construction — and the remainder keeps its place."""
    per = n >> 3
    out = _ARANGE[:n].copy()
    out[:8 * per].reshape(per, 8)[...] = _ARANGE[:8 * per].reshape(8, per).T
    return out


_ARANGE = np.arange(64 * 64 * 32, dtype=np.int32)


def test_remap_is_the_same_bijection(pkg):
    """Every grid with gx, gy <= 64 and gz <= 32 — grids of fewer than 8 workgroups (per = 0)
    and sizes that are no multiple of 8 among them: workgroup L computes tile (x, y, z) =
    (T % gx, (T / gx) % gy, T / gx / gy) of T = _remapped(n)[L], the division form's tile."""
    for n in (1, 5, 8, 13, 45, 64, 4099):  # the transposition against the kernels' former expression
        L = np.arange(n)
        assert np.array_equal(_remapped(n), np.where(L < (n >> 3 << 3), (L & 7) * (n >> 3) + (L >> 3), L))
        assert np.array_equal(np.sort(_remapped(n)), L)
    # (x, y, z) is that tile iff x + gx (y + gy z) = T with 0 <= x < gx, 0 <= y < gy, 0 <= z
    for gz in range(1, 33):
        for gy in range(1, 65):
            for gx in range(1, 65):
                x, y, z = got = pkg.tile_index(gx, gy, gz)
                assert np.array_equal((z * gy + y) * gx + x, _remapped(gx * gy * gz)), (gx, gy, gz)
                assert x.max() < gx and y.max() < gy and got.min() >= 0, (gx, gy, gz)
    m = pkg.tile_map(3, 2, 1)
    assert (m["per"], m["full"]) == (0, 0)  # fewer than 8 workgroups: every index keeps its place
    assert np.array_equal(pkg.tile_index(3, 2, 1), [[0, 1, 2, 0, 1, 2], [0, 0, 0, 1, 1, 1], [0] * 6])
    m = pkg.tile_map(5, 3, 3)
    assert (m["per"], m["full"]) == (5, 40)  # 45 workgroups: 40 remapped, 5 keep their place
