"""Change codes on the GPU (ffa_change_code_u8 in csrc/change.hip through ops.change_codes): the recode of two class
rasters through a table, compared with ``==`` against lut[np.minimum(a, K), np.minimum(b, K)]."""
import numpy as np
import pytest
import torch

from change_oracle import oracle_codes
from zone_stats_oracle import H0, W0, base_rasters

pytestmark = pytest.mark.gpu


def random_lut(K, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (K + 1, K + 1)).astype(np.uint8)


def flat_pair(n, K, seed):
    """two uint8 vectors of n values drawn in 0..K-1 with some 255 and some values just above K - 1"""
    g = np.random.default_rng(seed)
    a, b = (g.integers(0, K, n).astype(np.uint8) for _ in range(2))
    a[g.random(n) < 0.05] = 255
    b[g.random(n) < 0.05] = min(K, 255)
    return a, b


def codes(a, b, lut, **kw):
    from flairhip import ops
    out = ops.change_codes(torch.tensor(a).cuda(), torch.tensor(b).cuda(), lut, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == a.shape
    return out.cpu().numpy()


@pytest.mark.parametrize("K", [1, 19, 32])
def test_sizes_around_the_16_byte_step(cuda, K):
    lut = random_lut(K, seed=K)
    for n in (1, 15, 16, 17, H0 * W0):
        a, b = flat_pair(n, K, seed=n + K)
        assert np.array_equal(codes(a, b, lut), oracle_codes(a, b, lut)), n
    a, b = base_rasters(seed=11)[0], base_rasters(seed=12)[0]
    got = codes(a, b, torch.tensor(lut).cuda())  # a 2-D pair and a device table
    assert np.array_equal(got, oracle_codes(a, b, lut)) and got.shape == (H0, W0)


@pytest.mark.parametrize("which", ["before", "after", "out"])
@pytest.mark.parametrize("shift", [1, 3])
def test_views_at_odd_byte_offsets(cuda, which, shift):
    from flairhip import ops
    K, n = 19, 1000 + 7
    lut = random_lut(K, seed=3)
    a, b = flat_pair(n, K, seed=shift)
    off = {w: (shift if w == which else 0) for w in ("before", "after", "out")}
    d = {}
    for w, host in (("before", a), ("after", b)):
        buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        d[w] = buf[off[w]:off[w] + n]
        d[w].copy_(torch.tensor(host))
    obuf = torch.full((n + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    out = obuf[off["out"]:off["out"] + n]
    assert (d[which] if which != "out" else out).data_ptr() % 16 == shift  # the allocator aligns the buffers
    res = ops.change_codes(d["before"], d["after"], lut, out=out)
    torch.cuda.synchronize()
    assert res is out and np.array_equal(out.cpu().numpy(), oracle_codes(a, b, lut))
    rest = obuf.cpu().numpy()
    assert (rest[:off["out"]] == 0xEE).all() and (rest[off["out"] + n:] == 0xEE).all()  # nothing beyond the view


def test_in_place_and_refused_overlaps(cuda):
    from flairhip import ops
    K = 19
    lut = random_lut(K, seed=9)
    a, b = base_rasters(seed=11)[0], base_rasters(seed=12)[0]
    want = oracle_codes(a, b, lut)
    d_a, d_b = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    assert ops.change_codes(d_a, d_b, lut, out=d_b) is d_b
    assert np.array_equal(d_b.cpu().numpy(), want) and np.array_equal(d_a.cpu().numpy(), a)
    d_b = torch.tensor(b).cuda()
    ops.change_codes(d_a, d_b, lut, out=d_a)
    assert np.array_equal(d_a.cpu().numpy(), want) and np.array_equal(d_b.cpu().numpy(), b)
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        ops.change_codes(buf[:32], buf[32:], lut, out=buf[16:48])
    with pytest.raises(ValueError, match="lut"):
        ops.change_codes(buf[:32], buf[32:], np.zeros((34, 34), np.uint8))
    with pytest.raises(ValueError, match="lut"):
        ops.change_codes(buf[:32], buf[32:], np.zeros((1, 1), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ops.change_codes(buf[:32].to(torch.int32), buf[32:], lut)


def test_transition_tables(cuda):
    from flair_zonal_detection.change import transition_lut
    a, b = base_rasters(seed=11)[0], base_rasters(seed=12)[0]
    lut, specs = transition_lut(None, 19)
    got = codes(a, b, lut)
    assert np.array_equal(got, oracle_codes(a, b, lut))
    changed = (a != b) & (a < 19) & (b < 19)
    assert np.array_equal(got[changed], b[changed]) and (got[~changed] == 255).all() and changed.sum() > 10000
    # overlapping specs: the earlier one wins
    lut, specs = transition_lut(["*:6", "4:*", "4:6", "*:*"], 19)
    got = codes(a, b, lut)
    assert np.array_equal(got, oracle_codes(a, b, lut))
    assert (got[changed & (b == 6)] == 0).all() and (got[changed & (a == 4) & (b != 6)] == 1).all()
    assert not (got == 2).any() and (got[changed & (a != 4) & (b != 6)] == 3).all()
    assert (changed & (a == 4) & (b == 6)).sum() > 0
