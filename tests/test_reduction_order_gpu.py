"""The summation ORDER of the reduction tails (csrc/norm_pool.hip reduce_partials / partials_fold_kernel, csrc/conv_wgrad.hip
wgrad_reduce3x3_kernel<32> / wgrad_reduce_kernel<32>), pinned bit for bit: how many loads these kernels keep in flight is
free to change, the association of their additions is not.

Finalize order.  ops._bn_finalize on hand-made partial rows with npix = 1, so that `mean` is the double sum of column 0
rounded once to f32.  The order, as the kernels state it:
  * up to 1024 rows: lane l (of 32) adds rows l, l + 32, l + 64, ... ascending in double; lane 0 then adds the 32 lane sums
    ascending in double;
  * above 1024 rows partials_fold_kernel first leaves R = 64 rows in f32: row r is the sum of the rows p = r (mod 64), taken
    by 32 lanes (lane l adds p = r + 64 (l + 32 m) for m = 0, 1, ... in f32), the lane sums then added ascending in f32; the 64
    rows then go through the order above.
Values are +-2^k, k uniform in [0, 100] from a fixed seed, and each value meets its negative on another row: partial sums
are far from exact in double (53 bits against a spread of 100), the exact total is 0 or one value, and what comes out is what
the roundings of this association left.  (Independent signs do not do it: the total then stays near 2^100, where the f32
result has an ulp of 2^77 and the associations differ by 2^48 -- the power check below failed on such inputs.)
test_the_inputs_tell_orders_apart shows on the CPU that a shuffled lane assignment gives other bits for these inputs.

Finisher order.  csrc/conv_wgrad.hip promises that wgrad_reduce3x3_kernel and wgrad_reduce_kernel agree bit for bit (same
lane / slab order); FFA_WG_REDUCE_V1=1 selects the latter for a layer that takes the former by default.

These tests pin the order, not a change: they were written next to deeper-load versions of these kernels,
passed on them and on the library of the commit before alike (run once against it), and stay although those versions were
measured no faster and are not in the tree.
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
MOM, EPS = 0.1, 1e-5
MAX_PARTIALS, FOLD_ROWS, LANES = 1024, 64, 32
ROWS = (1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 4099)
CHANNELS = (8, 40)


def _rows(rows, C):
    """[rows, 2, C] f32 of +-2^k, k in [0, 100]; per column and channel the values come as +v / -v on two rows drawn at
    random (one row is left alone when the count is odd), so that the exact sum is 0 or one value and what a kernel
    returns is what its roundings left"""
    rng = np.random.default_rng(1000 * C + rows)
    out = np.zeros((rows, 2, C), np.float64)
    for col in range(2):
        for c in range(C):
            order = rng.permutation(rows)
            v = (rng.integers(0, 2, size=rows) * 2 - 1) * np.exp2(rng.integers(0, 101, size=rows).astype(np.float64))
            half = rows // 2
            out[order[:half], col, c] = v[:half]
            out[order[half:2 * half], col, c] = -v[:half]
            if rows % 2:
                out[order[-1], col, c] = v[-1]
    return out.astype(np.float32)


def _fold(part, shuffled=False):
    """partials_fold_kernel: [n, 2, C] f32 -> [64, 2, C] f32.  shuffled: the rows of an output row are dealt to the lanes
    in another order (each lane still adds its rows ascending), for the power check"""
    n = part.shape[0]
    out = np.zeros((FOLD_ROWS,) + part.shape[1:], np.float32)
    for r in range(FOLD_ROWS):
        lanes = np.zeros((LANES,) + part.shape[1:], np.float32)
        mine = np.arange(r, n, FOLD_ROWS)
        lane_of = np.arange(mine.size) % LANES
        if shuffled:
            lane_of = np.random.default_rng(r).permutation(lane_of)
        for lane in range(LANES):
            for p in mine[lane_of == lane]:
                lanes[lane] = lanes[lane] + part[p]
        acc = np.zeros(part.shape[1:], np.float32)
        for lane in range(LANES):
            acc = acc + lanes[lane]
        out[r] = acc
    return out


def _lane_sum(part, lane_of_row=None):
    """reduce_partials: [n, 2, C] f32 (n <= 1024) -> [2, C] float64.  lane_of_row: another assignment of rows to lanes (each
    lane still adds its rows ascending), for the power check"""
    n = part.shape[0]
    assert n <= MAX_PARTIALS
    lane_of_row = np.arange(n) % LANES if lane_of_row is None else lane_of_row
    lanes = np.zeros((LANES,) + part.shape[1:], np.float64)
    for p in range(n):
        lanes[lane_of_row[p]] = lanes[lane_of_row[p]] + part[p].astype(np.float64)
    acc = np.zeros(part.shape[1:], np.float64)
    for lane in range(LANES):
        acc = acc + lanes[lane]
    return acc


def _expected_mean(part, lane_of_row=None, fold_shuffled=False):
    if part.shape[0] > MAX_PARTIALS:
        part = _fold(part, fold_shuffled)
    return _lane_sum(part, lane_of_row)[0].astype(np.float32)  # npix = 1: mean = sum / 1.0, rounded once


def test_the_inputs_tell_orders_apart():
    """from 33 rows on (below that every lane holds one row and only the lane order is left) a shuffled assignment of
    rows to lanes changes f32 bits of the mean, for both channel counts; above 1024 rows the assignment shuffled is the
    fold's (the 64 f32 rows it leaves are few and close enough for the double sum behind it to be exact in any order)"""
    for C in CHANNELS:
        for rows in ROWS:
            if rows < 33:
                continue
            part = _rows(rows, C)
            if rows > MAX_PARTIALS:
                b = _expected_mean(part, fold_shuffled=True)
            else:
                b = _expected_mean(part, np.random.default_rng(7).permutation(rows) % LANES)
            a = _expected_mean(part)
            assert not np.array_equal(a.view(np.uint32), b.view(np.uint32)), (C, rows)


def test_a_changed_lane_order_of_32_rows_is_told_apart():
    """at 31 / 32 rows the association left is the order of the 32 lane sums: descending differs from ascending"""
    for C in CHANNELS:
        for rows in (31, 32):
            part = _rows(rows, C).astype(np.float64)[:, 0]
            up, down = np.zeros(C), np.zeros(C)
            for p in range(rows):
                up, down = up + part[p], down + part[rows - 1 - p]
            assert not np.array_equal(up.astype(np.float32).view(np.uint32), down.astype(np.float32).view(np.uint32))


@gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("C", CHANNELS)
def test_bn_finalize_adds_the_partial_rows_in_the_stated_order(cuda, C, rows):
    from flairhip import ops
    part = _rows(rows, C)
    want = _expected_mean(part)
    _, _, mean, _ = ops._bn_finalize(torch.from_numpy(part).to(cuda), rows, 1, C, None, None, None, None, MOM, EPS)
    torch.cuda.synchronize()
    got = mean.cpu().numpy()
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"\nbn_finalize C={C} rows={rows}: {diff.size} of {C} channels differ from the stated order")
    assert diff.size == 0, [(int(c), float(got[c]), float(want[c])) for c in diff[:8]]


def _slabs(lib, ops, B, H, W, Co, Ci, cot, cit):
    need = lib.ffa_conv_wgrad_workspace_bytes(ops._dtype_id(torch.bfloat16), 3, 3, 1, Co, Ci, B, H, W)
    slabs, rest = divmod(need, cot * 9 * cit * 4)  # cot, cit: the channel counts padded to whole blocks
    assert need > 0 and rest == 0, need
    return slabs


# Co, Ci, B, H, W, slabs.  Co * ceil(Ci / 32) >= 512 blocks and more than 8 slabs: wgrad_reduce3x3_kernel<32> by default,
# wgrad_reduce_kernel<32> under FFA_WG_REDUCE_V1=1.
#   128 -> 128: four (co, ci) blocks of 64 x 64 per pixel tile, hence 256 / 4 = 64 slabs at the most.  B = 3, 40 x 72 has
#     45 pixel tiles of 8 x 32 and as many slabs (no multiple of 32: ragged lanes); B = 8, 64 x 128 reaches the 64 slabs
#     this layer has in the training step (two slabs per lane).
#   32 -> 512 (the widest this route gets: 64 x 32 blocks, two k groups with a slab each): 96 slabs at B = 3 (three per
#     lane, a ragged tail inside an unrolled walk of two or four), 128 at B = 4 (four per lane), 32 x 64 pixels.
WG_CASES = [(128, 128, 3, 40, 72, 45), (128, 128, 8, 64, 128, 64), (512, 32, 3, 32, 64, 96), (512, 32, 4, 32, 64, 128)]


@gpu
@pytest.mark.parametrize("Co,Ci,B,H,W,expect", WG_CASES, ids=[f"{c[1]}to{c[0]}_B{c[2]}_{c[3]}x{c[4]}" for c in WG_CASES])
def test_wgrad_finishers_agree_bit_for_bit(cuda, lib, monkeypatch, Co, Ci, B, H, W, expect):
    from flairhip import ops
    slabs = _slabs(lib, ops, B, H, W, Co, Ci, Co, Ci)
    print(f"\nwgrad {Ci}->{Co} B={B} {H}x{W}: {slabs} slabs")
    assert slabs == expect and slabs > 8 and Co * -(-Ci // 32) >= 512, slabs
    g = torch.Generator().manual_seed(B * H + W + Co)
    x = torch.randn(B, H, W, Ci, generator=g).to(torch.bfloat16).to(cuda)
    dy = torch.randn(B, H, W, Co, generator=g).to(torch.bfloat16).to(cuda)
    monkeypatch.delenv("FFA_WG_REDUCE_V1", raising=False)
    dw2 = ops.conv_wgrad(x, dy, Co, Ci, 3, 3, 1, 1)
    monkeypatch.setenv("FFA_WG_REDUCE_V1", "1")
    dw1 = ops.conv_wgrad(x, dy, Co, Ci, 3, 3, 1, 1)
    monkeypatch.delenv("FFA_WG_REDUCE_V1")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw2).all()) and float(dw2.abs().max()) > 0
    assert torch.equal(dw1, dw2), f"{int((dw1 != dw2).sum())} of {dw1.numel()} elements differ"
