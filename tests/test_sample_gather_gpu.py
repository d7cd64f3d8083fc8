"""A batch gathered from a device-resident sample store (csrc/sample_gather.hip): ops.gather_layout is the layout pass
of ops.d4_layout reading image index[b] of a raw store, with the reference's elevation pre-processing on the way, and
ops.gather_labels the label pass with the reference's label rule.  The gather is a selection plus a permutation, so the
comparisons against the existing kernels are exact; the elevation modes are also held to a float64 computation within
the bound the project keeps for this family of kernels (tests/test_kernels_gpu.py, raw raster samples)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALL_CODES = np.arange(16, dtype=np.uint8)
N, B = 5, 7
INDEX = np.array([4, 0, 2, 2, 0, 4, 1], dtype=np.int32)  # repeats, and both ends of [0, N)
# the 16 codes over batches of 7
CODE_SETS = [ALL_CODES[0:7], ALL_CODES[7:14], np.array([14, 15, 5, 10, 0, 3, 12], dtype=np.uint8)]
KINDS = {"u8": torch.uint8, "u16": torch.uint16, "i16": torch.int16, "f32": torch.float32}


def reference_transform(arr: np.ndarray, code: int) -> np.ndarray:
    """the reference's apply_transforms (augmentations.py:25-32) for the choice a code stands for, in plain numpy"""
    if code & 1:
        arr = np.flip(arr, axis=-1)
    if code & 2:
        arr = np.flip(arr, axis=-2)
    k = (code >> 2) & 3
    if k:
        arr = np.rot90(arr, k=k, axes=(-2, -1))
    return np.ascontiguousarray(arr)


def transform_batch(x: np.ndarray, codes) -> np.ndarray:
    return np.stack([reference_transform(x[b], int(c)) for b, c in enumerate(codes)])


def reshape_label_ohe(arr: np.ndarray, num_classes: int) -> np.ndarray:
    """the reference's rule (flair_hub/data/utils_data/label.py:12-14), restated"""
    if arr.shape[0] == 1:
        arr = arr.squeeze(0)
    return np.stack([arr == i for i in range(num_classes)], axis=0)


def _samples(kind: str, shape, seed: int) -> np.ndarray:
    r = np.random.RandomState(seed)
    if kind == "u8":
        return r.randint(0, 256, shape).astype(np.uint8)
    if kind == "u16":
        return r.randint(0, 12000, shape).astype(np.uint16)
    if kind == "i16":
        return r.randint(-3000, 3000, shape).astype(np.int16)
    return (r.randn(*shape) * 100).astype(np.float32)


def _plain_layout(x, dtype, mean, std, cp):
    from flairhip import ops
    if mean is None:
        return ops.nchw_to_nhwc(x, dtype, cp)
    if x.dtype == torch.uint8:
        return ops.u8_nchw_to_nhwc(x, dtype, mean, std, cp)
    return ops.raw_nchw_to_nhwc(x, dtype, mean, std, cp)


# ---- 1. elevation = 0: the gather is d4_layout on the selected images, bit for bit ------------------------------------


@pytest.mark.parametrize("n", [24, 40])  # one 32-pixel tile; a ragged second one
@pytest.mark.parametrize("kind", list(KINDS))
def test_gather_layout_equals_d4_layout_of_the_selected_images(cuda, kind, n):
    from flairhip import ops
    base = _samples(kind, (N, 10, n, n), seed=n + len(kind))
    index = torch.from_numpy(INDEX).to(cuda)
    g = torch.Generator().manual_seed(n)
    checked = 0
    for C in (1, 5, 10):
        store = torch.from_numpy(np.ascontiguousarray(base[:, :C])).to(cuda)
        picked = torch.from_numpy(np.ascontiguousarray(base[:, :C][INDEX])).to(cuda)  # numpy: any sample type
        mean = (torch.rand(C, generator=g) * 200 + 3).to(cuda)
        std = (torch.rand(C, generator=g) * 90 + 7).to(cuda)
        for cp in (8, 16):
            if cp < C:
                continue
            for dtype in (torch.bfloat16, torch.float32):
                for norm in ((True, False) if kind == "f32" else (True,)):
                    m, s = (mean, std) if norm else (None, None)
                    for cs in CODE_SETS:
                        codes = torch.from_numpy(cs).to(cuda)
                        got = ops.gather_layout(store, index, dtype, codes, m, s, cp)
                        want = ops.d4_layout(picked, dtype, codes, m, s, cp)
                        assert got.shape == (B, n, n, cp) and got.dtype == dtype
                        if not torch.equal(got, want):
                            bad = [b for b in range(B) if not torch.equal(got[b], want[b])]
                            raise AssertionError(f"{kind} n={n} C={C} cp={cp} {dtype} norm={norm} codes {cs.tolist()}: "
                                                 f"images {bad} differ")
                        assert not got[..., C:].any(), "padding channels must stay zero"
                        checked += 1
    assert checked == 3 * (20 if kind == "f32" else 10)
    assert set(np.concatenate(CODE_SETS).tolist()) == set(range(16))


@pytest.mark.parametrize("kind", list(KINDS))
def test_gather_layout_without_codes_takes_a_plane_that_is_not_square(cuda, kind):
    """codes=None is the identity: the plain layout kernel of the sample type on the selected images, 24 x 40"""
    from flairhip import ops
    base = _samples(kind, (N, 5, 24, 40), seed=7)
    store = torch.from_numpy(base).to(cuda)
    index = torch.from_numpy(INDEX).to(cuda)
    picked = torch.from_numpy(np.ascontiguousarray(base[INDEX])).to(cuda)
    mean = torch.tensor([100.0, 90.0, 80.0, 70.0, 60.0], device=cuda)
    std = torch.tensor([50.0, 40.0, 30.0, 20.0, 10.0], device=cuda)
    for dtype in (torch.bfloat16, torch.float32):
        for norm in ((True, False) if kind == "f32" else (True,)):
            m, s = (mean, std) if norm else (None, None)
            got = ops.gather_layout(store, index, dtype, None, m, s, 8)
            assert got.shape == (B, 24, 40, 8)
            assert torch.equal(got, _plain_layout(picked, dtype, m, s, 8))
    # the streamed path: a batch of raw tensors is a store of N = B samples read with arange(B)
    ident = torch.arange(N, dtype=torch.int32, device=cuda)
    assert torch.equal(ops.gather_layout(store, ident, torch.float32, None, mean, std, 16),
                       _plain_layout(store, torch.float32, mean, std, 16))


def test_gather_layout_group_shares_index_stride_and_code_over_a_series(cuda):
    """group = T: T consecutive output images share one code (d4_layout's convention)"""
    from flairhip import ops
    T, C, n = 3, 4, 10
    base = _samples("u16", (N * T, C, n, n), 5)
    store = torch.from_numpy(base).to(cuda)
    index = torch.arange(N * T, dtype=torch.int32, device=cuda)
    codes = torch.tensor([13, 0, 6, 9, 3], dtype=torch.uint8, device=cuda)
    mean, std = torch.full((C,), 1000.0, device=cuda), torch.full((C,), 300.0, device=cuda)
    assert torch.equal(ops.gather_layout(store, index, torch.bfloat16, codes, mean, std, 16, group=T),
                       ops.d4_layout(store, torch.bfloat16, codes, mean, std, 16, group=T))


# ---- 2. the elevation modes -------------------------------------------------------------------------------------------


def _dem(kind: str, n: int) -> np.ndarray:
    """2-band elevation samples: band 0 the surface model, band 1 the terrain below it"""
    r = np.random.RandomState(n)
    if kind == "f32":
        z1 = (r.randn(N, n, n) * 50 + 300).astype(np.float32)
        z0 = (z1 + np.abs(r.randn(N, n, n)).astype(np.float32) * 10).astype(np.float32)
        return np.stack([z0, z1], axis=1)
    return _samples(kind, (N, 2, n, n), n)


@pytest.mark.parametrize("n", [12, 33])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mode", [1, 2])
def test_gather_layout_elevation_modes(cuda, mode, kind, n):
    """mode 1: the channel z0 - z1 (calc_elevation); mode 2: (z0, z0 - z1) (calc_elevation_stack_dsm).  Exactly
    d4_layout of the f32 tensor subtracted on the host, and within the family's bound of the float64 computation:
    2e-6 * scale for f32 outputs, 2^-7 * scale for bf16, scale = max(1, max |ref|)."""
    from flairhip import ops
    z = _dem(kind, n)
    store = torch.from_numpy(z).to(cuda)
    index = torch.from_numpy(INDEX).to(cuda)
    zf = z.astype(np.float32)
    diff = zf[:, 0] - zf[:, 1]  # f32, as the kernel widens the sample type
    host = np.stack([diff], axis=1) if mode == 1 else np.stack([zf[:, 0], diff], axis=1)
    zd = z.astype(np.float64)
    exact = np.stack([zd[:, 0] - zd[:, 1]], axis=1) if mode == 1 else np.stack([zd[:, 0], zd[:, 0] - zd[:, 1]], axis=1)
    c_out = mode
    mean_l, std_l = ([5.0], [8.0]) if mode == 1 else ([300.0, 5.0], [60.0, 8.0])
    mean, std = torch.tensor(mean_l, device=cuda), torch.tensor(std_l, device=cuda)
    picked = torch.from_numpy(np.ascontiguousarray(host[INDEX])).to(cuda)
    for cs in CODE_SETS:
        codes = torch.from_numpy(cs).to(cuda)
        for norm in ((True, False) if kind == "f32" else (True,)):
            m, s = (mean, std) if norm else (None, None)
            ref = exact[INDEX]
            if norm:
                ref = (ref - np.array(mean_l)[None, :, None, None]) / np.array(std_l)[None, :, None, None]
            ref = torch.from_numpy(transform_batch(ref, cs)).permute(0, 2, 3, 1)  # float64 NHWC
            scale = max(1.0, float(ref.abs().max()))
            for dtype in (torch.bfloat16, torch.float32):
                got = ops.gather_layout(store, index, dtype, codes, m, s, 8, elevation=mode)
                assert got.shape == (B, n, n, 8) and not got[..., c_out:].any()
                assert torch.equal(got, ops.d4_layout(picked, dtype, codes, m, s, 8))
                err = (got[..., :c_out].double().cpu() - ref).abs().max().item()
                tol = 2e-6 if dtype == torch.float32 else 2 ** -7
                print(f"elevation {mode} {kind} n={n} {dtype} norm={norm}: error {err:.3e}, bound {tol * scale:.3e}")
                assert err <= tol * scale


# ---- 3. labels ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [33, 70])  # 70 crosses the 64-byte label tile
@pytest.mark.parametrize("K", [1, 19, 255])
def test_gather_labels_equals_the_reference_rule(cuda, K, n):
    """argmax(reshape_label_ohe(label, K)): v < K stays v, v >= K becomes 0 (the one-hot is all false)"""
    from flairhip import ops
    raw = np.random.RandomState(n + K).randint(0, 256, (N, n, n)).astype(np.uint8)
    raw[0, 0, :4] = [0, max(K - 1, 0), min(K, 255), 255]  # both sides of the rule's edge, and the 255 of FLAIR's nodata
    rule = np.stack([reshape_label_ohe(raw[i][None], K).argmax(0) for i in range(N)]).astype(np.uint8)
    assert (rule[raw >= K] == 0).all() and (rule[raw < K] == raw[raw < K]).all() and (raw >= K).any()
    store = torch.from_numpy(raw).to(cuda)
    index = torch.from_numpy(INDEX).to(cuda)
    for cs in CODE_SETS:
        got = ops.gather_labels(store, index, K, torch.from_numpy(cs).to(cuda))
        assert got.dtype == torch.uint8 and got.shape == (B, n, n)
        assert torch.equal(got.cpu(), torch.from_numpy(transform_batch(rule[INDEX], cs)))
    assert torch.equal(ops.gather_labels(store, index, K).cpu(), torch.from_numpy(rule[INDEX]))


def test_gather_labels_without_codes_takes_a_plane_that_is_not_square(cuda):
    from flairhip import ops
    raw = np.random.RandomState(3).randint(0, 30, (N, 24, 70)).astype(np.uint8)
    got = ops.gather_labels(torch.from_numpy(raw).to(cuda), torch.from_numpy(INDEX).to(cuda), 19)
    assert torch.equal(got.cpu(), torch.from_numpy(np.where(raw < 19, raw, 0).astype(np.uint8)[INDEX]))


# ---- 4. refusals, before any launch -------------------------------------------------------------------------------------


def test_gather_ops_refuse_what_they_cannot_do(cuda):
    from flairhip import ops
    store = torch.zeros(N, 2, 8, 8, dtype=torch.uint8, device=cuda)
    labels = torch.zeros(N, 8, 8, dtype=torch.uint8, device=cuda)
    mean, std = torch.zeros(2, device=cuda), torch.ones(2, device=cuda)
    ok = torch.tensor([0, 4], dtype=torch.int32)
    codes = torch.zeros(2, dtype=torch.uint8, device=cuda)
    assert ops.gather_layout(store, ok, torch.float32, codes, mean, std).shape == (2, 8, 8, 16)  # a host index is copied
    for bad in (torch.tensor([0, N], dtype=torch.int32), torch.tensor([-1, 0], dtype=torch.int32)):
        with pytest.raises(ValueError):  # a host index is validated
            ops.gather_layout(store, bad, torch.float32, codes, mean, std)
        with pytest.raises(ValueError):
            ops.gather_labels(labels, bad, 19, codes)
    with pytest.raises(ValueError):  # int64 index
        ops.gather_layout(store, ok.long().to(cuda), torch.float32, codes, mean, std)
    with pytest.raises(ValueError):  # empty index
        ops.gather_layout(store, ok[:0].to(cuda), torch.float32, None, mean, std)
    with pytest.raises(ValueError):  # integer samples without mean / std
        ops.gather_layout(store, ok, torch.float32, codes)
    with pytest.raises(ValueError):  # rotations of a plane that is not square
        ops.gather_layout(torch.zeros(N, 2, 8, 16, device=cuda), ok, torch.float32, codes)
    with pytest.raises(ValueError):
        ops.gather_labels(torch.zeros(N, 8, 16, dtype=torch.uint8, device=cuda), ok, 19, codes)
    with pytest.raises(ValueError):  # the elevation modes need the two bands
        ops.gather_layout(torch.zeros(N, 3, 8, 8, device=cuda), ok, torch.float32, codes, elevation=1)
    with pytest.raises(ValueError):
        ops.gather_layout(store, ok, torch.float32, codes, mean, std, elevation=3)
    with pytest.raises(ValueError):  # one code per image
        ops.gather_layout(store, ok, torch.float32, torch.zeros(3, dtype=torch.uint8, device=cuda), mean, std)
    with pytest.raises(ValueError):  # a pitch that does not hold the channels / is no multiple of 8
        ops.gather_layout(store, ok, torch.float32, codes, mean, std, cp=12)
    with pytest.raises(ValueError):  # store on the host
        ops.gather_layout(store.cpu(), ok, torch.float32, None, mean, std)
    with pytest.raises(ValueError):  # a store of another sample type
        ops.gather_layout(store.double(), ok, torch.float32, None, mean, std)
    with pytest.raises(ValueError):
        ops.gather_labels(labels.float(), ok, 19)
    with pytest.raises(ValueError):
        ops.gather_labels(labels, ok, 0)
    with pytest.raises(ValueError):
        ops.gather_labels(labels, ok, 257)
