"""ffa_eval_stats (csrc/eval_stats.hip) through ops.eval_stats: labels, confusion counts, per-class pixel counts and
per-class sums of -log softmax[target] from one pass over the logits, against float64 on the very bytes the kernel read.

Inputs: seeded 4 * randn logits stored in the tensor's dtype; about 2 % of the pixels carry an exact two-way tie at the
maximum; about 3 % of the targets are 255 (ignored) and the last class never occurs as a target (for K > 1).
Shapes: 1, 63, 255, 257 and 4099 pixels (one lane, a ragged wave, a ragged tile, two tiles, several blocks) and
2 x 363 x 363 = 263 538 pixels, the smallest batch of squares above the kernel's grid cap of 1024 blocks x 256 threads,
where blocks walk more than one tile.  K / pitch: 1/8, 13/16, 19/32, 32/32 -- one per size of the kernel's LDS column.
class_nll is held to the bound the project holds ffa_softmax_ce's loss to: REL * sum (|lse| + |z_t|) (tests/insitu.py).
"""
import functools

import pytest
import torch

from insitu import REL

pytestmark = pytest.mark.gpu

F64 = torch.float64
NPIX = [1, 63, 255, 257, 4099, 2 * 363 * 363]
CLASSES = [(1, 8), (13, 16), (19, 32), (32, 32)]
DTYPES = [torch.bfloat16, torch.float32]


def first_max(z64):
    """index of the first maximum over the last axis, without relying on argmax's choice among ties"""
    k = z64.shape[-1]
    idx = torch.arange(k, device=z64.device).expand_as(z64)
    return torch.where(z64 == z64.max(-1, keepdim=True).values, idx, k).min(-1).values


@functools.lru_cache(maxsize=None)
def case(npix, K, cp, dtype):
    """inputs on the GPU and their float64 reference, built once and shared: nobody writes to them"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * npix % 9973 + 37 * K + cp + (dtype == torch.float32))
    z = (4.0 * torch.randn(npix, cp, generator=g)).to(dtype)
    if K > 1:  # planted ties: two distinct classes share the pixel's maximum, as stored
        n_tie = max(1, npix // 50)
        rows = torch.randperm(npix, generator=g)[:n_tie]
        a = torch.randint(0, K, (n_tie,), generator=g)
        b = (a + 1 + torch.randint(0, K - 1, (n_tie,), generator=g)) % K
        top = (z[rows, :K].float().max(-1).values + 1.0).to(dtype)
        z[rows, a] = top
        z[rows, b] = top
    t = torch.randint(0, max(K - 1, 1), (npix,), generator=g).to(torch.uint8)  # class K - 1 is absent (K > 1)
    t[torch.rand(npix, generator=g) < 0.03] = 255
    shape = (2, 363, 363) if npix == 2 * 363 * 363 else (1, 1, npix)
    z, t = z.reshape(*shape, cp).to(dev), t.reshape(shape).to(dev)
    z64 = z[..., :K].to(F64).reshape(npix, K)
    tl = t.reshape(-1).long()
    valid = tl < K
    tc = tl.clamp(max=K - 1)
    lse = torch.logsumexp(z64, -1)
    zt = z64.gather(1, tc[:, None])[:, 0]
    pred = first_max(z64)
    onehot = torch.zeros(npix, K, dtype=F64, device=dev)
    onehot[valid, tc[valid]] = 1.0
    ref = {"pred": pred.to(torch.uint8).reshape(shape),
           "nll": (onehot * (lse - zt)[:, None]).sum(0), "mag": (onehot * (lse.abs() + zt.abs())[:, None]).sum(0),
           "count": onehot.sum(0).long(),
           "confmat": torch.bincount(tc[valid] * K + pred[valid], minlength=K * K).reshape(K, K),
           "ties": int(((z64 == z64.max(-1, keepdim=True).values).sum(-1) > 1).sum())}
    return z, t, ref


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("K,cp", CLASSES)
@pytest.mark.parametrize("npix", NPIX)
def test_every_output_against_float64(cuda, npix, K, cp, dtype):
    from flairhip import ops
    z, t, ref = case(npix, K, cp, dtype)
    if K > 1:
        assert ref["ties"] >= 1  # the planted ties are there
    before = torch.arange(K * K, dtype=torch.int64, device=cuda).reshape(K, K) * 3
    cm = before.clone()
    pred, nll, cnt = ops.eval_stats(z, t, K, confmat=cm)
    assert pred.dtype == torch.uint8 and pred.shape == t.shape and torch.equal(pred, ref["pred"])
    _, _, _, ce_pred = ops.softmax_ce(z, t, torch.ones(K, device=cuda), K, want_pred=True)
    assert same(pred, ce_pred)
    assert torch.equal(cm, before + ref["confmat"])
    assert cnt.dtype == torch.int64 and torch.equal(cnt, ref["confmat"].sum(1)) and torch.equal(cnt, ref["count"])
    assert nll.dtype == F64 and nll.shape == (K,)
    err, tol = (nll - ref["nll"]).abs(), REL * ref["mag"]
    print(f"class_nll: worst error / bound = {(err / tol.clamp(min=1e-300)).max().item():.3e}")
    assert bool((err <= tol).all()), (err, tol)
    if K > 1:  # the absent class: exactly nothing
        assert nll[K - 1].item() == 0.0 and cnt[K - 1].item() == 0
    # a second call accumulates into confmat, overwrites the rest with the same bytes
    pred2, nll2, cnt2 = ops.eval_stats(z, t, K, confmat=cm)
    assert torch.equal(cm, before + 2 * ref["confmat"])
    assert same(pred, pred2) and same(nll, nll2) and same(cnt, cnt2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("npix,K,cp", [(4099, 19, 32), (2 * 363 * 363, 13, 16)])
def test_weighted_sum_of_the_class_losses_is_the_loss_of_softmax_ce(cuda, npix, K, cp, dtype):
    from flairhip import ops
    z, t, ref = case(npix, K, cp, dtype)
    w = torch.linspace(0.5, 2.0, K, dtype=torch.float32, device=cuda)
    w[2] = 0.0
    loss, _, _, _ = ops.softmax_ce(z, t, w, K)
    _, nll, cnt = ops.eval_stats(z, t, K, want_pred=False)
    w64 = w.to(F64)
    wsum = (w64 * ref["count"]).sum()
    mine = (w64 * nll).sum() / (w64 * cnt).sum()
    tol = 2 * REL * (w64 * ref["mag"]).sum() / wsum  # the bound of either side, once each
    print(f"loss {loss.item():.9f} from class sums {mine.item():.9f} bound {tol.item():.3e}")
    assert abs(loss.to(F64).item() - mine.item()) <= tol.item()
    assert abs(mine.item() - ((w64 * ref["nll"]).sum() / wsum).item()) <= tol.item() / 2


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_skipped_outputs_leave_the_others_unchanged(cuda, dtype):
    from flairhip import ops
    K, cp = 19, 32
    z, t, ref = case(4099, K, cp, dtype)
    cm = torch.zeros(K, K, dtype=torch.int64, device=cuda)
    pred, nll, cnt = ops.eval_stats(z, t, K, confmat=cm)
    cm_a = torch.zeros_like(cm)
    p, n, c = ops.eval_stats(z, t, K, confmat=cm_a, want_pred=False)
    assert p is None and same(n, nll) and same(c, cnt) and same(cm_a, cm)
    p, n, c = ops.eval_stats(z, t, K, confmat=None)
    assert same(p, pred) and same(n, nll) and same(c, cnt)
    cm_b = torch.zeros_like(cm)
    p, n, c = ops.eval_stats(z, t, K, confmat=cm_b, want_class_nll=False)
    assert n is None and c is None and same(p, pred) and same(cm_b, cm)
    p, n, c = ops.eval_stats(z, t, K, want_class_nll=False)  # the label alone
    assert n is None and c is None and same(p, pred)
    assert ops.eval_stats(z, t, K, want_pred=False, want_class_nll=False) == (None, None, None)


def test_targets_at_an_odd_address(cuda):
    """the kernel reads targets and writes labels byte by byte: a slice one byte into a buffer gives the same results"""
    from flairhip import ops
    K, cp = 13, 16
    z, t, ref = case(4099, K, cp, torch.bfloat16)
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=cuda)
    buf[1:] = t.reshape(-1)
    off = buf[1:].reshape(t.shape)
    assert off.data_ptr() % 2 == 1 and off.is_contiguous()
    cm, cm_off = (torch.zeros(K, K, dtype=torch.int64, device=cuda) for _ in range(2))
    a = ops.eval_stats(z, t, K, confmat=cm)
    b = ops.eval_stats(z, off, K, confmat=cm_off)
    assert all(same(x, y) for x, y in zip(a, b)) and same(cm, cm_off)
    assert torch.equal(cm, ref["confmat"])


def test_no_pixels_gives_zeros(cuda):
    from flairhip import ops
    K = 5
    z = torch.empty(1, 1, 0, 8, dtype=torch.float32, device=cuda)
    t = torch.empty(1, 1, 0, dtype=torch.uint8, device=cuda)
    cm = torch.full((K, K), 7, dtype=torch.int64, device=cuda)
    pred, nll, cnt = ops.eval_stats(z, t, K, confmat=cm)
    assert pred.numel() == 0 and bool((cm == 7).all())
    assert torch.equal(nll, torch.zeros(K, dtype=F64, device=cuda)) and not bool(cnt.any())


def test_refused_calls_do_not_launch(cuda, lib):
    from flairhip import lib as L
    from flairhip import ops
    z, t, _ = case(257, 19, 32, torch.float32)
    with pytest.raises(L.FlairHipError):
        ops.eval_stats(z, t, 33)                                    # K beyond the kernels' 32
    with pytest.raises(L.FlairHipError):
        ops.eval_stats(z[..., :16].contiguous(), t, 19)             # pitch below K
    z12 = torch.zeros(1, 1, 257, 12, dtype=torch.float32, device=cuda)
    with pytest.raises(L.FlairHipError):
        ops.eval_stats(z12, t, 4)                                   # pitch not a multiple of 8
    with pytest.raises(ValueError):
        ops.eval_stats(z, t.long(), 19)
    with pytest.raises(ValueError):
        ops.eval_stats(z, t[..., :100].contiguous(), 19)
    with pytest.raises(ValueError):
        ops.eval_stats(z.permute(0, 1, 3, 2), t, 19)                 # not contiguous
    for bad in (torch.zeros(19, 19, dtype=torch.int32, device=cuda), torch.zeros(18, 19, dtype=torch.int64, device=cuda),
                torch.zeros(19, 19, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops.eval_stats(z, t, 19, confmat=bad)
    # the library's own checks: nothing is written
    pred = torch.full((257,), 0xAB, dtype=torch.uint8, device=cuda)
    cm = torch.full((32 * 32,), -5, dtype=torch.int64, device=cuda)
    nll = torch.full((32,), -1.0, dtype=F64, device=cuda)
    cnt = torch.full((32,), -3, dtype=torch.int64, device=cuda)
    ws = torch.empty(lib.ffa_eval_stats_workspace_bytes(), dtype=torch.uint8, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    tail = (pred.data_ptr(), cm.data_ptr(), nll.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), s)
    for K, cp in ((33, 40), (33, 32), (4, 12), (19, 16), (0, 8)):
        assert lib.ffa_eval_stats(L.F32, z.data_ptr(), t.data_ptr(), 257, K, cp, *tail) == -1, (K, cp)
        assert b"eval_stats" in lib.ffa_last_error()
    assert lib.ffa_eval_stats(L.F32, z.data_ptr(), t.data_ptr(), 257, 19, 32, pred.data_ptr(), cm.data_ptr(),
                              nll.data_ptr(), None, ws.data_ptr(), ws.numel(), s) == -1   # half of the pair
    assert lib.ffa_eval_stats(L.F32, z.data_ptr(), t.data_ptr(), 257, 19, 32, pred.data_ptr(), cm.data_ptr(),
                              nll.data_ptr(), cnt.data_ptr(), ws.data_ptr(), 16, s) == -3  # FFA_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((pred == 0xAB).all()) and bool((cm == -5).all()) and bool((nll == -1.0).all()) and bool((cnt == -3).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_one_call_captured_in_a_graph_replays_the_eager_bytes(cuda, dtype):
    from flairhip import ops
    K, cp = 19, 32
    z, t, ref = case(4099, K, cp, dtype)
    eager_cm = torch.zeros(K, K, dtype=torch.int64, device=cuda)
    pred, nll, cnt = ops.eval_stats(z, t, K, confmat=eager_cm)  # also sizes the workspace before the capture
    cm = torch.zeros_like(eager_cm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.eval_stats(z, t, K, confmat=cm)
    for n in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        assert same(out[0], pred) and same(out[1], nll) and same(out[2], cnt)
        assert torch.equal(cm, n * eager_cm)
