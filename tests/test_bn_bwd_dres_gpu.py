"""ffa_bn_bwd in relu mode 1 with a residual gradient (the bn2 of a BasicBlock): the reduction pass leaves the masked
gradient g = dy * (y > 0) in dres and the apply pass reads x and dres only (csrc/norm_pool.hip, BnBwdStoreOp).

Per storage type and channel count, at the pixel counts 1, 7, 16 PL + 1 (three blocks, the last with one pixel) and
3 PL U - 1 / + 1 (the tail guard on either side of a full iteration; PL = 256 / (C / 8) pixel lanes, U = 4 (bf16) or 2 (f32)
vectors in flight):
  * the call goes through Checker.bn_bwd of tests/insitu.py (float64 reference, its bounds, no tolerance of this file);
  * dres is exactly dy * (y > 0);
  * dx, dgamma, dbeta equal, bit for bit, those of the same call without dres -- which still reads dy and y in the apply
    pass, the data path this one replaces;
  * stages 4 (reduction), 8 (finalize), 2 (apply) issued as three ffa_bn_bwd_stages calls give the outputs of the one call;
  * dres aliasing dy (in place) gives the outputs of the call with a buffer of its own.
C = 8 and 2048 take the chunked walk of the apply pass (256 % (C / 8) == 0), C = 24 the grid-stride walk with an idle
lane in the reduction, C = 64 is the step's own smallest residual layer.
"""
import pytest
import torch

from insitu import Checker
from test_norm_pool_edges_gpu import _call, _forward64, _geometry, _inputs, _stats64

gpu = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def _pixel_counts(C, dtype):
    _, PL, U = _geometry(C, dtype)
    return sorted({1, 7, 16 * PL + 1, 3 * PL * U - 1, 3 * PL * U + 1})


def _stages(ops, L, c, y, mean, rstd, dres, stage_calls):
    """ffa_bn_bwd_stages once per entry of stage_calls, mode 1 -> dx, dgamma, dbeta"""
    lib = L.load()
    x, C = c["x"], c["C"]
    dx = torch.empty_like(x)
    dgb = torch.empty((2, C), dtype=F32, device=x.device)
    ws = ops.workspace(lib.ffa_bn_workspace_bytes(C), x.device, "bn")
    for st in stage_calls:
        L.check(lib.ffa_bn_bwd_stages(ops._dt(x), x.data_ptr(), c["dy"].data_ptr(), y.data_ptr(), c["gamma"].data_ptr(),
                                      c["beta"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                      dres.data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(), x.numel() // C, C, 1,
                                      ws.data_ptr(), ws.numel(), st, ops._stream()), "bn_bwd")
    torch.cuda.synchronize()
    return dx, dgb[0], dgb[1]


@gpu
@pytest.mark.parametrize("C", [8, 24, 64, 2048])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_bn_bwd_with_residual_gradient(cuda, C, dtype):
    from flairhip import lib as L
    from flairhip import ops
    ck = Checker("full", chunk=1)
    counts = _pixel_counts(C, dtype)
    for npix in counts:
        c = _inputs(C, npix, dtype, seed=C + npix + 11, large_mean=dtype == F32, device=cuda)
        mean, rstd, scale, shift = _stats64(c["x"], c["gamma"], c["beta"])
        y = _forward64(c["x"], scale, shift, c["res"], dtype)
        dy0 = c["dy"].clone()
        dx, dres, dgamma, dbeta = ops.bn_bwd(c["x"], c["dy"], y, c["gamma"], c["beta"], mean, rstd, True, True)
        torch.cuda.synchronize()
        assert torch.equal(c["dy"], dy0), "the call changed dy"
        ck.bn_bwd(_call("bn_bwd", C, npix, mode=1), c["x"], c["dy"], y, c["gamma"], c["beta"], mean, rstd, True, dx, dres,
                  dgamma, dbeta)
        g = torch.where(y > 0, c["dy"], torch.zeros_like(c["dy"]))
        assert torch.equal(dres, g), f"npix={npix}: dres is not dy * (y > 0)"

        dx0, none, dgamma0, dbeta0 = ops.bn_bwd(c["x"], c["dy"], y, c["gamma"], c["beta"], mean, rstd, True, False)
        torch.cuda.synchronize()
        assert none is None
        for name, a, b in (("dx", dx, dx0), ("dgamma", dgamma, dgamma0), ("dbeta", dbeta, dbeta0)):
            assert torch.equal(a, b), f"npix={npix}: {name} differs from the call without dres"

        dres3 = torch.full_like(c["x"], 3.0)
        dx3, dgamma3, dbeta3 = _stages(ops, L, c, y, mean, rstd, dres3, (4, 8, 2))
        for name, a, b in (("dx", dx, dx3), ("dres", dres, dres3), ("dgamma", dgamma, dgamma3), ("dbeta", dbeta, dbeta3)):
            assert torch.equal(a, b), f"npix={npix}: {name} differs between one call and stages 4, 8, 2"

        inplace = dict(c, dy=c["dy"].clone())
        dxa, dgammaa, dbetaa = _stages(ops, L, inplace, y, mean, rstd, inplace["dy"], (3,))
        for name, a, b in (("dx", dx, dxa), ("dres", dres, inplace["dy"]), ("dgamma", dgamma, dgammaa),
                           ("dbeta", dbeta, dbetaa)):
            assert torch.equal(a, b), f"npix={npix}: {name} differs when dres aliases dy"
    bad = [f"{r.get('case')}: {r.line()}" for r in ck.results if not r.ok]
    worst = max(ck.results, key=lambda r: r["worst"])
    print(f"\nbn_bwd mode 1 + dres C={C}: {len(ck.results)} checks, worst {worst.get('case')}: {worst.line()}")
    assert len(ck.results) == 4 * len(counts), len(ck.results)
    assert not bad, bad[:20]


@gpu
def test_dres_overlapping_an_input_is_refused(cuda):
    """dres may be dy itself; x, y, dx or a shifted view of dy are argument errors, and nothing is launched"""
    from flairhip import lib as L
    from flairhip import ops
    C, npix = 8, 64
    c = _inputs(C, npix, F32, seed=5, device=cuda)
    mean, rstd, scale, shift = _stats64(c["x"], c["gamma"], c["beta"])
    y = _forward64(c["x"], scale, shift, c["res"], F32)
    big = torch.zeros(2 * npix * C, device=cuda)
    shifted = dict(c, dy=big[: npix * C].view_as(c["x"]))
    for case, dres in ((c, c["x"]), (c, y), (shifted, big[8: npix * C + 8])):
        with pytest.raises(L.FlairHipError):
            _stages(ops, L, case, y, mean, rstd, dres, (3,))
