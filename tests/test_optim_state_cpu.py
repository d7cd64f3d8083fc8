"""flairhip.optim.HipAdamW / HipAdam: loading a state that torch's optimizer saved.  The constructor and load_state_dict()
need no GPU (only step() does), so the layout they must leave behind is checked here: the kernel reads ``step`` through a
device pointer, and ``torch.optim.Optimizer.load_state_dict`` leaves a default optimizer's ``step`` -- a CPU tensor, or a
Python number in checkpoints of older versions -- where it was and takes ``capturable: False`` from the saved groups."""
import copy

import pytest
import torch

from helpers import ROOT  # noqa: F401  (sets sys.path)

SHAPES = [(4, 3), (7,), (1,), (2, 3, 3, 3)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).requires_grad_() for s in SHAPES]


def _torch_state(kind, steps=3):
    """the state dict of a default torch.optim.AdamW / Adam (not fused, not capturable) after three steps"""
    ps = _params(1)
    opt = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(ps, lr=2e-3, betas=(0.9, 0.95), weight_decay=0.02)
    g = torch.Generator().manual_seed(2)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    sd = opt.state_dict()
    assert sd["param_groups"][0]["capturable"] is False and sd["state"][0]["step"].device.type == "cpu"
    return copy.deepcopy(sd), ps


def _with_step_as(sd, how):
    sd = copy.deepcopy(sd)
    for st in sd["state"].values():
        if how == "python-float":
            st["step"] = float(st["step"])
        elif how == "f64-tensor":
            st["step"] = st["step"].to(torch.float64)
        elif how == "one-element-tensor":
            st["step"] = st["step"].reshape(1)
    return sd


@pytest.mark.parametrize("how", ["cpu-tensor", "python-float", "f64-tensor", "one-element-tensor"])
@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_a_default_torch_state_loads_into_the_device_layout(kind, how):
    from flairhip.optim import HipAdam, HipAdamW
    saved, ref_ps = _torch_state(kind)
    sd = _with_step_as(saved, how)
    ps = [p.detach().clone().requires_grad_() for p in ref_ps]
    ours = (HipAdamW if kind == "adamw" else HipAdam)(ps, lr=1.0)
    ours.load_state_dict(sd)
    for grp in ours.param_groups:
        assert grp["capturable"] is True
        assert grp["lr"] == 2e-3 and grp["betas"] == (0.9, 0.95) and grp["weight_decay"] == 0.02
        assert grp["decoupled_weight_decay"] is (kind == "adamw") and grp["amsgrad"] is False
    assert len(ours.state) == len(ps)
    for i, p in enumerate(ps):
        st = ours.state[p]
        assert torch.is_tensor(st["step"]) and st["step"].dim() == 0 and st["step"].dtype == torch.float32
        assert st["step"].device == p.device and float(st["step"]) == 3.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == torch.float32 and st[k].device == p.device and st[k].shape == p.shape
            assert st[k].is_contiguous() and torch.equal(st[k], saved["state"][i][k])
        # the loaded counter is the optimizer's own: stepping must not move the caller's dict
        if torch.is_tensor(sd["state"][i]["step"]):
            assert st["step"].data_ptr() != sd["state"][i]["step"].data_ptr()
    # and back: torch's optimizer takes state_dict() of the result and steps like the optimizer the state came from.
    # (``capturable`` describes where the step counters live; torch's CPU implementation refuses the flag, so the way
    # back to a CPU optimizer clears it, as loading a GPU checkpoint into a CPU torch optimizer always requires.)
    back = copy.deepcopy(ours.state_dict())
    for grp in back["param_groups"]:
        grp["capturable"] = False
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    qs = [p.detach().clone().requires_grad_() for p in ref_ps]
    again = cls(qs, lr=1.0)
    again.load_state_dict(back)
    cont = cls(ref_ps, lr=1.0)
    cont.load_state_dict(saved)
    g = torch.Generator().manual_seed(3)
    for p, q in zip(ref_ps, qs):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    again.step()
    cont.step()
    for p, q in zip(ref_ps, qs):
        assert torch.equal(p, q)
        assert float(again.state[q]["step"]) == 4.0


def test_a_device_lr_keeps_its_identity_and_takes_the_loaded_value():
    from flairhip.optim import HipAdamW
    saved, ref_ps = _torch_state("adamw")
    ps = [p.detach().clone().requires_grad_() for p in ref_ps]
    lr = torch.tensor(0.5, dtype=torch.float32)
    ours = HipAdamW(ps, lr=lr)
    ours.load_state_dict(saved)
    assert ours.param_groups[0]["lr"] is lr and float(lr) == float(torch.tensor(2e-3, dtype=torch.float32))
    # a tensor lr in the loaded groups where a number was held becomes a number (no tensor of another device slips in)
    sd = copy.deepcopy(saved)
    sd["param_groups"][0]["lr"] = torch.tensor(4e-3, dtype=torch.float64)
    ours = HipAdamW(ps, lr=1.0)
    ours.load_state_dict(sd)
    assert isinstance(ours.param_groups[0]["lr"], float) and ours.param_groups[0]["lr"] == 4e-3


def test_amsgrad_states_are_refused_and_our_own_state_dict_loads_unchanged():
    from flairhip.optim import HipAdamW
    saved, ref_ps = _torch_state("adamw")
    ps = [p.detach().clone().requires_grad_() for p in ref_ps]
    bad = copy.deepcopy(saved)
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(NotImplementedError):
        HipAdamW(ps).load_state_dict(bad)
    a = HipAdamW(ps)
    a.load_state_dict(saved)
    b = HipAdamW(ps)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for p in ps:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a.state[p][k], b.state[p][k]) and a.state[p][k].dtype == b.state[p][k].dtype
    assert b.param_groups[0]["capturable"] is True


def test_step_refuses_a_state_on_the_host_before_it_reaches_the_library():
    """CPU parameters are refused first (there is no CPU path); the state check itself is exercised on its own"""
    from flairhip.optim import HipAdamW
    p = torch.zeros(5, requires_grad=True)
    good = {"step": torch.zeros(()), "exp_avg": torch.zeros(5), "exp_avg_sq": torch.zeros(5)}
    HipAdamW._check_state(p, good)
    for key, value in (("step", 3.0), ("step", torch.zeros((), dtype=torch.float64)),
                       ("exp_avg", torch.zeros(5, dtype=torch.bfloat16)), ("exp_avg_sq", None),
                       ("step", torch.zeros((), device="meta"))):
        with pytest.raises(TypeError, match=key):
            HipAdamW._check_state(p, dict(good, **{key: value}))
    with pytest.raises(ValueError):
        HipAdamW._check_state(p, dict(good, exp_avg=torch.zeros(4)))
    with pytest.raises(ValueError):
        HipAdamW._check_state(p, dict(good, exp_avg_sq=torch.zeros(10)[::2]))
