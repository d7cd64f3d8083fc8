"""flairhip.operands on CPU tensors: what makes a cached operand stale, and what does not."""
import pytest
import torch

from flairhip.nn import HipBatchNorm2d
from flairhip.operands import OperandCache, bump_state_epoch


class _Counting:
    """build closure that counts its calls and returns a new object each time"""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


@pytest.fixture
def setup():
    """(cache, request() -> value, build, sources, bn): one entry over a weight, an optional (absent) scale, a bias and
    a BatchNorm, already built once"""
    cache, build = OperandCache(), _Counting()
    src = {"w": torch.ones(4, 3), "b": torch.zeros(4), "extra": (torch.bfloat16,)}
    bn = HipBatchNorm2d(4)

    def request():
        return cache.get("k", src["w"], None, src["b"], bn=bn, build=build, extra=src["extra"])
    first = request()
    assert build.calls == 1
    return cache, request, build, src, bn, first


def test_unchanged_sources_return_the_cached_object(setup):
    _, request, build, _, _, first = setup
    assert request() is first and request() is first
    assert build.calls == 1


def _write_weight(src, bn):
    src["w"].mul_(2.0)


def _write_bias(src, bn):
    src["b"].add_(1.0)


def _replace_weight(src, bn):
    src["w"] = src["w"].clone()  # equal contents, another address


def _replace_bias(src, bn):
    src["b"] = src["b"].clone()


def _epoch(src, bn):
    bump_state_epoch()


def _note_batch(src, bn):
    bn.note_batch()


def _write_running_var(src, bn):
    bn.running_var.mul_(0.5)


def _write_running_mean(src, bn):
    bn.running_mean.add_(0.25)


def _write_bn_weight(src, bn):
    with torch.no_grad():
        bn.weight.mul_(3.0)


def _write_bn_bias(src, bn):
    with torch.no_grad():
        bn.bias.add_(1.0)


def _other_extra(src, bn):
    src["extra"] = (torch.float32,)


@pytest.mark.parametrize("change", [_write_weight, _write_bias, _replace_weight, _replace_bias, _epoch, _note_batch,
                                    _write_running_var, _write_running_mean, _write_bn_weight, _write_bn_bias,
                                    _other_extra], ids=lambda f: f.__name__.lstrip("_"))
def test_each_change_alone_triggers_exactly_one_rebuild(setup, change):
    _, request, build, src, bn, first = setup
    change(src, bn)
    second = request()
    assert second is not first and build.calls == 2
    assert request() is second and build.calls == 2


@pytest.mark.parametrize("foreach", [True, False])
def test_an_optimizer_step_makes_the_entry_stale(foreach):
    """the fused-optimizer rule: torch's fused kernels leave ``_version`` alone, so the step hook must do it for any
    optimizer (checked here through the state epoch, which a version-only stamp would not see)"""
    from flairhip.operands import state_epoch
    p = torch.nn.Parameter(torch.ones(8))
    cache, build = OperandCache(), _Counting()
    first = cache.get("k", p, build=build)
    p.grad = torch.ones(8)
    before = state_epoch()
    torch.optim.AdamW([p], lr=1e-2, foreach=foreach).step()
    assert state_epoch() == before + 1
    assert cache.get("k", p, build=build) is not first and build.calls == 2


def test_entries_with_different_keys_never_share_a_value():
    w = torch.ones(4)
    cache, build = OperandCache(), _Counting()
    keys = [(torch.bfloat16, False, (True, False, False)), (torch.bfloat16, False, (False, False, False)),
            (torch.bfloat16, True, (True, False, False)), (torch.float32, False, (True, False, False)), "name"]
    values = [cache.get(k, w, build=build) for k in keys]
    assert build.calls == len(keys) and len({id(v) for v in values}) == len(keys)
    assert [cache.get(k, w, build=build) for k in reversed(keys)] == values[::-1]
    assert build.calls == len(keys)


def test_restamp_makes_a_stale_entry_current_without_building(setup):
    cache, request, build, src, bn, first = setup
    entry = cache.entries["k"]
    assert entry.current()
    src["w"].mul_(2.0)
    bump_state_epoch()
    bn.note_batch()
    assert not entry.current()
    entry.restamp()
    assert entry.current()
    assert request() is first and build.calls == 1


def test_repack_mark_is_kept_with_the_entry():
    w = torch.ones(4)
    cache = OperandCache()
    cache.get("whole", w, build=object, repack=(False,))
    cache.get("block", w, build=object, repack=(True, (2, 2)))
    cache.get("folded", w, torch.ones(4), build=object)
    assert {k: e.repack for k, e in cache.entries.items()} == {"whole": (False,), "block": (True, (2, 2)),
                                                               "folded": None}
    assert all(e.sources[0] is w for e in cache.entries.values())
