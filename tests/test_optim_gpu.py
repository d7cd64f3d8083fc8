"""flairhip.optim.HipAdamW / HipAdam (csrc/optim.hip, ffa_adamw_multi) against torch.optim.AdamW / Adam -- the optimizer
the reference constructs at flair_hub/tasks/tasks_module.py:385-389 -- on the GPU box: same trajectory, same state.

And against float64: Checker.adamw of tests/insitu.py restates the update of csrc/optim.hip from the f32 p, g, m, v, lr and
step the kernel received and holds p, exp_avg and exp_avg_sq to it per element, within a bound made of the kernel's own
rounding points (ulp + 8 x 2^-24 x the magnitudes, the errors of m, v and the denominator carried into p; derived in
Checker.adamw's docstring, emulated and attacked with mutants on the CPU in tests/test_insitu_checker.py).  Cases: decoupled x
maximize x weight decay {0, 0.02} x eps {1e-8, 1e-3}; tensors of 1, 4095, 4096, 4097, 8192 and 12289 elements; descriptor
tables of 72, 73, 144 and 145 tensors with multi-block tensors at their ends, in the middle and in every launch; p, g or the
moments alone at element offsets 1, 2, 3; two param_groups; skipped steps and a state loaded at step 1000; lr on the device;
a captured step replayed with lr rewritten in between; vector and scalar path bit for bit; a state that a default
torch.optim.AdamW / Adam saved (step counters on the host, capturable: False), loaded from disk and continued for two steps; a
hand-assigned host state refused before any launch.  Gradients span 1e-9 .. 10 per
element with exact zeros, so eps decides some quotients and not others.
One MI355X run (37 tests, 6.6 s): largest error as a fraction of the bound over all cases (f32 only):
  adamw_multi_kernel   p 0.199   exp_avg 0.288   exp_avg_sq 0.341
The f32 emulation on the CPU gives p 0.196, exp_avg 0.272, exp_avg_sq 0.250 over steps 1 .. 1e5.  No case exceeded its bound;
no kernel bug was found."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _params(cuda, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(64, 5, 7, 7), (64,), (128, 64, 3, 3), (19,), (4097,), (3, 4096), (1,), (256, 128, 3, 3), (33, 17)]
    shapes += [(7,)] * 80  # more tensors than one launch's descriptor table holds (72)
    ps = [torch.randn(*s, generator=g).to(cuda).requires_grad_() for s in shapes]
    # a parameter that is a misaligned view (element offset 1 of a larger buffer): the kernel's scalar path
    buf = torch.randn(5001, generator=g).to(cuda)
    ps.append(buf[1:].detach().requires_grad_())
    return ps


@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_trajectory_and_state_match_torch(cuda, kind):
    from flairhip.optim import HipAdam, HipAdamW
    ours_p, ref_p = _params(cuda, 1), _params(cuda, 1)
    kw = dict(lr=3e-3, betas=(0.9, 0.95), weight_decay=0.02 if kind == "adamw" else 0.01)
    ours = (HipAdamW if kind == "adamw" else HipAdam)(ours_p, **kw)
    ref = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(ref_p, fused=True, **kw)
    g = torch.Generator().manual_seed(9)
    for step in range(6):
        lr = 3e-3 * (1.0 + 0.3 * step)
        for opt in (ours, ref):
            for grp in opt.param_groups:
                grp["lr"] = lr
        for a, b in zip(ours_p, ref_p):
            if step == 2 and a.numel() == 19:
                a.grad = b.grad = None  # a parameter that skips a step keeps its own step count
                continue
            gr = torch.randn(a.shape, generator=g).to(cuda)
            a.grad, b.grad = gr.clone(), gr.clone()
        ours.step()
        ref.step()
    torch.cuda.synchronize()
    worst = 0.0
    for a, b in zip(ours_p, ref_p):
        sa, sb = ours.state[a], ref.state[b]
        assert float(sa["step"]) == float(sb["step"])
        for x, y in ((a, b), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
            d = (x.detach() - y.detach()).abs().max().item()
            worst = max(worst, d / (y.detach().abs().max().item() + 1e-12))
    assert worst <= 2e-6, worst  # same formula and order as torch's fused kernel; at most an ulp of libm difference


def test_state_dict_round_trips_through_torchs_optimizer(cuda):
    from flairhip.optim import HipAdamW
    ps, qs = _params(cuda, 2)[:6], _params(cuda, 2)[:6]
    ours = HipAdamW(ps, lr=1e-3, weight_decay=0.01)
    for p in ps:
        p.grad = torch.ones_like(p)
    ours.step()
    ref = torch.optim.AdamW(qs, lr=1e-3, weight_decay=0.01, fused=True, capturable=True)
    import copy
    ref.load_state_dict(copy.deepcopy(ours.state_dict()))  # (torch keeps the tensors it is handed: no aliasing wanted)
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    for p, q in zip(ps, qs):
        p.grad, q.grad = torch.full_like(p, 0.5), torch.full_like(q, 0.5)
    ours.step()
    ref.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, qs):
        assert (p - q).detach().abs().max().item() <= 2e-6 * float(q.detach().abs().max())


def test_rejects_what_it_does_not_implement(cuda):
    from flairhip.optim import HipAdamW
    with pytest.raises(NotImplementedError):
        HipAdamW([torch.zeros(3, device=cuda, requires_grad=True)], amsgrad=True)
    p = torch.zeros(3, requires_grad=True)  # CPU tensor: no CPU path
    p.grad = torch.ones(3)
    with pytest.raises(TypeError):
        HipAdamW([p]).step()


# ---- the kernel against float64 (tests/insitu.py, Checker.adamw) ---------------------------------------------------------
# Every case snapshots p, g, exp_avg, exp_avg_sq around one step() and hands them, with the step count and learning rate the
# kernel read, to the float64 restatement of the update: per element, at the rounding bound derived in Checker.adamw.

_measured = {}  # quantity -> largest error as a fraction of its bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for what, frac in sorted(_measured.items()):
        print(f"\nMEASURED adamw_multi_kernel {what:11s} {frac:6.3f} of the float64 bound", end="")


def _grad_like(shape, g, cuda):
    """gradient scales 1e-9 .. 10 element by element (eps matters for some, not for others) and exact zeros"""
    scale = 10.0 ** torch.randint(-9, 2, shape, generator=g).float()
    gr = torch.randn(shape, generator=g) * scale
    gr.view(-1)[::97] = 0
    return gr.to(cuda)


def _checked_step(opt, ck, label, run=None):
    """one opt.step() (or run()) with every tensor of every group checked against float64 -> the checker"""
    before = []
    for gi, grp in enumerate(opt.param_groups):
        for p in grp["params"]:
            st = opt.state.get(p, {})
            before.append((gi, p, p.detach().clone(), None if p.grad is None else p.grad.detach().clone(),
                           st["exp_avg"].clone() if st else torch.zeros_like(p),
                           st["exp_avg_sq"].clone() if st else torch.zeros_like(p),
                           float(st["step"]) if st else 0.0))
    (run or opt.step)()
    torch.cuda.synchronize()
    for i, (gi, p, p0, g0, m0, v0, s0) in enumerate(before):
        grp, st = opt.param_groups[gi], opt.state.get(p, {})
        if g0 is None:  # a tensor without a gradient is not touched and keeps its step count
            assert torch.equal(p.detach(), p0) and (float(st["step"]) if st else 0.0) == s0, (label, i)
            if st:
                assert torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0), (label, i)
            continue
        assert torch.equal(p.grad, g0), "the step must not write the gradient"
        assert float(st["step"]) == s0 + 1.0, (label, i, float(st["step"]), s0)
        res = ck.adamw({"op": "adamw", "call": len(ck.results), "module": f"{label} tensor {i} n={p.numel()}"}, p0, g0,
                       m0, v0, st["step"], grp["lr"], p, st["exp_avg"], st["exp_avg_sq"], grp["betas"], grp["eps"],
                       grp["weight_decay"], opt.decoupled, grp["maximize"])
        for r in res:
            _measured[r["what"]] = max(_measured.get(r["what"], 0.0), r["worst"])
    return ck


def _assert_ok(ck, expect_min):
    bad = [r.line() for r in ck.results if not r.ok]
    print(f"\n{len(ck.results)} checks, worst err/bound " + ", ".join(
        f"{w} {max(r['worst'] for r in ck.results if r['what'] == w):.3g}" for w in ("p", "exp_avg", "exp_avg_sq")))
    assert len(ck.results) >= expect_min, len(ck.results)
    assert not bad, bad[:20]


ADAM_SIZES = (1, 4095, 4096, 4097, 8192, 12289)  # one element; around one block's 4096; two full blocks; three and one


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
@pytest.mark.parametrize("wd", [0.0, 0.02])
@pytest.mark.parametrize("maximize", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_update_matches_float64(cuda, kind, maximize, wd, eps):
    """decoupled x maximize x weight decay (0: Adam skips its L2 branch) x eps, three steps from empty state, lr a float"""
    from flairhip.optim import HipAdam, HipAdamW
    from insitu import Checker
    g = torch.Generator().manual_seed(11)
    ps = [torch.randn(n, generator=g).to(cuda).requires_grad_() for n in ADAM_SIZES]
    opt = (HipAdamW if kind == "adamw" else HipAdam)(ps, lr=3e-3, betas=(0.9, 0.95), eps=eps, weight_decay=wd,
                                                     maximize=maximize)
    ck = Checker("full")
    for step in range(3):
        for p in ps:
            p.grad = _grad_like(p.shape, g, cuda)
        _checked_step(opt, ck, f"{kind} step {step + 1}")
    _assert_ok(ck, 3 * 3 * len(ADAM_SIZES))


def _table_positions(n):
    """multi-block tensors at the first, a middle and the last descriptor of a full table, at the first descriptor of the
    second launch, in the middle of it and at the very end of the last launch"""
    return sorted({i for i in (0, 35, 71, 72, 72 + 35, 143, 144, n - 1) if i < n})


@pytest.mark.parametrize("n", [72, 73, 144, 145])
def test_descriptor_tables_and_block_search(cuda, n):
    """exactly one and two full tables, and one tensor more: the binary search over first_block with multi-block tensors
    (12289 and 8193 elements: four and three blocks) between one-block neighbours, in every launch"""
    from flairhip.optim import HipAdamW
    from insitu import Checker
    g = torch.Generator().manual_seed(n)
    big = _table_positions(n)
    sizes = [7 + i % 5 for i in range(n)]
    for k, i in enumerate(big):
        sizes[i] = 12289 if k % 2 == 0 else 8193
    ps = [torch.randn(s, generator=g).to(cuda).requires_grad_() for s in sizes]
    opt = HipAdamW(ps, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01)
    ck = Checker("full")
    for step in range(2):
        for p in ps:
            p.grad = _grad_like(p.shape, g, cuda)
        _checked_step(opt, ck, f"table of {n}, step {step + 1}")
    _assert_ok(ck, 2 * 3 * n)


def _view(n, off, g, cuda, fill=None):
    """n elements at element offset `off` of a fresh allocation (off = 0: 16-byte aligned)"""
    buf = (torch.randn(n + off, generator=g) if fill is None else torch.full((n + off,), float(fill))).to(cuda)
    v = buf[off:]
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


def _one_tensor_step(cuda, seed, n, off_p=0, off_g=0, off_mv=0, kind="adamw"):
    """two steps of one tensor whose operands sit at the given element offsets -> (checker, p, exp_avg, exp_avg_sq)"""
    from flairhip.optim import HipAdam, HipAdamW
    from insitu import Checker
    g = torch.Generator().manual_seed(seed)
    p = _view(n, off_p, g, cuda).detach().requires_grad_()
    grads = [_grad_like((n,), g, cuda) for _ in range(2)]
    opt = (HipAdamW if kind == "adamw" else HipAdam)([p], lr=3e-3, betas=(0.9, 0.95), weight_decay=0.02)
    opt.state[p] = {"step": torch.zeros((), dtype=torch.float32, device=cuda), "exp_avg": _view(n, off_mv, g, cuda, 0.0),
                    "exp_avg_sq": _view(n, off_mv, g, cuda, 0.0)}
    ck = Checker("full")
    for step in range(2):
        gv = _view(n, off_g, g, cuda)
        gv.copy_(grads[step])
        p.grad = gv
        assert p.grad.data_ptr() == gv.data_ptr()
        _checked_step(opt, ck, f"offsets p {off_p} g {off_g} m/v {off_mv}, step {step + 1}")
    st = opt.state[p]
    return ck, p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


@pytest.mark.parametrize("which", ["p", "g", "mv"])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_views_at_element_offsets(cuda, which, off):
    """4, 8 and 12 bytes off the 16-byte grid, on the parameter alone, on the gradient alone (the data-parallel bucket:
    p, m, v aligned) and on the moments alone: the scalar path, three full blocks and a ragged one"""
    ck, _, _, _ = _one_tensor_step(cuda, 5, 12289 + 4096, **{{"p": "off_p", "g": "off_g", "mv": "off_mv"}[which]: off})
    _assert_ok(ck, 6)


@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_vector_and_scalar_paths_round_alike(cuda, kind):
    """the same inputs give the same bits run to run, and with the gradient alone at an element offset of 1, 2 or 3 (scalar
    path) the bits of the all-aligned run (vector path): a replica's update must not depend on where its gradient sits in
    the bucket.  (The parameter at an offset: test_views_at_element_offsets, inside the float64 bound.)"""
    n = 3 * 4096 + 1234
    ck, p_a, m_a, v_a = _one_tensor_step(cuda, 6, n, kind=kind)
    _assert_ok(ck, 6)
    for off_g in (0, 1, 2, 3):
        ck, p_b, m_b, v_b = _one_tensor_step(cuda, 6, n, off_g=off_g, kind=kind)
        assert torch.equal(p_a, p_b) and torch.equal(m_a, m_b) and torch.equal(v_a, v_b), off_g


def test_param_groups_step_counts_and_device_lr(cuda):
    """two groups with their own lr / weight decay / betas / eps (the second one's lr a device tensor that changes between
    steps), more tensors than one table in the first; tensors that skip steps and a state loaded with step = 1000 keep
    their own counts"""
    import copy
    from flairhip.optim import HipAdamW
    from insitu import Checker
    g = torch.Generator().manual_seed(21)
    a = [torch.randn(s, generator=g).to(cuda).requires_grad_() for s in [4097, 19, 8192] + [5] * 75]
    b = [torch.randn(s, generator=g).to(cuda).requires_grad_() for s in (12289, 33, 1)]
    lr_b = torch.tensor(7e-4, dtype=torch.float32, device=cuda)
    opt = HipAdamW([{"params": a}, {"params": b, "lr": lr_b, "weight_decay": 0.1, "betas": (0.8, 0.9), "eps": 1e-6}],
                   lr=3e-3, betas=(0.9, 0.999), weight_decay=0.01)
    ck = Checker("full")
    for step in range(5):
        if step == 3:  # every tensor of group b continues from step 1000, a[1] from 500
            sd = copy.deepcopy(opt.state_dict())
            for k in (len(a), len(a) + 1, len(a) + 2):
                sd["state"][k]["step"] = torch.tensor(1000.0)
            sd["state"][1]["step"] = torch.tensor(500.0)
            opt.load_state_dict(sd)
            assert opt.param_groups[1]["lr"].is_cuda
        for i, p in enumerate(a + b):
            skip = (step == 1 and i in (0, 2, len(a))) or (step == 2 and i == 2)
            p.grad = None if skip else _grad_like(p.shape, g, cuda)
        opt.param_groups[1]["lr"].fill_(7e-4 * (1 + step))
        _checked_step(opt, ck, f"groups, step {step + 1}")
    _assert_ok(ck, 3 * (5 * (len(a) + len(b)) - 4))
    steps = [float(opt.state[p]["step"]) for p in (a[0], a[1], a[2], a[3], b[0], b[1])]
    assert steps == [4.0, 502.0, 3.0, 5.0, 1002.0, 1002.0], steps


def test_captured_step_replays_with_the_lr_on_the_device(cuda):
    """one torch.cuda.graph capture of step(), replayed three times with lr rewritten on the device and new gradients
    copied into the static buffers in between: every replay reads the new lr and the advanced step counts"""
    from flairhip.graph import make_capturable
    from flairhip.optim import HipAdamW
    from insitu import Checker
    g = torch.Generator().manual_seed(31)
    ps = [torch.randn(s, generator=g).to(cuda).requires_grad_() for s in [12289, 4096, 3] + [6] * 72]
    opt = HipAdamW(ps, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.02)
    make_capturable(opt)
    lr = opt.param_groups[0]["lr"]
    assert torch.is_tensor(lr) and lr.is_cuda
    for p in ps:
        p.grad = _grad_like(p.shape, g, cuda)
    ck = Checker("full")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _checked_step(opt, ck, "eager warm-up")  # creates the state and the descriptor tables
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[ps[0]]["step"]) == 1.0, "capturing must not run the step"
    for k in range(3):
        lr.fill_(1e-3 * (2 + k))
        for p in ps:
            p.grad.copy_(_grad_like(p.shape, g, cuda))
        _checked_step(opt, ck, f"replay {k + 1}", run=graph.replay)
        assert float(opt.state[ps[-1]]["step"]) == 2.0 + k
    _assert_ok(ck, 4 * 3 * len(ps))


# ---- a state that torch's optimizer saved ------------------------------------------------------------------------------------
# torch's default Adam / AdamW (not fused, not capturable: what the reference constructs) keeps ``step`` in a CPU tensor and
# saves ``capturable: False``; torch.optim.Optimizer.load_state_dict hands both through as they are.  The kernel reads the
# counter through a device pointer, so HipAdamW.load_state_dict has to move it (tests/test_optim_state_cpu.py holds the layout
# to that without a GPU); here the loaded state is continued on the kernel and held to float64 and to torch's own next steps.


@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_a_default_torch_state_from_disk_continues_on_the_kernel(cuda, kind, tmp_path):
    from flairhip.optim import HipAdam, HipAdamW
    from insitu import Checker
    g = torch.Generator().manual_seed(41)
    ref_p = _params(cuda, 7)[:6] + [torch.randn(12289, generator=g).to(cuda).requires_grad_()]
    kw = dict(lr=3e-3, betas=(0.9, 0.95), weight_decay=0.02 if kind == "adamw" else 0.01)
    ref = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(ref_p, **kw)
    assert not ref.param_groups[0]["capturable"] and not ref.param_groups[0]["fused"]
    for _ in range(3):
        for q in ref_p:
            q.grad = _grad_like(q.shape, g, cuda)
        ref.step()
    assert ref.state[ref_p[0]]["step"].device.type == "cpu"  # the case: a counter on the host
    torch.save(ref.state_dict(), tmp_path / "optimizer.pt")
    sd = torch.load(tmp_path / "optimizer.pt", map_location="cpu")
    ours_p = [q.detach().clone().requires_grad_() for q in ref_p]
    ours = (HipAdamW if kind == "adamw" else HipAdam)(ours_p, lr=1.0)
    ours.load_state_dict(sd)
    assert all(grp["capturable"] is True for grp in ours.param_groups) and ours.param_groups[0]["lr"] == 3e-3
    for p in ours_p:
        st = ours.state[p]
        assert st["step"].is_cuda and st["step"].dtype == torch.float32 and st["step"].dim() == 0
        assert st["exp_avg"].is_cuda and st["exp_avg_sq"].is_cuda and st["exp_avg"].dtype == torch.float32
    ck = Checker("full")
    for step in range(2):
        for p, q in zip(ours_p, ref_p):
            gr = _grad_like(p.shape, g, cuda)
            p.grad, q.grad = gr.clone(), gr.clone()
        _checked_step(ours, ck, f"{kind} continued from torch's state, step {4 + step}")
        ref.step()
    torch.cuda.synchronize()
    _assert_ok(ck, 2 * 3 * len(ours_p))
    for p, q in zip(ours_p, ref_p):
        d, bound = (p - q).detach().abs().max().item(), 2e-6 * float(q.detach().abs().max())
        print(f"n={p.numel():6d} max|p - q| {d:.3e}  bound {bound:.3e}")
        assert d <= bound, (p.numel(), d, bound)
        assert float(ours.state[p]["step"]) == 5.0


def test_step_refuses_a_hand_assigned_host_state_before_any_launch(cuda):
    """a ``step`` counter on the host, assigned by hand: the kernel would dereference a host address.  step() raises before
    it launches anything: the parameter, the moments and the other group's tensors are untouched"""
    from flairhip.optim import HipAdamW
    g = torch.Generator().manual_seed(43)
    a = torch.randn(300, generator=g).to(cuda).requires_grad_()
    b = torch.randn(50, generator=g).to(cuda).requires_grad_()
    opt = HipAdamW([{"params": [a]}, {"params": [b]}], lr=1e-2)
    for p in (a, b):
        p.grad = torch.ones_like(p)
    opt.step()  # a valid state and pointer tables first: the refusal must not depend on a first step
    torch.cuda.synchronize()
    a0, b0 = a.detach().clone(), b.detach().clone()
    m0 = opt.state[a]["exp_avg"].clone()
    for bad in (torch.ones(()), 1.0, torch.ones((), dtype=torch.float64, device=cuda)):
        opt.state[b]["step"] = bad  # the SECOND group: the first one's launch must not have happened either
        with pytest.raises(TypeError, match="step"):
            opt.step()
        torch.cuda.synchronize()
        assert torch.equal(a, a0) and torch.equal(b, b0) and torch.equal(opt.state[a]["exp_avg"], m0)
        assert float(opt.state[a]["step"]) == 1.0
    opt.state[b]["step"] = torch.ones((), dtype=torch.float32, device=cuda)
    opt.state[b]["exp_avg"] = torch.zeros(50)  # a moment on the host
    with pytest.raises(TypeError, match="exp_avg"):
        opt.step()
    opt.state[b]["exp_avg"] = torch.zeros(50, device=cuda)
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[a]["step"]) == 2.0 and float(opt.state[b]["step"]) == 2.0 and not torch.equal(a, a0)
