"""Training augmentation on the device (csrc/augment.hip): per-sample flips and rotations by k * 90 degrees inside the
layout / label passes, steered by batch["AUG"].  The feature is a permutation, so every comparison is exact: against
the existing layout / label kernels run on a numpy-transformed input, against tests/golden/augment_d4.npz (the
reference's own outputs), through the model, the task, the captured training step and the trainer."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import MOD, ROOT, TASK, make_pair

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
LPIS, DEM, S2 = "ALL_LABEL-LPIS", "DEM_ELEV", "SENTINEL2_TS"
ALL_CODES = np.arange(16, dtype=np.uint8)


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
    """the existing kernel for the sample type: the yardstick"""
    from flairhip import ops
    if mean is None:
        return ops.nchw_to_nhwc(x, dtype, cp)
    if x.dtype == torch.uint8:
        return ops.u8_nchw_to_nhwc(x, dtype, mean, std, cp)
    return ops.raw_nchw_to_nhwc(x, dtype, mean, std, cp)


# ---- 1. d4_layout against the existing layout kernels ------------------------------------------------------------


@pytest.mark.parametrize("n", [10, 33, 128, 512])
@pytest.mark.parametrize("kind", ["u8", "u16", "i16", "f32"])
def test_d4_layout_equals_the_plain_kernel_on_a_transformed_input(cuda, kind, n):
    """a batch of 16 samples carrying the 16 codes; every (normalisation, destination type, C, pitch) of the sample type"""
    from flairhip import ops
    base = _samples(kind, (16, 10, n, n), seed=n + len(kind))
    want_src = transform_batch(base, ALL_CODES)
    codes = torch.from_numpy(ALL_CODES).to(cuda)
    g = torch.Generator().manual_seed(n)
    checked = 0
    for C in (1, 2, 3, 5, 10):
        x = torch.from_numpy(np.ascontiguousarray(base[:, :C])).to(cuda)
        xt = torch.from_numpy(np.ascontiguousarray(want_src[:, :C])).to(cuda)
        mean = (torch.rand(C, generator=g) * 200 + 3).to(cuda)
        std = (torch.rand(C, generator=g) * 90 + 7).to(cuda)
        for cp in (8, 16):
            if cp < C:
                continue
            for dtype in (torch.bfloat16, torch.float32):
                for norm in ((True, False) if kind == "f32" else (True,)):
                    m, s = (mean, std) if norm else (None, None)
                    got = ops.d4_layout(x, dtype, codes, m, s, cp)
                    want = _plain_layout(xt, dtype, m, s, cp)
                    assert got.shape == (16, n, n, cp) and got.dtype == dtype
                    if not torch.equal(got, want):
                        bad = [b for b in range(16) if not torch.equal(got[b], want[b])]
                        raise AssertionError(f"{kind} n={n} C={C} cp={cp} {dtype} norm={norm}: codes {bad} differ")
                    assert not got[..., C:].any(), "padding channels must stay zero"
                    checked += 1
    assert checked == (36 if kind == "f32" else 18)


def test_d4_layout_code_zero_is_the_plain_kernel_and_high_bits_are_masked(cuda):
    from flairhip import ops
    x = torch.from_numpy(_samples("u8", (3, 5, 64, 64), 1)).to(cuda)
    mean, std = torch.full((5,), 110.0, device=cuda), torch.full((5,), 50.0, device=cuda)
    want = ops.u8_nchw_to_nhwc(x, torch.bfloat16, mean, std, 16)
    zero = torch.zeros(3, dtype=torch.uint8, device=cuda)
    assert torch.equal(ops.d4_layout(x, torch.bfloat16, zero, mean, std, 16), want)
    assert torch.equal(ops.d4_layout(x, torch.bfloat16, zero + 0xF0, mean, std, 16), want)


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_d4_layout_group_shares_a_code_over_the_dates_of_a_series(cuda, kind):
    from flairhip import ops
    B, T, C, n = 5, 4, 10, 10
    base = _samples(kind, (B, T, C, n, n), 3)
    codes = np.array([13, 0, 6, 9, 3], dtype=np.uint8)
    want_src = transform_batch(base, codes)  # one code for all T x C planes of a sample
    x = torch.from_numpy(base).to(cuda).reshape(B * T, C, n, n)
    xt = torch.from_numpy(want_src).to(cuda).reshape(B * T, C, n, n)
    mean, std = (None, None) if kind == "f32" else (torch.full((C,), 1000.0, device=cuda), torch.full((C,), 300.0, device=cuda))
    for dtype in (torch.bfloat16, torch.float32):
        got = ops.d4_layout(x, dtype, torch.from_numpy(codes).to(cuda), mean, std, 16, group=T)
        assert torch.equal(got, _plain_layout(xt, dtype, mean, std, 16))
        assert not got[..., C:].any()


def test_d4_ops_refuse_what_they_cannot_do(cuda):
    from flairhip import ops
    codes = torch.zeros(2, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):  # non-square
        ops.d4_layout(torch.zeros(2, 3, 8, 16, device=cuda), torch.float32, codes)
    with pytest.raises(ValueError):
        ops.d4_labels(torch.zeros(2, 8, 16, dtype=torch.uint8, device=cuda), codes)
    with pytest.raises(ValueError):
        ops.d4_onehot_to_index(torch.zeros(2, 4, 8, 16, device=cuda), codes)
    with pytest.raises(ValueError):  # integer samples without mean / std
        ops.d4_layout(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=cuda), torch.float32, codes)
    with pytest.raises(ValueError):  # one code per sample
        ops.d4_layout(torch.zeros(3, 3, 8, 8, device=cuda), torch.float32, codes)
    with pytest.raises(ValueError):  # codes on the host
        ops.d4_layout(torch.zeros(2, 3, 8, 8, device=cuda), torch.float32, codes.cpu())
    with pytest.raises(ValueError):
        ops.d4_layout(torch.zeros(2, 3, 8, 8, device=cuda), torch.float32, codes.to(torch.int64))


# ---- 2. labels ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [10, 33, 64, 128, 512])
def test_d4_labels_equals_numpy(cuda, n):
    from flairhip import ops
    t = np.random.RandomState(n).randint(0, 256, (16, n, n)).astype(np.uint8)
    got = ops.d4_labels(torch.from_numpy(t).to(cuda), torch.from_numpy(ALL_CODES).to(cuda))
    assert torch.equal(got.cpu(), torch.from_numpy(transform_batch(t, ALL_CODES)))


@pytest.mark.parametrize("n", [10, 33, 128, 512])
def test_d4_onehot_to_index_equals_numpy(cuda, n):
    from flairhip import ops
    r = np.random.RandomState(n + 1)
    cls = r.randint(0, 19, (16, n, n))
    onehot = np.ascontiguousarray(np.eye(19, dtype=np.float32)[cls].transpose(0, 3, 1, 2))
    codes = torch.from_numpy(ALL_CODES).to(cuda)
    got = ops.d4_onehot_to_index(torch.from_numpy(onehot).to(cuda), codes)
    assert torch.equal(got.cpu(), torch.from_numpy(transform_batch(cls.astype(np.uint8), ALL_CODES)))
    # ties: a few distinct values per pixel, the first maximum wins (np.argmax's rule, ffa_onehot_to_index's rule)
    ties = r.randint(0, 3, (16, 7, n, n)).astype(np.float32)
    got = ops.d4_onehot_to_index(torch.from_numpy(ties).to(cuda), codes)
    want = transform_batch(ties, ALL_CODES).argmax(1).astype(np.uint8)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(got, ops.onehot_to_index(torch.from_numpy(transform_batch(ties, ALL_CODES)).to(cuda)))


@pytest.mark.parametrize("row", range(16))
def test_goldens_through_the_device_path(cuda, row):
    """the reference's own outputs (tests/golden/augment_d4.npz), reproduced by the kernels from the golden inputs"""
    from flairhip import ops
    d = np.load(os.path.join(GOLD, "augment_d4.npz"))
    code = int(d["codes"][row])
    codes = torch.tensor([code], dtype=torch.uint8, device=cuda)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)

    def out(key):
        return d[f"out{code:02d}_{key}"]

    mean, std = torch.full((5,), 110.0, device=cuda), torch.full((5,), 50.0, device=cuda)
    for dtype in (torch.bfloat16, torch.float32):
        assert torch.equal(ops.d4_layout(dev(d["in_" + MOD])[None], dtype, codes, mean, std, 16),
                           ops.u8_nchw_to_nhwc(dev(out(MOD))[None], dtype, mean, std, 16))
        assert torch.equal(ops.d4_layout(dev(d["in_" + DEM])[None], dtype, codes, cp=16),
                           ops.nchw_to_nhwc(dev(out(DEM))[None], dtype, 16))
        m4, s4 = mean[:4].contiguous(), std[:4].contiguous()
        assert torch.equal(ops.d4_layout(dev(d["in_" + S2]), dtype, codes, m4, s4, 16, group=3),
                           ops.raw_nchw_to_nhwc(dev(out(S2)), dtype, m4, s4, 16))
    label = out(TASK).argmax(0).astype(np.uint8)
    assert torch.equal(ops.d4_onehot_to_index(dev(d["in_" + TASK])[None], codes).cpu()[0], torch.from_numpy(label))
    assert torch.equal(ops.d4_labels(dev(d["in_" + TASK].argmax(0).astype(np.uint8))[None], codes).cpu()[0],
                       torch.from_numpy(label))


# ---- 3. model and task ----------------------------------------------------------------------------------------------


def _host_transformed(batch: dict, codes, spatial_keys) -> dict:
    """the batch the reference's dataset would have produced: every modality and label transformed on the host"""
    out = {}
    for k, v in batch.items():
        if k in spatial_keys:
            out[k] = torch.from_numpy(transform_batch(v.cpu().numpy(), codes)).to(v.device)
        else:
            out[k] = v
    return out


def _check_model_and_step(task, batch, codes, spatial_keys):
    dev = next(task.parameters()).device
    aug = dict(batch)
    aug["AUG"] = torch.from_numpy(np.asarray(codes, dtype=np.uint8)).to(dev)
    host = _host_transformed(batch, codes, spatial_keys)
    task.eval()
    with torch.no_grad():
        la, aa = task.model(aug)
        lh, ah = task.model(host)
        assert sorted(la) == sorted(lh) and sorted(aa) == sorted(ah)
        for k in la:
            assert torch.equal(la[k], lh[k]), f"logits of {k} differ"
        for k in aa:
            assert torch.equal(aa[k], ah[k]), f"auxiliary logits {k} differ"
        plain = task.model(batch)[0]
        assert any(not torch.equal(plain[k], la[k]) for k in la), "the codes did nothing"
        loss_a, preds_a, targets_a = task.step(aug, training=False)
        loss_h, preds_h, targets_h = task.step(host, training=False)
    assert torch.equal(loss_a, loss_h), (loss_a.item(), loss_h.item())
    for k in preds_h:
        assert torch.equal(preds_a[k], preds_h[k]) and torch.equal(targets_a[k], targets_h[k]), k
    # prediction never augments
    with torch.no_grad():
        pa, pp = task.predict_step(aug), task.predict_step(batch)
    for k in pp:
        assert torch.equal(pa[k], pp[k])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_unet_logits_and_step_equal_the_host_transformed_batch(cuda, precision):
    task, _, _ = make_pair(precision=precision, seed=5)
    g = torch.Generator().manual_seed(8)
    codes = [13, 0, 6, 11]
    # the reference schema (f32 imagery, one-hot label) and the compact one (uint8 imagery + NORM, uint8 indices)
    t = torch.randint(0, 19, (4, 64, 64), generator=g)
    ref = {MOD: torch.randn(4, 5, 64, 64, generator=g).to(cuda),
           TASK: F.one_hot(t, 19).permute(0, 3, 1, 2).float().contiguous().to(cuda)}
    _check_model_and_step(task, ref, codes, {MOD, TASK})
    compact = {MOD: torch.randint(0, 255, (4, 5, 64, 64), generator=g, dtype=torch.uint8).to(cuda),
               MOD + "_NORM": torch.tensor([[110.0] * 5, [50.0] * 5]).to(cuda), TASK: t.to(torch.uint8).to(cuda)}
    _check_model_and_step(task, compact, codes, {MOD, TASK})


def test_fusion_logits_and_step_equal_the_host_transformed_batch(cuda):
    """two modalities of different sizes, two tasks (one-hot and index labels), an auxiliary decoder"""
    from flairhip.configs import fusion_unet_config
    from flair_hub.tasks.module_setup import build_segmentation_module
    from oracle.seeded_weights import fill_state_dict
    cfg = fusion_unet_config(precision="bf16")
    task = build_segmentation_module(cfg, {MOD: 96, DEM: 64}, "train")
    task.model.load_state_dict(fill_state_dict(task.model.state_dict()))
    task = task.to(cuda)
    g = torch.Generator().manual_seed(9)
    batch = {MOD: torch.randn(3, 5, 96, 96, generator=g).to(cuda), DEM: torch.randn(3, 2, 64, 64, generator=g).to(cuda),
             TASK: F.one_hot(torch.randint(0, 19, (3, 96, 96), generator=g), 19).permute(0, 3, 1, 2).float().contiguous().to(cuda),
             LPIS: torch.randint(0, 23, (3, 96, 96), generator=g).to(cuda)}
    _check_model_and_step(task, batch, [9, 14, 1], {MOD, DEM, TASK, LPIS})


def test_sentinel_logits_and_step_equal_the_host_transformed_batch(cuda):
    """SENTINEL2_TS alone (U-TAE): the codes reach all T dates of a sample through group = T"""
    from flairhip.configs import fusion_unet_config
    from flair_hub.tasks.module_setup import build_segmentation_module
    from oracle.seeded_weights import fill_utae_state_dict, fill_state_dict
    cfg = fusion_unet_config(precision="fp32", aux_loss=False)
    cfg["modalities"]["inputs"] = {m: (m == S2) for m in cfg["modalities"]["inputs"]}
    cfg["modalities"]["inputs_channels"][S2] = list(range(1, 11))
    cfg["modalities"]["aux_loss"] = {m: False for m in cfg["modalities"]["aux_loss"]}
    task = build_segmentation_module(cfg, {S2: 10}, "train")
    sd = task.model.state_dict()
    utae = {k: v for k, v in sd.items() if k.startswith("encoders.SENTINEL")}
    rest = {k: v for k, v in sd.items() if k not in utae}
    filled = fill_state_dict(rest) if rest else {}
    filled.update(fill_utae_state_dict(utae))
    task.model.load_state_dict(filled)
    task = task.to(cuda)
    g = torch.Generator().manual_seed(10)
    batch = {S2: torch.randn(3, 5, 10, 10, 10, generator=g).to(cuda),
             "SENTINEL2_DATES": torch.randint(0, 365, (3, 5), generator=g).float().to(cuda),
             TASK: torch.randint(0, 19, (3, 40, 40), generator=g).to(torch.uint8).to(cuda),
             LPIS: torch.randint(0, 23, (3, 40, 40), generator=g).to(cuda)}
    _check_model_and_step(task, batch, [4, 7, 10], {S2, TASK, LPIS})


# ---- 4. captured training step ----------------------------------------------------------------------------------------

GRAPH_CODES = [[5, 12], [0, 9], [14, 3], [6, 6]]


def _train(graph: bool):
    """tests/test_graph_gpu.py's comparison (same seeded model twice, eager against replay), every batch with "AUG\""""
    from flairhip.graph import GraphedTrainStep, make_capturable
    task, _, _ = make_pair(precision="bf16", seed=11)
    task.train()
    g = torch.Generator().manual_seed(1)
    batches = [{MOD: torch.randn(2, 5, 64, 64, generator=g).cuda(),
                TASK: torch.randint(0, 19, (2, 64, 64), generator=g).to(torch.uint8).cuda(),
                "AUG": torch.tensor(c, dtype=torch.uint8).cuda()} for c in GRAPH_CODES]
    opt = torch.optim.AdamW(task.model.parameters(), lr=1e-3, weight_decay=0.01)
    losses = []
    if graph:
        state = {k: v.clone() for k, v in task.state_dict().items()}
        stepper = GraphedTrainStep(task, opt, batches[0], warmup_steps=2)
        task.load_state_dict(state)
        for st in opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
        assert stepper.static_batch["AUG"].is_cuda and stepper.static_batch["AUG"].dtype == torch.uint8
        for b in batches:
            losses.append(stepper(b).item())
    else:
        make_capturable(opt)
        for b in batches:
            loss = task.training_step(b, 0)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.item())
    torch.cuda.synchronize()
    w = task.model.state_dict()[f"encoders.{MOD}.seg_model.layer2.0.conv1.weight"].float().cpu()
    return losses, w


def test_graph_replay_with_new_codes_matches_eager(cuda):
    le, we = _train(False)
    lg, wg = _train(True)
    assert le == lg, (le, lg)  # the criterion of tests/test_graph_gpu.py: the replayed trajectory is the eager one
    assert torch.equal(we, wg)


def test_graph_replay_reads_the_codes_from_the_device(cuda):
    """a frozen model (learning rate 0, no weight decay): the loss of a replay depends on the batch alone, so the same
    data under other codes must give another loss, and the first codes again the first loss"""
    from flairhip.graph import GraphedTrainStep
    task, _, _ = make_pair(precision="bf16", seed=12)
    task.train()
    g = torch.Generator().manual_seed(2)
    batch = {MOD: torch.randn(2, 5, 64, 64, generator=g).cuda(),
             TASK: torch.randint(0, 19, (2, 64, 64), generator=g).to(torch.uint8).cuda(),
             "AUG": torch.tensor([0, 0], dtype=torch.uint8).cuda()}
    opt = torch.optim.AdamW(task.model.parameters(), lr=0.0, weight_decay=0.0)
    stepper = GraphedTrainStep(task, opt, batch, warmup_steps=2)

    def loss_with(codes):
        b = dict(batch)
        b["AUG"] = torch.tensor(codes, dtype=torch.uint8).cuda()
        return stepper(b).item()

    a, b, c, a2 = loss_with([0, 0]), loss_with([4, 1]), loss_with([10, 7]), loss_with([0, 0])
    assert a == a2
    assert len({a, b, c}) == 3, (a, b, c)
    # and each equals the eager step of the host-transformed batch
    host = _host_transformed({k: v for k, v in batch.items() if k != "AUG"}, [4, 1], {MOD, TASK})
    assert task.step(host, training=True)[0].item() == b


# ---- 5. trainer ---------------------------------------------------------------------------------------------------------


def _record(task):
    seen = {"train": [], "val": [], "predict": []}
    for name, hook in (("train", "training_step"), ("val", "validation_step"), ("predict", "predict_step")):
        orig = getattr(task, hook)

        def wrapped(batch, *a, _orig=orig, _name=name, **kw):
            # (no device -> host copy from inside a stream capture: there only the keys are noted)
            read = not torch.cuda.is_current_stream_capturing()
            seen[_name].append({k: (v.detach().cpu().clone() if (k == "AUG" and read) else None) for k, v in batch.items()})
            return _orig(batch, *a, **kw)

        setattr(task, hook, wrapped)
    return seen


def _host_batches(n, B=2, with_aug=None):
    g = torch.Generator().manual_seed(2)
    out = []
    for i in range(n):
        b = {MOD: torch.randn(B, 5, 64, 64, generator=g), TASK: torch.randint(0, 19, (B, 64, 64), generator=g)}
        if with_aug is not None:
            b["AUG"] = torch.tensor(with_aug[i], dtype=torch.uint8)
        out.append(b)
    return out


@pytest.mark.parametrize("optimizer", ["default", "torch"])
@pytest.mark.parametrize("hip_graph", [False, True])
def test_trainer_adds_the_codes_to_training_batches_only(cuda, hip_graph, optimizer):
    from flairhip.augment import draw_codes, rank_epoch_rng
    from flair_hub.tasks.trainers import HipTrainer
    task, _, cfg = make_pair(precision="bf16", seed=3)
    cfg["hyperparams"].update({"learning_rate": 1e-3, "total_steps": 12})
    cfg["modalities"]["pre_processings"]["use_augmentation"] = True
    assert task.config["modalities"]["pre_processings"]["use_augmentation"] is True
    cfg["hyperparams"]["torch_optimizer"] = optimizer == "torch"  # the trainer captures the step for either
    seen = _record(task)
    losses = []
    orig = task.on_train_batch_end
    task.on_train_batch_end = lambda loss, batch, i: (losses.append(float(loss)), orig(loss, batch, i))[1]
    tr = HipTrainer(max_epochs=2, hip_graph=hip_graph, seed=7)
    tr.fit(task, train_dataloaders=_host_batches(3), val_dataloaders=_host_batches(2))
    tr.predict(task, dataloaders=_host_batches(1))
    assert len(losses) == 6 and all(np.isfinite(losses))
    # eager: every training batch passes training_step; graph mode: the two eager steps and the capture
    assert len(seen["train"]) == (6 if not hip_graph else 3)
    assert (tr.graph_built, tr.graph_replays, tr.eager_steps) == ((True, 4, 2) if hip_graph else (False, 0, 6))
    assert all("AUG" in b for b in seen["train"])
    assert seen["val"] and not any("AUG" in b for b in seen["val"])
    assert seen["predict"] and not any("AUG" in b for b in seen["predict"])
    want = draw_codes(2 * 3, rng=rank_epoch_rng(7, tr.rank, 0)).reshape(3, 2)
    for i, b in enumerate(seen["train"][:2]):
        assert b["AUG"].dtype == torch.uint8 and np.array_equal(b["AUG"].numpy(), want[i])


def test_trainer_leaves_the_batches_alone_without_the_key_and_keeps_codes_a_dataset_drew(cuda):
    from flair_hub.tasks.trainers import AugmentedLoader, HipTrainer
    task, _, cfg = make_pair(precision="bf16", seed=3)
    assert cfg["modalities"]["pre_processings"]["use_augmentation"] is False
    seen = _record(task)
    HipTrainer(max_epochs=1).fit(task, train_dataloaders=_host_batches(2))
    assert len(seen["train"]) == 2 and not any("AUG" in b for b in seen["train"])
    # a dataset that draws its own codes: passed through untouched, with the key on or off
    own = [[4, 9], [15, 2]]
    for on in (False, True):
        task, _, cfg = make_pair(precision="bf16", seed=3)
        cfg["modalities"]["pre_processings"]["use_augmentation"] = on
        seen = _record(task)
        HipTrainer(max_epochs=1).fit(task, train_dataloaders=_host_batches(2, with_aug=own))
        assert [b["AUG"].tolist() for b in seen["train"]] == own
    # two ranks draw different transforms; a rank draws the same again
    cfg["modalities"]["pre_processings"]["use_augmentation"] = True
    draws = []
    for rank in (0, 1, 0):
        loader = AugmentedLoader(_host_batches(4, B=8), cfg, seed=7, rank=rank)
        assert len(loader) == 4
        draws.append(np.concatenate([b["AUG"].numpy() for b in loader]))
    assert not np.array_equal(draws[0], draws[1]) and np.array_equal(draws[0], draws[2])
