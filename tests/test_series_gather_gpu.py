"""Sentinel time series gathered from the device sample store (csrc/series_gather.hip): ops.gather_series against the
streamed definition -- ops.d4_layout(group=T) / ops.nchw_to_nhwc and ops.detect_pad_images on the f32 batch that
pad_collate_flair builds from the same samples -- bit for bit; the aerial + Sentinel-2 fusion model fed from the store
against the same model fed the streamed raw batch (logits, loss, every parameter gradient: bit for bit, since everything
after the new entry is shared); and a captured training step replayed with a second index vector."""
import numpy as np
import pytest
import torch

from helpers import TASK
from test_data_module_cpu import config_of, gold, on_disk  # noqa: F401  (gold, on_disk: fixtures)

pytestmark = pytest.mark.gpu
MOD, S2 = "AERIAL_RGBI", "SENTINEL2_TS"
LENGTHS = [1, 4, 2, 4, 3]
KINDS = {"uint8": np.uint8, "uint16": np.uint16, "int16": np.int16, "float32": np.float32}
PLANES = [(2, 2), (10, 10), (12, 12), (33, 33)]  # 12: four samples per load; 33: crosses the 32-pixel tile
CHANNELS = [(1, 8), (3, 8), (3, 16), (10, 16)]   # (C, Cp); 10 channels: two passes through LDS
INDEX = {1: [2], 4: [3, 1, 1, 0]}                # B: the samples (repeated; longest series 2 resp. 4)
CODES = {1: ([5], [10]), 4: ([0, 1, 2, 3], [4, 5, 6, 7], [12, 9, 15, 6])}  # all eight codes and the aliased high k


def make_store(kind, C, H, W, pad_value, seed):
    """5 samples of lengths 1, 4, 2, 4, 3; date 2 of sample 1 is constant (at pad_value where the type can hold it)"""
    from flairhip.sample_store import SeriesStore
    r = np.random.RandomState(seed)
    dt = KINDS[kind]
    D = sum(LENGTHS)
    if kind == "float32":
        data = (r.randn(D, C, H, W) * 100).astype(np.float32)  # negative and non-integer values
    else:
        info = np.iinfo(dt)
        data = r.randint(info.min, info.max + 1, (D, C, H, W)).astype(dt)
    const = pad_value if kind in ("int16", "float32") else 0
    data[1 + 2] = const
    st = SeriesStore(len(LENGTHS), D, (C, H, W), dt, pad_value=pad_value, device="cuda")
    st.fill(0, data, r.randint(-200, 200, D), LENGTHS)
    assert st.is_pad.sum().item() == int(const == pad_value) and st.is_pad[3].item() == int(const == pad_value)
    return st, data


def streamed(data, index, T):
    """the f32 [B*T, C, H, W] tensor of the streamed path: pad_collate_flair over the samples, longer T padded on"""
    from flair_hub.data.utils_data.padding import pad_collate_flair, pad_tensor
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    samples = [{S2: torch.tensor(data[off[i]:off[i + 1]], dtype=torch.float32)} for i in index]
    x = pad_collate_flair(samples)[S2]
    x = torch.stack([pad_tensor(s, T, 0) for s in x])
    return x.reshape((len(index) * T,) + tuple(x.shape[2:])).contiguous().cuda()


def check(st, data, index, T, dtype, codes, cp, pad_value, what):
    from flairhip import ops
    x = streamed(data, index, T)
    dev_codes = None if codes is None else torch.tensor(codes, dtype=torch.uint8).cuda()
    want = ops.nchw_to_nhwc(x, dtype, cp) if codes is None else ops.d4_layout(x, dtype, dev_codes, cp=cp, group=T)
    want_pad = ops.detect_pad_images(x, pad_value)
    got, pad = ops.gather_series(st, torch.tensor(index, dtype=torch.int32), T, dtype, dev_codes, cp, 0.0, pad_value)
    assert got.dtype == dtype and got.shape == want.shape and pad.dtype == torch.uint8
    assert torch.equal(pad, want_pad), (what, pad.tolist(), want_pad.tolist())
    assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), what
    return got, pad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_gather_series_equals_the_streamed_layout_and_pad_detection(cuda, kind, dtype):
    n = 0
    for pad_value in (0.0, -1.0):  # fill is 0 in both: the tail is flagged in the first, not in the second
        for (H, W) in PLANES:
            for (C, cp) in CHANNELS:
                st, data = make_store(kind, C, H, W, pad_value, seed=H * 100 + C)
                for B, index in INDEX.items():
                    longest = max(LENGTHS[i] for i in index)
                    for T in (longest, longest + 2):
                        for codes in (None,) + CODES[B]:
                            _, pad = check(st, data, index, T, dtype, codes, cp, pad_value,
                                           (kind, pad_value, H, W, C, cp, B, T, codes))
                            tail = [t >= LENGTHS[i] for i in index for t in range(T)]
                            assert pad.cpu()[torch.tensor(tail)].tolist() == [int(pad_value == 0.0)] * sum(tail)
                            n += 1
    assert n == 2 * 4 * 4 * (2 * 3 + 2 * 4)


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_gather_series_without_codes_takes_planes_that_are_not_square(cuda, kind):
    for (C, cp) in CHANNELS:
        st, data = make_store(kind, C, 6, 10, 0.0, seed=C)
        for dtype in (torch.bfloat16, torch.float32):
            check(st, data, [4, 1, 0], 6, dtype, None, cp, 0.0, (kind, C, cp, dtype))


def test_a_stored_date_constant_at_the_pad_value_is_flagged_and_keeps_its_values(cuda):
    st, data = make_store("int16", 3, 10, 10, -1.0, seed=1)
    got, pad = check(st, data, [1, 0], 4, torch.float32, [7, 2], 8, -1.0, "constant date")
    assert pad.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]  # date 2 of sample 1; the padded dates hold 0, not -1
    assert (got[2, :, :, :3] == -1).all() and (got[2, :, :, 3:] == 0).all() and (got[5] == 0).all()


def test_gather_series_drops_what_a_device_index_cannot_be_checked_for(cuda):
    """the values of a device index stay on the device: one outside [0, N) is clamped, and a series longer than T loses
    its last dates: the result is the first T dates of the clamped samples"""
    from flairhip import ops
    st, data = make_store("uint8", 3, 10, 10, 0.0, seed=2)
    T = 2
    short, pad = ops.gather_series(st, torch.tensor([1, 9, -4], dtype=torch.int32).cuda(), T, torch.float32, None, 8)
    full, fpad = ops.gather_series(st, torch.tensor([1, 4, 0], dtype=torch.int32), 4, torch.float32, None, 8)
    full, fpad = full.view(3, 4, 10, 10, 8), fpad.view(3, 4)
    assert torch.equal(short.view(3, T, 10, 10, 8), full[:, :T]) and torch.equal(pad.view(3, T), fpad[:, :T])
    with pytest.raises(ValueError):
        ops.gather_series(st, torch.tensor([1], dtype=torch.int32), T, torch.float32)  # a host index is checked


# ---- the model fed from the store ------------------------------------------------------------------------------------------


def model_config(meta, root, precision, pre=None):
    from flairhip.configs import unet_resnet34_config
    cfg = unet_resnet34_config(in_channels=5, precision=precision, batch_size=4)
    data = config_of(meta, "s2", root)
    for key in ("labels", "paths", "tasks"):
        cfg[key] = data[key]
    cfg["labels_configs"][TASK]["label_channel_nomenclature"] = 1
    cfg["modalities"]["inputs"] = data["modalities"]["inputs"]
    cfg["modalities"]["inputs_channels"] = data["modalities"]["inputs_channels"]
    cfg["modalities"]["normalization"] = data["modalities"]["normalization"]
    cfg["modalities"]["pre_processings"] = dict(data["modalities"]["pre_processings"], **(pre or {}))
    # the smallest U-TAE the class accepts: every width a multiple of 16 (adjust_fm_length makes six stages of 16)
    cfg["models"]["multitemp_model"].update(encoder_widths=[16, 16], decoder_widths=[16, 16], out_conv=[16, 19],
                                            n_head=16, d_model=64, d_k=4)
    cfg["hyperparams"]["seed"] = 7
    return cfg


def build(cfg, batch_size, **kw):
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    train, val, test = get_datasets(cfg)
    dm = FlairDataModule(cfg, train, val, test, num_workers=0, batch_size=batch_size, drop_last=True,
                         use_augmentations=False, **kw)
    dm.setup("fit")
    return dm


def make_task(cfg, store):
    from flair_hub.tasks.module_setup import build_segmentation_module
    torch.manual_seed(3)
    task = build_segmentation_module(cfg, {MOD: 64, S2: 10}, "train").cuda()
    utae = task.model.encoders[S2]
    utae.mlp_dropout = utae.attn_dropout = 0.0
    task.attach_store(store)
    return task


def to_cuda(batch, codes):
    out = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    out["AUG"] = torch.tensor(codes, dtype=torch.uint8).cuda()
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_fusion_model_from_the_store_equals_the_streamed_batch(cuda, gold, on_disk, precision):
    meta, _ = gold
    cfg = model_config(meta, on_disk, precision)
    res = build(cfg, 4, cache="device", series_cache=True)
    raw = build(cfg, 4, cache="none", device_prepare=True)
    assert res.store is not None and list(res.store.series) == [S2] and res.store.series[S2].data.is_cuda
    codes = [6, 13, 0, 11]
    b_res = to_cuda(next(iter(res.val_dataloader())), codes)
    b_raw = to_cuda(next(iter(raw.val_dataloader())), codes)
    raw.teardown()
    assert set(b_res) == {"INDEX", f"ID_{TASK}", "SENTINEL2_DATES", "AUG"} and S2 in b_raw and MOD in b_raw
    assert b_res[f"ID_{TASK}"] == b_raw[f"ID_{TASK}"] and torch.equal(b_res["SENTINEL2_DATES"], b_raw["SENTINEL2_DATES"])
    assert tuple(b_raw[S2].shape) == (4, 5, 3, 10, 10)  # ragged: lengths 3, 5, 2, 4
    task = make_task(cfg, res.store)
    task.eval()
    with torch.no_grad():
        la, lb = task.model(b_res)[0], task.model(b_raw)[0]
        plain = task.model(dict(b_res, AUG=torch.zeros(4, dtype=torch.uint8).cuda()))[0]
    assert torch.equal(la[TASK], lb[TASK]), "logits differ between the resident and the streamed batch"
    assert not torch.equal(plain[TASK], la[TASK]), "the codes did nothing"
    # one training step: loss and every parameter gradient
    task.train()
    assert not task.mod_dropout
    grads = []
    for batch in (b_res, b_raw):
        task.zero_grad(set_to_none=True)
        loss = task.step(batch, training=True)[0]
        loss.backward()
        grads.append((loss.detach().clone(), {n: p.grad.clone() for n, p in task.named_parameters() if p.grad is not None}))
    (loss_a, ga), (loss_b, gb) = grads
    print(f"{precision}: loss resident {loss_a.item()!r} streamed {loss_b.item()!r}, {len(ga)} gradients")
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b)
    assert ga.keys() == gb.keys() and any(n.startswith(f"model.encoders.{S2}") for n in ga)
    assert [n for n in ga if not torch.equal(ga[n], gb[n])] == []


def test_a_captured_step_replays_with_a_second_index_vector(cuda, gold, on_disk):
    """monthly averages: T = 12 for every batch, so the step is captured once; a frozen model (learning rate 0, no
    weight decay, no dropout), so a training step's loss depends on the batch alone"""
    from flairhip.graph import GraphedTrainStep
    meta, _ = gold
    cfg = model_config(meta, on_disk, "bf16", {"temporal_average_sentinel2": "monthly"})
    res = build(cfg, 2, cache="device", series_cache=True)
    first, second = [to_cuda(b, c) for b, c in zip(res.val_dataloader(), ([3, 8], [5, 14]))]
    assert tuple(first["SENTINEL2_DATES"].shape) == tuple(second["SENTINEL2_DATES"].shape) == (2, 12)
    assert first["INDEX"].tolist() == [4, 5] and second["INDEX"].tolist() == [6, 7]
    task = make_task(cfg, res.store)
    task.train()
    opt = torch.optim.AdamW(task.model.parameters(), lr=0.0, weight_decay=0.0)
    stepper = GraphedTrainStep(task, opt, first, warmup_steps=2)
    assert stepper.static_batch["INDEX"].is_cuda
    l1, l2, l1_again = stepper(first).item(), stepper(second).item(), stepper(first).item()
    eager = [task.step(b, training=True)[0].item() for b in (first, second)]
    print(f"replayed {l1!r} {l2!r} {l1_again!r}; eager {eager!r}")
    assert l1 == l1_again and l1 != l2
    assert [l1, l2] == eager
