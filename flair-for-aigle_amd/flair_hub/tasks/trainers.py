"""Training / prediction drivers -- counterpart of the reference's flair_hub/tasks/trainers.py
(train :35-108 builds a pytorch_lightning.Trainer and calls fit/validate; predict :111-136).

Lightning is replaced by HipTrainer: one process per GPU, the SegmentationTask hooks are called in
Lightning's order, gradients are averaged across ranks by flairhip.distributed.GradSync (RCCL over
xGMI, overlapped with backward) in place of Lightning's DDP strategy.  Callbacks, loggers and
checkpoint policies of the reference are orchestration outside the hot path; what is kept is the
best-checkpoint-on-val_miou save so that stages can reload it.
"""
from __future__ import annotations

import logging
import os
from typing import Any, Dict, Iterable, Optional

import torch
import torch.distributed as dist

from flairhip.distributed import GradSync, ShardedLoader, ensure_process_group

logger = logging.getLogger(__name__)


def check_batchnorm_and_batch_size(config: Dict[str, Any], seg_module: torch.nn.Module) -> None:
    """Abort on BatchNorm with batch size 1 (reference :17-32): batch statistics of one sample are degenerate."""
    from flairhip.nn import HipBatchNorm2d
    if config["hyperparams"]["batch_size"] == 1 and any(isinstance(m, HipBatchNorm2d) for m in seg_module.modules()):
        raise SystemExit("BatchNorm layers need a batch size > 1 for training")


def _to_device(batch: dict, device) -> dict:
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


class DevicePrefetcher:
    """Host batches -> device batches, one batch ahead on a copy stream: while the device runs step k the host fetches
    batch k+1 from the loader and its H2D copy proceeds next to the compute kernels (the reference schema moves 25 MB
    per tile -- f32 imagery + f32 one-hot labels -- i.e. ~15 ms of PCIe time per 32-tile batch, as long as the step
    itself).  Pinned loader output (DataLoader(pin_memory=True)) makes the copies asynchronous; pageable tensors
    still work, their copies just block the host."""

    def __init__(self, loader: Iterable, device: torch.device):
        self.loader, self.device = loader, device
        self.stream = torch.cuda.Stream(device)

    def __len__(self) -> int:
        return len(self.loader)

    def _stage(self, host: Optional[dict]):
        if host is None:
            return None
        with torch.cuda.stream(self.stream):
            dev = _to_device(host, self.device)
            done = torch.cuda.Event()
            done.record(self.stream)
        return dev, done

    def __iter__(self):
        it = iter(self.loader)
        cur = self._stage(next(it, None))
        while cur is not None:
            batch, done = cur
            main = torch.cuda.current_stream(self.device)
            main.wait_event(done)
            for v in batch.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(main)  # allocated on the copy stream, consumed on the compute stream
            yield batch  # the consumer enqueues step k and comes back for more
            cur = self._stage(next(it, None))  # fetch + copy of batch k+1 overlap step k on the device


class AugmentedLoader:
    """Training loader + ``batch["AUG"]``: one flip / rotation code per sample (flairhip.augment.draw_codes, the
    reference's use_augmentation draws), a pinned uint8 [B] host tensor that the prefetcher stages like every other
    entry; the layout and label kernels apply it on the device.  The generator is seeded from (seed, rank, epoch), so
    ranks draw different transforms and a rerun draws the same.  A batch that already carries "AUG" (a dataset drawing
    its own, as the reference's does) is left alone."""

    def __init__(self, loader: Iterable, config: Dict[str, Any], seed: int = 0, rank: int = 0):
        self.loader, self.seed, self.rank, self.epoch = loader, seed, rank, 0
        mods = config["modalities"]
        # the entries whose leading dimension is the batch size: labels first, then the active inputs
        self.keys = list(config.get("labels", [])) + [m for m, on in mods.get("inputs", {}).items() if on]

    def __len__(self) -> int:
        return len(self.loader)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch
        if isinstance(self.loader, ShardedLoader) or getattr(self.loader, "rank_sharded", False):
            self.loader.set_epoch(epoch)  # a new permutation per epoch (shared by the ranks, as Lightning draws it, or
            # of the rank's own fixed share for the loaders of flair_hub.data.datamodule)

    def rng(self):
        from flairhip.augment import rank_epoch_rng
        return rank_epoch_rng(self.seed, self.rank, self.epoch)

    def __iter__(self):
        from flairhip.augment import draw_codes
        rng = self.rng()
        for batch in self.loader:
            if "AUG" not in batch:
                # a batch of the resident path carries the sample indices instead of images and labels
                key = "INDEX" if torch.is_tensor(batch.get("INDEX")) else \
                    next((k for k in self.keys if k in batch and torch.is_tensor(batch[k])), None)
                if key is None:
                    raise KeyError("use_augmentation: the batch holds none of the configured labels / inputs")
                codes = torch.from_numpy(draw_codes(int(batch[key].shape[0]), rng=rng))
                batch = dict(batch)
                batch["AUG"] = codes.pin_memory() if torch.cuda.is_available() else codes
            yield batch


def _capturable(optimizer) -> bool:
    """the optimizers whose step GraphedTrainStep can capture: torch's Adam / AdamW and flairhip.optim.HipAdamW / HipAdam
    (what SegmentationTask._init_optimizer builds on the GPU by default; they derive from torch.optim.Optimizer alone).
    All of them keep step counters and, after make_capturable, the learning rate on the device.  SGD stays eager."""
    from flairhip.optim import HipAdamW
    return isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW, HipAdamW))


class HipTrainer:
    """The subset of pytorch_lightning.Trainer the reference relies on.

    ``hip_graph=True``: fit() runs two ordinary steps (they size every workspace, fill the weight-pack plan and create the
    optimizer state), captures forward + loss + backward + optimizer step into a hipGraph at the third
    (flairhip.graph.GraphedTrainStep; several ranks: graph(forward + backward) -> GradSync.reduce_grads -> graph(optimizer))
    and replays it for every later batch of the captured shapes and dtypes.  Captured: Adam / AdamW, torch's or
    flairhip.optim's.  Eager, by design: SGD; modality dropout (the model draws on the host per step); a batch whose
    tensors differ in key, shape or dtype from the captured one (that step alone: the batches after it replay again).
    What a fit did is left on the trainer, and train() returns that trainer:
      ``graph_built``   a GraphedTrainStep was constructed
      ``graph_replays`` optimizer steps that were replays of it
      ``eager_steps``   optimizer steps that ran eagerly (the two before the capture and every fallback)
    graph_replays + eager_steps is the number of optimizer steps of the last fit()."""

    def __init__(self, accelerator: str = "gpu", devices: int = 1, strategy: str = "auto", num_nodes: int = 1,
                 max_epochs: int = 1, default_root_dir: Optional[str] = None, monitor: str = "val_miou",
                 monitor_mode: str = "max", max_steps: Optional[int] = None, hip_graph: bool = False,
                 callbacks: Optional[Iterable] = None, **unused):
        if accelerator not in ("gpu", "cuda", "auto"):
            raise RuntimeError("HipTrainer drives the MI355X path only (accelerator='gpu'); the CPU restatement "
                               "lives in oracle/ and is test infrastructure")
        self.max_epochs, self.max_steps = max_epochs, max_steps
        # forward + loss + backward + optimizer captured once and replayed per batch (flairhip.graph.GraphedTrainStep;
        # several ranks: graph(forward + backward) -> bucketed all-reduce -> graph(optimizer)); batches of another
        # shape and modality dropout fall back to eager steps
        self.hip_graph = bool(hip_graph)
        self.default_root_dir = default_root_dir
        self.monitor, self.monitor_mode = monitor, monitor_mode
        # prediction writers (flair_hub.writer.PredictionWriter): predict() calls their write_on_batch_end after every
        # predict_step and their on_predict_epoch_end at the end, as Lightning does for a BasePredictionWriter
        self.callbacks = list(callbacks or [])
        local = int(os.environ.get("LOCAL_RANK", "0"))
        # FFA_DIST_BACKEND=gloo rehearses several ranks on a one-GPU box: they then share cuda:0
        ndev = max(torch.cuda.device_count(), 1)
        self.device = torch.device("cuda", local % ndev if os.environ.get("FFA_DIST_BACKEND") == "gloo" else local)
        # Lightning's DDP strategy sets the process group up itself (reference trainers.py:81-91 only names the
        # strategy); under torchrun (WORLD_SIZE > 1) so does this trainer, before anything collective happens
        ensure_process_group(self.device)
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        if devices not in (None, "auto") and int(devices) * int(num_nodes) > 1 and self.world_size == 1:
            raise RuntimeError(f"HipTrainer: {devices} device(s) x {num_nodes} node(s) requested but this is a single "
                               "process: launch one process per GPU with `python -m torch.distributed.run "
                               "--nproc-per-node N ...` (the trainer never spawns ranks itself)")
        self.seed = int(unused.get("seed", 0))
        self.estimated_stepping_batches = 0
        self.callback_metrics: Dict[str, Any] = {}
        self.best_model_path = None
        self.optimizers = []
        self.graph_built, self.graph_replays, self.eager_steps = False, 0, 0  # of the last fit(): see the class docstring

    # ---- fit -------------------------------------------------------------------------------------

    def _shard(self, loader, shuffle=None, drop_last=True):
        """the rank's share of a loader (what Lightning's DistributedSampler injection does under DDP)"""
        if loader is None or self.world_size == 1 or isinstance(loader, ShardedLoader):
            return loader
        if getattr(loader, "rank_sharded", False):  # flair_hub.data.datamodule: already the rank's fixed share
            return loader
        return ShardedLoader(loader, self.rank, self.world_size, shuffle=shuffle, seed=self.seed, drop_last=drop_last)

    @staticmethod
    def _attach_store(model, datamodule) -> None:
        """a data module with a device-resident sample store yields 'INDEX' batches: the model gathers them from it"""
        store = getattr(datamodule, "store", None)
        if store is not None and hasattr(model, "attach_store"):
            model.attach_store(store)

    def fit(self, model, datamodule=None, train_dataloaders: Optional[Iterable] = None,
            val_dataloaders: Optional[Iterable] = None) -> None:
        torch.cuda.set_device(self.device)
        model.to(self.device)
        model.trainer = self
        if datamodule is not None:
            datamodule.setup("fit")
            self._attach_store(model, datamodule)
            train_dataloaders = datamodule.train_dataloader()
            val_dataloaders = datamodule.val_dataloader() if hasattr(datamodule, "val_dataloader") else None
        train_dataloaders = self._shard(train_dataloaders, drop_last=True)
        val_dataloaders = self._shard(val_dataloaders, shuffle=False, drop_last=False)
        if model.config.get("modalities", {}).get("pre_processings", {}).get("use_augmentation", False):
            # flips and rotations by k * 90 degrees, drawn per sample here and applied inside the layout / label kernels
            train_dataloaders = AugmentedLoader(train_dataloaders, model.config, self.seed, self.rank)
        steps_per_epoch = len(train_dataloaders)
        self.estimated_stepping_batches = self.max_steps or steps_per_epoch * self.max_epochs

        opt_cfg = model.configure_optimizers()
        optimizer = opt_cfg["optimizer"] if isinstance(opt_cfg, dict) else opt_cfg
        sched_cfg = opt_cfg.get("lr_scheduler") if isinstance(opt_cfg, dict) else None
        scheduler = sched_cfg["scheduler"] if sched_cfg else None
        interval = sched_cfg.get("interval", "epoch") if sched_cfg else None
        model._lr_scheduler = scheduler
        self.optimizers = [optimizer]
        use_graph = self.hip_graph and not getattr(model, "mod_dropout", False) and _capturable(optimizer)
        self.graph_built, self.graph_replays, self.eager_steps = False, 0, 0
        graph_ddp = use_graph and self.world_size > 1
        # exact_unused: a parameter no rank produced a gradient for keeps grad = None, as under the reference's
        # ddp_find_unused_parameters_true and as in the single-GPU path (AdamW then skips it instead of decaying it);
        # graph mode runs without autograd hooks: the finished gradients are handed to reduce_grads()
        # graph mode reduces after backward (nothing to overlap with): one collective over all gradients; reduce_grads takes
        # every decision about a collective from values that are equal on all ranks (its docstring), so the two eager steps
        # before the capture and an eager fallback on one rank's odd batch keep the ranks' sequences of collectives equal
        sync = GradSync(model, hooks=not graph_ddp, exact_unused=True, **({"bucket_bytes": 1 << 30} if graph_ddp else {}))

        def reduce_now():
            ps = [p for p in model.parameters() if p.grad is not None]
            sync.reduce_grads(ps, [p.grad for p in ps])

        best = None
        done = False
        graphed, graph_sig, loss = None, None, None
        for epoch in range(self.max_epochs):
            model.train()
            if isinstance(train_dataloaders, (ShardedLoader, AugmentedLoader)) or \
                    getattr(train_dataloaders, "rank_sharded", False):
                train_dataloaders.set_epoch(epoch)  # a new shared permutation per epoch, as Lightning does
            for i, batch in enumerate(DevicePrefetcher(train_dataloaders, self.device)):
                if use_graph and graphed is None and model.global_step >= 2:
                    # two ordinary steps first: they size every workspace, fill the weight-pack plan and create the
                    # optimizer state, so the capture itself needs no warm-up steps that would move the weights
                    from flairhip.graph import GraphedTrainStep
                    # nothing may keep the previous step's autograd graph alive: its AccumulateGrad nodes are bound
                    # to the stream they were created on, and running them from the capture stream aborts the capture
                    loss = None
                    graphed = GraphedTrainStep(model, optimizer, {k: v for k, v in batch.items() if torch.is_tensor(v)},
                                               warmup_steps=0, grad_reduce=sync.reduce_grads if graph_ddp else None)
                    graph_sig = {k: (tuple(v.shape), v.dtype) for k, v in batch.items() if torch.is_tensor(v)}
                    self.graph_built = True
                if graphed is not None and graph_sig == {k: (tuple(v.shape), v.dtype) for k, v in batch.items()
                                                         if torch.is_tensor(v)}:
                    loss = graphed({k: v for k, v in batch.items() if torch.is_tensor(v)})
                    self.graph_replays += 1
                else:
                    self.eager_steps += 1
                    loss = model.training_step(batch, i)
                    optimizer.zero_grad(set_to_none=True)
                    loss.backward()
                    if graph_ddp:
                        reduce_now()
                    else:
                        sync.finish()
                    optimizer.step()
                if scheduler is not None and interval == "step":
                    scheduler.step()
                model.global_step += 1
                model.on_train_batch_end(loss, batch, i)
                if self.max_steps and model.global_step >= self.max_steps:
                    done = True
                    break
            model.on_train_epoch_end()
            if val_dataloaders is not None:
                self.validate(model, dataloaders=val_dataloaders)
                score = self.callback_metrics.get(self.monitor)
                if score is not None:
                    score = float(score)
                    better = best is None or (score > best if self.monitor_mode == "max" else score < best)
                    if better:
                        best = score
                        self._save_best(model, epoch, score)
                if scheduler is not None and interval == "epoch":
                    monitor = sched_cfg.get("monitor")
                    scheduler.step(self.callback_metrics[monitor]) if monitor else scheduler.step()
            if done:
                break
        sync.remove()

    def _save_best(self, model, epoch: int, score: float) -> None:
        if self.rank != 0 or not self.default_root_dir:
            return
        os.makedirs(self.default_root_dir, exist_ok=True)
        path = os.path.join(self.default_root_dir, f"ckpt-epoch={epoch:02d}-{self.monitor}={score:.2f}.ckpt")
        torch.save({"state_dict": model.state_dict(), "epoch": epoch}, path)
        self.best_model_path = path

    # ---- validate / predict ----------------------------------------------------------------------

    @torch.no_grad()
    def validate(self, model, datamodule=None, dataloaders: Optional[Iterable] = None):
        model.to(self.device)
        model.trainer = self
        if datamodule is not None:
            datamodule.setup("validate")
            self._attach_store(model, datamodule)
            dataloaders = datamodule.val_dataloader()
        dataloaders = self._shard(dataloaders, shuffle=False, drop_last=False)
        model.eval()
        for i, batch in enumerate(dataloaders):
            model.validation_step(_to_device(batch, self.device), i)
        model.on_validation_epoch_end()
        self.callback_metrics.update({k: (float(v) if torch.is_tensor(v) else v) for k, v in model._logged.items()})
        return [dict(self.callback_metrics)]

    @torch.no_grad()
    def predict(self, model, datamodule=None, dataloaders: Optional[Iterable] = None, return_predictions: bool = True):
        model.to(self.device)
        model.trainer = self
        if datamodule is not None:
            datamodule.setup("predict")
            dataloaders = datamodule.predict_dataloader()
        dataloaders = self._shard(dataloaders, shuffle=False, drop_last=False)  # every rank predicts its own share
        model.eval()
        writers = [c for c in self.callbacks if hasattr(c, "write_on_batch_end")]
        outs = []
        for i, batch in enumerate(dataloaders):
            dev_batch = _to_device(batch, self.device)
            out = model.predict_step(dev_batch, i)
            for w in writers:
                w.write_on_batch_end(self, model, out, None, dev_batch, i, 0)
            if return_predictions:
                outs.append(out)
        for c in self.callbacks:
            if hasattr(c, "on_predict_epoch_end"):
                c.on_predict_epoch_end(self, model)
        return outs


def train(config: Dict[str, Any], data_module, seg_module, out_dir: str) -> HipTrainer:
    """Same role as the reference's train(): build the trainer from config['hardware'] / ['hyperparams'], fit,
    then run a final validation."""
    check_batchnorm_and_batch_size(config, seg_module)
    hw = config.get("hardware", {})
    trainer = HipTrainer(accelerator=hw.get("accelerator", "gpu"), devices=hw.get("gpus_per_node", 1),
                         strategy=hw.get("strategy", "auto"), num_nodes=hw.get("num_nodes", 1),
                         max_epochs=config["hyperparams"]["num_epochs"], default_root_dir=out_dir,
                         monitor=config.get("saving", {}).get("ckpt_monitor", "val_miou"),
                         monitor_mode=config.get("saving", {}).get("ckpt_monitor_mode", "max"),
                         hip_graph=bool(hw.get("hip_graph", False)))
    trainer.fit(seg_module, datamodule=data_module)
    trainer.validate(seg_module, datamodule=data_module)
    return trainer


def predict(config: Dict[str, Any], data_module, seg_module, out_dir: str):
    """Same role as the reference's predict() (:111-136): a PredictionWriter writes PRED_<label file> rasters
    (tasks.write_files), accumulates the confusion matrix against the label files and leaves metrics.json and
    confmat_predict.npy under out_dir.  ``tasks.metrics_only`` without ``tasks.predict`` scores the rasters of an
    earlier run instead of predicting.  -> the writer (its accumulated_confmats hold the matrices)"""
    from flair_hub.writer.prediction_writer import PredictionWriter
    writer = PredictionWriter(config, output_dir=os.path.join(out_dir), write_interval="batch")
    tasks = config.get("tasks", {})
    if tasks.get("metrics_only", False) and not tasks.get("predict", True):
        writer.load_predictions_and_compute_metrics()
        return writer
    hw = config.get("hardware", {})
    trainer = HipTrainer(accelerator=hw.get("accelerator", "gpu"), devices=hw.get("gpus_per_node", 1),
                         strategy=hw.get("strategy", "auto"), num_nodes=hw.get("num_nodes", 1), callbacks=[writer])
    trainer.predict(seg_module, datamodule=data_module, return_predictions=False)
    return writer
