"""FlairDataModule -- counterpart of the reference's flair_hub/data/datamodule.py (:9-121), plus the device-resident
sample cache.

Three batch schemas leave this module ('Training from a dataset on disk'):

* reference (``cache="none"``, ``device_prepare=False``): the reference's DataLoaders over flair_dataset -- normalised
  float32 inputs, one-hot labels, ``ID_<task>``, padded time series;
* streamed raw (``cache="none"``, ``device_prepare=True``): raw samples as decoded, ``<MOD>_NORM`` f32 [2, C_out],
  uint8 label channels and the ``RAW_LABELS`` marker; the device normalises, takes the elevation difference and applies
  the label rule;
* resident (``cache="device"``): on the first setup every patch of the train and validation splits is decoded once into
  a flairhip.sample_store.SampleStore, and a batch is ``{"INDEX": int32 [B] (pinned), "ID_<task>": [...]}``.  With
  ``series_cache=True`` the Sentinel time series go into the store as well (ragged, one SeriesStore per modality),
  and the batch also carries ``"<SENSOR>_DATES"``: float32 [B, T], the samples' date offsets zero-padded to the longest
  series of the batch -- the reference's own key, and what tells the model and the captured step the batch's T.
  Without it (the default) an enabled ``*_TS`` input keeps the whole dataset on the streamed path.

Sharding of the two device schemas: rank r owns the fixed share ``r::world_size`` of a split (it stores nothing else)
and draws a seeded permutation of that share per epoch; the rank is the process group's, or RANK / WORLD_SIZE of the
launcher when the group does not exist yet (the store is built before the trainer).  This is NOT DistributedSampler's rule, which reshuffles the
whole split across the ranks every epoch; with a resident store a global reshuffle would move patches between cards."""
from __future__ import annotations

import logging
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader

from flair_hub.data.dataloader import MONO_KEYS, elevation_mode, flair_dataset
from flair_hub.data.utils_data.padding import pad_collate_flair

logger = logging.getLogger(__name__)

MAX_DECODE_THREADS = 16   # never sized by os.cpu_count(): a shared machine shows far more CPUs than a job may use
FILL_CHUNK = 64           # patches per pinned staging buffer while the store is filled
CACHE_SHARE = 0.6         # default budget: this share of the device memory that is free when the store is built


def rank_share(n: int, rank: int, world_size: int) -> np.ndarray:
    """the samples of a split rank ``rank`` owns: rank, rank + world_size, ... (disjoint, and together the split)"""
    return np.arange(int(rank), int(n), max(int(world_size), 1), dtype=np.int64)


def epoch_permutation(n: int, seed: int, rank: int, epoch: int) -> np.ndarray:
    """the order a rank visits the n samples of its share in one epoch: reproducible per (seed, rank, epoch)"""
    return np.random.RandomState([int(seed) & 0xffffffff, int(rank), int(epoch), 0x5a]).permutation(int(n))


def _rank_world():
    """(rank, world size) of this process: the process group's when there is one, otherwise what the launcher put into
    RANK / WORLD_SIZE (torchrun) -- the data module is set up before HipTrainer creates the group"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    rank = int(os.environ.get("RANK", "0") or 0)
    if world < 1 or not 0 <= rank < world:
        raise RuntimeError(f"RANK={rank} / WORLD_SIZE={world} name no rank of a process group")
    return rank, world


def _rank_device() -> torch.device:
    """the card of this process, by HipTrainer's rule: LOCAL_RANK (ranks sharing cards in the gloo rehearsal)"""
    local = int(os.environ.get("LOCAL_RANK", "0") or 0)
    ndev = max(torch.cuda.device_count(), 1)
    return torch.device("cuda", local % ndev if os.environ.get("FFA_DIST_BACKEND") == "gloo" else local)


class RankShareLoader:
    """Batches over a rank's fixed share of a split.  ``fetch(positions)`` turns positions of the share (in visiting
    order) into a batch dict.  Training: a new seeded permutation per epoch (set_epoch); validation: ascending order."""

    rank_sharded = True  # HipTrainer._shard leaves such a loader alone

    def __init__(self, n: int, batch_size: int, fetch: Callable[[np.ndarray], dict], shuffle: bool, drop_last: bool,
                 seed: int = 0, rank: int = 0, ahead=None):
        """``ahead``: an executor; batch k + 1 is then fetched on it while the consumer works on batch k"""
        self.n, self.batch_size, self.fetch, self.ahead = int(n), int(batch_size), fetch, ahead
        self.shuffle, self.drop_last, self.seed, self.rank, self.epoch = shuffle, drop_last, int(seed), int(rank), 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return self.n // self.batch_size if self.drop_last else -(-self.n // self.batch_size)

    def order(self) -> np.ndarray:
        return epoch_permutation(self.n, self.seed, self.rank, self.epoch) if self.shuffle else np.arange(self.n)

    def __iter__(self):
        order = self.order()
        parts = [order[b * self.batch_size:(b + 1) * self.batch_size] for b in range(len(self))]
        if self.ahead is None:
            for part in parts:
                yield self.fetch(part)
            return
        pending = self.ahead.submit(self.fetch, parts[0]) if parts else None
        for b in range(len(parts)):
            batch = pending.result()
            pending = self.ahead.submit(self.fetch, parts[b + 1]) if b + 1 < len(parts) else None
            yield batch


class _StoreFallback(Exception):
    """a sample the store cannot take: the split stays streamed (the message names the patch)"""


def default_cache_bytes(device) -> int:
    free, _total = torch.cuda.mem_get_info(device)
    return int(free * CACHE_SHARE)


class FlairDataModule:
    def __init__(self, config, dict_train: Optional[Dict] = None, dict_val: Optional[Dict] = None,
                 dict_test: Optional[Dict] = None, num_workers: int = 1, batch_size: int = 2, drop_last: bool = True,
                 use_augmentations: bool = True, cache: str = "none", cache_bytes: Optional[int] = None,
                 device_prepare: Optional[bool] = None, seed: Optional[int] = None, device=None,
                 series_cache: bool = False):
        if cache not in ("none", "device"):
            raise ValueError(f"cache must be 'none' or 'device', got {cache!r}")
        self.config = config
        self.dict_train, self.dict_val, self.dict_test = dict_train, dict_val, dict_test
        self.batch_size, self.num_workers, self.drop_last = batch_size, num_workers, drop_last
        self.use_augmentations = use_augmentations
        self.cache, self.cache_bytes = cache, cache_bytes
        self.series_cache = bool(series_cache)  # cache="device" only: time series enter the store too
        # raw samples + device-side preparation: what the resident path needs, and optional for the streamed one
        self.device_prepare = (cache == "device") if device_prepare is None else bool(device_prepare)
        self.seed = int(config.get("hyperparams", {}).get("seed", 0) if seed is None else seed)
        self.device = device
        self.train_dataset = self.val_dataset = self.pred_dataset = None
        self.store = None            # the SampleStore once it is built (HipTrainer attaches it to the model)
        self._store_tried = False
        self._offsets: Dict[str, int] = {}
        self._shares: Dict[str, np.ndarray] = {}
        self._norm_cache = None
        self._rank, self._world = 0, 1
        self._pool: Optional[ThreadPoolExecutor] = None    # decodes the patches of a streamed raw batch
        self._ahead: Optional[ThreadPoolExecutor] = None   # builds the next streamed raw batch while this one trains

    def prepare_data(self):
        pass

    # ---- datasets -------------------------------------------------------------------------------------------------------

    def _create_flair_dataset(self, dict_paths: Dict, use_augmentations, device_prepare: bool = False) -> flair_dataset:
        return flair_dataset(self.config, dict_paths=dict_paths, use_augmentations=use_augmentations,
                             device_prepare=device_prepare)

    def setup(self, stage: Optional[str] = None):
        if stage in ("fit", "validate"):
            if self.train_dataset is None:
                # device_prepare: the augmentation is not the dataset's -- the trainer draws the codes (batch['AUG'])
                aug = None if self.device_prepare else self.use_augmentations
                self.train_dataset = self._create_flair_dataset(self.dict_train, aug, self.device_prepare)
                self.val_dataset = self._create_flair_dataset(self.dict_val, None, self.device_prepare)
            if self.cache == "device" and not self._store_tried:
                self._store_tried = True
                self._build_store()
        elif stage == "predict":
            # one pass at batch size 1: nothing to gain from a store; the reference schema feeds the existing path
            self.pred_dataset = self._create_flair_dataset(self.dict_test, None, False)

    # ---- the device-resident store --------------------------------------------------------------------------------------

    def _norm_vectors(self, sample: dict) -> Dict[str, Optional[torch.Tensor]]:
        """{modality: f32 [2, C_out] or None}: supplied once, here, not per sample"""
        if self._norm_cache is None:
            out = {}
            for mod, v in self.train_dataset.norm_vectors().items():
                if isinstance(v, str):  # 'scaling': unsigned integers over their type's maximum, floats unchanged
                    t = sample[mod]
                    if t.dtype == torch.float32:
                        v = None
                    elif t.dtype in (torch.uint8, torch.uint16):
                        c = t.shape[0]
                        v = torch.tensor([[0.0] * c, [255.0 if t.dtype == torch.uint8 else 65535.0] * c])
                    else:
                        raise ValueError(f"norm_type 'scaling' takes unsigned integer or float samples, got {t.dtype}")
                out[mod] = v
            self._norm_cache = out
        return self._norm_cache

    def _store_spec(self, sample: dict):
        inputs = {m: (tuple(sample[m].shape), np.dtype(str(sample[m].dtype).replace("torch.", "")))
                  for m in MONO_KEYS if m in sample}
        labels = {t: tuple(sample[t].shape) for t in self.config["labels"]}
        return inputs, labels

    _TOO_LARGE = ("sample cache: %d patches need %.1f MB, the budget is %.1f MB: falling back to the streamed loaders "
                  "(a split is never stored in part)")

    def _build_store(self) -> None:
        from flairhip import ops
        from flairhip.sample_store import SampleStore, SeriesStore, store_bytes
        inputs_on = [m for m, on in self.config["modalities"]["inputs"].items() if on]
        series = [m for m in inputs_on if m.endswith("_TS")]
        if series and not self.series_cache:
            logger.info("sample cache: %s are time series of variable length and stay streamed: no store", series)
            return
        rank, world = self._rank, self._world = _rank_world()
        splits = {"train": self.train_dataset, "val": self.val_dataset}
        for ds in splits.values():
            ds.keep_dem_bands = True  # the store keeps both DEM bands; its kernel takes the difference
            ds.keep_series_raw = bool(series)  # ... and the series in their decoded sample type
        try:
            self._shares = {k: rank_share(len(ds), rank, world) for k, ds in splits.items()}
            n = sum(len(s) for s in self._shares.values())
            if n == 0:
                logger.info("sample cache: this rank's share is empty: no store")
                return
            k0 = next(k for k in splits if len(self._shares[k]))
            sample = splits[k0][int(self._shares[k0][0])]
            inputs, labels = self._store_spec(sample)
            need = store_bytes(n, inputs, labels)
            device = torch.device(self.device) if self.device is not None else _rank_device()
            budget = self.cache_bytes if self.cache_bytes is not None else default_cache_bytes(device)
            if need > budget:  # without the series, whose size is known only once they are decoded
                logger.info(self._TOO_LARGE, n, need / 1e6, budget / 1e6)
                return
            mode = elevation_mode(self.config)
            ids = {t: [] for t in self.config["labels"]}
            store = SampleStore(n, inputs, labels,
                                {t: len(self.config["labels_configs"][t]["value_name"]) for t in self.config["labels"]},
                                self._norm_vectors(sample),
                                {m: (mode if m == "DEM_ELEV" else ops.ELEV_NONE) for m in inputs}, device, ids)
            # the series are small: the one decoding pass keeps them on the host, and their sum of lengths sizes the
            # ragged stores afterwards
            held = {m: [] for m in series}
            at, offsets = 0, {}
            try:
                for k, ds in splits.items():
                    offsets[k] = at
                    at = self._fill(store, ds, self._shares[k], at, held)
            except _StoreFallback as why:
                logger.info("sample cache: %s: falling back to the streamed loaders (a split is never stored in part)",
                            why)
                return
            if series:
                spec = {m: (sum(len(a) for a, _ in held[m]), tuple(held[m][0][0].shape[1:]), held[m][0][0].dtype)
                        for m in series}
                need = store_bytes(n, inputs, labels, spec)
                if need > budget:
                    logger.info(self._TOO_LARGE, n, need / 1e6, budget / 1e6)
                    return
                pad_value = self.config["models"]["multitemp_model"].get("pad_value", 0)
                for m, (total, shape, dt) in spec.items():
                    st = SeriesStore(n, total, shape, dt, pad_value, device)
                    for c0 in range(0, n, FILL_CHUNK):
                        part = held[m][c0:c0 + FILL_CHUNK]
                        st.fill(c0, np.concatenate([a for a, _ in part]), np.concatenate([d for _, d in part]),
                                [len(a) for a, _ in part])
                    store.attach_series(m, st)
            if store.device.type == "cuda":
                torch.cuda.synchronize(store.device)
            self._offsets = offsets
            self.store = store
            logger.info("sample cache: %d patches (%.1f MB) resident on %s", n, store.bytes / 1e6, store.device)
        finally:
            for ds in splits.values():
                ds.keep_dem_bands = False
                ds.keep_series_raw = False

    def _series_of(self, sample: dict, mod: str, first) -> tuple:
        """(series in its stored sample type, float32 diff_dates) of one decoded sample, or _StoreFallback"""
        from flairhip.sample_store import series_dtype
        patch = next((sample[f"ID_{t}"] for t in self.config["labels"] if f"ID_{t}" in sample), "?")
        arr = sample.get(mod)
        if arr is None:
            raise _StoreFallback(f"{patch} has no {mod}")
        arr = np.asarray(arr)
        if arr.shape[0] == 0:
            raise _StoreFallback(f"the {mod} series of {patch} is empty after filtering")
        pp = self.config["modalities"].get("pre_processings", {})
        averaged = bool(pp.get("temporal_average_sentinel2" if mod == "SENTINEL2_TS" else "temporal_average_sentinel1"))
        arr = np.ascontiguousarray(arr.astype(series_dtype(arr.dtype, averaged), copy=False))
        if first is not None and (arr.shape[1:] != first.shape[1:] or arr.dtype != first.dtype):
            raise _StoreFallback(f"the {mod} planes of {patch} are {arr.shape[1:]} {arr.dtype}, those before it "
                                 f"{first.shape[1:]} {first.dtype}")
        return arr, np.asarray(sample[mod.replace("_TS", "_DATES")]).astype(np.float32)

    def _fill(self, store, ds: flair_dataset, share: np.ndarray, at: int, held: Optional[Dict[str, list]] = None) -> int:
        """decode the rank's share of one split once, in chunks through pinned buffers; -> the next free slot.
        ``held``: {time-series modality: [(series, diff_dates) per sample]}, kept on the host"""
        workers = max(1, min(MAX_DECODE_THREADS, int(self.num_workers) or 1))
        keys = list(store.inputs) + list(store.labels)
        pin = torch.cuda.is_available() and store.device.type == "cuda"
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for c0 in range(0, len(share), FILL_CHUNK):
                samples = list(pool.map(lambda i: ds[int(i)], share[c0:c0 + FILL_CHUNK]))
                for mod, rows in (held or {}).items():
                    for s in samples:
                        rows.append(self._series_of(s, mod, rows[0][0] if rows else None))
                chunk = {}
                for key in keys:
                    host = torch.stack([s[key] for s in samples])
                    chunk[key] = host.pin_memory() if pin else host
                store.fill(at, chunk)
                if pin:
                    torch.cuda.synchronize(store.device)  # the staging buffers are released next
                for t in store.ids:
                    store.ids[t] += [s[f"ID_{t}"] for s in samples]
                at += len(samples)
        return at

    # ---- loaders --------------------------------------------------------------------------------------------------------

    def _index_loader(self, split: str, shuffle: bool, drop_last: bool) -> RankShareLoader:
        store, off = self.store, self._offsets[split]
        rank = self._rank  # the rank whose share the store holds
        pin = torch.cuda.is_available()

        def fetch(pos: np.ndarray) -> dict:
            idx = torch.from_numpy((off + pos).astype(np.int32))
            batch = {"INDEX": idx.pin_memory() if pin else idx}
            for t in self.config["labels"]:
                batch[f"ID_{t}"] = store.ids_of(t, idx)
            for mod, st in store.series.items():  # [B, T], T the longest series of the batch
                batch[mod.replace("_TS", "_DATES")] = st.dates_of(idx)
            return batch

        return RankShareLoader(len(self._shares[split]), self.batch_size, fetch, shuffle, drop_last, self.seed, rank)

    def _raw_collate(self, samples: List[dict]) -> dict:
        batch = pad_collate_flair(samples)
        for mod, v in self._norm_vectors(samples[0]).items():
            if v is None and mod == "DEM_ELEV" and elevation_mode(self.config) == 1:
                # 'without' / 'scaling' of float samples: the raw 2-band DEM still goes through the layout kernel that
                # takes the difference, which is chosen by this entry -- the identity (x - 0) / 1 is exact
                v = torch.tensor([[0.0], [1.0]])
            if v is not None:
                batch[mod + "_NORM"] = v
        batch["RAW_LABELS"] = torch.ones(1, dtype=torch.uint8)
        return batch

    def _raw_loader(self, ds: flair_dataset, shuffle: bool, drop_last: bool) -> RankShareLoader:
        rank, world = _rank_world()
        share = rank_share(len(ds), rank, world)
        if self._pool is None:  # one pool per module, whatever the number of loaders made from it
            self._pool = ThreadPoolExecutor(max_workers=max(1, min(MAX_DECODE_THREADS, int(self.num_workers) or 1)))
            self._ahead = ThreadPoolExecutor(max_workers=1)
        pool = self._pool

        def fetch(pos: np.ndarray) -> dict:
            return self._raw_collate(list(pool.map(lambda i: ds[int(i)], share[pos])))

        return RankShareLoader(len(share), self.batch_size, fetch, shuffle, drop_last, self.seed, rank, self._ahead)

    def teardown(self, stage: Optional[str] = None) -> None:
        """release the decode threads (Lightning's hook name); the module can be set up again afterwards"""
        for pool in (self._pool, self._ahead):
            if pool is not None:
                pool.shutdown(wait=True)
        self._pool = self._ahead = None

    def _create_dataloader(self, dataset, batch_size: int, shuffle: bool, drop_last: bool):
        # worker processes are spawned, not forked: the raster readers keep thread pools a forked child would inherit
        # mid-flight
        extra = {"multiprocessing_context": "spawn"} if self.num_workers else {}
        return DataLoader(dataset=dataset, batch_size=batch_size, shuffle=shuffle, num_workers=self.num_workers,
                          drop_last=drop_last, collate_fn=pad_collate_flair, **extra)

    def _loader(self, split: str, ds, shuffle: bool):
        if self.store is not None:
            return self._index_loader(split, shuffle, self.drop_last)
        if self.device_prepare:
            return self._raw_loader(ds, shuffle, self.drop_last)
        return self._create_dataloader(ds, self.batch_size, shuffle=shuffle, drop_last=self.drop_last)

    def train_dataloader(self):
        return self._loader("train", self.train_dataset, True)

    def val_dataloader(self):
        return self._loader("val", self.val_dataset, False)

    def predict_dataloader(self):
        return self._create_dataloader(self.pred_dataset, batch_size=1, shuffle=False, drop_last=False)

    def input_img_sizes(self) -> Optional[Dict[str, int]]:
        """H = W per stored modality when the resident path is active (its batches carry no image to look at)"""
        return self.store.img_sizes() if self.store is not None else None
