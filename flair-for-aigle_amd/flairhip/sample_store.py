"""Device-resident sample store: the patches of a dataset split, decoded once and kept in HBM as raw samples.

Per mono-temporal modality one raw tensor [N, C, h, w] in the rasters' sample type (uint8 aerial bands, the 2-band
float32 DEM), per task one uint8 label tensor [N, H, W] (the raw label channel) and per modality the [2, C_out]
normalisation vectors.  A training step then needs no image over PCIe: its batch is an int32 index vector, and
ops.gather_layout / ops.gather_labels (csrc/sample_gather.hip) read the indexed samples through the augmentation's
gather while they normalise, take the elevation difference, pad the channels and apply the label rule -- the layout
pass the step makes anyway.  About 1.6 MB per FLAIR-HUB patch (512 x 512 x 5 uint8 + labels + DEM), so a rank's share
of a split fits the 288 GB of an MI355X.

Time series (``*_TS``) are of variable length.  They enter the store only on request (``series=``), each as a
ragged SeriesStore: the dates of all samples back to back, an offset vector and a pad flag per date;
ops.gather_series (csrc/series_gather.hip) turns an index vector into the padded batch the U-TAE expects and its pad
flags.  Without ``series=`` they stay on the streamed path, as before."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

NP_TO_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.int16): torch.int16,
               np.dtype(np.float32): torch.float32}


def series_bytes(n: int, dates: int, shape: Tuple[int, int, int], dtype) -> int:
    """device bytes of a SeriesStore of ``n`` samples with ``dates`` dates in all: the data [D, C, h, w], the int32
    offsets [n + 1] and the uint8 pad flags [D]"""
    return int(dates) * int(np.prod(shape)) * np.dtype(dtype).itemsize + 4 * (int(n) + 1) + int(dates)


def store_bytes(n: int, inputs: Dict[str, Tuple[Tuple[int, int, int], np.dtype]], labels: Dict[str, Tuple[int, int]],
                series: Optional[Dict[str, Tuple[int, Tuple[int, int, int], np.dtype]]] = None) -> int:
    """bytes of a store of ``n`` samples: inputs {modality: ((C, h, w), sample type)}, labels {task: (H, W)},
    series {modality: (D = dates of all samples, (C, h, w), sample type)} (series_bytes each)"""
    per = sum(int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in inputs.values())
    per += sum(int(h) * int(w) for h, w in labels.values())
    return int(n) * per + sum(series_bytes(n, d, shape, dt) for d, shape, dt in (series or {}).values())


def series_dtype(decoded, averaged: bool) -> np.dtype:
    """the stored sample type of a series: float32 for a temporal average (the float64 mean rounded once, what
    ``torch.tensor(v, dtype=torch.float32)`` does on the streamed path), otherwise the decoded type when it is one of
    the four stored kinds and float32 when it is not"""
    decoded = np.dtype(decoded)
    return decoded if not averaged and decoded in NP_TO_TORCH else np.dtype(np.float32)


class SeriesStore:
    """The time series of one modality for ``n`` samples, ragged: ``data`` [D, C, h, w] on the device holds the dates
    of all samples back to back, exactly as the dataset yields them before augmentation and before the float32 cast;
    ``offsets`` int32 [n + 1] (device; ``offsets_host`` the numpy copy) says where a sample's dates start; ``is_pad``
    uint8 [D] (device) is 1 where every element of the stored date equals ``pad_value`` -- what detect_pad_images
    reports for that date on the streamed path, a real acquisition constant at the pad value included; ``dates``
    float32 [D] (host) are the samples' diff_dates.  Samples are appended in order by fill()."""

    def __init__(self, n: int, dates: int, shape: Tuple[int, int, int], dtype, pad_value: float = 0.0, device="cuda"):
        if n < 1 or dates < n:
            raise ValueError(f"SeriesStore: {n} samples with {dates} dates (every sample needs at least one)")
        if dates >= 2 ** 31:
            raise ValueError(f"SeriesStore: {dates} dates do not fit the int32 offsets")
        if np.dtype(dtype) not in NP_TO_TORCH:
            raise ValueError(f"SeriesStore: samples are {np.dtype(dtype)}; uint8 / uint16 / int16 / float32 are stored")
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"SeriesStore: (C, h, w) expected, got {tuple(shape)}")
        self.n, self.total, self.device = int(n), int(dates), torch.device(device)
        self.shape, self.np_dtype, self.pad_value = tuple(int(v) for v in shape), np.dtype(dtype), float(pad_value)
        self.data = torch.empty((self.total,) + self.shape, dtype=NP_TO_TORCH[self.np_dtype], device=self.device)
        self.is_pad = torch.empty(self.total, dtype=torch.uint8, device=self.device)
        self.offsets_host = np.zeros(self.n + 1, dtype=np.int32)
        self.offsets: Optional[torch.Tensor] = None  # on the device once the last sample is in
        self.dates = np.zeros(self.total, dtype=np.float32)
        self.filled = 0

    @property
    def bytes(self) -> int:
        return series_bytes(self.n, self.total, self.shape, self.np_dtype)

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets_host)

    def fill(self, start: int, data, dates, lengths: Optional[Sequence[int]] = None) -> None:
        """samples ``start ..``: one sample's series [len, C, h, w] with its diff_dates [len], or a chunk of several
        back to back with their ``lengths``.  numpy arrays of the store's sample type; samples come in order."""
        data = np.ascontiguousarray(data)
        dates = np.asarray(dates)
        lengths = [int(data.shape[0])] if lengths is None else [int(v) for v in lengths]
        at = int(self.offsets_host[start]) if 0 <= start <= self.n else -1
        if start != self.filled or start + len(lengths) > self.n or min(lengths, default=0) < 1 or \
                sum(lengths) != data.shape[0] or dates.shape != (data.shape[0],) or at + data.shape[0] > self.total or \
                tuple(data.shape[1:]) != self.shape or data.dtype != self.np_dtype:
            raise ValueError(f"SeriesStore.fill: {tuple(data.shape)} {data.dtype} with lengths {lengths} at sample {start} "
                             f"does not fit [{self.total}, {self.shape}] {self.np_dtype} ({self.filled} samples in)")
        d = data.shape[0]
        flags = (data.reshape(d, -1).astype(np.float32) == np.float32(self.pad_value)).all(axis=1).astype(np.uint8)
        self.data[at:at + d].copy_(torch.from_numpy(data))
        self.is_pad[at:at + d].copy_(torch.from_numpy(flags))
        self.dates[at:at + d] = dates.astype(np.float32)
        self.offsets_host[start + 1:start + 1 + len(lengths)] = at + np.cumsum(lengths)
        self.filled = start + len(lengths)
        if self.filled == self.n:
            if int(self.offsets_host[-1]) != self.total:
                raise ValueError(f"SeriesStore.fill: {int(self.offsets_host[-1])} dates came, {self.total} were announced")
            self.offsets = torch.from_numpy(self.offsets_host).to(self.device)

    def dates_of(self, index) -> torch.Tensor:
        """float32 [B, T] on the host: the diff_dates of the samples ``index``, zero-padded to the longest of them --
        the '<SENSOR>_DATES' entry pad_collate_flair builds"""
        idx = [int(i) for i in (index.tolist() if torch.is_tensor(index) else index)]
        off = self.offsets_host
        T = max(int(off[i + 1] - off[i]) for i in idx)
        out = torch.zeros((len(idx), T), dtype=torch.float32)
        for b, i in enumerate(idx):
            out[b, :off[i + 1] - off[i]] = torch.from_numpy(self.dates[off[i]:off[i + 1]])
        return out


def series_batch_reference(store: SeriesStore, index, T: Optional[int] = None, codes=None, cp: Optional[int] = None,
                           fill: float = 0.0, pad_value: float = 0.0):
    """ops.gather_series as a numpy definition: -> (float32 [B*T, H, W, cp], uint8 [B*T]).  Each indexed sample is cast
    to float32, flipped / rotated in the reference's order (flip axis -1 if bit 0 of its code, flip axis -2 if bit 1,
    rot90 by bits 2-3), the samples are collated by pad_collate_flair (padded with ``fill``; ``T`` above the longest
    adds further padded dates) and laid out NHWC with zero pad channels; pad is 1 where a padded image is constant at
    ``pad_value``.  The compute type's rounding is not part of it (float32 out)."""
    from flair_hub.data.utils_data.padding import pad_collate_flair, pad_tensor
    idx = [int(i) for i in (index.tolist() if torch.is_tensor(index) else index)]
    data, off = store.data.cpu().numpy(), store.offsets_host
    samples = []
    for b, i in enumerate(idx):
        if not 0 <= i < store.n:
            raise ValueError(f"series_batch_reference: index {i} outside [0, {store.n})")
        x = data[off[i]:off[i + 1]].astype(np.float32)
        if codes is not None:
            code = int(codes[b]) & 15
            if code & 1:
                x = np.flip(x, axis=-1)
            if code & 2:
                x = np.flip(x, axis=-2)
            x = np.rot90(x, k=code >> 2, axes=(-2, -1))
        samples.append({"SENTINEL2_TS": torch.from_numpy(np.ascontiguousarray(x))})
    x = pad_collate_flair(samples, pad_value=fill)["SENTINEL2_TS"]  # [B, longest, C, H, W]
    T = x.shape[1] if T is None else int(T)
    if T < x.shape[1]:
        raise ValueError(f"series_batch_reference: the longest indexed series has {x.shape[1]} dates, T = {T}")
    x = torch.stack([pad_tensor(s, T, fill) for s in x]).numpy()
    B, _, C, H, W = x.shape
    flat = x.reshape(B * T, C, H, W)
    cp = ops.pad_channels(C) if cp is None else int(cp)
    out = np.zeros((B * T, H, W, cp), dtype=np.float32)
    out[..., :C] = flat.transpose(0, 2, 3, 1)
    pad = (flat.reshape(B * T, -1) == np.float32(pad_value)).all(axis=1).astype(np.uint8)
    return out, pad


class SampleStore:
    def __init__(self, n: int, inputs: Dict[str, Tuple[Tuple[int, int, int], np.dtype]],
                 labels: Dict[str, Tuple[int, int]], num_classes: Dict[str, int],
                 norms: Optional[Dict[str, Optional[torch.Tensor]]] = None,
                 elevation: Optional[Dict[str, int]] = None, device="cuda", ids: Optional[Dict[str, Sequence]] = None,
                 series: Optional[Dict[str, SeriesStore]] = None):
        """``inputs``: {modality: ((C, h, w), numpy sample type)}; ``labels``: {task: (H, W)}; ``num_classes``: {task: K};
        ``norms``: {modality: f32 [2, C_out] (mean, std) or None}; ``elevation``: {modality: ops.ELEV_*};
        ``ids``: {task: the N label paths}, handed out as ``ID_<task>`` by ids_of(); ``series``: {time-series modality:
        its SeriesStore over the same N samples} (attach_series adds one later)."""
        if n < 1:
            raise ValueError("SampleStore: an empty split cannot be stored")
        for mod in inputs:
            if mod.endswith("_TS"):
                raise ValueError(f"SampleStore: {mod} is a time series of variable length: it goes into series= as a "
                                 f"SeriesStore, or stays on the streamed path")
        self.n, self.device = int(n), torch.device(device)
        self.elevation = {m: int((elevation or {}).get(m, ops.ELEV_NONE)) for m in inputs}
        self.num_classes = {t: int(k) for t, k in num_classes.items()}
        self.ids = {t: list(v) for t, v in (ids or {}).items()}
        self._spec = (dict(inputs), dict(labels))
        self.inputs: Dict[str, torch.Tensor] = {}
        for mod, (shape, dt) in inputs.items():
            if np.dtype(dt) not in NP_TO_TORCH:
                raise ValueError(f"SampleStore: {mod} samples are {np.dtype(dt)}; uint8 / uint16 / int16 / float32 are stored")
            if self.elevation[mod] != ops.ELEV_NONE and shape[0] != 2:
                raise ValueError(f"SampleStore: the elevation modes need the 2 bands of {mod}, got {shape[0]}")
            self.inputs[mod] = torch.empty((self.n,) + tuple(shape), dtype=NP_TO_TORCH[np.dtype(dt)], device=self.device)
        self.labels = {t: torch.empty((self.n, int(h), int(w)), dtype=torch.uint8, device=self.device)
                       for t, (h, w) in labels.items()}
        self.norm: Dict[str, Optional[torch.Tensor]] = {}
        for mod in inputs:
            v = (norms or {}).get(mod)
            c_out = self.channels(mod)
            if v is None:
                if self.inputs[mod].dtype != torch.float32:
                    raise ValueError(f"SampleStore: {mod} holds integer samples: mean / std are required")
                self.norm[mod] = None
                continue
            v = torch.as_tensor(v, dtype=torch.float32)
            if v.ndim != 2 or v.shape[0] != 2 or v.shape[1] != c_out:
                raise ValueError(f"SampleStore: {mod} needs [2, {c_out}] normalisation vectors (one entry per output "
                                 f"channel), got {tuple(v.shape)}")
            self.norm[mod] = v.to(self.device).contiguous()
        self.filled = 0
        self.series: Dict[str, SeriesStore] = {}
        for mod, st in (series or {}).items():
            self.attach_series(mod, st)

    def attach_series(self, mod: str, st: SeriesStore) -> None:
        if not isinstance(st, SeriesStore) or st.n != self.n or st.device.type != self.device.type:
            raise ValueError(f"SampleStore: the series store of {mod} must hold the same {self.n} samples on {self.device}")
        self.series[mod] = st

    # ---- size ----------------------------------------------------------------------------------------------------------

    @property
    def bytes(self) -> int:
        return store_bytes(self.n, *self._spec) + sum(st.bytes for st in self.series.values())

    def fits(self, budget_bytes: int) -> bool:
        return self.bytes <= int(budget_bytes)

    def channels(self, mod: str) -> int:
        """channels the modality's encoder sees (after the elevation pre-processing)"""
        return ops.ELEV_CHANNELS[self.elevation[mod]] or self._spec[0][mod][0][0]

    def img_sizes(self) -> Dict[str, int]:
        sizes = {m: int(t.shape[-1]) for m, t in self.inputs.items()}
        sizes.update({m: int(st.shape[-1]) for m, st in self.series.items()})
        return sizes

    # ---- filling -------------------------------------------------------------------------------------------------------

    def fill(self, start: int, chunk: Dict[str, torch.Tensor]) -> None:
        """samples ``start .. start + n`` from host tensors {modality or task: [n, ...]} (pinned buffers make the
        copies asynchronous; the caller must not reuse a buffer before synchronize())"""
        for key, src in chunk.items():
            dst = self.inputs[key] if key in self.inputs else self.labels[key]
            n = src.shape[0]
            if start < 0 or start + n > self.n or tuple(src.shape[1:]) != tuple(dst.shape[1:]) or src.dtype != dst.dtype:
                raise ValueError(f"SampleStore.fill: {key} chunk {tuple(src.shape)} {src.dtype} at {start} does not fit "
                                 f"{tuple(dst.shape)} {dst.dtype}")
            dst[start:start + n].copy_(src, non_blocking=True)
            self.filled = max(self.filled, start + n)

    # ---- batches -------------------------------------------------------------------------------------------------------

    def input_nhwc(self, mod: str, index: torch.Tensor, dtype: torch.dtype, codes: Optional[torch.Tensor] = None,
                   cp: Optional[int] = None) -> torch.Tensor:
        norm = self.norm[mod]
        mean, std = (None, None) if norm is None else (norm[0], norm[1])
        return ops.gather_layout(self.inputs[mod], index, dtype, codes, mean, std, cp, self.elevation[mod])

    def targets(self, task: str, index: torch.Tensor, codes: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.gather_labels(self.labels[task], index, self.num_classes[task], codes)

    def ids_of(self, task: str, index) -> list:
        return [self.ids[task][int(i)] for i in (index.tolist() if torch.is_tensor(index) else index)]

    def batch(self, index: torch.Tensor, codes: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float32
              ) -> dict:
        """the samples ``index`` (int32 [B], host or device) without a model: {modality: NHWC tensor of ``dtype``
        (normalised, channel-padded), task: uint8 class indices [B, H, W]}, flipped / rotated by ``codes``"""
        if codes is not None:
            codes = codes.to(self.device)
        out = {m: self.input_nhwc(m, index, dtype, codes) for m in self.inputs}
        out.update({t: self.targets(t, index, codes) for t in self.labels})
        return out
