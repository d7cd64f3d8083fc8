"""Device-resident sample store: the patches of a dataset split, decoded once and kept in HBM as raw samples.

Per mono-temporal modality one raw tensor [N, C, h, w] in the rasters' sample type (uint8 aerial bands, the 2-band
float32 DEM), per task one uint8 label tensor [N, H, W] (the raw label channel) and per modality the [2, C_out]
normalisation vectors.  A training step then needs no image over PCIe: its batch is an int32 index vector, and
ops.gather_layout / ops.gather_labels (csrc/sample_gather.hip) read the indexed samples through the augmentation's
gather while they normalise, take the elevation difference, pad the channels and apply the label rule -- the layout
pass the step makes anyway.  About 1.6 MB per FLAIR-HUB patch (512 x 512 x 5 uint8 + labels + DEM), so a rank's share
of a split fits the 288 GB of an MI355X.

Time series (``*_TS``) are of variable length and never enter the store: they stay on the streamed path."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

NP_TO_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.int16): torch.int16,
               np.dtype(np.float32): torch.float32}


def store_bytes(n: int, inputs: Dict[str, Tuple[Tuple[int, int, int], np.dtype]], labels: Dict[str, Tuple[int, int]]
                ) -> int:
    """bytes of a store of ``n`` samples: inputs {modality: ((C, h, w), sample type)}, labels {task: (H, W)}"""
    per = sum(int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in inputs.values())
    per += sum(int(h) * int(w) for h, w in labels.values())
    return int(n) * per


class SampleStore:
    def __init__(self, n: int, inputs: Dict[str, Tuple[Tuple[int, int, int], np.dtype]],
                 labels: Dict[str, Tuple[int, int]], num_classes: Dict[str, int],
                 norms: Optional[Dict[str, Optional[torch.Tensor]]] = None,
                 elevation: Optional[Dict[str, int]] = None, device="cuda", ids: Optional[Dict[str, Sequence]] = None):
        """``inputs``: {modality: ((C, h, w), numpy sample type)}; ``labels``: {task: (H, W)}; ``num_classes``: {task: K};
        ``norms``: {modality: f32 [2, C_out] (mean, std) or None}; ``elevation``: {modality: ops.ELEV_*};
        ``ids``: {task: the N label paths}, handed out as ``ID_<task>`` by ids_of()."""
        if n < 1:
            raise ValueError("SampleStore: an empty split cannot be stored")
        for mod in inputs:
            if mod.endswith("_TS"):
                raise ValueError(f"SampleStore: {mod} is a time series of variable length: it stays on the streamed path")
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

    # ---- size ----------------------------------------------------------------------------------------------------------

    @property
    def bytes(self) -> int:
        return store_bytes(self.n, *self._spec)

    def fits(self, budget_bytes: int) -> bool:
        return self.bytes <= int(budget_bytes)

    def channels(self, mod: str) -> int:
        """channels the modality's encoder sees (after the elevation pre-processing)"""
        return ops.ELEV_CHANNELS[self.elevation[mod]] or self._spec[0][mod][0][0]

    def img_sizes(self) -> Dict[str, int]:
        return {m: int(t.shape[-1]) for m, t in self.inputs.items()}

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
