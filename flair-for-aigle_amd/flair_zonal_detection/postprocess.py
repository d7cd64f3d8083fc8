"""Logits -> uint8 outputs -- counterpart of the reference's flair_zonal_detection/postprocess.py
(convert :9-30).  'argmax': first maximum over the class axis as uint8 with a leading singleton axis;
'class_prob': round-half-even of softmax * 255.  Both run as one HIP kernel over NHWC logits
(ffa_predict_u8); inside the tile loop the margin crop is fused into the same kernel so only 1 byte
per pixel leaves the GPU (the reference ships 76 B/pixel of f32 logits to the host and loops in numpy).

convert_to_cog (reference :33-52, GDAL's COG driver): the overview pyramid is computed on the GPU
(ffa_overview_pyramid_u8, csrc/overview.hip) and the cloud-optimised file is written by geotiff.write_cog.
"""
from __future__ import annotations

import logging
import os

import numpy as np
import torch

from flairhip import nn as hnn
from flairhip import ops

logger = logging.getLogger(__name__)


def _as_device_nhwc(img):
    """(C,H,W) numpy / torch logits -> [1,H,W,32] f32 NHWC on the GPU (+ class count)."""
    if isinstance(img, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32))
    else:
        t = img.detach().float()
    if t.ndim != 3:
        raise ValueError("Expected logits with shape (C, H, W)")
    if t.shape[0] > hnn.LOGIT_PITCH:
        raise ValueError(f"at most {hnn.LOGIT_PITCH} classes are supported, got {t.shape[0]}")
    return ops.nchw_to_nhwc(t.cuda()[None].contiguous(), torch.float32, hnn.LOGIT_PITCH), t.shape[0]


def convert(img, img_type: str):
    """Same contract as the reference: (C,H,W) logits -> uint8 (1,H,W) for 'argmax', (C,H,W) for 'class_prob';
    any other type raises ValueError.  numpy in -> numpy out, torch in -> torch (device) out."""
    if img_type not in ("class_prob", "argmax"):
        raise ValueError(f"Unknown output type: {img_type}")
    nhwc, k = _as_device_nhwc(img)
    out = ops.predict_u8(nhwc, k, img_type)  # [1,H,W] or [1,K,H,W]
    out = out if img_type == "argmax" else out[0]
    return out.cpu().numpy() if isinstance(img, np.ndarray) else out


COG_RESAMPLING = ("nearest", "mode", "average")
_ONE_UPLOAD_BYTES = 2 << 30  # above this the bands go to the GPU one at a time (they are independent)


def overview_levels_host(base: np.ndarray, blocksize: int = 512, method: str = "nearest", ignore=None) -> list:
    """[base, level 1, ..., level L] as host uint8 arrays [bands, H_l, W_l]: the overviews of ``base`` ([bands, H, W],
    an array or a memmap) from ops.overview_pyramid.  The raster is uploaded whole, or band by band when it is a memmap
    or passes 2 GiB."""
    bands, H, W = base.shape
    L = ops.overview_levels(H, W, blocksize)
    levels = [base] + [np.empty((bands, -(-H // (1 << l)), -(-W // (1 << l))), np.uint8) for l in range(1, L + 1)]
    if L == 0:
        return levels
    whole = not isinstance(base, np.memmap) and base.nbytes < _ONE_UPLOAD_BYTES
    for lo, hi in ([(0, bands)] if whole else [(b, b + 1) for b in range(bands)]):
        dev = torch.from_numpy(np.ascontiguousarray(base[lo:hi])).cuda()
        for l, lv in enumerate(ops.overview_pyramid(dev, block=blocksize, method=method, ignore=ignore), 1):
            levels[l][lo:hi] = lv.cpu().numpy()
    return levels


def convert_to_cog(input_path: str, output_path: str, overview_resampling: str = "nearest", blocksize: int = 512,
                   ignore=None) -> None:
    """The reference's contract: the GeoTIFF ``input_path`` becomes the cloud-optimised GeoTIFF ``output_path`` (LZW,
    ``blocksize`` tiles, overviews down to one block) and is removed; a missing input raises FileNotFoundError.
    ``overview_resampling``: "nearest" (the reference's choice), "mode" (class rasters; ``ignore``: a value that does
    not vote, e.g. the 255 of a zone clip) or "average" (probabilities, confidence).  uint8 rasters only."""
    from flair_zonal_detection.geotiff import GeoTiffError, write_cog
    from flair_zonal_detection.raster import open_raster
    if not os.path.isfile(input_path):
        raise FileNotFoundError(f"Input file not found: {input_path}")
    if os.path.realpath(input_path) == os.path.realpath(output_path):
        # the output is renamed into place and the input removed afterwards: on one path that deletes the only copy
        raise ValueError(f"COG conversion needs an output path other than its input: {input_path}")
    if overview_resampling not in COG_RESAMPLING:
        raise ValueError(f"overview_resampling must be one of {COG_RESAMPLING}, got {overview_resampling!r}")
    scratch = None
    src = open_raster(input_path)
    try:
        dtypes = {str(np.dtype(d)) for d in src.dtypes}
        if dtypes != {"uint8"}:
            raise GeoTiffError(f"{input_path}: COG conversion handles uint8 rasters, this one is {', '.join(sorted(dtypes))}")
        bands, H, W = int(src.count), int(src.height), int(src.width)
        if bands * H * W < _ONE_UPLOAD_BYTES:
            base = src.read()
        else:  # keep a very large raster out of RAM: decode band by band into a scratch file
            scratch = output_path + ".raw"
            base = np.memmap(scratch, dtype=np.uint8, mode="w+", shape=(bands, H, W))
            for b in range(bands):
                base[b] = src.read(b + 1)
        levels = overview_levels_host(base, blocksize, overview_resampling, ignore)
        bounds, res = src.bounds, src.res
        crs = getattr(src, "crs", None)
        write_cog(output_path, levels, bounds.left, bounds.top, tuple(res), crs=str(crs) if crs else None,
                  blocksize=blocksize, compress="lzw", geokeys=getattr(src, "geokeys", ()),
                  geoascii=getattr(src, "geoascii", ""), geodoubles=getattr(src, "geodoubles", ()),
                  nodata=getattr(src, "nodata", None))
        del levels, base
    finally:
        src.close()
        if scratch is not None and os.path.exists(scratch):
            os.remove(scratch)
    os.remove(input_path)
