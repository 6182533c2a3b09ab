"""Checkpoint loading shared by the VAE and the text encoder: a safetensors reader without the ``safetensors`` package,
one strict state-dict loader and the ``from_pretrained`` body around them."""
from __future__ import annotations

import json
import os
import struct
from typing import Callable, Dict, Optional

import numpy as np
import torch

# the format is an 8-byte little-endian header length, a JSON header, then the raw tensor bytes
_ST_DTYPES = {"F32": np.float32, "F16": np.float16, "F64": np.float64}


def read_safetensors(path: str, skip=None) -> Dict[str, torch.Tensor]:
    """every tensor of a safetensors file as fp32; names for which skip(name) is true are not read"""
    with open(path, "rb") as f:
        raw = f.read()
    (n,) = struct.unpack("<Q", raw[:8])
    header = json.loads(raw[8:8 + n].decode("utf-8"))
    base = 8 + n
    out = {}
    for name, info in header.items():
        if name == "__metadata__" or (skip is not None and skip(name)):
            continue
        b0, b1 = info["data_offsets"]
        dt = info["dtype"]
        if dt == "BF16":
            a = np.frombuffer(raw, dtype=np.uint16, count=(b1 - b0) // 2, offset=base + b0).astype(np.uint32) << 16
            t = torch.from_numpy(a.view(np.float32).copy())
        elif dt in _ST_DTYPES:
            npd = _ST_DTYPES[dt]
            t = torch.from_numpy(np.frombuffer(raw, dtype=npd, count=(b1 - b0) // np.dtype(npd).itemsize, offset=base + b0).copy())
        else:
            raise ValueError(f"{path}: tensor {name} has unsupported dtype {dt}")
        out[name] = t.reshape(info["shape"]).float()
    return out


def load_strict(module, sd: Dict[str, torch.Tensor], rename: Callable[[str], str] = lambda n: n,
                ignore: Callable[[str], bool] = lambda n: False, fixup: Optional[Callable] = None):
    """Load ``sd`` into ``module`` so that every key of the module is present with its shape and no other key is.  A key
    whose name after ``rename`` satisfies ``ignore`` is dropped; ``fixup(name, tensor)`` may reshape a tensor
    before the shape check.  Ends with ``module.invalidate()`` and returns the module."""
    who = type(module).__name__
    own = module.state_dict()
    got = {}
    for name, t in sd.items():
        name = rename(name)
        if ignore(name):
            continue
        if name not in own:
            raise KeyError(f"{who}: unexpected key {name}")
        if fixup is not None:
            t = fixup(name, t)
        if tuple(t.shape) != tuple(own[name].shape):
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {tuple(own[name].shape)}")
        got[name] = t
    missing = sorted(set(own) - set(got))
    if missing:
        raise KeyError(f"{who}: missing keys {missing[:8]}{' ...' if len(missing) > 8 else ''}")
    module.load_state_dict(got)
    module.invalidate()
    return module


def read_pretrained(config_cls, root: str, subfolder: Optional[str], weights: str, skip=None):
    """(config, state dict) of a diffusers / transformers model folder: ``config.json`` and the safetensors file ``weights``"""
    d = os.path.join(root, subfolder) if subfolder else root
    with open(os.path.join(d, "config.json")) as f:
        cfg = config_cls.from_dict(json.load(f))
    return cfg, read_safetensors(os.path.join(d, weights), skip=skip)
