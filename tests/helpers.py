"""Helpers shared by the VAE and text-encoder tests (a plain module, imported explicitly)."""
import json
import struct

import torch


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def write_safetensors(path, tensors):
    """a safetensors file of the given tensors: int64 stays I64, everything else is written as F32"""
    header, blobs, off = {}, [], 0
    for name, t in tensors.items():
        t = t.detach().cpu().contiguous()
        a = (t if t.dtype == torch.int64 else t.float()).numpy()
        b = a.tobytes()
        header[name] = {"dtype": "I64" if t.dtype == torch.int64 else "F32", "shape": list(a.shape),
                        "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    hb = json.dumps(header).encode()
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(hb)) + hb + b"".join(blobs))
