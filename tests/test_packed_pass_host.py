"""CPU checks of what the table-driven passes over the packed state share on the host: _lib.BlockTable (the device table of a
launch whose workgroups bisect ``starts``; csrc/packed_pass.h) and packed_train._order_by_name (resume by tensor name)."""
import ctypes
import os

import numpy as np
import pytest
import torch

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 5]


@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _item_bytes(table):
    isz = ctypes.sizeof(table.host._type_)
    raw = table.items.numpy().tobytes()
    assert len(raw) == isz * table.n
    return [raw[i * isz:(i + 1) * isz] for i in range(table.n)]


def test_block_table_prefix_sums_and_subset(lib):
    from diffusion_pruning_amd import _lib
    items = (_lib.AdamWItem * len(SIZES))()
    for i, n in enumerate(SIZES):                    # (descriptors that differ in every field; nothing dereferences them here)
        it = items[i]
        it.p, it.g, it.m, it.v, it.shadow, it.n = 0x1000 * (i + 1), 0x2000 * (i + 1), 0x3000 * (i + 1), 0x4000 * (i + 1), 8 * i, n
    blocks = [lib.aptp_adamw_blocks(n) for n in SIZES]
    assert blocks == [1, 1, 1, 1, 1, 1, 2, 3] == [lib.aptp_group_adamw_blocks(n) for n in SIZES]
    t = _lib.BlockTable(items, blocks, torch.device("cpu"))
    assert t.starts.dtype == torch.int32 and t.items.dtype == torch.uint8
    assert t.starts.tolist() == [0] + np.cumsum(blocks).tolist()
    assert t.n == len(SIZES) and t.total == t.starts[-1].item() == sum(blocks)
    assert t.host is items and bytes(items) == b"".join(_item_bytes(t))
    assert t.args() == (t.items.data_ptr(), t.starts.data_ptr(), t.n, t.total)
    whole = _item_bytes(t)
    s = t.subset([3, 0])
    assert _item_bytes(s) == [whole[3], whole[0]] and bytes(s.host) == whole[3] + whole[0]
    assert s.starts.tolist() == [0, blocks[3], blocks[3] + blocks[0]] and s.n == 2 and s.total == s.starts[-1].item()
    s = t.subset([7, 6, 2])
    assert _item_bytes(s) == [whole[7], whole[6], whole[2]] and s.starts.tolist() == [0, 3, 5, 6] and s.total == 6
    assert t.starts.tolist() == [0] + np.cumsum(blocks).tolist() and _item_bytes(t) == whole      # (the parent table is untouched)
    with pytest.raises(AssertionError):
        _lib.BlockTable(items, blocks[:-1], torch.device("cpu"))


def _order_before(names, own, who):
    """the match-by-name stanza as PackedAdamW.load_state_dict and PackedEMA.load_state_dict each had it"""
    pos = {n: i for i, n in enumerate(names)}
    missing = [n for n in own if n not in pos]
    if not (not missing and len(pos) == len(names) == len(own)):        # (raised by hand: pytest rewrites an assert's message here)
        raise AssertionError(f"{who}: the saved state belongs to another expert / tensor list (missing {missing[:3]}, "
                             f"{len(names)} saved vs {len(own)} here)")
    return [pos[n] for n in own]


def _outcome(fn, *args):
    try:
        return ("order", fn(*args))
    except AssertionError as e:
        return ("refused", str(e))


@pytest.mark.parametrize("who", ["PackedAdamW", "PackedEMA"])
def test_order_by_name(who):
    from diffusion_pruning_amd.packed_train import _order_by_name
    own = ["a::packed", "a::packed_bias", "b::gamma", "b::beta", "c::packed"]
    cases = {
        "same": list(own),
        "permuted": [own[i] for i in (3, 0, 4, 2, 1)],
        "missing": own[:2] + own[3:],
        "replaced": own[:2] + ["x::gamma"] + own[3:],
        "duplicated": own[:4] + [own[0]],
        "duplicated and complete": own + [own[1]],
        "extra": own + ["d::packed"],
        "empty": [],
    }
    for label, saved in cases.items():
        got, want = _outcome(_order_by_name, saved, own, who), _outcome(_order_before, saved, own, who)
        assert got == want, label
    assert _order_by_name(cases["permuted"], own, who) == [1, 4, 3, 0, 2]
    for label in ("missing", "replaced", "duplicated", "duplicated and complete", "extra", "empty"):
        kind, text = _outcome(_order_by_name, cases[label], own, who)
        assert kind == "refused" and text.startswith(who + ": the saved state belongs to another expert"), label
    assert "missing ['b::gamma']" in _outcome(_order_by_name, cases["missing"], own, who)[1]
