"""Host tests of diffusion_pruning_amd/scratch.py (no GPU): the key, the growing counter pool, the workspace and the
unit-statistics arena, on CPU tensors with the module's reads of torch.cuda replaced by a fake stream handle and capture flag."""
import threading
import types

import pytest
import torch

from diffusion_pruning_amd import scratch

CPU = torch.device("cpu")
GPU = torch.device("cuda", 0)          # only named: the fake allocator below hands out CPU tensors for it


@pytest.fixture()
def fake(monkeypatch):
    """empty caches and a fake current stream / capture flag; counts allocations and stream waits"""
    st = types.SimpleNamespace(stream=100, capturing=False, allocs=0, syncs=0)

    def alloc(n, dtype, device, zero):
        st.allocs += 1
        return (torch.zeros if zero else torch.empty)(n, dtype=dtype)

    def sync():
        st.syncs += 1

    monkeypatch.setattr(scratch, "_stream_handle", lambda: st.stream)
    monkeypatch.setattr(scratch, "_capturing", lambda: st.capturing)
    monkeypatch.setattr(scratch, "_current_device", lambda: 0)
    monkeypatch.setattr(scratch, "_sync_stream", sync)
    monkeypatch.setattr(scratch, "_alloc", alloc)
    for name in ("_pools", "_ws", "_arenas"):
        monkeypatch.setattr(scratch, name, {})
    monkeypatch.setattr(scratch, "capture_keep", [])
    monkeypatch.setattr(scratch, "USTAT", True)
    monkeypatch.setattr(scratch, "USTAT_NREP", 8)
    monkeypatch.setattr(scratch._tls, "ustat", None, raising=False)
    return st


def _span(t):
    return range(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())


def _disjoint(a, b):
    ra, rb = _span(a), _span(b)
    return ra.stop <= rb.start or rb.stop <= ra.start


def test_key_reads_device_stream_domain_and_capture_flag(fake):
    assert scratch.key(CPU) == (0, 100, None, False)
    assert scratch.key(torch.device("cuda", 3)).device_index == 3
    fake.stream, fake.capturing = 7, True
    with scratch.scratch_domain("teacher"):
        k = scratch.key(CPU)
    assert k == scratch.Key(device_index=0, stream_handle=7, domain="teacher", capturing=True)


def test_counters_map_stream_and_domain_to_slabs(fake):
    a = scratch.counters(CPU)
    assert a.shape == (scratch.N_COUNTERS,) and a.dtype == torch.int32 and int(a.abs().sum()) == 0
    assert scratch.counters(CPU).data_ptr() == a.data_ptr()
    fake.capturing = True                                   # eager and captured launches share the slab
    assert scratch.counters(CPU).data_ptr() == a.data_ptr()
    fake.capturing = False
    fake.stream = 101
    b = scratch.counters(CPU)
    fake.stream = 100
    with scratch.scratch_domain("teacher"):
        c = scratch.counters(CPU)
        seen = {}
        t = threading.Thread(target=lambda: seen.setdefault("ptr", scratch.counters(CPU).data_ptr()))   # the domain is per thread
        t.start()
        t.join()
        assert scratch.counters(CPU).data_ptr() == c.data_ptr()
    assert seen["ptr"] == a.data_ptr()
    assert _disjoint(a, b) and _disjoint(a, c) and _disjoint(b, c)
    assert scratch.counters(CPU).data_ptr() == a.data_ptr()
    assert scratch.counter_keys(CPU) == 3


def test_counter_pool_grows_and_keeps_addresses(fake):
    first = scratch.counters(CPU)
    p0 = first.data_ptr()
    first[5] = 1                                            # growth must neither move nor clear a slab in use
    slabs = [first]
    for i in range(1, 40):
        with scratch.scratch_domain(f"k{i}"):
            s = scratch.counters(CPU)
        assert int(s.abs().sum()) == 0 and s.numel() == scratch.N_COUNTERS
        slabs.append(s)
        assert scratch.counters(CPU).data_ptr() == p0 and int(first[5]) == 1
    assert scratch.counter_keys(CPU) == 40
    spans = sorted((_span(s) for s in slabs), key=lambda r: r.start)
    assert all(x.stop <= y.start for x, y in zip(spans, spans[1:]))
    # a chunk whenever fewer than half a chunk is free: 40 keys of 16-slab chunks take 3, each followed by one wait
    assert fake.allocs == fake.syncs == len(scratch._pools[0]["chunks"]) == 3
    for i in range(1, 40):                                  # and every key still finds its own slab
        with scratch.scratch_domain(f"k{i}"):
            assert scratch.counters(CPU).data_ptr() == slabs[i].data_ptr()


def test_counters_never_allocate_during_capture(fake):
    fake.capturing = True
    assert scratch.counters(CPU) is None                    # no pool yet: the caller falls back
    assert fake.allocs == 0 and fake.syncs == 0 and scratch._pools == {} and scratch.counter_keys(CPU) == 0
    fake.capturing = False
    known = scratch.counters(CPU)
    assert fake.allocs == 1
    fake.capturing = True
    assert scratch.counters(CPU).data_ptr() == known.data_ptr()
    got = []
    for i in range(scratch.N_SLABS - 1):                    # new keys inside ONE capture: the free slabs, then None
        with scratch.scratch_domain(f"c{i}"):
            got.append(scratch.counters(CPU))
    assert all(s is not None for s in got) and len({s.data_ptr() for s in got} | {known.data_ptr()}) == scratch.N_SLABS
    with scratch.scratch_domain("one too many"):
        assert scratch.counters(CPU) is None
    assert scratch.counters(CPU).data_ptr() == known.data_ptr()
    assert fake.allocs == 1 and fake.syncs == 1 and scratch.counter_keys(CPU) == scratch.N_SLABS
    fake.capturing = False                                  # the next eager call tops the pool up
    assert scratch.counters(CPU).data_ptr() == known.data_ptr()
    assert fake.allocs == 2 and fake.syncs == 2
    fake.capturing = True
    with scratch.scratch_domain("one too many"):
        late = scratch.counters(CPU)
    assert late is not None and int(late.abs().sum()) == 0 and fake.allocs == 2


def test_workspace_is_grow_only_and_capture_buffers_are_kept(fake):
    w = scratch.workspace(1000, CPU)
    assert w.dtype == torch.uint8 and w.numel() == 1 << 20                      # the floor
    assert scratch.workspace(1 << 20, CPU).data_ptr() == w.data_ptr() and fake.allocs == 1
    big = scratch.workspace((1 << 20) + 1, CPU)
    assert big.numel() == (1 << 20) + 1 and fake.allocs == 2                    # eager: exactly what was asked for
    assert scratch.workspace(5, CPU).data_ptr() == big.data_ptr()
    assert scratch.capture_keep == []
    with scratch.scratch_domain("teacher"):                                     # another key, another buffer
        assert scratch.workspace(5, CPU).data_ptr() != big.data_ptr()
    fake.capturing = True
    c1 = scratch.workspace(3 << 20, CPU)                                        # the capture flag is part of the key
    assert c1.data_ptr() != big.data_ptr() and [b.data_ptr() for b in scratch.capture_keep] == [c1.data_ptr()]
    assert scratch.workspace(1 << 20, CPU).data_ptr() == c1.data_ptr()
    c2 = scratch.workspace((3 << 20) + 1, CPU)
    assert c2.numel() >= 1.5 * c1.numel()
    assert [b.data_ptr() for b in scratch.capture_keep] == [c1.data_ptr(), c2.data_ptr()]
    assert scratch.workspace(4 << 20, CPU).data_ptr() == c2.data_ptr()


def test_ustat_arena_offsets_high_water_mark_and_zeroing(fake):
    B, unit = 2, 10
    scratch.ustat_begin(GPU, unit)
    u1, un, units1, nrep = scratch.ustat_alloc(B, 320)
    assert (un, units1, nrep) == (10, 32, 8)
    u2, _, units2, _ = scratch.ustat_alloc(B, 645)                              # a ragged last unit counts
    assert units2 == 65
    n1, n2 = nrep * B * units1 * 2, nrep * B * units2 * 2
    assert u1.numel() == n1 and u2.numel() == n2 and u1.dtype == torch.int64
    buf = scratch._tls.ustat["buf"]
    assert u1.data_ptr() == buf.data_ptr() and u2.data_ptr() == buf.data_ptr() + 8 * n1
    assert scratch.ustat_alloc(16, 320)[3] == 2                                 # more samples, fewer replicas: nrep * B <= 4 * USTAT_NREP
    n3 = 2 * 16 * 32 * 2
    assert scratch.ustat_alloc(B, scratch._USTAT_WORDS * unit) is None          # does not fit: nothing handed out
    scratch.ustat_end()
    assert scratch.ustat_alloc(B, 320) is None                                  # closed
    ent = scratch._arenas[scratch.key(GPU)]
    assert ent["used"] == n1 + n2 + n3 and fake.allocs == 1
    buf.fill_(3)
    scratch.ustat_begin(GPU, unit)                                              # reuse: exactly the used prefix is zeroed
    assert scratch._tls.ustat["buf"].data_ptr() == buf.data_ptr() and fake.allocs == 1
    assert int(buf[:ent["used"]].abs().sum()) == 0 and bool((buf[ent["used"]:] == 3).all())
    scratch.ustat_alloc(B, 320)
    scratch.ustat_end()
    assert ent["used"] == n1 + n2 + n3                                          # a high-water mark
    assert scratch.capture_keep == []


def test_ustat_arena_created_under_capture_is_fully_used_and_kept(fake):
    fake.capturing = True
    scratch.ustat_begin(GPU, 10)
    ent = scratch._arenas[scratch.key(GPU)]
    assert ent["used"] == scratch._USTAT_WORDS and int(ent["buf"].abs().sum()) == 0
    assert [b.data_ptr() for b in scratch.capture_keep] == [ent["buf"].data_ptr()]
    scratch.ustat_alloc(2, 320)
    scratch.ustat_end()
    assert ent["used"] == scratch._USTAT_WORDS
    fake.capturing = False
    scratch.ustat_begin(GPU, 10)                                                # the eager arena of the same stream is another one
    assert scratch._tls.ustat["buf"].data_ptr() != ent["buf"].data_ptr() and len(scratch.capture_keep) == 1
    scratch.ustat_end()


@pytest.mark.parametrize("device,unit", [(GPU, 0), (GPU, -1), (CPU, 10)])
def test_ustat_begin_without_unit_or_gpu_opens_no_arena(fake, device, unit):
    scratch.ustat_begin(device, unit)
    assert scratch._tls.ustat is None and scratch.ustat_alloc(2, 320) is None
    scratch.ustat_end()
    assert fake.allocs == 0 and scratch._arenas == {}


def test_ops_names_are_the_scratch_objects():
    from diffusion_pruning_amd import ops
    assert ops.scratch_domain is scratch.scratch_domain and ops._domain is scratch.domain
    assert ops._tile_counters is scratch.counters and ops._N_COUNTERS == scratch.N_COUNTERS == 1 << 16
    assert ops._workspace is scratch.workspace and ops._ws_capture_keep is scratch.capture_keep
    assert (ops.ustat_begin, ops.ustat_end, ops._ustat_alloc) == (scratch.ustat_begin, scratch.ustat_end, scratch.ustat_alloc)
    assert (ops.USTAT, ops.USTAT_NREP) == (scratch.USTAT, scratch.USTAT_NREP)
