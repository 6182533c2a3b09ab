"""Host-side logic of the stream lanes of pipeline.ExpertDispatchLoop: which lane a group runs on (plan_lanes), how a plan is cut
into waves that fit the graph LRU (plan_waves), the order in which the host issues a wave's items (round_robin), and what the
constructor and the call refuse.  No GPU."""
import random

import pytest
import torch

from diffusion_pruning_amd import pipeline as P

BUCKETS = (1, 2, 4, 8)


def key_of(group):
    return (group[0], group[2])                       # (expert, bucket): what of a captured step's key differs inside one call


def cost(bucket):
    return 4 + bucket


def random_plan(rng):
    """8-40 groups in plan order: experts ascending, some experts cut into several chunks of the largest bucket (equal keys)
    followed by a smaller rest"""
    n = rng.randint(8, 40)
    groups, e, row = [], 0, 0
    while len(groups) < n:
        chunks = rng.choice((1, 1, 1, 2, 3))
        for c in range(chunks):
            if len(groups) == n:
                break
            bucket = BUCKETS[-1] if c < chunks - 1 else rng.choice(BUCKETS)
            groups.append((e, list(range(row, row + bucket)), bucket))
            row += bucket
        e += 1
    return groups


def lane_costs(groups, lanes, n_lanes):
    load = [0] * n_lanes
    for g, lane in zip(groups, lanes):
        load[lane] += cost(g[2])
    return load


def test_plan_lanes_properties_on_random_plans():
    rng = random.Random(0)
    repeated = 0
    for trial in range(200):
        groups = random_plan(rng)
        assert 8 <= len(groups) <= 40
        keys = [key_of(g) for g in groups]
        repeated += len(set(keys)) < len(keys)
        for n_lanes in (1, 2, 3, 4):
            lanes = P.plan_lanes(groups, n_lanes, key_of)
            assert len(lanes) == len(groups) and all(isinstance(v, int) and 0 <= v < n_lanes for v in lanes)
            by_key = {}
            for k, lane in zip(keys, lanes):
                assert by_key.setdefault(k, lane) == lane                 # equal keys, equal lanes
            assert lanes == P.plan_lanes(list(groups), n_lanes, key_of)   # deterministic
            assert lanes == P.plan_lanes(groups, n_lanes, key_of, pinned={}, cost=cost)      # the default cost is 4 + bucket
            if n_lanes == 1:
                assert lanes == [0] * len(groups)
            # Greedy list scheduling: the lane that ends up fullest held at most the average load when it took its last job,
            # so it ends at most one job above the average.  A job is a key: its groups travel together.
            jobs = {}
            for g, k in zip(groups, keys):
                jobs[k] = jobs.get(k, 0) + cost(g[2])
            load = lane_costs(groups, lanes, n_lanes)
            assert sum(load) == sum(jobs.values())
            assert max(load) <= sum(jobs.values()) / n_lanes + max(jobs.values())
    assert repeated > 50                                                  # plans with repeated keys were among them


def test_plan_lanes_keeps_pins():
    rng = random.Random(1)
    for trial in range(100):
        groups = random_plan(rng)
        keys = sorted(set(key_of(g) for g in groups))
        for n_lanes in (1, 2, 3, 4):
            pinned = {k: rng.randrange(n_lanes) for k in rng.sample(keys, rng.randint(1, len(keys)))}
            pinned[("not in the plan", 1)] = 0
            lanes = P.plan_lanes(groups, n_lanes, key_of, pinned)
            assert lanes == P.plan_lanes(groups, n_lanes, key_of, dict(pinned))
            by_key = {}
            for g, lane in zip(groups, lanes):
                assert 0 <= lane < n_lanes
                assert by_key.setdefault(key_of(g), lane) == lane
                if key_of(g) in pinned:
                    assert lane == pinned[key_of(g)]


def test_plan_lanes_order_of_placement():
    g = [(0, [0], 1), (1, [1, 2], 2), (2, list(range(3, 11)), 8), (3, [11], 1), (4, [12, 13, 14, 15], 4)]
    # costs 5, 6, 12, 5, 8: longest first -> 12 to lane 0, 8 to lane 1, 6 to lane 1 (14), the first 5 to lane 0 (17), the second
    # 5 to lane 1 (19)
    assert P.plan_lanes(g, 2, key_of) == [0, 1, 0, 1, 1]
    # equal costs: plan order, lowest lane first
    assert P.plan_lanes([(e, [e], 1) for e in range(8)], 4, key_of) == [0, 1, 2, 3, 0, 1, 2, 3]
    # a pin counts as load before anything else is placed
    assert P.plan_lanes([(e, [e], 1) for e in range(4)], 2, key_of, pinned={(3, 1): 0}) == [1, 0, 1, 0]
    # another cost model moves groups, and only that
    assert P.plan_lanes(g, 2, key_of, cost=lambda b: 1) == [0, 1, 0, 1, 0]
    assert P.plan_lanes([], 3, key_of) == []
    with pytest.raises(ValueError):
        P.plan_lanes(g, 0, key_of)
    with pytest.raises(ValueError):
        P.plan_lanes(g, 2, key_of, pinned={(0, 1): 2})


def test_plan_waves_hold_at_most_max_keys_consecutive():
    rng = random.Random(2)
    for trial in range(100):
        keys = [key_of(g) for g in random_plan(rng)]
        for max_keys in (1, 2, 3, 16, 64):
            waves = P.plan_waves(keys, max_keys)
            assert [i for w in waves for i in w] == list(range(len(keys)))       # consecutive, every group once
            assert all(w and len({keys[i] for i in w}) <= max_keys for w in waves)
            for a, b in zip(waves, waves[1:]):                                    # greedy: the next group did not fit
                assert len({keys[i] for i in a} | {keys[b[0]]}) > max_keys
    assert P.plan_waves([], 4) == []
    assert P.plan_waves(["a", "a", "b", "c", "c", "a"], 2) == [[0, 1, 2], [3, 4, 5]]
    with pytest.raises(ValueError):
        P.plan_waves(["a"], 0)


def test_round_robin_keeps_lane_order_and_takes_turns():
    rng = random.Random(3)
    for trial in range(100):
        n_lanes = rng.randint(1, 4)
        groups = random_plan(rng)
        lanes = P.plan_lanes(groups, n_lanes, key_of)
        queues = [[] for _ in range(n_lanes)]
        for gi, lane in enumerate(lanes):
            queues[lane].append([(gi, step) for step in range(rng.randint(1, 7))])
        issued = list(P.round_robin(queues))
        assert sorted(item for _, item in issued) == sorted(it for q in queues for grp in q for it in grp)   # everything, once
        for lane in range(n_lanes):
            mine = [item for ln, item in issued if ln == lane]
            assert all(lanes[gi] == lane for gi, _ in mine)
            assert mine == [it for grp in queues[lane] for it in grp]     # a group's items in order, groups in plan order
        # one item per lane in turn: after r rounds every lane has issued min(r, what it has)
        left = [sum(len(grp) for grp in q) for q in queues]
        pos = 0
        while any(left):
            turn = [lane for lane in range(n_lanes) if left[lane]]
            assert [ln for ln, _ in issued[pos:pos + len(turn)]] == turn
            pos += len(turn)
            left = [max(0, v - 1) for v in left]
        assert pos == len(issued)
    assert list(P.round_robin([])) == [] and list(P.round_robin([[], [[]]])) == []
    assert list(P.round_robin([[["a0", "a1"], ["b0"]], [["c0"]]])) == [(0, "a0"), (1, "c0"), (0, "a1"), (0, "b0")]


def test_constructor_and_call_refusals():
    for bad in (0, 5, -1, 2.0, "2", None):
        with pytest.raises(ValueError, match="lanes"):
            P.ExpertDispatchLoop(None, lanes=bad)
    for ok in (1, 2, 3, 4):
        loop = P.ExpertDispatchLoop(None, lanes=ok)
        assert loop.lanes == ok and loop.lane_streams == [] and loop.stream_probe is None
    assert P.ExpertDispatchLoop(None).lanes == 1 and P.MAX_LANES == 4
    # eager concurrency is refused before anything is looked at, let alone launched: this loop has no model and no router
    with pytest.raises(ValueError, match="lanes=2 needs use_graph=True"):
        P.ExpertDispatchLoop(None, lanes=2)(torch.zeros(1, 77, 8), torch.zeros(1, 4, 2, 2), use_graph=False)
    assert P.DispatchOutput(latents=None, arch_indices=None, arch_vectors_quantized=None).lanes is None
