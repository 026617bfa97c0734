"""The lanes of the counting passes without a GPU (``csrc/spl_lanes.h`` through ``spl_lanes_plan_host``): the native rule against its
restatement, op for op; both under the hazard checker of ``lanecases.py`` on the hand-written sequences and on seeded random ones, in
every configuration of streams; and the property the benchmark's gain rests on -- the second shard's slots and range kernels on the
other lane, behind no range kernel of the step, and its tail on that lane too, behind no other shard's."""
import pytest

import lanecases as L
from spliser_amd import native

CONFIGS = [dict(two=True, tail=True, foreign=False), dict(two=True, tail=True, foreign=True), dict(two=False, tail=True, foreign=False), dict(two=False, tail=False, foreign=False)]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def _native(calls, cfg):
    n_tables = 1 + max([c[1] for c in calls if c[0] in (L.COUNT, L.DOWNLOAD)] + [0])
    n_sets = 1 + max([c[1] for c in calls if c[0] == L.RELAYOUT] + [c[2] for c in calls if c[0] == L.COUNT] + [0])
    return native.lanes_plan_host(calls, n_tables, n_sets, cfg["two"], cfg["tail"], cfg["foreign"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "two=%d tail=%d foreign=%d" % (c["two"], c["tail"], c["foreign"]))
@pytest.mark.parametrize("name", sorted(L.SEQUENCES))
def test_hand_written_sequences(built, name, cfg):
    calls = L.SEQUENCES[name]
    plan = _native(calls, cfg)
    assert plan == L.restated_plan(calls, cfg["two"], cfg["tail"], cfg["foreign"])
    L.check(calls, plan, cfg["tail"])
    if not cfg["two"]:
        assert all(p["lane"] == 0 for p in plan)
    if not cfg["tail"]:
        assert all(not p["ops"] and not p["piped"] for p in plan)


@pytest.mark.parametrize("cfg", CONFIGS[:3], ids=lambda c: "two=%d foreign=%d" % (c["two"], c["foreign"]))
def test_random_sequences(built, cfg):
    lanes_used = set()
    for seed in range(1500):
        calls = L.random_calls(seed)
        plan = _native(calls, cfg)
        assert plan == L.restated_plan(calls, cfg["two"], cfg["tail"], cfg["foreign"]), seed
        L.check(calls, plan)
        lanes_used |= {p["lane"] for p in plan}
    assert lanes_used == ({0, 1} if cfg["two"] else {0})


def test_the_checker_sees_a_missing_wait(built):
    """The checker is no rubber stamp: the bench step's plan with one wait taken out fails it, whichever wait it is."""
    calls = L.bench_steps(3, 4, barriers=False)
    plan = _native(calls, CONFIGS[0])
    waits = [(i, k) for i, p in enumerate(plan) for k, op in enumerate(p["ops"]) if op[0] == L.WAIT]
    assert len(waits) >= 6
    for i, k in waits:
        broken = [dict(p, ops=list(p["ops"])) for p in plan]
        del broken[i]["ops"][k]
        with pytest.raises(AssertionError):
            L.check(calls, broken)


@pytest.mark.parametrize("foreign", [False, True])
def test_the_second_shard_runs_beside_the_first(built, foreign):
    calls = L.bench_steps(2, 5)
    plan = _native(calls, dict(two=True, tail=True, foreign=foreign))
    g, nodes = L.check(calls, plan)
    for step in range(5):
        r1, c1, r2, c2, bar = plan[5 * step:5 * step + 5]
        n1, n2 = nodes[5 * step + 1], nodes[5 * step + 3]
        assert (r1["lane"], c1["lane"], r2["lane"], c2["lane"]) == (0, 0, 1, 1) and c1["piped"] and c2["piped"]
        assert not g.before(n1["range"], nodes[5 * step + 2]["slots"]) and not g.before(n1["range"], n2["range"])
        assert not c1["ops"] and not c2["ops"]                       # no wait packet in front of a range kernel
        if step and not foreign:
            assert not r1["ops"] and r2["ops"] == [(L.WAIT, L.SIDE, L.EV_TAIL, step - 1)]       # the barrier, through the last tail: no marker
            assert bar["ops"] == [(L.WAIT, L.MAIN, L.EV_TAIL, step), (L.WAIT, L.MAIN, L.EV_STAIL, step)]
        # the second shard's tail stays on its lane: it does not stand behind the first shard's range kernel or tail
        assert c2["tail_stream"] == L.SIDE and c1["tail_stream"] == L.TAIL
        assert not g.before(n1["range"], n2["tail"]) and not g.before(n1["tail"], n2["tail"])


def test_a_sets_consecutive_passes_take_turns_with_three_shards(built):
    calls = L.bench_steps(3, 4, barriers=False)
    plan = _native(calls, CONFIGS[0])
    lanes = [[plan[6 * step + 2 * k + 1]["lane"] for step in range(4)] for k in range(3)]
    assert lanes == [[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1]]
    one = _native(L.bench_steps(1, 4, barriers=False), CONFIGS[0])
    assert {p["lane"] for p in one} == {0}                           # a set alone keeps its lane


def test_bad_arguments_are_refused(built):
    with pytest.raises(native.SpliserNativeError):
        native.lanes_plan_host([(9, 0, 0, 0)], 1, 1)
    with pytest.raises(native.SpliserNativeError):
        native.lanes_plan_host([(L.COUNT, 3, 0, 1)], 2, 1)
    with pytest.raises(native.SpliserNativeError):
        native.lanes_plan_host([(L.RELAYOUT, 0, 1, 0)], 1, 65)
