"""``readsets`` -- the plan every command visits a source's read sets by -- driven with stand-ins: a source of each kind (decoded in
shares, whole on a device, by the host's threads, the Python reader's) and a ``native.Context`` that records what is asked of it.
What is asserted is the sequence of calls, per thread.  No GPU, no native library."""
import threading
import types

import numpy as np
import pytest

from spliser_amd import coverage as cov, native, readsets


class Log(object):
    """Events in the order they happen, each with the thread it happened on."""

    def __init__(self):
        self.events, self.lock = [], threading.Lock()

    def __call__(self, *event):
        with self.lock:
            self.events.append((threading.current_thread(),) + event)      # (the object: an ident may be used again)

    def by_thread(self):
        out = {}
        for e in self.events:
            out.setdefault(e[0], []).append(e[1:])
        return list(out.values())

    def flat(self):
        return [e[1:] for e in self.events]


class FakeSoA(object):
    def __init__(self, log, n):
        self.log, self.n = log, n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.log("soa freed")


class FakeReads(object):
    def __init__(self, log):
        self.log, self.n = log, 0

    def add_bam(self, source, chrom):
        self.log("add_bam", chrom)
        self.n += source.held[chrom]
        return source.held[chrom]

    def add_bam_share(self, source, k, chrom):
        self.log("add_bam_share", k, chrom)
        self.n += source.share_held[k].get(chrom, 0)
        return source.share_held[k].get(chrom, 0)

    def add_soa(self, soa, seg):
        assert isinstance(soa, FakeSoA)
        self.log("add_soa", seg)
        self.n += soa.n[seg]

    def finish(self):
        self.log("finish")
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.log("set freed")


@pytest.fixture
def world(monkeypatch):
    """-> the log; ``native.Context`` records into it, and so does every thread ``readsets`` starts."""
    log = Log()

    class FakeContext(object):
        def __init__(self, device):
            self.device = device
            log("context", device)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            log("context closed", self.device)

        def begin_reads(self):
            log("begin_reads")
            return FakeReads(log)

        def upload_soa(self, segments, max_ends=None, with_strand=False, with_keys=False):
            (arrays,) = segments
            log("upload_soa", arrays.n, list(max_ends), with_strand, with_keys, arrays.xs is not None, arrays.name_key is not None)
            return FakeSoA(log, [arrays.n])

    class CountingThread(threading.Thread):
        started = []

        def start(self):
            CountingThread.started.append(self)
            threading.Thread.start(self)

    monkeypatch.setattr(native, "Context", FakeContext)
    monkeypatch.setattr(readsets, "threading", types.SimpleNamespace(Thread=CountingThread, Lock=threading.Lock))
    log.threads = CountingThread.started
    return log


class FakeBam(native.BamFile):
    """A BAM source without a file: ``on_device`` is what ``join_decoders`` says."""

    def __init__(self, on_device, held=None, shares=None, share_held=None, sets=None, log=None):
        self.on, self.held, self.share_held, self.sets, self.log = on_device, held or {}, share_held, sets or {}, log
        if shares is not None:
            self.shares = shares
        self.ref_names, self.ref_lengths = ["c1", "c2", "c3", "c4"], [1000] * 4

    def join_decoders(self):
        return self.on

    def share_ref(self, k, chrom):
        return self.share_held[k].get(chrom, 0), 0

    def reads(self, chrom):
        self.log("reads", chrom)
        return self.sets.get(chrom)

    def close(self):
        pass


class FakeSam(object):
    """The Python reader's source: read sets by name, and nothing else."""

    def __init__(self, sets, log):
        self.sets, self.log, self.ref_names = sets, log, list(sets)

    def reads(self, chrom):
        self.log("reads", chrom)
        return self.sets.get(chrom)


class Set(object):
    def __init__(self, n, keys=True, xs=True, max_end=None):
        self.n = n
        self.pos, self.flag = np.arange(n, dtype=np.int32) + 1, np.zeros(n, np.uint16)
        self.cig_off, self.cigar = np.arange(n + 1, dtype=np.uint32), np.full(n, 50 << 4, np.uint32)
        self.name_key = np.arange(n, dtype=np.uint64) + 7 if keys else None
        self.xs = np.full(n, 43, np.uint8) if xs else None
        if max_end is not None:
            self.max_end = max_end


def _visits(log):
    def visit(dr, chrom):
        log("visit", chrom, dr.n)
    return visit


# ---- a decode in shares -----------------------------------------------------------------------------------------------------
def _in_shares(c3_in_share_1=0):
    """Two shares over c1..c3: c1 lies in share 0, c2 is cut across both, share 1 lists c3 and holds ``c3_in_share_1`` reads of it."""
    return FakeBam(True, shares=[(5, ["c1", "c2"]), (7, ["c2", "c3"])], share_held=[{"c1": 10, "c2": 4}, {"c2": 6, "c3": c3_in_share_1}])


def test_shares_a_thread_and_a_context_per_share_each_visits_what_it_holds(world):
    readsets.over_fused_sets(_in_shares(), (5, 7), ["c1", "c2", "c3"], _visits(world))
    assert len(world.threads) == 2
    per_thread = sorted(world.by_thread())
    assert {e[0] for e in world.events} == set(world.threads)
    assert len(per_thread) == 2 and threading.current_thread() not in {e[0] for e in world.events}
    assert per_thread == [
        [("context", 5), ("begin_reads",), ("add_bam_share", 0, "c1"), ("finish",), ("visit", "c1", 10), ("set freed",),
         ("begin_reads",), ("add_bam_share", 0, "c2"), ("finish",), ("visit", "c2", 4), ("set freed",), ("context closed", 5)],
        [("context", 7), ("begin_reads",), ("add_bam_share", 1, "c2"), ("finish",), ("visit", "c2", 6), ("set freed",), ("context closed", 7)]]
    assert "c3" not in [e[-1] for e in world.flat() if e[0] == "add_bam_share"]      # (nobody holds it: not added, not visited)


def test_plans_of_the_three_kinds(world):
    plans = readsets.plans_of(_in_shares(), (5, 7), ["c3", "c2", "c1"])
    assert [(d, [c for c, _ in entries]) for d, entries in plans] == [(5, ["c2", "c1"]), (7, ["c2"])]       # (the order of ``chroms``)
    assert all(add is not None for _, entries in plans for _, add in entries)
    whole = readsets.plans_of(FakeBam(True, held={"c1": 1}), (3, 4), ["c1", "c2"])
    assert [(d, [c for c, _ in entries]) for d, entries in whole] == [(3, ["c1", "c2"])] and all(add is not None for _, add in whole[0][1])
    for source in (FakeBam(False), FakeSam({}, world)):
        assert readsets.plans_of(source, (3, 4), ["c1", "c2"]) == [(3, [("c1", None), ("c2", None)])]
    assert world.events == []


# ---- whole on a device ------------------------------------------------------------------------------------------------------
def test_whole_on_the_first_device_a_chromosome_without_reads_is_neither_finished_nor_visited(world):
    source = FakeBam(True, held={"c1": 5, "c2": 0, "c3": 2})
    readsets.over_fused_sets(source, (3, 4), ["c1", "c2", "c3"], _visits(world))
    assert len(world.threads) == 1
    assert world.flat() == [
        ("context", 3), ("begin_reads",), ("add_bam", "c1"), ("finish",), ("visit", "c1", 5), ("set freed",),
        ("begin_reads",), ("add_bam", "c2"), ("set freed",),
        ("begin_reads",), ("add_bam", "c3"), ("finish",), ("visit", "c3", 2), ("set freed",), ("context closed", 3)]


# ---- reads on the host: a file the host's threads decoded, the Python reader's ------------------------------------------------
def _on_host(kind, sets, log):
    return FakeBam(False, sets=sets, log=log) if kind == "bam" else FakeSam(sets, log)


@pytest.mark.parametrize("kind", ["bam", "sam"])
@pytest.mark.parametrize("with_keys,with_strand", [(False, False), (True, False), (False, True)])
def test_host_reads_go_up_as_arrays_with_what_was_asked_for(world, kind, with_keys, with_strand):
    sets = {"c1": Set(3, max_end=160), "c3": Set(0), "c4": Set(2)}           # (c2: no such reference; c3: no read; c4: no max_end)
    readsets.over_fused_sets(_on_host(kind, sets, world), (2,), ["c1", "c2", "c3", "c4"], _visits(world), with_keys=with_keys, with_strand=with_strand)

    def went_up(n, max_end):
        return [("upload_soa", n, [max_end], with_strand, with_keys, with_strand, with_keys), ("begin_reads",), ("add_soa", 0), ("finish",)]
    assert world.flat() == ([("context", 2), ("reads", "c1")] + went_up(3, 160) + [("visit", "c1", 3), ("set freed",), ("soa freed",), ("reads", "c2"), ("reads", "c3"), ("reads", "c4")]
                            + went_up(2, None) + [("visit", "c4", 2), ("set freed",), ("soa freed",), ("context closed", 2)])


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_host_reads_without_what_was_asked_for_are_refused(world, kind):
    sets = {"c1": Set(3, keys=False, xs=False)}
    with pytest.raises(native.SpliserNativeError, match="the reads of c1 were decoded without name keys") as err:
        readsets.over_fused_sets(_on_host(kind, sets, world), (0,), ["c1"], _visits(world), with_keys=True)
    assert err.value.code == -1
    with pytest.raises(native.SpliserNativeError, match="c1: reads without strand bytes") as err:
        readsets.over_fused_sets(_on_host(kind, sets, world), (0,), ["c1"], _visits(world), with_strand=True)
    assert err.value.code == -1
    assert not [e for e in world.flat() if e[0] in ("upload_soa", "visit")]
    readsets.over_fused_sets(_on_host(kind, sets, world), (0,), ["c1"], _visits(world))         # (neither asked for: neither missed)
    assert [e for e in world.flat() if e[0] == "visit"] == [("visit", "c1", 3)]


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_the_first_error_is_raised_when_every_thread_has_ended(world):
    first_raised, seen = threading.Event(), {}

    def visit(dr, chrom):
        world("visit", chrom, dr.n)
        if dr.n == 10:                                    # share 0, c1: the first error; its thread goes no further
            seen["a"] = threading.current_thread()
            first_raised.set()
            raise KeyError("first")
        seen["b"] = threading.current_thread()            # share 1: waits until share 0's thread has ended, visits all it holds, then fails too
        assert first_raised.wait(5)
        seen["a"].join(5)
        assert not seen["a"].is_alive()
        if chrom == "c3":
            raise ValueError("second")

    with pytest.raises(KeyError, match="first"):
        readsets.over_fused_sets(_in_shares(c3_in_share_1=3), (5, 7), ["c1", "c2", "c3"], visit)
    assert len(world.threads) == 2 and not any(t.is_alive() for t in world.threads)
    assert seen["a"] is not seen["b"] and {seen["a"], seen["b"]} == set(world.threads)
    visits = [e for e in world.flat() if e[0] == "visit"]
    assert sorted(visits) == [("visit", "c1", 10), ("visit", "c2", 6), ("visit", "c3", 3)]            # (share 0's c2 was behind its error)
    assert world.flat().count(("set freed",)) == 3 and sorted(e for e in world.flat() if e[0] == "context closed") == [("context closed", 5), ("context closed", 7)]


def test_the_fragment_refusals_come_from_one_place():
    class NoKeys(object):
        mate_keys = False

    class InShares(object):
        mate_keys, shares = True, [(0, []), (1, [])]
    with pytest.raises(native.SpliserNativeError, match="needs a source decoded with name keys"):
        readsets.check_fragment_source(NoKeys())
    with pytest.raises(native.SpliserNativeError, match="decoded on one device: mates can lie either side of a share's cut"):
        readsets.check_fragment_source(InShares())


# ---- nothing to visit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["shares", "whole", "host", "sam"])
def test_no_chromosome_no_thread_no_context(world, source):
    source = {"shares": _in_shares(), "whole": FakeBam(True), "host": FakeBam(False, log=world), "sam": FakeSam({}, world)}[source]
    readsets.over_fused_sets(source, (0, 1), [], _visits(world))
    assert world.events == [] and world.threads == []


# ---- coverage's form: a generator on the calling thread ---------------------------------------------------------------------
def test_coverage_sets_of_source_yields_in_order_and_holds_a_set_open_until_the_next_is_asked_for(world):
    source = FakeBam(True, held={"c1": 5, "c2": 0, "c3": 2})
    source.ref_lengths = [1000, 2000, 3000, 4000]
    sets = cov.sets_of_source(source, 6, ["c3", "c2", "c1"])
    assert world.events == []                                        # (a generator: nothing before the first set is asked for)
    chrom, length, dr = next(sets)
    assert (chrom, length, dr.n) == ("c3", 3000, 2)
    assert world.flat() == [("context", 6), ("begin_reads",), ("add_bam", "c3"), ("finish",)]          # (open: the consumer holds it)
    chrom, length, dr = next(sets)
    assert (chrom, length, dr.n) == ("c1", 1000, 5)
    assert world.flat()[4:] == [("set freed",), ("begin_reads",), ("add_bam", "c2"), ("set freed",), ("begin_reads",), ("add_bam", "c1"), ("finish",)]
    assert list(sets) == []
    assert world.flat()[-2:] == [("set freed",), ("context closed", 6)]
    assert world.threads == [] and {e[0] for e in world.events} == {threading.current_thread()}


def test_coverage_sets_of_source_host_reads_their_length_and_their_keys(world):
    sets = {"c1": Set(3, max_end=160), "c2": Set(2, max_end=0), "c3": Set(1, keys=False, max_end=9)}
    source = FakeSam(sets, world)
    source.mate_keys = True
    got = [(chrom, length) for chrom, length, _ in cov.sets_of_source(source, 0, ["c1", "c2"], with_keys=True)]
    assert got == [("c1", 160)]                                      # (no header length: the reads' max_end; c2: no read covers a base)
    assert [e for e in world.flat() if e[0] == "upload_soa"] == [("upload_soa", 3, [160], False, True, False, True), ("upload_soa", 2, [0], False, True, False, True)]
    with pytest.raises(native.SpliserNativeError, match="name keys"):
        list(cov.sets_of_source(source, 0, ["c3"], with_keys=True))
    source.mate_keys = False
    with pytest.raises(native.SpliserNativeError, match="name keys"):
        list(cov.sets_of_source(source, 0, [], with_keys=True))


def test_coverage_sets_of_source_refuses_a_file_in_shares_in_words(world):
    with pytest.raises(native.SpliserNativeError, match="decoded in 2 shares"):
        list(cov.sets_of_source(_in_shares(), 0, ["c1"]))
    assert world.events == []
