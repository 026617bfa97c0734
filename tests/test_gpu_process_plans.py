"""``process_sites``' planning (spliser_amd/process.py) held to the oracle on the worlds of plancases.py: several shards on one
context, the second plan after a read reached beyond its slot -- found before anything was handed over, after one shard was, in
the streaming loop, on a context that holds pieces of cut chromosomes, with shards composed differently from the first plan's --,
several shards per context after a decode in shares, shares asked for and the decode ending on the host, a file that is not sorted
by reference over three shards.  Every cell is one ``process`` call of a few thousand reads; test_plancases_host.py checks on the CPU
that the worlds are what the cells take them for.

Every run asserts: the .SpliSER.tsv is the oracle's, byte for byte; which decoder read the file; which plans ran on which context
(the ``[process] device N: first plan`` / ``exact plan`` lines, and ``shard.pack``'s calls per device thread with the shards they
gave); what was handed to the writer, how often, and that a chromosome handed over again carries bit-identical arrays; that no
thread is left behind.

What a second plan hands over again today (pinned here): with the reads on the device, the chromosomes of every shard
counted before the overhang was found -- a shard is counted once the NEXT one is laid out, so those up to two shards before the
understated reference's --; in the streaming loop, every chromosome before the understated one.  The writer takes the second
hand-over for one it has already written and ignores it.  The double hand-over is left as it is: it costs a second pass over a few
shards of a file whose header is wrong, and changes nothing in the file.

Seconds per test on an MI355X (``--durations=0``, one run): one context 0.05-0.11 (the first test of a session 0.36, with the
library's start), three contexts 0.15-0.22, five 0.30-0.32; ``test_process_reads_beyond_the_reference_length`` of
test_gpu_configs.py, one context, 0.15 in the same run.  A cell's time is its contexts': 0.03-0.1 s each to create and as much for
its site tables, one after the other on one GPU, whatever the lengths and however few the reads."""
import re
import threading

import numpy as np
import pytest

import plancases as P
from spliser_amd import native, process as proc, shard

pytestmark = pytest.mark.gpu

FR = dict(isStranded=True, strandedType="fr", isbeta2Cryptic=True)
KEYS = ("beta1", "beta2_simple", "beta2_cryptic", "beta2_weighted", "sse", "beta2s_reads")


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    root = tmp_path_factory.mktemp("plans")
    out = {}
    for name in P.NAMES:
        w = P.world(name)
        prefix = str(root / name)
        P.write_files(w, prefix)
        out[name] = (w, prefix)
    return out


@pytest.fixture(scope="module")
def want(worlds, oracle_lib):
    """The oracle's text of a world, computed once per (world, strandedness)."""
    cache = {}

    def get(name, stranded):
        if (name, stranded) not in cache:
            w, prefix = worlds[name]
            cache[(name, stranded)] = P.oracle_tsv(oracle_lib, prefix + ".bed", w.names, w.sets, stranded, bool(stranded))
        return cache[(name, stranded)]
    return get


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


class Run(object):
    """One ``process`` call and what was seen of it."""


def run(worlds, want, monkeypatch, capfd, tmp_path, name, devices, gpu_decode, stranded=None):
    w, prefix = worlds[name]
    monkeypatch.setenv("SPL_PROCESS_TIMING", "1")
    r = Run()
    r.world, r.handed, r.packs, r.shares, r.held, r.declined = w, [], [], None, None, None
    real_add, real_pack, real_join = proc._TsvWriter.add, shard.pack, native.BamFile.join_decoders
    seen = threading.Lock()

    def add(self, chrom, arr, res):
        with seen:
            r.handed.append((self, chrom, {k: np.array(res[k], copy=True) for k in KEYS}))
        return real_add(self, chrom, arr, res)

    def pack(items, concat_reads=True, extents=None):
        shards = real_pack(items, concat_reads=concat_reads, extents=extents)
        tid = {c: k for k, c in enumerate(w.names)}
        first = all(hi == w.lengths[tid[c]] + P.SLACK for c, (_, hi) in extents.items())
        with seen:
            r.packs.append((threading.current_thread(), "first" if first else "exact", [list(sh.chroms) for sh in shards]))
        return shards

    def join(self):
        ok = real_join(self)
        with seen:
            r.shares = list(getattr(self, "shares", None) or [])
            if not ok:
                r.declined = self.decline_reason()
            if ok and r.held is None and getattr(self, "shares", None):       # (reads, largest end) of every share, per reference
                r.held = [[self.share_ref(k, c) for c in w.names] for k in range(len(self.shares))]
        return ok
    monkeypatch.setattr(proc._TsvWriter, "add", add)
    monkeypatch.setattr(shard, "pack", pack)
    monkeypatch.setattr(native.BamFile, "join_decoders", join)
    proc.wait_deferred_close()
    before = set(threading.enumerate())
    capfd.readouterr()
    out = str(tmp_path / "out")
    r.timings = proc.process(prefix + ".bam", prefix + ".bed", out, log=lambda m: None, devices=devices, gpuDecode=gpu_decode,
                             **(FR if stranded else {}))
    proc.wait_deferred_close()
    monkeypatch.setattr(shard, "pack", real_pack)      # (the checks below plan for themselves: not the call's plans)
    r.threads_left = [t for t in threading.enumerate() if t not in before]
    r.err = capfd.readouterr().err
    r.lines = re.findall(r"\[process\] device (\d+): (first|exact) plan", r.err)
    r.text = open(out + ".SpliSER.tsv").read()
    r.table = P.table_of(prefix + ".bed", stranded)
    # 1. the file is the oracle's (a chromosome written twice, or not at all, is a difference as well)
    assert r.text == want(name, stranded)
    # 5. every thread the call started has ended: a device thread that died in a `finally` would otherwise pass unnoticed
    assert not r.threads_left
    return r


def check(r, decoder, n_contexts, calls=1, exact_contexts=(), handed_twice=(), maybe_twice=()):
    """``exact_contexts``: the chromosome lists of the contexts that plan a second time.  ``handed_twice``: the chromosomes the writer
    is handed a second time (``maybe_twice``: those for which it depends on which thread brings a cut chromosome's last piece)."""
    w = r.world
    # 2. the decoder
    assert r.timings["bam_decode"] == decoder
    # 3. the plans: the lines on stderr ...
    assert [k for _, k in r.lines].count("first") == n_contexts * calls
    assert [k for _, k in r.lines].count("exact") == len(exact_contexts)
    assert all(d == "0" for d, _ in r.lines)
    # ... and, per device thread, what was planned: first plan, then an exact one on exactly the contexts that hold the overhang;
    # the shards are those the host test states for these chromosomes
    by_thread = {}
    for thread, kind, shards in r.packs:      # (the Thread objects, kept: an ident may be used again)
        by_thread.setdefault(thread, []).append((kind, shards))
    assert len(by_thread) == n_contexts * calls and len(r.packs) == len(r.lines)
    replanned = []
    for plans in by_thread.values():
        chroms = [c for sh in plans[0][1] for c in sh]
        first, exact = P.plans(w, r.table, chroms)
        assert plans[0] == ("first", [sh.chroms for sh in first])
        assert len(plans) <= 2
        if len(plans) == 2:
            assert plans[1] == ("exact", [sh.chroms for sh in exact])
            replanned.append(chroms)
    assert sorted(replanned) == sorted(list(c) for c in exact_contexts)
    # 4. the hand-over, of the writer whose file it is (a file not sorted by reference is counted twice, by a second writer)
    writers = []
    for wr, _, _ in r.handed:
        if not any(wr is x for x in writers):
            writers.append(wr)
    assert len(writers) == calls
    times = {}
    for wr, chrom, res in r.handed:
        if wr is writers[-1]:
            times.setdefault(chrom, []).append(res)
    assert sorted(times) == sorted(c for c in r.table.chrom_index if r.table.chrom_arrays(c).n)
    for chrom, got in times.items():
        for other in got[1:]:
            for k in KEYS:
                assert np.array_equal(_bits(got[0][k]), _bits(other[k])), (chrom, k)
        if chrom in maybe_twice:
            assert len(got) in (1, 2), chrom
        else:
            assert len(got) == (2 if chrom in handed_twice else 1), chrom
    if not exact_contexts:
        assert all(len(got) == 1 for got in times.values())


ALL6 = ["c1", "c2", "c3", "c4", "c5", "c6", "empty", "ghost"]


# ---- one context ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gpu_decode", [False, True])
def test_three_shards(worlds, want, monkeypatch, capfd, tmp_path, gpu_decode):
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "three_shards", (0,), gpu_decode)
    check(r, "device" if gpu_decode else "host", 1)


@pytest.mark.parametrize("stranded", [None, "fr"])
@pytest.mark.parametrize("gpu_decode", [False, True])
def test_overhang_last(worlds, want, monkeypatch, capfd, tmp_path, gpu_decode, stranded):
    """The overhang is in the third shard.  Reads on the device: it is found when the third shard is laid out, while the second is
    about to be counted -- the first shard's chromosomes have been handed over and are handed over again.  Streaming: it is found
    when c6's turn comes, after c1 to c5."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "overhang_last", (0,), gpu_decode, stranded)
    check(r, "device" if gpu_decode else "host", 1, exact_contexts=[ALL6], handed_twice=["c1", "c2"] if gpu_decode else ["c1", "c2", "c3", "c4", "c5"])


@pytest.mark.parametrize("gpu_decode", [False, True])
def test_overhang_first(worlds, want, monkeypatch, capfd, tmp_path, gpu_decode):
    """The second plan begins before anything has been handed over, and has one shard where the first had two."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "overhang_first", (0,), gpu_decode)
    check(r, "device" if gpu_decode else "host", 1, exact_contexts=[["c1", "c2", "c3", "c4", "empty", "ghost"]])


@pytest.mark.parametrize("gpu_decode", [False, True])
def test_overhang_middle(worlds, want, monkeypatch, capfd, tmp_path, gpu_decode):
    """The understated reference's reads reach into the next one's slot, onto its sites: counted there, they would be in its beta1."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "overhang_middle", (0,), gpu_decode)
    check(r, "device" if gpu_decode else "host", 1, exact_contexts=[["c1", "c2", "c3", "empty", "ghost"]], handed_twice=[] if gpu_decode else ["c1"])


@pytest.mark.parametrize("gpu_decode", [False, None])
def test_unsorted_three_shards(worlds, want, monkeypatch, capfd, tmp_path, gpu_decode):
    """Half of c1 behind the last reference: the device declines the file, the host's threads find it unsorted at its end and
    ``process`` counts again with a new writer -- three shards both times, and no exact plan."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "unsorted_three_shards", (0,), gpu_decode)
    check(r, "host", 1, calls=2)


# ---- shares --------------------------------------------------------------------------------------------------------------------
def shares_of(r, n):
    """-> (the chromosomes of every context, the cut ones) from what the shares hold; every share holds reads, two chromosomes are cut."""
    w = r.world
    assert r.held is not None and len(r.held) == n
    reads = np.array([[x[0] for x in row] for row in r.held])
    assert np.all(reads.sum(axis=1) > 0) and reads.sum(axis=0).tolist() == [rs.n for rs in w.sets]
    cut = [c for c, col in zip(w.names, reads.T) if np.count_nonzero(col) > 1]
    assert len(cut) >= 2
    listed = {c: [k for k, (_, names) in enumerate(r.shares) if c in names] or [0] for c in r.table.chrom_index}
    contexts = [sorted((c for c in listed if k in listed[c]), key=lambda c: w.names.index(c) if c in w.names else 1 << 30) for k in range(n)]
    return contexts, cut, reads


def overhanging(r, n):
    """The contexts whose share holds reads of the understated reference beyond the room the first plan gives it."""
    w = r.world
    u = w.names.index(w.understated)
    room = max(w.lengths[u] + P.SLACK, int(r.table.chrom_arrays(w.understated).pos.max()))
    return [k for k in range(n) if r.held[k][u][0] and r.held[k][u][1] > room]


@pytest.mark.parametrize("n", [3, 5])
def test_cut(worlds, want, monkeypatch, capfd, tmp_path, n):
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "cut", (0,) * n, None)
    shares_of(r, n)
    check(r, "device", n)


@pytest.mark.parametrize("stranded", [None, "fr"])
@pytest.mark.parametrize("n", [3, 5])
def test_cut_overhang(worlds, want, monkeypatch, capfd, tmp_path, n, stranded):
    """The last context holds a piece of a cut chromosome and the understated reference, and plans twice; the overhang is in its
    second shard, found before the first is counted: nothing is handed over twice."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "cut_overhang", (0,) * n, None, stranded)
    contexts, cut, reads = shares_of(r, n)
    over = overhanging(r, n)
    assert over == [n - 1]
    assert any(reads[k][r.world.names.index(c)] for k in over for c in cut)      # a piece of a cut chromosome on a context that plans twice
    check(r, "device", n, exact_contexts=[contexts[k] for k in over])


@pytest.mark.parametrize("stranded", [None, "fr"])
def test_cut_overhang_late(worlds, want, monkeypatch, capfd, tmp_path, stranded):
    """The overhang is in the last context's THIRD shard: its first shard -- the rest of c2, cut, and c3 -- is counted and handed
    over, then the context plans again and counts it again.  The piece of c2 is written into the partial counters a second time
    and, if the other piece was there already, the sums go through ``spl_sse`` and to the writer a second time, the same."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "cut_overhang_late", (0, 0, 0), None, stranded)
    contexts, cut, reads = shares_of(r, 3)
    assert overhanging(r, 3) == [2] and contexts[2][:2] == ["c2", "c3"] and "c2" in cut and "c3" not in cut
    check(r, "device", 3, exact_contexts=[contexts[2]], handed_twice=["c3"], maybe_twice=["c2"])


@pytest.mark.parametrize("stranded", [None, "fr"])
def test_cut_three_shards(worlds, want, monkeypatch, capfd, tmp_path, stranded):
    """Several shards per context, a chromosome cut between contexts."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "cut_three_shards", (0, 0, 0), None, stranded)
    contexts, _, _ = shares_of(r, 3)
    assert len(P.plans(r.world, r.table, contexts[2])[0]) >= 2
    check(r, "device", 3)


def test_declined(worlds, want, monkeypatch, capfd, tmp_path):
    """Three shares are planned, the device decoder hands the file (CIGARs parked in CG tags) to the host's threads: every context
    streams the chromosomes it is the first listed for, and nobody counts one twice."""
    r = run(worlds, want, monkeypatch, capfd, tmp_path, "declined", (0, 0, 0), None)
    assert r.held is None and len(r.shares) == 3 and "CG tag" in r.declined
    check(r, "host", 3)
