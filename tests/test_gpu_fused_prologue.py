"""The fused range kernel takes everything uniform about its chunk from ONE descriptor per slot of its grid (spl_fused_slot: made
per chunk by spl_layout_map_kernel, put in slot order by spl_chunk_order_kernel) -- the chunk's number, its place in the arrays,
the CIGAR offsets at all its tile boundaries, the POS of its first read, a marker for a slot without a chunk -- asks for the
bucket entry of that POS beside the first tile's reads and resolves the window's base only behind the first tile's stage; a
thread's places in a tile are 32-bit offsets from the cell and from the ops' window.  Cases built to where each of these can go
wrong, at both chunk sizes: the fused pass against the oracle and against the same shard through layout + range (SPL_FUSED=0),
bit for bit -- the counters and the beta2 / SSE doubles -- unstranded and in one stranded mode."""
import numpy as np
import pytest

import limitcases as L
from limitcases import M, N, S
from spliser_amd import native, samio

pytestmark = pytest.mark.gpu

TILE, CHUNK, CHUNK_BIG = L.TILE, L.CHUNK, L.CHUNK_BIG
MODES = [(0, 0), (2, 1)]                        # unstranded; rf in combine mode


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _check(ctx, oracle_lib, monkeypatch, case, chunks=(CHUNK, CHUNK_BIG)):
    """fused == layout + range == oracle, counters and SSE, in both modes and at every chunk size asked for (the oracle once a mode)."""
    sites = case.table.sites()
    t, r = case.table, case.reads
    counted = 0
    for stranded, combine in MODES:
        want = oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar,
                                    stranded, combine)
        cryptic = (stranded + combine) % 2 == 0
        want_sse = oracle_lib.beta2_sse(t.pos, t.part_off, t.part_pos, t.part_site, t.alpha, t.edge_cnt, want[0], want[1], want[2], cryptic)
        counted += int(want[0].sum()) + int(want[1].sum())
        for chunk in chunks:
            monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
            for fused in (False, True):
                monkeypatch.setenv("SPL_FUSED", "1" if fused else "0")
                got = L.count_device(ctx, sites, case.segments, stranded, combine, cryptic)
                tag = (case.name, "stranded", stranded, "combine", combine, "chunk", chunk, "fused", fused)
                assert got.fused == fused, tag
                for w, g in zip(want, got.counters):
                    assert np.array_equal(w, g), tag
                for w, g in zip(want_sse, got.sse):
                    assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=w.dtype.kind == "f"), tag
    assert counted > 0, case.name               # (the case counts something at all)


def _mixed(rng, classes):
    return [L._mixed_read(rng, int(c)) for c in classes]


def _shifted(recs, shift):
    return L.reads_from([(f, p - shift, ops) for f, p, ops in recs]), shift


# ---- where segments begin and end -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [CHUNK, CHUNK_BIG])
def test_segments_that_begin_in_every_tile_of_a_cell(chunk, ctx, oracle_lib, monkeypatch):
    """Segments with different shifts end to end in one set of arrays: they begin at array indexes = 0, 1, 1023, 1024, 1025 and
    chunk - 1 (mod chunk) -- a first chunk that starts in tile 0, in tile 1 (one read before its boundary is tile 0's last read), exactly
    on a tile boundary and in the cell's last tile, with one read in it -- one of them, in the middle, has no reads at all, and
    the last one ends at an index = 1 (mod chunk): its last chunk is one read of tile 0."""
    starts = [0, 1, chunk + 1023, 2 * chunk + 1024, 2 * chunk + 1024, 3 * chunk + 1025, 5 * chunk - 1, 6 * chunk + 1]
    rng = np.random.default_rng(chunk)
    segments = []
    for k in range(len(starts) - 1):
        n = starts[k + 1] - starts[k]
        segments.append(_shifted(_mixed(rng, rng.choice([0, 0, 0, 1, 1, 2, 3, 4, 5], n)), 300 + 4100 * k))
    assert [rs.n for rs, _ in segments][3] == 0 and sum(rs.n for rs, _ in segments) == 6 * chunk + 1
    case = L.Case("prologue_segments_%d" % chunk, L._tile_table(), segments, "segments from indexes 1, 1023, 1024, 1025, chunk - 1 on")
    _check(ctx, oracle_lib, monkeypatch, case, chunks=(chunk,))


# ---- how many chunks: XCD shares with empty slots, with one chunk, of unequal length --------------------------------------------

_POOL = {}


def _bulk(n):
    """n simple, once- and twice-spliced reads over _tile_table's sites, made array by array (133 k reads one by one take seconds)."""
    if "all" not in _POOL:
        rng = np.random.default_rng(65)
        big = 65 * CHUNK
        cls = rng.choice([0, 0, 0, 1, 1, 2], big)
        # (stretches of one class: the chunks' cost estimates differ, and so does their order inside an XCD's share)
        cls[(np.arange(big) // 3000) % 3 == 1] = 0
        off = np.concatenate(([0], np.cumsum(1 + 2 * cls))).astype(np.int64)
        at = off[:-1]
        m_len, n_len = rng.integers(5, 60, (big, 3)).astype(np.uint32), (7 * rng.integers(1, 9, (big, 2))).astype(np.uint32)
        cig = np.zeros(off[-1], np.uint32)
        cig[at] = (m_len[:, 0] << 4) | M
        for j in (1, 2):
            sel = cls >= j
            cig[at[sel] + 2 * j - 1] = (n_len[sel, j - 1] << 4) | N
            cig[at[sel] + 2 * j] = (m_len[sel, j] << 4) | M
        _POOL["all"] = (30000 + rng.integers(-40, 2700, big).astype(np.int64), rng.choice([0, 16, 99, 147], big).astype(np.uint16), off, cig)
    pos, flag, off, cig = _POOL["all"]
    return samio.ReadSet(pos[:n].copy(), flag[:n].copy(), off[:n + 1].astype(np.uint32), cig[:off[n]].copy())


@pytest.mark.parametrize("n_chunks", [1, 7, 8, 9, 63, 64, 65])
def test_chunk_counts_around_the_xcd_shares(n_chunks, ctx, oracle_lib, monkeypatch):
    """Eight slots or sixteen a share: shares with nothing but empty slots (1, 7, 8 chunks: one block of 8 goes to one XCD), with
    one chunk beside empty slots (9), of unequal length (63, 65) and equal (64) -- every chunk counted once, no empty slot counted."""
    case = L.Case("prologue_chunks_%d" % n_chunks, L._tile_table(), [(_bulk(n_chunks * CHUNK - 701), 0)], "%d chunks" % n_chunks)
    _check(ctx, oracle_lib, monkeypatch, case, chunks=(CHUNK,))


# ---- a chunk's first read at the edges of the position index -----------------------------------------------------------------------

def test_first_read_left_of_the_position_index_and_right_of_the_last_site(ctx, oracle_lib, monkeypatch):
    """The window's base comes from the bucket entry of the chunk's first POS - 1, asked for in the prologue and resolved behind the
    first tile's stage.  One segment's first read lies far left of the index's first bucket (the clamp to bucket 0: the window
    begins at the first site), the next one's right of the last site (the index's last, empty bucket: window base = the number of
    distinct positions, every commit a global one); then the same two places with a once-spliced first read, the left one in
    front of a chunk and 21 reads.  All segments hold simple and once-spliced reads over the sites."""
    rng = np.random.default_rng(7)
    body = lambda n: _mixed(rng, rng.choice([0, 0, 1], n))
    left = [(0, 40, [(50, M)])] + body(700)
    right = [(16, 30000 + 7 * 400 + 5000, [(50, M)])] + body(TILE + 300)
    right_spliced = [(0, 30000 + 7 * 400 + 900, [(20, M), (70, N), (20, M)])] + body(333)
    left_spliced = [(16, 3, [(11, M), (14, N), (30, M)])] + body(CHUNK + 20)
    case = L.Case("prologue_index_edges", L._tile_table(), [_shifted(left, 0), _shifted(right, 1700), _shifted(right_spliced, 0), _shifted(left_spliced, 0)],
                  "first POS outside the position index")
    _check(ctx, oracle_lib, monkeypatch, case)


# ---- reads on a tile boundary ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["wide", "one_op"])
def test_reads_on_both_sides_of_every_tile_boundary(kind, ctx, oracle_lib, monkeypatch):
    """wide: tiles of mostly WIDE reads (nine ops: a tile's ops take more than one stage of 4 TILE words, its records more than the
    record area -- halves), the last read of every tile and the first of the next WIDE ones; one_op: the same places hold one-op
    reads, between reads of every class.  The boundaries' op offsets are the descriptor's."""
    rng = np.random.default_rng(len(kind))
    n = 2 * CHUNK_BIG + 300
    cls = rng.choice([4, 4, 4, 0, 1, 2], n) if kind == "wide" else rng.integers(0, 6, n)
    for b in range(TILE, n, TILE):
        cls[b - 1] = cls[b] = 4 if kind == "wide" else 0
    case = L.Case("prologue_boundary_" + kind, L._tile_table(), [(L.reads_from(_mixed(rng, cls)), 0)], "reads at indexes k TILE - 1, k TILE")
    _check(ctx, oracle_lib, monkeypatch, case)


# ---- the end of the arrays ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 2, 3])
def test_arrays_that_end_inside_a_thread_s_four_reads_and_inside_a_quad_of_ops(r, ctx, oracle_lib, monkeypatch):
    """n_rec = r (mod 4): the last thread takes its reads one by one, guarded by the cell's own count; the ops' array ends r words
    into its last quad (n_ops = r mod 4: the quad's first word is the op at n_ops - r), which is loaded word by word."""
    rng = np.random.default_rng(40 + r)
    n = CHUNK + TILE + 4 + r
    recs = _mixed(rng, rng.integers(0, 6, n - 8)) + _mixed(rng, [0] * 8)
    more = (r - sum(len(ops) for _, _, ops in recs)) % 4
    for k in range(more):                       # (a soft clip in front: one op more, still counted in place)
        f, p, ops = recs[n - 2 - k]
        recs[n - 2 - k] = (f, p, [(3, S)] + ops)
    rs = L.reads_from(recs)
    assert rs.n % 4 == r and len(rs.cigar) % 4 == r
    _check(ctx, oracle_lib, monkeypatch, L.Case("prologue_end_%d" % r, L._tile_table(), [(rs, 0)], "n_rec, n_ops = %d (mod 4)" % r))
