"""The hand-built DEFLATE cases of deflatecases.py on the CPU: first that every case is what it says -- zlib takes or refuses it as
listed, the plain reader agrees with zlib, the tables, bit positions, run lengths and sweeps reach the limits they name -- then the
cases through the kernel's body under the wave emulator (tests/hostsim: the same source, every access bounds-checked), where the
harness runs a block three ways (default, a writing pass per tile, the denser kernel's token room), compares their tokens and bytes,
guards the token room and counts which way every tile went.  test_gpu_inflate_limits.py runs the same cases on the card.

Mutants of spl_inflate_wave.h tried against this file and against test_inflate_wave_host.py (CPU only, scratch copies):
  caught here, not there    the `cap` check of build_lut removed (literal_table_over / distance_table_over);
                            symbol 16 not carrying the last literal length into the distance lengths (rep16_across_boundary)
  caught by both            one nibble of 0x1230200 changed; run == 127 in emit_from; need >= in place of need >
  equivalent, dropped       lit2 taken when pos <= stop (every walk uses decode(): the lanes' hand-over moves with it, bytes and status
                            cannot tell); the window's cut-off dist < RING - 16 (distance RING - 16 then takes the memory path, whose
                            source lies behind `flushed`); 0xfff dropped for distance symbols 30 / 31 (build_lut is never given more
                            than 30 distance lengths, the fixed code included: the line cannot be reached)
A literal run of 257 inside one lane, which the list of limits asked for, cannot be: a lane's symbols begin in its SUB_BITS = 256 bits."""
import ctypes
import os

import numpy as np
import pytest

import deflatecases as dc
from test_inflate_wave_host import load_emulator

IN_PLACE, MISFIT, CUT_SHORT, WRITING_PASS = range(4)     # (the harness's counters, in its order)
DEFAULT, ALL_WRITING, SMALL = range(3)                   # (its three runs of a block)


@pytest.fixture(scope="module")
def emul():
    return load_emulator()


def run(lib, cases, room=dc.SPL_Z_TOKEN_STRIDE, tokens=False):
    """-> status, each block's stretch of the output, the path counters [block][run][path], the last block's token stream"""
    image, blocks, starts, total = dc.image_of(cases)
    img = np.frombuffer(image, np.uint8).copy()
    out = np.full(total + 128, 0xA5, np.uint8)
    status = np.full(len(cases), 0xffffffff, np.uint32)
    paths = np.zeros((len(cases), 3, 4), np.uint32)
    tok, n_tok = np.zeros(dc.SPL_Z_TOKEN_STRIDE if tokens else 16, np.uint8), ctypes.c_uint32(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.emul_inflate_blocks_room(p(img), p(blocks), ctypes.c_uint32(len(cases)), p(out), p(status), ctypes.c_uint32(room), p(paths),
                                      p(tok) if tokens else None, ctypes.byref(n_tok))
    assert rc == 0, "block %d (%s): the emulated wave broke a rule of spl_wave.h, the three runs disagree or the token room's guard is damaged (%d)" % (
        (-1 - rc) % 100000, cases[(-1 - rc) % 100000].name, rc)
    got = out.tobytes()
    assert got[total:] == b"\xa5" * 128
    return status, [got[at:at + len(c.data)] for at, c in zip(starts, cases)], paths, tok[:n_tok.value].tobytes()


# ---- the cases are what they say (no kernel) -----------------------------------------------------------------------------------

def test_zlib_and_the_plain_reader_on_every_case():
    n = {"legal": 0, "refuse": 0, "lenient": 0}
    for c in dc.named_cases() + dc.sweep(False):
        z = dc.zlib_takes(c.comp)
        try:
            mine = dc.inflate(c.comp)
        except dc.Refused:
            mine = None
        if c.kind == "legal":
            assert z == c.data and mine == z, c.name
        elif c.info.get("stream_is_legal"):              # (refused for the out_len it comes with, not for its bits)
            assert z is not None and mine == z and len(z) != len(c.data), c.name
        elif c.kind == "refuse":
            assert z is None and (mine is None) != bool(c.info.get("reader_takes")), c.name   # (reader_takes: only the table's room is against it)
        else:
            assert z is None and mine is not None, c.name
        assert c.limit and len(c.comp) <= 65536 and 0 < len(c.data) <= 65536
        n[c.kind] += 1
    assert n["legal"] > 250 and n["refuse"] >= 30 and n["lenient"] >= 1


def test_the_plain_reader_on_zlibs_own_streams():
    import zlib
    rng = np.random.default_rng(1)
    for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
        data = (b"".join(bytes(rng.integers(0, 256, 7, dtype=np.uint8)) * int(rng.integers(1, 9)) for _ in range(300)))
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        assert dc.inflate(c.compress(data) + c.flush()) == data


def test_tables_reach_their_sizes():
    """build_lut's sizing rule restated (dc.table_entries): the stored figures are what the rule gives, and they are the tables' sizes."""
    lit, dist = dc._spread(dc.LIT_MOST[0], 286), dc._spread(dc.DIST_MOST[0], 30)
    assert dc.table_entries(lit, dc.ROOT_L) == dc.LIT_MOST[1] == dc.LUT_L
    assert dc.table_entries(dist, dc.ROOT_D) == dc.DIST_MOST[1] == dc.LUT_D
    assert sum(2.0 ** -n for n in lit if n) == 1.0 and sum(2.0 ** -n for n in dist if n) == 1.0 and max(lit) == max(dist) == 15
    full = {c.name: c for c in dc.named_cases()}["tables_full"]
    assert full.info["lit"] == lit and full.info["dist"] == dist
    assert dc.table_entries(dc._spread(dc.LIT_OVER[0], 286), dc.ROOT_L) == dc.LIT_OVER[1] > dc.LUT_L
    assert dc.table_entries(dc._spread(dc.DIST_OVER[0], 30), dc.ROOT_D) == dc.DIST_OVER[1] > dc.LUT_D
    for lens in (dc._spread(dc.LIT_OVER[0], 286), dc._spread(dc.DIST_OVER[0], 30)):
        assert sum(2.0 ** -n for n in lens if n) < 1.0  # (not over-subscribed: it is the table's room that refuses them)
    assert sorted(set(dc.COMB_LIT) - {0}) == list(range(1, 16)) and sorted(set(dc.COMB_DIST) - {0}) == list(range(1, 16))
    assert 15 - dc.ROOT_L == 6


def test_symbols_begin_where_the_cases_say():
    by = {c.name: c for c in dc.named_cases()}
    lit, dist = dc.canonical(dc.COMB_LIT), dc.canonical(dc.COMB_DIST)
    assert lit[284][1] + dc.LEN_EXTRA[27] + dist[29][1] + dc.DIST_EXTRA[29] == 48 == 15 + 5 + 15 + 13
    c = by["longest_symbol_lane_end"]
    assert (c.info["at"] - c.info["base"]) % dc.SUB_BITS == dc.SUB_BITS - 1 and (c.info["at"] - c.info["base"]) % dc.TILE_BITS != dc.TILE_BITS - 1
    c = by["longest_symbol_tile_end"]
    assert (c.info["at"] - c.info["base"]) % dc.TILE_BITS == dc.TILE_BITS - 1
    assert 48 > 32 and dc.TILE_PAD * 32 >= 48 + 32       # (it ends in the words behind the tile, which hold it and the word a read takes with it)
    c = by["longest_symbol_data_end"]
    assert c.info["n_bits"] - c.info["at"] == 48 + 3 and len(c.comp) * 8 - c.info["at"] < 64
    assert by["longest_symbol_bit31"].info["at"] % 32 == 31
    for c in (by["longest_symbol_lane_end"], by["longest_symbol_tile_end"], by["longest_symbol_bit31"], by["longest_symbol_data_end"]):
        assert c.info["base"] % 32 == 0 and len(c.data) > 32768
    for name in ("lit2_ends_on_stop", "lit2_ends_past_stop"):
        assert (by[name].info["at"] - by[name].info["base"]) % dc.SUB_BITS == dc.SUB_BITS - 2
    assert lit[dc.A][1] == 1 and lit[dc.B][1] == 2 and lit[dc.D_][1] == dc.ROOT_L and lit[dc.C_][1] == dc.ROOT_L + 1
    runs = set()
    for c in dc.named_cases():
        if "run" in c.info:
            at, end, base = c.info["at"], c.info["end"], c.info["base"]
            assert (at - base) // dc.SUB_BITS == (end - 1 - base) // dc.SUB_BITS, c.name      # (all in one lane)
            assert c.data.count(bytes([dc.A]) * c.info["run"]) >= 1 or "shifted" in c.name
            runs.add((c.info["run"], "shifted" in c.name, (end - base) % dc.SUB_BITS == 0))
    assert {r[0] for r in runs} == {127, 128, 129, 255, 256}
    assert any(r[2] for r in runs) and any(r[1] and r[0] >= 128 for r in runs) and any(not r[1] and r[0] >= 128 for r in runs)
    for phase in (1, 17, 31):
        assert by["section_at_bit_%d" % phase].info["at"] % 32 == phase
    assert by["tile_over_tokcap"].info["per_tile"] > dc.TOKCAP
    assert dc.TOKCAP_SMALL < by["tile_over_tokcap_small"].info["per_tile"] <= dc.TOKCAP
    assert len(by["out_len_65536"].data) == 65536 and len(by["in_len_65536"].comp) == 65536


def test_the_sweep_covers_what_it_says():
    full, thin = dc.sweep_params(True), dc.sweep_params(False)
    dists = set(range(1, 65)) | {dc.RING - 17, dc.RING - 16, dc.RING - 15, 255, 256, 257, 258, 32767, 32768}
    lens = {3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 257, 258}
    assert set(full) == {(d, n, p) for d in dists for n in lens for p in range(16)} and len(full) == len(set(full))
    assert {d for d, _, _ in thin} == dists and {n for _, n, _ in thin} == lens and {p for _, _, p in thin} == set(range(16))
    for d in list(range(1, 9)) + [dc.RING - 17, dc.RING - 16, dc.RING - 15]:
        assert {n for dd, n, _ in thin if dd == d} == lens
    assert set(thin) <= set(full) and len(thin) < 400
    for d, n, p in thin[::17]:                          # (the match begins where the name says)
        c = dc.sweep_block(d, n, p)
        assert (len(c.data) - 2 * n - 1) % 16 == p and len(c.data) - 2 * n - 1 >= d


# ---- the cases through the wave emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def named_run(emul):
    cases = dc.refusals_between_legal(dc.named_cases())
    return (cases,) + run(emul, cases)


def test_named_cases_under_the_emulator(named_run):
    cases, status, got, _, _ = named_run
    for k, c in enumerate(cases):
        if c.kind != "legal":                           # (between two legal ones: their bytes and status are checked like everyone's)
            assert cases[k - 1].kind == "legal" and cases[k + 1].kind == "legal"
        dc.check(c, status[k], got[k])


def test_every_path_of_a_tile_is_taken(named_run):
    cases, status, _, paths, _ = named_run
    by = {c.name: k for k, c in enumerate(cases)}
    total = paths.astype(np.int64).sum(axis=0)
    print("tiles in place / with a misfit lane / cut short / by the writing pass: default run %s, all by the writing pass %s, TOKCAP_SMALL %s" %
          tuple(list(total[r]) for r in range(3)))
    assert all(total[DEFAULT][p] > 0 for p in (IN_PLACE, MISFIT, CUT_SHORT, WRITING_PASS))
    assert total[ALL_WRITING][IN_PLACE] == 0 and total[ALL_WRITING][WRITING_PASS] > 0
    assert paths[by["guess_sees_end_of_block"]][DEFAULT][MISFIT] > 0
    # (wrong guesses: lanes write their tokens twice, behind the places, and a tile holds up to two rooms' worth uncut -- but not when
    #  every tile takes the writing pass; right guesses: the places do not fit, the writing pass takes the tile and cuts it)
    assert paths[by["tile_over_tokcap"]][ALL_WRITING][CUT_SHORT] > 0 and paths[by["tile_over_tokcap"]][DEFAULT][MISFIT] > 0
    k = by["tile_over_tokcap_small"]
    assert paths[k][ALL_WRITING][CUT_SHORT] == 0 and paths[k][SMALL][MISFIT] + paths[k][SMALL][CUT_SHORT] > 0
    k = by["tile_over_tokcap_right_guesses"]
    assert paths[k][DEFAULT][CUT_SHORT] > 0 and paths[k][DEFAULT][WRITING_PASS] > 0 and paths[k][DEFAULT][MISFIT] == 0
    k = by["tile_over_tokcap_small_right_guesses"]
    assert paths[k][DEFAULT][CUT_SHORT] == 0 and paths[k][SMALL][CUT_SHORT] > 0
    k = by["longest_symbol_tile_end"]                   # (whole tiles of 64 lanes, as the case's arithmetic assumes)
    assert paths[k][DEFAULT][CUT_SHORT] == 0 and status[k] == 0


def test_the_sweep_under_the_emulator(emul):
    """The covering subset by default (every distance, length and phase once and more; all lengths at the distances below 8, at 8
    and around RING - 16); SPL_EMUL_SWEEP_EVERY=n takes every n-th block of the FULL product instead (1: all 14 560, about an hour)."""
    every = int(os.environ.get("SPL_EMUL_SWEEP_EVERY", "0"))
    cases = dc.sweep(False) if every == 0 else [dc.sweep_block(*p) for p in dc.sweep_params(True)[::every]]
    status, got, _, _ = run(emul, cases)
    for k, c in enumerate(cases):
        dc.check(c, status[k], got[k])


def _tokens(stream):
    """-> [(offset, 'run' or 'match')] of a token stream"""
    at, out = 0, []
    while at < len(stream):
        if stream[at] < 0x80:
            out.append((at, "run"))
            at += stream[at] + 2
        else:
            out.append((at, "match"))
            at += 3
    assert at == len(stream)
    return out


def test_tokens_on_every_offset_of_the_beat_and_across_the_fifos_wrap(emul):
    seen = {"run": set(), "match": set()}
    for c in dc.named_cases():
        if c.name.startswith("token_offsets_"):
            status, got, _, stream = run(emul, [c], tokens=True)
            dc.check(c, status[0], got[0])
            for at, kind in _tokens(stream):
                seen[kind].add(at % dc.FIFO)
    for kind in ("run", "match"):
        assert {o % 64 for o in seen[kind]} == set(range(64)), kind
        assert {o % dc.FIFO for o in seen[kind]} >= {o % dc.FIFO for o in range(125, 131)}, kind


@pytest.mark.parametrize("room", [256, 1024, 8192, 40000])
def test_less_token_room_than_the_stride(emul, room):
    """A block given less room than SPL_Z_TOKEN_STRIDE: SPL_Z_TOKENS or the right bytes, and nothing behind the room it was GIVEN
    (the harness keeps guard bytes there, for all three runs)."""
    cases = [c for c in dc.named_cases() if c.kind == "legal" and (len(c.data) < 6000 or c.name in ("tables_full", "out_len_65536", "in_len_65536"))]
    cases += [dc.sweep_block(*p) for p in dc.sweep_params(False)[::9]]
    status, got, _, _ = run(emul, cases, room=room)
    n_ok = 0
    for k, c in enumerate(cases):
        assert status[k] in (dc.OK, dc.TOKENS), (c.name, int(status[k]))
        if status[k] == dc.OK:
            assert got[k] == c.data, c.name
            n_ok += 1
        else:
            assert 2 * len(c.data) > room - 64, c.name   # (a byte of output is two bytes of tokens at most, a run of one literal: not refused for nothing)
    assert n_ok > 0


@pytest.mark.parametrize("variant", dc.PERVERSE)
def test_perverse_writers_make_legal_streams(emul, variant):
    """What test_gpu_inflate_limits.py writes whole BAM files with: BAM-like bytes, parsed the way `variant` names -- zlib reads them
    back, they fit a BGZF block, the parse is what it says, and the emulator inflates them."""
    import zlib
    rng = np.random.default_rng(9)
    recs = [b"read%05d\0" % k + bytes(rng.integers(0, 4, 40, dtype=np.uint8) * 17) + bytes([60, 0, 0, 0]) * 3 + b"F" * 40 for k in range(400)]
    payload = b"".join(recs[int(k)] if rng.random() < 0.3 else recs[i] for i, k in enumerate(rng.integers(0, 400, 400)))[:0xC000]
    comp = dc.perverse_deflate(payload, variant)
    assert zlib.decompress(comp, -15) == payload and len(comp) + 26 <= 0x10000
    syms = dc.parse(payload, {"len3_farthest": "len3_farthest", "longest_far": "longest_far"}.get(variant, "greedy"))
    matches = [s for s in syms if not isinstance(s, int)]
    assert len(matches) > 100
    if variant == "len3_farthest":
        assert {m[0] for m in matches} == {3} and max(m[1] for m in matches) > 16384
    if variant == "longest_far":
        assert min(m[1] for m in matches) >= dc.RING - 15 and max(m[0] for m in matches) > 100
    case = dc.Case(variant, "a whole payload, " + variant, "legal", comp, payload, None, {})
    status, got, _, _ = run(emul, [case])
    dc.check(case, status[0], got[0])
