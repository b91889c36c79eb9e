"""The crafted streams of feed_chain_lib.py are what they claim to be (no GPU): the serial walk finds exactly the records
they were built from, every trap is where -- and as plausible as -- its case says, and the layouts reach the branch of the
bgzf_chain_* kernels they are named for.  A construction mistake fails here, not as a seeming kernel bug on the GPU."""
import struct

import pytest

import feed_chain_lib as fc

SMALL = [fc.tiny_blocks, fc.false_start_inside, fc.four_decoys, fc.broken_behind_anchor, fc.broken_far_apart,
         fc.broken_twice_in_a_row, fc.broken_at_super_end, lambda: fc.inside_long_record(False),
         lambda: fc.inside_long_record(True), lambda: fc.record_2_5_mib(False), lambda: fc.record_2_5_mib(True),
         lambda: fc.break_streams(True)[0], lambda: fc.break_streams(False)[0], lambda: fc.break_streams(True)[1],
         lambda: fc.break_streams(True)[2], fc.sub_ragged, fc.sub_long]
BIG = [lambda: fc.record_16_mib(0), lambda: fc.record_16_mib(1)]


def _first_pass(c, end=None):
    """every block's own guess and the broken links, for the super-batch whose data is raw[:end]"""
    bounds = [x for x in c.bgzf()[1] if end is None or x <= end]
    guesses = fc.spec(c.raw, bounds, c.head_len, end)
    return bounds, guesses, fc.broken_links(c.raw, guesses, end)


@pytest.mark.parametrize("make", SMALL + BIG)
def test_walk_finds_the_records_the_stream_was_built_from(make):
    c = make()
    recs, stop = fc.records_of(c)
    assert len(recs) == c.n_records
    assert b"".join(recs) == c.raw[c.head_len:stop]
    assert (stop == len(c.raw)) == (not c.flags & 8)          # only a stream cut inside a record leaves a tail
    clen = len(c.contigs[0][1])
    for r in recs:                                             # each one is a record the engine keeps
        bs, ref_id, pos, l_name, mapq, _, n_cig, flag, l_seq = struct.unpack_from("<IiiBBHHHI", r, 0)
        assert bs + 4 == len(r) and ref_id == 0 and mapq == 40 and flag & ~0x10 == 0 and n_cig == 1
        assert struct.unpack_from("<I", r, 36 + l_name)[0] == l_seq << 4 and 0 < pos and pos + l_seq < clen and l_seq >= 30
    assert set(c.contigs[0][1]) <= set("ACGT")
    # the layout holds the stream, block for block
    bgzf, bounds = c.bgzf()
    assert fc.tl.bgzf_inflate(bgzf) == c.raw and bounds[-1] == bounds[-2] == len(c.raw)


@pytest.mark.parametrize("make", SMALL)
def test_fake_chains_are_plausible_and_end_where_stated(make):
    c = make()
    true_starts = {a for a, _ in fc.walk(c.raw, c.head_len)[0]} | {fc.walk(c.raw, c.head_len)[1]}
    ends = [e for e in fc.super_ends(c.bgzf()[1], c.head_len, c.max_batch, int(c.env.get("PSSBAM_FEED_SUPER_BYTES", 0)) or None)]
    for f in c.fakes:
        assert f.at in c.bgzf()[1] or c.name in ("false_start_inside", "four_decoys")   # a block begins at the chain
        o = f.at
        for _ in range(f.n):
            assert fc.plausible(c.raw, o) and o not in true_starts
            # the kernels relax their rules near the end of a super-batch's data: no fake record starts there
            assert not any(e - fc.NEAR_END < o < e for e in ends), (c.name, o, ends)
            o += 4 + fc.u32(c.raw, o)
        if f.on_boundary:
            assert o in true_starts
        else:
            assert o not in true_starts and not fc.plausible(c.raw, o)
            assert fc.chain(c.raw, f.at) == (f.n, o)


def test_tiny_blocks_split_length_words_and_hold_the_empty_blocks():
    c = fc.tiny_blocks()
    bounds = c.bgzf()[1]
    sizes = {b - a for a, b in zip(bounds[:-1], bounds[1:])}
    assert {0, 1, 3, 4, 35, 36, 37} <= sizes and max(sizes) <= 37
    starts = [a for a, _ in fc.walk(c.raw, c.head_len)[0]]
    pieces = {sum(1 for x in bounds if s < x < s + 4) + 1 for s in starts}    # blocks a record's length word lies in
    assert {2, 3, 4} <= pieces
    assert any(0 < b - s < 36 for s in starts for b in bounds if b > s and b - s < 36)   # a candidate < 36 bytes before a block's end
    assert bounds.count(c.note["empty"]) >= 3 and bounds.count(c.note["eof"]) >= 2 and bounds.count(len(c.raw)) == 3
    assert 0 < c.note["empty"] < c.note["eof"] < len(c.raw)
    raw_bgzf = c.bgzf()[0]
    assert raw_bgzf.count(fc.tl.BGZF_EOF) >= 2 and raw_bgzf.index(fc.tl.BGZF_EOF) < len(raw_bgzf) - 28 * 2


def test_false_start_inside_a_block_is_taken_first():
    c = fc.false_start_inside()
    bounds, guesses, broken = _first_pass(c)
    b = bounds.index(c.note["block"])
    f = c.fakes[0]
    assert bounds[b] < f.at < c.note["true_start"] < bounds[b + 1]           # fake and true start in one block
    assert fc.plausible_offsets(c.raw, bounds[b], f.at) == []               # nothing in front of the fake
    assert guesses[b][0] == f.at and guesses[b][1] > f.n                    # the block claims the fakes and true records
    assert len(broken) == 1 and broken[0] < b and guesses[broken[0]][2] == c.note["true_start"]   # the host record's end


def test_four_decoys_exhaust_the_tries():
    c = fc.four_decoys()
    bounds, guesses, broken = _first_pass(c)
    b = bounds.index(c.note["block"])
    assert bounds[b] < c.note["true_start"] < bounds[b + 1]
    assert fc.plausible_offsets(c.raw, bounds[b], c.note["true_start"]) == [f.at for f in c.fakes] and len(c.fakes) == fc.TRIES
    for f in c.fakes:                                                        # none of the chains survives its second record
        assert fc.chain(c.raw, f.at)[0] == 1
    assert guesses[b] == (None, 0, 0)                                        # the block reports "no record" ...
    assert any(c.note["true_start"] <= a < bounds[b + 1] for a, _ in fc.walk(c.raw, c.head_len)[0])   # ... and holds some
    assert len(broken) == 1 and guesses[broken[0]][2] == c.note["true_start"]


def test_where_the_broken_links_lie():
    c = fc.broken_behind_anchor()
    bounds, guesses, broken = _first_pass(c)
    assert bounds[1] == c.fakes[0].at and guesses[1][0] == c.fakes[0].at and broken[0] == 0
    assert guesses[0][1] == 1                                                # block 0 starts the host record only

    c = fc.broken_far_apart()
    bounds, guesses, broken = _first_pass(c)
    b1, b2 = (bounds.index(f.at) for f in c.fakes)
    assert guesses[b1][0] == c.fakes[0].at and guesses[b2][0] == c.fakes[1].at
    first = [b for b in broken if b < b2 - 8]
    second = [b for b in broken if b >= b2 - 8]
    assert first and second and min(first) >= 64 and min(second) - max(first) > 64, broken

    c = fc.broken_twice_in_a_row()
    bounds, guesses, broken = _first_pass(c)
    b1, b2 = (bounds.index(f.at) for f in c.fakes)
    assert b2 == b1 + 1 and broken == [b1 - 1, b1], broken
    assert guesses[b1 - 1][1] > 1 and guesses[b1][0] == c.fakes[0].at and guesses[b2][0] == c.fakes[1].at


def test_fake_tail_at_the_end_of_a_super_batch():
    c = fc.broken_at_super_end()
    supers = c.supers()
    end0, f = supers[0][-1][1], c.fakes[0]
    assert len(supers) >= 2 and end0 == c.note["end0"]
    bounds, guesses, broken = _first_pass(c, end0)
    assert bounds[-2] == f.at and bounds[-1] == end0                         # the fake chain is the last block
    assert f.at + fc.NEAR_END < end0 < f.at + c.note["first_len"]            # its first record runs past the data
    assert guesses[-1][0] == f.at and guesses[-1][2] > end0                  # ... and is taken for the tail
    spans = fc.walk(c.raw, c.head_len)[0]
    assert spans[c.note["host"]][0] < f.at and spans[c.note["host"]][1] > end0   # the true tail is the host record
    assert broken and max(broken) < len(guesses) - 1


@pytest.mark.parametrize("trailer", [False, True])
def test_fake_chain_in_a_block_inside_a_long_record(trailer):
    c = fc.inside_long_record(trailer)
    bounds, guesses, broken = _first_pass(c)
    a, e = fc.walk(c.raw, c.head_len)[0][c.note["host"]]
    inside = [b for b in range(len(bounds) - 1) if a < bounds[b] and bounds[b + 1] < e]
    b = bounds.index(c.fakes[0].at)
    assert len(inside) >= 4 and b in inside and guesses[b][0] == c.fakes[0].at    # the record spans the blocks around them too
    assert broken and min(broken) < inside[0]
    assert (fc.chain(c.raw, c.fakes[0].at)[1] == e) == (not trailer) or not trailer


@pytest.mark.parametrize("with_fakes", [False, True])
def test_super_batches_in_which_no_record_starts(with_fakes):
    c = fc.record_2_5_mib(with_fakes)
    supers = c.supers()
    a, e = fc.walk(c.raw, c.head_len)[0][c.note["long"]]
    assert e - a == 4 + 2621440
    starts = [s for s, _ in fc.walk(c.raw, c.head_len)[0]]
    empty = [k for k, sb in enumerate(supers) if not any(sb[0][0] <= s < sb[-1][1] for s in starts)]
    assert len(empty) >= 2 and empty[1] == empty[0] + 1 and empty[0] >= 1 and empty[-1] + 1 < len(supers)   # the carry grows twice
    lo, hi = supers[empty[0]][0][0], supers[empty[0]][-1][1]
    for f in c.fakes:                                                        # the fake chains lie in the first of them
        assert lo < f.at and f.at + 1000 < hi and f.at in c.bgzf()[1]
    if with_fakes:                                                           # ... where their blocks claim them against the carried record
        bounds = [x for x in c.bgzf()[1] if lo <= x <= hi]
        guesses = fc.spec(c.raw, bounds, a, hi)
        assert guesses[0] == (a, 1, e) and all(guesses[bounds.index(f.at)][0] == f.at for f in c.fakes)
        assert fc.broken_links(c.raw, guesses, hi)[0] == 0


def test_the_16_mib_records():
    for over in (0, 1):
        c = fc.record_16_mib(over)
        a, e = fc.walk(c.raw, c.head_len)[0][c.note["long"]]
        assert e - a == 4 + (1 << 24) + over and fc.u32(c.raw, a) == fc.MAX_RECORD + over
        assert len(c.supers()) == 1 and 17_000_000 > len(c.raw) > (1 << 24)


def test_break_streams():
    cx, cy, cy0 = fc.break_streams(True)
    whole, stop = fc.records_of(cx)
    assert len(whole) == 299 and len(cx.raw) - stop > 36 and stop + 4 + fc.u32(cx.raw, stop) == len(cx.raw) + 37
    # without the break the cut record would swallow the head of what follows, and a chain would go on from there
    assert cy0.raw == cy.raw[cy.head_len:] and cy0.head_len == 0 and cy.head_len > 37
    assert fc.break_streams(False)[0].raw[:len(cx.raw)] == cx.raw


def test_sub_batches():
    c = fc.sub_ragged()
    supers = c.supers()
    spans = fc.walk(c.raw, c.head_len)[0]
    subs = [s for sb in supers for s in sb]
    assert len(subs) >= 3 and all(b - a <= 131072 for a, b in subs)
    inner = [b for sb in supers for _, b in sb[:-1]]                        # sub-batch bounds inside a super-batch
    assert inner and all(any(a < x < e for a, e in spans) for x in inner)    # each is crossed by a record
    assert fc.super_batches(c.bgzf()[1], c.head_len, c.max_batch, 1 << 20) == [[(sb[0][0], sb[-1][1])] for sb in supers]
    c = fc.sub_long()
    starts = [s for s, _ in fc.walk(c.raw, c.head_len)[0]]
    subs = [s for sb in c.supers() for s in sb]
    assert sum(1 for a, b in subs if not any(a <= s < b for s in starts)) >= 10   # sub-batches without a record start
    assert any(len(sb) > 1 and not any(sb[0][0] <= s < sb[-1][1] for s in starts) for sb in c.supers())
