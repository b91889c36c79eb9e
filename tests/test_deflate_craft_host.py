"""The crafted deflate corpora (tests/deflate_craft_lib.py) held to zlib, every property they claim asserted from their
token lists and code lengths, and the same corpora through the host inflater pss_inflate_raw (host/inflate_fast.c).
Needs no GPU; tests/test_gpu_inflate_crafted.py feeds the same corpora to the device decoders."""
import ctypes as C
import zlib

import pytest

import __graft_entry__ as ge
import deflate_craft_lib as dc


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in dc.valid_case_objects()}


def walk(case):
    """every token of a case with its surroundings: (block index, block, token, output position in the BGZF block,
    position in the deflate block, literal run in front of it)"""
    pos, out = 0, []
    for bi, b in enumerate(case.blocks):
        if b["kind"] == "stored":
            pos += len(b["data"])
            continue
        start, run = pos, 0
        for t in b["tokens"]:
            out.append((bi, b, t, pos, pos - start, run))
            if isinstance(t, int):
                pos, run = pos + 1, run + 1
            else:
                pos, run = pos + t[0], 0
    return out


def code_bits(b, t):
    """(litlen code bits, distance code bits or None) of a token in block b"""
    if isinstance(t, int):
        return b["ll_lens"][t], None
    return b["ll_lens"][dc.len_symbol(t[0], len(t) > 2 and t[2])[0]], b["d_lens"][dc.dist_symbol(t[1])[0]]


def matches(case):
    return [w for w in walk(case) if not isinstance(w[2], int)]


# ---------------------------------------------------------------------------------------------------------------------
# the library against zlib
# ---------------------------------------------------------------------------------------------------------------------
def test_writer_primitives():
    assert dc.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == {0: (2, 3), 1: (3, 3), 2: (4, 3), 3: (5, 3), 4: (6, 3), 5: (0, 2), 6: (14, 4), 7: (15, 4)}   # RFC 1951 3.2.2
    assert dc.comb_lens(16, 14) == list(range(1, 15)) + [15, 15]
    for n in range(2, 287):
        assert dc.kraft(dc.complete_lens(n)) == 1 << 15 and dc.kraft(dc.deepest_comb(n)) == 1 << 15
        assert max(dc.deepest_comb(n)) == (15 if n >= 16 else n - 1)
    assert [dc.len_symbol(l)[0] for l in (3, 10, 11, 12, 13, 257, 258)] == [257, 264, 265, 265, 266, 284, 285]
    assert dc.len_symbol(258, True) == (284, 5, 31)
    assert [dc.dist_symbol(d)[0] for d in (1, 4, 5, 6, 7, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 28, 29, 29]
    assert dc.replay([1, 2, 3, (5, 3), (3, 1)]) == bytearray([1, 2, 3, 1, 2, 3, 1, 2, 2, 2, 2])
    data = bytes(range(200)) * 3
    assert bytes(dc.replay(dc.greedy_tokens(data))) == data and len(dc.greedy_tokens(data)) < 210
    frame = dc.bgzf_frame(dc.Deflate().fixed(list(b"hello"), final=True).payload(), b"hello")
    assert zlib.decompress(frame, 31) == b"hello" and int.from_bytes(frame[16:18], "little") + 1 == len(frame)


def test_valid_cases_inflate_under_zlib_to_the_replayed_bytes():
    names = set()
    for name, payload, want in dc.valid_cases():
        d = zlib.decompressobj(-15)
        got = d.decompress(payload)
        assert got == want and d.eof and not d.unused_data and not d.unconsumed_tail, name
        assert len(want) <= 65536 and len(payload) + 25 <= 65535, name
        assert name not in names
        names.add(name)
    assert dc.valid_cases(0) == dc.valid_cases(0)       # deterministic


def test_invalid_cases_are_refused_by_zlib():
    seen = set()
    for name, payload, isize in dc.invalid_cases():
        assert isize > 0 and name not in seen, name
        seen.add(name)
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(payload)
        except zlib.error:
            continue
        assert not (d.eof and len(got) == isize), name
    want = {f"distance_{by}_beyond_output_at_{pos}" for by in (1, 100) for pos in (0, 1, 100)} | {
        "output_past_isize_by_literal", "output_past_isize_by_match", "output_short_of_isize", "litlen_symbol_286", "litlen_symbol_287",
        "distance_symbol_30", "distance_symbol_31", "oversubscribed_litlen_set", "oversubscribed_distance_set", "oversubscribed_code_length_set",
        "incomplete_litlen_set", "incomplete_distance_set_two_codes", "header_starts_with_16", "header_repeat_past_the_end",
        "no_code_for_symbol_256", "stored_len_nlen_mismatch", "stored_len_past_payload", "btype_3", "ends_in_mid_token", "ends_without_final_block"}
    assert want <= seen and set(dc.LENIENT) <= seen
    for c in dc.invalid_case_objects():                 # the writer's intent travels with the lenient cases, and only with them
        assert (c.intended is not None) == (c.name in dc.LENIENT) and (c.intended is None or len(c.intended) == c.isize), c.name


# ---------------------------------------------------------------------------------------------------------------------
# what the valid corpus claims to contain
# ---------------------------------------------------------------------------------------------------------------------
def test_corpus_code_lengths(cases):
    c = cases["ll_codes_10_to_15_bits"]
    used = {code_bits(b, t)[0] for _, b, t, *_ in walk(c)} | {c.blocks[0]["ll_lens"][256]}
    assert set(range(10, 16)) <= used
    assert any(code_bits(b, t)[0] >= 10 and code_bits(b, t)[1] <= 2 for _, b, t, *_ in matches(c))       # long litlen code, short distance code
    c = cases["dist_codes_9_to_15_bits"]
    assert set(range(9, 16)) <= {code_bits(b, t)[1] for _, b, t, *_ in matches(c)}
    assert any(code_bits(b, t)[0] <= 5 and code_bits(b, t)[1] >= 12 for _, b, t, *_ in matches(c))       # ... and the reverse
    assert any(t[1] == 32768 for _, _, t, *_ in matches(c))
    c = cases["all_286_and_30_symbols"]
    b = c.blocks[0]
    assert len(b["ll_lens"]) == 286 and all(b["ll_lens"]) and len(b["d_lens"]) == 30 and all(b["d_lens"])
    assert max(b["ll_lens"]) == 15 and max(b["d_lens"]) == 15
    lo, do = dc.token_symbols(b["tokens"])
    assert sorted(lo) == list(range(286)) and sorted(do) == list(range(30))
    for name in ("all_286_and_30_symbols", "every_length_fixed"):
        ms = [t for _, _, t, *_ in matches(cases[name])]
        assert {t[0] for t in ms} == set(range(3, 259)), name
        assert any(t[0] == 258 and len(t) > 2 and t[2] for t in ms) and any(t[0] == 258 and len(t) == 2 for t in ms), name   # 258 both ways
    b = cases["eob_plus_one_literal"].blocks[0]
    assert sorted(s for s, l in enumerate(b["ll_lens"]) if l) == [33, 256] and b["d_lens"] == [0]
    b = cases["literal_only_dynamic"].blocks[0]
    assert b["d_lens"] == [0] and all(isinstance(t, int) for t in b["tokens"]) and max(b["ll_lens"]) == 15
    c = cases["one_distance_code_of_length_1"]
    assert c.blocks[0]["d_lens"] == [1] and len(matches(c)) >= 3


def test_corpus_dynamic_headers(cases):
    b = cases["hdr_16_carries_litlen_length"].blocks[0]
    n, hlit = 0, len(b["ll_lens"])
    for it in b["header"]:
        if n == hlit:
            assert it == (16, 4) and b["ll_lens"][-1] == 2 and b["d_lens"] == [2, 2, 2, 2]     # 16 is the distance part's first code
            break
        n += 1 if isinstance(it, int) else it[1]
    else:
        raise AssertionError("no header code starts at the litlen / distance boundary")
    assert {dc.dist_symbol(t[1])[0] for _, _, t, *_ in matches(cases["hdr_16_carries_litlen_length"])} == {0, 1, 2, 3}
    b = cases["hdr_runs_17_18_16_and_boundary"].blocks[0]
    n, hlit, crossing = 0, len(b["ll_lens"]), []
    for it in b["header"]:
        m = 1 if isinstance(it, int) else it[1]
        if n < hlit < n + m:
            crossing.append(it)
        n += m
    assert crossing == [(18, 34)]                      # one run of zeros across the boundary
    items = b["header"]
    assert {(17, 3), (17, 10), (18, 11), (18, 138)} <= set(it for it in items if not isinstance(it, int))
    assert any(items[i] == (16, 6) and items[i + 1] == (16, 6) for i in range(len(items) - 1))
    b = cases["hdr_smallest_hclen"].blocks[0]
    assert b["hclen"] == 5 and [s for s in range(19) if b["cl_lens"][s]] == [0, 8, 16]
    for c in cases.values():                           # HCLEN is never larger than the block needs
        for b in c.blocks:
            if b["kind"] == "dynamic":
                assert b["hclen"] == max(4, max(i for i, s in enumerate(dc.CL_ORDER) if b["cl_lens"][s]) + 1)
                assert dc.kraft(b["ll_lens"]) == 1 << 15 and b["ll_lens"][256]
                assert dc.kraft(b["d_lens"]) in (0, 1 << 14, 1 << 15)


def test_corpus_matches(cases):
    for name in ("match_grid_fixed", "match_grid_dynamic"):
        have = {(t[1], (t[0] > t[1]) - (t[0] < t[1])) for _, _, t, *_ in matches(cases[name])}
        for d in dc.GRID_DISTS:
            assert (d, 1) in have or d >= 258, (name, d)
            assert (d, 0) in have or d < 3 or d > 258, (name, d)
            assert (d, -1) in have or d <= 3, (name, d)
    assert {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257} == set(dc.GRID_DISTS)
    for name in ("distance_32768_fixed", "dist_codes_9_to_15_bits"):
        assert {t[0] for _, _, t, *_ in matches(cases[name]) if t[1] == 32768} >= {3, 258}
    at0 = [n for n in cases if n.startswith("match_source_at_byte_0")]
    assert len(at0) >= 8
    for n in at0:
        assert sum(1 for _, _, t, pos, *_ in matches(cases[n]) if t[1] == pos) == 2, n      # source = byte 0 of the block's output
    for n in ("match_ends_at_isize", "match_run_ends_at_isize", "arena_distance_9"):
        assert not isinstance(cases[n].blocks[-1]["tokens"][-1], int), n
    assert {b["kind"] for _, b, t, _, in_block, _ in matches(cases["match_into_previous_block"]) if t[1] > in_block} == {"fixed", "dynamic"}
    assert {b["kind"] for b in cases["match_into_previous_block"].blocks} == {"fixed", "stored", "dynamic"}
    for n in ("literal_runs_255_256_600", "literal_runs_255_256_600_dynamic"):
        assert [run for *_, run in matches(cases[n])] == [255, 256, 600], n


def test_corpus_block_structure(cases):
    c = cases["empty_stored_at_every_bit_phase"]
    empty = [(i, b) for i, b in enumerate(c.blocks) if b["kind"] == "stored" and not b["data"]]
    assert {b["bit_start"] % 8 for _, b in empty} == set(range(8))
    assert all(0 < i < len(c.blocks) - 1 and c.blocks[i - 1]["kind"] == c.blocks[i + 1]["kind"] == "fixed" for i, _ in empty)
    c = cases["empty_fixed_blocks_not_final"]
    assert sum(1 for b in c.blocks[:-1] if b["kind"] == "fixed" and not b["tokens"]) >= 3
    assert cases["isize_0_empty_fixed"].expected == b"" and cases["isize_0_empty_fixed"].blocks[0]["kind"] == "fixed"
    assert cases["isize_0_empty_stored"].expected == b"" and cases["isize_0_empty_stored"].blocks[0]["kind"] == "stored"
    c = cases["300_dynamic_blocks"]
    assert len(c.blocks) == 300 and all(b["kind"] == "dynamic" for b in c.blocks) and 150 * 300 <= len(c.expected) <= 250 * 300
    assert len({tuple(b["ll_lens"]) for b in c.blocks}) > 250          # a table rebuild that matters, every time
    c = cases["nonzero_padding_behind_final_eob"]
    assert c.payload != c.df.payload(0) and c.payload[:-1] == c.df.payload(0)[:-1]
    for n, d in (("arena_distance_9", 9), ("arena_distance_3", 3)):
        ms = matches(cases[n])
        assert len(cases[n].expected) == 65535 and all(t == (3, d) for _, _, t, *_ in ms)
        assert len(ms) > 65535 // 4 + 1024                              # above seq_cap_of(isize) of csrc/inflate_wave.h
    assert set(dc.ARENA_CASES) <= set(cases)


def test_corpus_record_stream(cases):
    parts = [cases[n] for n in sorted(cases) if n.startswith("setA_records_")]
    data = dc.record_stream()
    assert b"".join(p.expected for p in parts) == data and len(parts) == (len(data) + 4095) // 4096 >= 20
    assert all(len(p.expected) == 4096 for p in parts[:-1])
    for p in parts:
        (b,) = p.blocks
        assert b["kind"] == "dynamic" and max(b["ll_lens"]) == 15
    assert sum(1 for p in parts if max(p.blocks[0]["d_lens"]) == 15) >= len(parts) // 2
    assert sum(len(matches(p)) for p in parts) > 1000                  # the matcher does find the records' repeats
    raw = dc.crafted_setA_bgzf()
    out, o = b"", 0
    while o < len(raw):
        n = int.from_bytes(raw[o + 16:o + 18], "little") + 1
        out += zlib.decompress(raw[o:o + n], 31)
        o += n
    assert out == data and raw.endswith(dc.bgzf_frame(b"\x03\x00", b""))   # ends in the BGZF EOF block


# ---------------------------------------------------------------------------------------------------------------------
# the host inflater
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inflate_raw():
    ge.build()
    L = C.CDLL(str(ge.load_pkg().LIB_HOST))
    L.pss_inflate_raw.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.pss_inflate_raw.restype = C.c_int
    st = C.create_string_buffer(32768)

    def run(payload, n):
        out = C.create_string_buffer(n + 16)
        out.raw = b"\xAA" * (n + 16)
        rc = L.pss_inflate_raw(st, payload, len(payload), out, n)
        assert out.raw[n:] == b"\xAA" * 16, "wrote behind the output"
        return rc, out.raw[:n]
    return run


def test_host_inflater_takes_every_valid_case(inflate_raw):
    for name, payload, want in dc.valid_cases():
        rc, got = inflate_raw(payload, len(want))
        assert rc == 0, (name, rc)
        assert got == want, name
        if want:
            assert inflate_raw(payload, len(want) - 1)[0] != 0, name
        assert inflate_raw(payload, len(want) + 1)[0] != 0, name


def test_host_inflater_refuses_every_invalid_case(inflate_raw):
    for c in dc.invalid_case_objects():
        rc, got = inflate_raw(c.payload, c.isize)
        if c.name in dc.LENIENT:
            # host/inflate_fast.c refuses over-subscribed codes only: an incomplete set whose missing codes never occur
            # decodes -- to exactly what the writer meant (the BGZF CRC then agrees); zlib refuses the set as such
            assert rc != 0 or got == c.intended, c.name
        else:
            assert rc != 0, c.name
