"""The inputs of the entropy decoder's built-scan tests, judged on the CPU (no
GPU, no kernel runs): every test here is a condition on what
tests/unscan_built.py and tests/unscan_corpus.py make, read from the bytes, the
offsets and the restatement alone, so that a GPU test which passes cannot have
missed the case it is there for.

- the catalogue: all 2,784 (table, symbol, bit phase) combinations, both extreme
  extra-bit patterns of every size; jpeg_scan.encode writes the same bytes and
  jpeg_unscan.decode reads the blocks back;
- the stuffed scan: interval lengths 2..24, a quarter of the bytes FF, FF 00
  pairs at every (interval address, pair address) mod 8, in the first and in
  the last eight bytes of an interval;
- the colour corpus: every status code at every position of the MCU, the DC
  predictor of each component alone;
- the marker cases: where the written markers lie against the 64-byte steps and
  the 4096-byte chunks of the search.
"""
import numpy as np
import pytest

import jpeg_scan as J
import jpeg_unscan as U
import unscan_built as B
import unscan_corpus


# ---------------------------------------------------------------------------
# A. the catalogue
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["444", "grey"])
def test_catalogue_holds_every_code_at_every_phase(sampling):
    b = B.catalogue(sampling)
    kinds = (0, 1) if sampling == "grey" else (0, 1, 2, 3)
    need = B.all_combinations(kinds)
    assert len(need) == (12 + 162) * len(kinds) // 2 * 8 and len(need) == (1392 if sampling == "grey" else 2784)
    seen, extremes = B.trace(b["components"], sampling, b["ri"])      # from the blocks alone
    assert seen == b["seen"] and extremes == b["extremes"]
    missing = need - seen
    assert not missing, (len(missing), sorted(missing)[:8])
    # both extreme patterns of the extra bits, all zeros (-(2^n - 1)) and all ones (2^n - 1), for every size
    sizes = {(k, n, v) for k in kinds for n in range(1, 11 if k & 1 else 12) for v in (0, 1)}
    assert sizes <= extremes, sorted(sizes - extremes)
    assert len(b["data"]) < 256 * 1024 and b["shapes"][0][1] == B.MCUS_PER_INTERVAL == b["ri"]
    assert max(int(np.abs(c[..., 0].astype(np.int64)).max()) for c in b["components"]) <= J.MAX_DC
    print("catalogue %s: %d combinations in %d MCUs, %d bytes" % (sampling, len(seen), b["shapes"][0][0] * 8,
                                                                   len(b["data"])))


@pytest.mark.parametrize("sampling", ["444", "grey"])
def test_catalogue_agrees_with_the_coder_and_the_restatement(sampling):
    b = B.catalogue(sampling)
    data, offs = J.encode(b["components"], sampling, b["ri"])
    assert data == b["data"] and list(offs) == list(b["offsets"])
    for offsets in (None, b["offsets"]):
        back, status, found, errors = U.decode(b["data"], sampling, b["shapes"], b["ri"], offsets)
        assert not status.any() and errors == 0 and found == (0 if offsets else len(status) - 1)
        assert all(np.array_equal(x, y) for x, y in zip(back, b["components"]))


def test_catalogue_as_420():
    """The 4:2:0 arrangement holds every block of the Y list, codes without a difference out of range and is
    inverted by the restatement."""
    b = B.catalogue("444")
    comps, shapes, ri = B.as_420(b)
    assert shapes[0] == (2 * shapes[1][0], 2 * shapes[1][1]) and shapes[1] == shapes[2]
    assert comps[0].size >= b["components"][0].size and len(b["components"][0].reshape(-1, 64)) % 8 == 0
    assert J.out_of_range(comps, "420", ri) == 0
    data, offs = J.encode(comps, "420", ri)
    back, status, found, errors = U.decode(data, "420", shapes, ri)
    assert not status.any() and (found, errors) == (len(offs) - 2, 0)
    assert all(np.array_equal(x, y) for x, y in zip(back, comps))
    # all four tables, every symbol (the phases are the catalogue's business)
    seen, _ = B.trace(comps, "420", ri)
    assert {(k, s) for k, s, _ in seen} == {(k, s) for k, s, _ in B.all_combinations((0, 1, 2, 3))}


# ---------------------------------------------------------------------------
# B. stuffing and the word cache
# ---------------------------------------------------------------------------
def test_stuffed_scan_places_the_pairs():
    blocks, data, offs = B.stuffed()
    n = len(offs) - 1
    assert blocks.shape[:2] == (1, n)
    chunks = [data[offs[i]:offs[i + 1] - (0 if i + 1 == n else 2)] for i in range(n)]
    assert {len(c) for c in chunks} == set(range(2, 25))            # every length, some shorter than a word
    coded = sum(len(c) for c in chunks)
    assert 4 * sum(c.count(b"\xff") for c in chunks) >= coded       # a quarter of the coded bytes
    assert all(c.count(b"\xff") == c.count(b"\xff\x00") for c in chunks)
    assert sum(c.endswith(b"\xff\x00") for c in chunks) >= 20 and sum(c.startswith(b"\xff\x00") for c in chunks) >= 20
    # a full block is 9 bytes at least, so no interval shorter than a word ends on a pair; some hold one
    assert any(len(c) < 8 and c.startswith(b"\xff\x00") for c in chunks)
    assert any(len(c) < 16 and c.endswith(b"\xff\x00") for c in chunks)
    every, first, last = B.pair_phases(data, offs)
    assert every == {(a, w) for a in range(8) for w in range(8)}    # w = 7: the FF ends a word, its 00 starts one
    assert first == set(range(8)) and last == set(range(8))
    back, status, found, errors = U.decode(data, "grey", [(1, n)], 1)
    assert not status.any() and (found, errors) == (n - 1, 0) and np.array_equal(back[0], blocks)
    assert J.decode(data, "grey", [(1, n)], 1)[0].tolist() == blocks.tolist()


# ---------------------------------------------------------------------------
# C. the colour corpus
# ---------------------------------------------------------------------------
def test_colour_corpus_reaches_every_status_at_every_position():
    cases, results = unscan_corpus.cases_and_expected()
    by_name = {c["name"]: (c, r) for c, r in zip(cases, results)}
    assert len(by_name) == len(cases)
    for sampling, nbytes in (("420", 1254), ("444", 1295)):
        comps, data, offs = unscan_corpus.base_colour(sampling)
        shapes, ri = unscan_corpus.COLOUR[sampling]
        bpm = 6 if sampling == "420" else 3
        assert len(data) == nbytes
        for name, found in (("clean located", len(offs) - 2), ("clean offsets", 0)):
            _, (blocks, status, got, errors) = by_name["%s %s" % (sampling, name)]
            assert not status.any() and (got, errors) == (found, 0)
            assert all(np.array_equal(x, y) for x, y in zip(blocks, comps))
        own = [(c, r) for c, r in zip(cases, results) if c["name"].startswith(sampling + " ")]
        assert all(c["sampling"] == sampling and c["shapes"] == shapes and c["ri"] == ri for c, _ in own)
        flips = [c for c, _ in own if " flip " in c["name"] and "offsets" not in c["name"]]
        assert len(flips) == -(-8 * nbytes // unscan_corpus.FLIP_EVERY)
        assert sum(1 for c, _ in own if " truncated to " in c["name"] and "offsets" not in c["name"]) == nbytes
        where = {}
        for _, (_, status, _, _) in own:
            for st in status.tolist():
                where.setdefault(st & 255, set()).add((st >> 8) % bpm)
        assert set(where) == {0, 1, 2, 3, 4, 5, 7, 8}, sorted(where)
        for code in (U.MARKER, U.END, U.CODE, U.INDEX):             # the failing block at every position of the MCU
            assert where[code] == set(range(bpm)), (sampling, U.NAMES[code], sorted(where[code]))
        # a failure inside an MCU leaves blocks of the same MCU decoded and the rest zero: the zero fill starts there
        assert any(st >> 8 and (st >> 8) % bpm for _, r in own for st in r[1].tolist())


def test_colour_dc_cases():
    cases, results = unscan_corpus.cases_and_expected()
    by_name = {c["name"]: r for c, r in zip(cases, results)}
    want = {"dc overflow in cb": (16 * 3 + 1, 1), "dc overflow in cr": (16 * 3 + 2, 2),
            "dc overflow in y at position 3": (4 * 6 + 3, 0)}
    for name, (block, comp) in want.items():
        blocks, status, _, _ = by_name[name]
        assert status.tolist() == [U.DC + 256 * block]
        top = [int(np.abs(b[..., 0].astype(np.int64)).max()) for b in blocks]
        assert top[comp] == 16 * 2047 and all(t <= 17 for i, t in enumerate(top) if i != comp), top
    for name, value, others in (("dc reaches 32767", 32767, "max"), ("dc reaches -32768", -32768, "min")):
        blocks, status, _, _ = by_name[name]
        assert status.tolist() == [0]
        assert [int(getattr(b[..., 0], others)()) for b in blocks] == [value] * 3
        assert all(int(b.reshape(-1, 64)[16, 0]) == value for b in blocks)     # each in its 17th block


def test_next_byte_cases():
    """The scan ends FF and the byte after it would make a marker of that: the expectation does not see it."""
    cases, results = unscan_corpus.cases_and_expected()
    named = [(c, r) for c, r in zip(cases, results) if "after" in c]
    assert {c["after"] for c, _ in named} == set(range(0xd0, 0xd8))
    assert {c["sampling"] for c, _ in named} == {"grey", "420", "444"}
    for c, (_, status, found, _) in named:
        assert c["data"][-1] == 0xff
        assert found == (0 if c["offsets"] is not None else len(U.markers(c["data"])))
        assert len(U.markers(c["data"] + bytes([c["after"]]))) == len(U.markers(c["data"])) + 1
        assert status[-1] != 0                                      # END or TAIL, never clean


# ---------------------------------------------------------------------------
# D. the marker search
# ---------------------------------------------------------------------------
def test_marker_cases_lie_on_the_edges_of_the_search():
    b = B.catalogue("grey")
    shapes, data, offs = B.grey_single(b)
    intervals = shapes[0][0] * shapes[0][1]
    assert intervals > 1000 and len(offs) == intervals + 1 and len(data) > 2 * B.CHUNK + 64
    cases = B.marker_cases(b)
    at = {name: (d, p) for name, d, p in cases}
    assert len(at) == len(cases) == 16
    positions = sorted({p for name, d, p in cases if name.startswith("marker at")})
    assert positions == [63, 191, 4094, 4095, 4096, 8191, len(data) - 2]
    assert 63 % 64 == 63 and 191 % 64 == 63 and 191 // 64 > 0     # lane 63 of a step: its number is the next step's
    assert 4095 % B.CHUNK == B.CHUNK - 1 and 8191 % B.CHUNK == B.CHUNK - 1 and 8191 // B.CHUNK > 0
    for name, d, p in cases:
        if not name.startswith("marker at"):
            continue
        mk = U.markers(d)
        assert len(d) == len(data) and p in mk
        j = mk.index(p)
        judged = j + 1 < intervals                                  # the marker after the last interval is not
        assert judged == (p != len(data) - 2)
        right = (d[p + 1] & 7) == j % 8
        assert right == name.endswith("its number")
        _, _, found, errors = U.decode(d, "grey", shapes, 1)
        clean_errors = sum(1 for i, q in enumerate(mk[:intervals - 1]) if q != p and (d[q + 1] & 7) != i % 8)
        assert errors == clean_errors + (1 if judged and not right else 0) and found == len(mk)
    # the numbers judged across a chunk's end: FF in byte 4095 or 8191, the number in the next chunk, once wrong
    assert sum(1 for name, d, p in cases if p % B.CHUNK == B.CHUNK - 1 and name.endswith("wrong number")) == 2
    d, p = at["ff at bytes - 1"]
    assert p == len(d) - 1 and d[p] == 0xff and p not in U.markers(d)
    d, _ = at["3000 markers first"]
    mk = U.markers(d)
    assert mk[:3000] == list(range(0, 6000, 2)) and len(mk) == 3000 + intervals - 1
    assert sum(1 for q in mk if q < B.CHUNK) == B.CHUNK // 2         # a chunk of nothing but markers
    assert intervals - 1 < 3000                                     # every stored marker is one of these
    _, status, found, errors = U.decode(d, "grey", shapes, 1)
    assert found == len(mk) and status.all() and errors > 0


def test_far_markers_lie_in_the_second_turn():
    zeros, blocks, data = B.far_markers()
    mk = U.markers(data)
    total = zeros + len(data)
    assert len(mk) == 10
    first = zeros + mk[0]
    assert first == B.LOCATE_WAVES * B.CHUNK - 1                    # FF ends chunk 32767, the number starts 32768
    assert all((zeros + p) // B.CHUNK == B.LOCATE_WAVES for p in mk[1:])   # one chunk beyond the waves
    chunks = -(-total // B.CHUNK)
    assert chunks == B.LOCATE_WAVES + 1 > 4 * 8192 and -(-chunks // 1024) == 33
    want, status, found, errors = B.far_expected(zeros, data)
    assert status[0] != 0 and not status[1:].any() and (found, errors) == (10, 0)
    assert np.array_equal(want[0].reshape(-1, 64)[2:], blocks.reshape(-1, 64)[2:])
    # the slices stand for the whole: on a scan short enough to decode whole, both ways agree
    small, sstatus, sfound, serrors = U.decode(bytes(100) + data, "grey", unscan_corpus.GREY_SHAPES,
                                               unscan_corpus.GREY_RI)
    part = B.far_expected(100, data)
    assert np.array_equal(small[0], part[0][0]) and np.array_equal(sstatus, part[1]) and (sfound, serrors) == part[2:]
    assert np.array_equal(part[0][0], want[0]) and np.array_equal(part[1], status)   # the zeros' count does not matter
