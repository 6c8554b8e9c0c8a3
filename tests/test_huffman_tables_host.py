"""Host tests of the caller's Huffman tables: hpdct_huffman_optimal
and hpdct_huffman_prepare against their plain-Python restatement in
tests/jpeg_tables.py, the header and the parser with tables, and the refusals
of the new device calls (fake pointers: nothing is launched).
"""
import ctypes
import os

import numpy as np
import pytest

import host_programs
import jpeg_scan as J
import jpeg_tables as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPT = ["pillow_opt_grey_rows.jpg", "pillow_opt_420_blocks3.jpg", "pillow_opt_444_norestart.jpg"]


def _read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _pairs(tables):
    return [(list(map(int, b)), list(map(int, v))) for b, v in tables]


def _same(hp, counts):
    bits, vals = hp.huffman_optimal(counts)
    want = T.optimal(counts)
    assert (list(map(int, bits)), list(map(int, vals))) == want
    return want


# ---------------------------------------------------------------------------
# hpdct_huffman_optimal
# ---------------------------------------------------------------------------
def test_optimal_equals_restatement(hp):
    rng = np.random.default_rng(20)
    for trial in range(150):
        c = rng.integers(0, 1 << int(rng.integers(1, 39)), 256) * (rng.random(256) < rng.random())
        if trial % 3 == 0:
            c = np.minimum(c, 3)            # many ties
        bits, vals = _same(hp, c)
        assert T.defect((bits, vals), 1) is None and sorted(vals) == np.flatnonzero(c).tolist()
        assert T.kraft(bits) <= 65535       # the all-ones code is nobody's
    assert _same(hp, np.zeros(256, np.int64)) == ([0] * 16, [])
    one = np.zeros(256, np.int64)
    one[200] = 9
    assert _same(hp, one) == ([1] + [0] * 15, [200])
    assert _same(hp, np.ones(256, np.int64))[0] == [0] * 7 + [255, 1] + [0] * 7
    with pytest.raises(hp.HpdctError):
        hp.huffman_optimal(np.zeros(255))
    L = hp.load_library()
    buf = (ctypes.c_uint8 * 2048)()
    assert L.hpdct_huffman_optimal(None, buf) == 1 and L.hpdct_huffman_optimal(buf, None) == 1
    big = np.zeros(256, np.uint64)
    big[3], big[9] = 1 << 54, 5
    assert [list(map(int, x)) for x in hp.huffman_optimal(big)] == list(T.optimal(big.tolist()))
    big[3] += 1                     # a count above 2^54 is refused
    with pytest.raises(hp.HpdctError) as e:
        hp.huffman_optimal(big)
    assert e.value.status == 1 and "2^54" in str(e.value)


def test_optimal_fibonacci_is_limited_to_16_bits(hp):
    """F(1..40): the unadjusted tree is 39 deep (every merge takes the running sum and the next count), beyond
    the 32 that T.81's own figures assume."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    c = np.zeros(256, np.int64)
    c[10:50] = fib
    adjusted = []
    T.optimal(c, adjusted)
    bits, vals = _same(hp, c)
    assert adjusted == [True] and sum(bits) == 40 and len(bits) == 16
    assert T.kraft(bits) <= 65535 and T.defect((bits, vals), 1) is None
    # the rarest symbols have the longest codes
    assert vals[-1] in (10, 11) and vals[0] in (48, 49)


def _fixture_counts(hp, name):
    data = _read(name)
    lay = hp.jpeg_parse_tables(data)
    sampling = "grey" if lay["components"] == 1 else lay["subsampling"]
    f = 16 if sampling == "420" else 8
    my, mx = -(-lay["height"] // f), -(-lay["width"] // f)
    shapes = [(my * f // 8, mx * f // 8)] + ([(my, mx)] * 2 if lay["components"] == 3 else [])
    scan = data[lay["scan_offset"]:lay["scan_offset"] + lay["scan_bytes"]]
    tables = _pairs(lay["tables"])
    blocks, status, found, errors = T.decode(scan, sampling, shapes, lay["restart_interval"], tables)
    assert not status.any() and errors == 0
    return lay, sampling, shapes, scan, tables, blocks


@pytest.mark.parametrize("name", OPT)
def test_optimal_is_no_worse_than_the_files_own_tables(hp, name):
    lay, sampling, shapes, scan, tables, blocks = _fixture_counts(hp, name)
    assert tables == T.norm(T.file_tables(_read(name))[0])
    # the restatement's coder gives the file's scan back under the file's tables
    again, _, oor = T.encode(blocks, sampling, lay["restart_interval"], tables)
    assert again == scan and oor == 0
    counts = T.histogram(blocks, sampling, lay["restart_interval"])
    for kind in range(4 if lay["components"] == 3 else 2):
        adjusted = []
        T.optimal(counts[kind], adjusted)
        mine = _same(hp, counts[kind])
        assert T.cost(counts[kind], mine) <= T.cost(counts[kind], tables[kind])
        if adjusted == [False]:
            annex = T.cost(counts[kind], J.TABLES[kind])
            assert annex is None or T.cost(counts[kind], mine) <= annex


# ---------------------------------------------------------------------------
# hpdct_huffman_prepare
# ---------------------------------------------------------------------------
def test_prepare_accepts_and_refuses(hp):
    L = hp.load_library()
    nbytes = int(L.hpdct_huffman_blob_bytes())
    assert nbytes == 2 * 256 * 4 + 2 * 16 * 4 + 4 * (256 * 2 + 18 * 4 + 18 * 4 + 256)
    for name in OPT:
        assert hp.huffman_prepare(hp.jpeg_parse_tables(_read(name))["tables"]).size == nbytes
    blob = hp.huffman_prepare(T.BUILT)
    assert not hp.huffman_prepare([None] * 4)[:4 * 544].any()          # four empty tables are legal: no code
    # the coder's part: (length << 16) | code at [symbol], AC luma, AC chroma, DC luma, DC chroma
    words = blob[:4 * 544].view(np.uint32)
    codes = J.codes_of(T.BUILT_AC)
    assert all(int(words[s]) == (ln << 16 | code) for s, (code, ln) in codes.items())
    dcodes = J.codes_of(T.BUILT_DC)
    assert all(int(words[512 + s]) == (ln << 16 | code) for s, (code, ln) in dcodes.items())
    assert int(words[512 + 11]) == (16 << 16) | 0xfffe and int(words[0x0a]) >> 16 == 16
    annex = hp.huffman_prepare([hp.huffman_table(k) for k in range(4)])
    assert int(annex[:4].view(np.uint32)[0]) == (4 << 16) | 0b1010           # EOB of the AC luminance table

    good = T.norm(J.TABLES)

    def refused(kind, table, nvals=None):
        assert T.defect(table, kind, nvals) is not None
        specs = hp._huffman_specs([table if k == kind else good[k] for k in range(4)])
        if nvals is not None:
            specs[kind].nvals = nvals
        buf = np.zeros(nbytes, np.uint8)
        assert L.hpdct_huffman_prepare(ctypes.addressof(specs), buf.ctypes.data, nbytes) == 1
        assert not buf.any()
        return L.hpdct_last_error_string().decode()

    names = ["DC luma", "AC luma", "DC chroma", "AC chroma"]
    for kind in range(4):
        bits, vals = good[kind]
        msg = refused(kind, (bits, vals), nvals=len(vals) - 1)
        assert names[kind] in msg and "not the sum of bits" in msg
        assert "above 256" in refused(kind, (bits, vals), nvals=257)
        assert "not the sum of bits" in refused(kind, (bits, vals), nvals=-1)
        assert "not the sum of bits" in refused(kind, (bits[:15] + [bits[15] + 1], vals))
        over = list(bits)
        over[0] = 3                                                  # three codes of one bit
        spare = [v for v in range(16 if kind % 2 == 0 else 256) if v not in vals][:3]
        assert "over-subscribed" in refused(kind, (over, spare + vals))
        assert "appears twice" in refused(kind, (bits, vals[:-1] + [vals[0]]))
    for kind in (0, 2):
        bits, vals = good[kind]
        assert "DC symbol is above 15" in refused(kind, (bits, vals[:-1] + [16]))
    assert "over-subscribed" in refused(1, ([2, 1] + [0] * 14, [1, 2, 3]))
    buf = np.zeros(nbytes, np.uint8)
    specs = hp._huffman_specs(good)
    assert L.hpdct_huffman_prepare(ctypes.addressof(specs), buf.ctypes.data, nbytes - 1) == 1
    assert L.hpdct_huffman_prepare(None, buf.ctypes.data, nbytes) == 1
    assert L.hpdct_huffman_prepare(ctypes.addressof(specs), None, nbytes) == 1
    assert L.hpdct_huffman_prepare(ctypes.addressof(specs), buf.ctypes.data, nbytes) == 0
    assert ctypes.sizeof(hp._HuffmanSpec) == 276


# ---------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------
def test_header_with_tables_round_trips(hp):
    tail = bytes([0x12, 0x34]) + b"\xff\xd9"
    for comps, sub in ((1, "444"), (3, "420"), (3, "444")):
        kw = dict(components=comps, subsampling=sub, restart_interval=5)
        plain = hp.jpeg_header(45, 77, **kw)
        assert hp.jpeg_header(45, 77, tables=None, **kw) == plain
        assert hp.jpeg_header(45, 77, tables=[hp.huffman_table(k) for k in range(4)], **kw) == plain
        lay = hp.jpeg_parse_tables(plain + tail)
        assert _pairs(lay["tables"]) == T.norm(J.TABLES[:2 * (2 if comps == 3 else 1)] + [None] * (2 if comps == 1 else 0))
        fib = np.zeros(256, np.int64)
        fib[:5] = [1, 1, 2, 3, 5]
        small = [hp.huffman_optimal(fib), hp.huffman_optimal(np.arange(256) % 7), T.BUILT_DC, T.BUILT_AC]
        for tables in (T.BUILT, small):
            head = hp.jpeg_header(45, 77, tables=tables, **kw)
            lay = hp.jpeg_parse_tables(head + tail)
            want = T.norm(tables)
            if comps == 1:
                want[2:] = [T.EMPTY, T.EMPTY]
            assert _pairs(lay["tables"]) == want
            assert (lay["height"], lay["width"], lay["components"], lay["restart_interval"]) == (45, 77, comps, 5)
            assert lay["scan_bytes"] == 2 and head[lay["scan_offset"] - 1:lay["scan_offset"]] == b"\x00"
            with pytest.raises(hp.HpdctError) as e:
                hp.jpeg_parse(head + tail)
            assert e.value.status == 2 and "Huffman" in str(e.value)
    with pytest.raises(hp.HpdctError) as e:
        hp.jpeg_header(8, 8, components=1, tables=[([1] + [0] * 15, [16]), None, None, None])
    assert e.value.status == 1 and "DC symbol is above 15" in str(e.value)


def _segments(data):
    out, i = {}, 2
    while data[i + 1] != 0xda:
        out.setdefault(data[i + 1], i)
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    out[0xda] = i
    return out


def test_parse_tables_refusals(hp):
    """test_parse_refusals of test_jpeg_unscan_host.py through hpdct_jpeg_parse_tables: the same verdicts, except
    that a table other than Annex K's is judged as hpdct_huffman_prepare judges it."""
    SCAN = bytes([0x12, 0x34, 0xff, 0x00, 0x56])
    head = bytearray(hp.jpeg_header(45, 77, components=3, subsampling="420", restart_interval=5))
    seg = _segments(head)
    sof, dqt, dht, sos = seg[0xc0], seg[0xdb], seg[0xc4], seg[0xda]

    def status(h=head, tail=SCAN + b"\xff\xd9", patch=()):
        h = bytearray(h)
        for at, value in patch:
            h[at] = value
        with pytest.raises(hp.HpdctError) as e:
            hp.jpeg_parse_tables(bytes(h) + tail)
        return e.value.status, str(e.value)

    assert hp.jpeg_parse_tables(bytes(head) + SCAN + b"\xff\xd9")["components"] == 3
    unsupported = {
        "SOF0": [(sof + 1, 0xc2)],
        "8 only": [(sof + 4, 12)],
        "16-bit DQT": [(dqt + 4, 0x10)],
        "components": [(sof + 9, 4)],
        "sampling": [(sof + 11, 0x21)],
        "Ss / Se": [(sos + 4 + 1 + 6 + 1, 62)],
    }
    for text, patch in unsupported.items():
        st, msg = status(patch=patch)
        assert st == 2 and text in msg, (text, st, msg)
    # a symbol of the DC luminance table: another table now.  7 is there already
    st, msg = status(patch=[(dht + 5 + 16 + 3, 7)])
    assert st == 1 and "appears twice" in msg and "component 0" in msg
    h = bytearray(head)
    h[dht + 5 + 16 + 3] = 13                                            # 0 1 2 13 4 ...: a legal table
    lay = hp.jpeg_parse_tables(bytes(h) + SCAN + b"\xff\xd9")
    assert list(lay["tables"][0][1]) == [0, 1, 2, 13] + list(range(4, 12))
    st, msg = status(patch=[(dht + 5 + 16 + 3, 16)])
    assert st == 1 and "DC symbol is above 15" in msg
    st, msg = status(patch=[(dht + 5 + 1, 4)])                          # four codes of two bits and five of three
    assert st == 1                                                      # (the segment's length no longer fits)
    # Cb and Cr on different Huffman tables: a fifth table, DC destination 2, selected by Cr
    extra = bytes([0xff, 0xc4, 0, 2 + 17 + 2, 0x02, 0, 2] + [0] * 14 + [0, 1])
    h5 = bytearray(head[:2] + extra + head[2:])
    at = len(extra) + sos + 4 + 1 + 2 * 2 + 1                           # Cr's table selectors
    st, msg = status(h=h5, patch=[(at, 0x21)])
    assert st == 2 and "Cb and Cr on different Huffman tables" in msg
    same = bytes([0xff, 0xc4, 0, 2 + 17 + 12, 0x02]) + bytes(J.DC_CHROMA[0]) + bytes(J.DC_CHROMA[1])
    h6 = bytearray(head[:2] + same + head[2:])
    h6[len(same) + sos + 4 + 1 + 2 * 2 + 1] = 0x21
    assert hp.jpeg_parse_tables(bytes(h6) + SCAN + b"\xff\xd9")["components"] == 3    # equal contents are accepted
    st, msg = status(patch=[(sos + 4 + 1 + 1, 0x30)])                   # Y selects a DC table nobody defined
    assert st == 1 and "missing" in msg
    st, msg = status(tail=SCAN + bytes(head[sos:]) + SCAN + b"\xff\xd9")
    assert st == 2 and "more than one scan" in msg
    whole = bytes(head) + SCAN + b"\xff\xd9"
    for bad in (b"", b"\xff", b"\xff\xd8", whole[1:], whole[:-2], whole[:-1], whole[:len(head) - 3], whole[:sof + 6],
                bytes(head) + SCAN, b"\x00" * 700):
        with pytest.raises(hp.HpdctError) as e:
            hp.jpeg_parse_tables(bad)
        assert e.value.status == 1, (len(bad), str(e.value))
    L = hp.load_library()
    lay = (ctypes.c_uint8 * 2048)()
    assert L.hpdct_jpeg_parse_tables(None, 10, lay, lay) == 1 and L.hpdct_jpeg_parse_tables(lay, 10, None, lay) == 1
    assert L.hpdct_jpeg_parse_tables(lay, 10, lay, None) == 1
    assert ctypes.sizeof(hp._JpegLayout) == 560


@pytest.mark.parametrize("name", OPT)
def test_jpeg_parse_still_refuses_optimised_files(hp, name):
    with pytest.raises(hp.HpdctError) as e:
        hp.jpeg_parse(_read(name))
    assert e.value.status == 2 and "Huffman table differs from the Annex K" in str(e.value)
    assert len(_read(name)) == {"pillow_opt_grey_rows.jpg": 524, "pillow_opt_420_blocks3.jpg": 696,
                                "pillow_opt_444_norestart.jpg": 457}[name]


# ---------------------------------------------------------------------------
# argument validation (fake pointers, never dereferenced)
# ---------------------------------------------------------------------------
Y, CB, CR, SC, INFO, OFFS, WS, ST, TAB, CNT = (1 << n for n in range(30, 40))


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def _msg(L):
    return L.hpdct_last_error_string().decode()


def test_histogram_arguments_rejected(hp):
    L = hp.load_library()

    def call(y=Y, cb=CB, cr=CR, h=16, w=32, sub=1, ri=0, flags=0, counts=CNT):
        return L.hpdct_scan_histogram(_p(y), _p(cb), _p(cr), h, w, sub, ri, flags, _p(counts), None)

    assert call(y=None) == 1 and "null" in _msg(L)
    assert call(counts=None) == 1 and "null" in _msg(L)
    assert call(cr=None) == 1 and "null" in _msg(L)
    assert call(h=24) == 1 and "multiples of 16" in _msg(L)
    assert call(h=0) == 1 and call(sub=2) == 1 and "subsampling" in _msg(L)
    assert call(ri=-1) == 1 and call(ri=65536) == 1 and "restart_interval" in _msg(L)
    assert call(flags=0x80) == 2
    assert call(y=Y + 8) == 1 and "aligned" in _msg(L)
    assert call(counts=CNT + 8) == 1 and "aligned" in _msg(L)
    assert call(counts=Y + 512) == 1 and "overlap" in _msg(L)
    assert call(counts=CB - 8192 + 16) == 1 and "overlap" in _msg(L)
    assert call(cb=Y + 1008) == 1 and "overlap" in _msg(L)


def test_encode_and_decode_tables_arguments_rejected(hp):
    L = hp.load_library()

    def enc(y=Y, cb=CB, cr=CR, h=16, w=32, sub=1, ri=0, flags=0, scan=SC, cap=4096, info=INFO, offs=OFFS, ws=WS,
            wsb=0, tab=TAB):
        return L.hpdct_encode_scan_tables(_p(y), _p(cb), _p(cr), h, w, sub, ri, flags, _p(scan), cap, _p(info),
                                          _p(offs), _p(ws), wsb, _p(tab), None)

    def dec(scan=SC, nbytes=4096, offs=OFFS, y=Y, cb=CB, cr=CR, h=16, w=32, sub=1, ri=0, flags=0, info=INFO, st=ST,
            ws=WS, wsb=0, tab=TAB):
        return L.hpdct_decode_scan_tables(_p(scan), nbytes, _p(offs), _p(y), _p(cb), _p(cr), h, w, sub, ri, flags,
                                          _p(info), _p(st), _p(ws), wsb, _p(tab), None)

    end = "workspace too small"         # the last thing judged before the tables: a call that is otherwise fine
    def split(wsb=0, **kw):
        a = dict(scan=SC, nbytes=4096, offs=OFFS, y=Y, cb=CB, cr=CR, h=16, w=32, sub=1, ri=0, flags=0, info=INFO, st=ST,
                 ws=WS, tab=TAB, min_bytes=1)
        a.update(kw)
        return L.hpdct_decode_scan_split_tables(_p(a["scan"]), a["nbytes"], _p(a["offs"]), _p(a["y"]), _p(a["cb"]),
                                                _p(a["cr"]), a["h"], a["w"], a["sub"], a["ri"], a["flags"],
                                                a["min_bytes"], _p(a["info"]), _p(a["st"]), _p(a["ws"]), wsb,
                                                _p(a["tab"]), None)

    assert split(min_bytes=-1) == 1 and "split_min_bytes" in _msg(L)
    assert split(min_bytes=-1, tab=None) == 1 and "split_min_bytes" in _msg(L)
    for call in (enc, dec, split):
        assert call() == 1 and end in _msg(L)
        assert call(tab=None) == 1 and end in _msg(L)
        assert call(y=None) == 1 and "null" in _msg(L)
        assert call(h=24) == 1 and "multiples of 16" in _msg(L)
        assert call(ri=65536) == 1 and "restart_interval" in _msg(L)
        assert call(flags=0x80) == 2
        assert call(info=INFO + 4) == 1 and "aligned" in _msg(L)
        assert call(cb=Y + 1008) == 1 and "overlap" in _msg(L)
        # the tables are judged once everything else holds (a workspace of the right size)
        assert call(wsb=1 << 20, tab=TAB + 8) == 1 and "d_tables must be 16-byte aligned" in _msg(L)
        assert call(wsb=1 << 20, tab=INFO - 16) == 1 and "info and tables buffers overlap" in _msg(L)
        assert call(wsb=1 << 20, tab=WS) == 1 and "workspace and tables buffers overlap" in _msg(L)
    assert enc(wsb=1 << 20, tab=SC + 4080) == 1 and "scan and tables buffers overlap" in _msg(L)
    assert dec(wsb=1 << 20, tab=Y + 1008) == 1 and "y and tables buffers overlap" in _msg(L)
    assert L.hpdct_scan_bound_tables(1, 1) == 421 and L.hpdct_scan_bound_tables(65, 1) == 417 * 65 + 4
    assert L.hpdct_scan_bound_tables(-1, 0) == -1 and L.hpdct_scan_bound_tables(1 << 62, 1) == -1
    assert L.hpdct_scan_bound(65, 1) == 415 * 65 + 4
    assert hp.scan_bound_tables(130, 2) == 417 * 130 + 8


# ---------------------------------------------------------------------------
# the stand-alone program under ASan + UBSan
# ---------------------------------------------------------------------------
def test_huffman_host_code_under_sanitizers(tmp_path):
    host_programs.sanitised_check("asan_huffman_check", tmp_path, "hpdct_scan.o")
