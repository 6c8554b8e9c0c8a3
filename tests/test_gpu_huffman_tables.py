"""GPU tests of the caller's Huffman tables: hpdct_scan_histogram,
hpdct_encode_scan_tables and hpdct_decode_scan_tables, exactly against their
plain-Python restatement in tests/jpeg_tables.py; the optimised files of another
writer (tests/golden/pillow_opt_*.jpg) and of jpeg_encode(optimize=True); the
decoders' lane dispatch at interval counts on both sides of its thresholds.
"""
import io
import os
import time

import numpy as np
import pytest

import jpeg_scan as J
import jpeg_tables as T
import unscan_corpus

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPT = ["pillow_opt_grey_rows.jpg", "pillow_opt_420_blocks3.jpg", "pillow_opt_444_norestart.jpg"]
_memo = {}


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _natural(zz):
    nat = np.zeros_like(zz)
    nat[..., J.ZIGZAG] = zz
    return nat


def _blob(hp, dev, tables):
    return _dev(hp.huffman_prepare(tables), dev)


def _geometry(comps, sampling):
    return 8 * comps[0].shape[0], 8 * comps[0].shape[1], "444" if sampling == "grey" else sampling


def _fixture(hp, name):
    """(file, layout, sampling, shapes, scan, tables, the restatement's blocks) of an optimised fixture, once."""
    if name not in _memo:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data = f.read()
        lay = hp.jpeg_parse_tables(data)
        sampling = "grey" if lay["components"] == 1 else lay["subsampling"]
        f = 16 if sampling == "420" else 8
        my, mx = -(-lay["height"] // f), -(-lay["width"] // f)
        shapes = [(my * f // 8, mx * f // 8)] + ([(my, mx)] * 2 if lay["components"] == 3 else [])
        scan = data[lay["scan_offset"]:lay["scan_offset"] + lay["scan_bytes"]]
        tables = [(list(map(int, b)), list(map(int, v))) for b, v in lay["tables"]]
        blocks, status, found, _ = T.decode(scan, sampling, shapes, lay["restart_interval"], tables)
        assert not status.any()
        _memo[name] = (data, lay, sampling, shapes, scan, tables, blocks, found)
    return _memo[name]


# ---------------------------------------------------------------------------
# hpdct_scan_histogram
# ---------------------------------------------------------------------------
def _check_hist(hp, dev, comps, sampling, intervals):
    h, w, sub = _geometry(comps, sampling)
    for order in ("zigzag", "natural"):
        arrays = [_dev(c if order == "zigzag" else _natural(c), dev) for c in comps]
        for ri in intervals:
            got = hp.scan_histogram(*arrays, height=h, width=w, subsampling=sub, restart_interval=ri, order=order)
            want = T.histogram(comps, sampling, ri)
            assert got.shape == (4, 256) and np.array_equal(got.cpu().numpy(), want), (order, ri)


@pytest.mark.parametrize("shape", [(3, 7), (1, 130)], ids=["24x56", "8x1040"])
def test_histogram_grey(hp, dev, shape):
    """8 x 1040: 130 blocks in one interval, more than one 64-block step of the coder, one workgroup here."""
    _check_hist(hp, dev, [unscan_corpus.sparse_blocks(shape, 5)], "grey", [0, 1, 3, shape[1]])


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_histogram_colour_frame(hp, oracle, dev, sampling):
    img = _dev(oracle.rand_u8(45 * 70 * 3, 11).reshape(45, 70, 3), dev)
    comps = [c.cpu().numpy() for c in hp.forward_rgb_frame(img, subsampling=sampling)]
    _check_hist(hp, dev, comps, sampling, [0, 1, 3, comps[1].shape[1]])


def test_histogram_clamp_edges_and_runs(hp, dev):
    """DC differences of +-2047 / +-2048, AC values of +-1023 / +-1024 (the clamps to categories 11 and 10), runs of
    15, 16, 17, 31 and 32 zeros, coefficient 63 non-zero (no EOB), the all-zero block."""
    b = np.zeros((2, 12, 64), np.int16)
    for i, dc in enumerate([2047, 0, -2048, 0, 2048, 1, -2047, -4095, 32767, -32768, 0, 0]):
        b[0, i, 0] = dc
    for i, v in enumerate([1023, -1023, 1024, -1024, 32767, -32768]):
        b[1, i, 1] = v
        b[1, i, 63] = 1 if i % 2 else 0
    for i, run in enumerate([15, 16, 17, 31, 32]):
        b[1, 6 + i, 1 + run] = 3
        b[0, i, 2 + run] = -1
        b[0, i, 63] = 7 * (i % 2)
    _check_hist(hp, dev, [b], "grey", [0, 1, 5, 12])
    counts = T.histogram([b], "grey", 0)
    assert counts[0, 11] >= 8 and counts[1, 0xf0] >= 6 and counts[1, 0x0a] >= 6 and counts[1, 0] < 24


def test_histogram_several_workgroups(hp, dev):
    """381 grey blocks (two workgroups of 256 lanes) and 6 x 46 MCUs of 4:2:0 (1,656 blocks, seven workgroups)."""
    _check_hist(hp, dev, [unscan_corpus.sparse_blocks((3, 127), 6)], "grey", [0, 127])
    comps = [unscan_corpus.sparse_blocks(s, 7 + i) for i, s in enumerate([(12, 92), (6, 46), (6, 46)])]
    _check_hist(hp, dev, comps, "420", [0, 46])


# ---------------------------------------------------------------------------
# hpdct_encode_scan_tables
# ---------------------------------------------------------------------------
def _check_encode(hp, dev, comps, sampling, ri, tables, order="zigzag"):
    want, want_offs, want_oor = T.encode(comps, sampling, ri, tables)
    h, w, sub = _geometry(comps, sampling)
    arrays = [_dev(c if order == "zigzag" else _natural(c), dev) for c in comps]
    scan, info, offs = hp.encode_scan(*arrays, height=h, width=w, subsampling=sub, restart_interval=ri, order=order,
                                      tables=_blob(hp, dev, tables))
    blocks = sum(c.shape[0] * c.shape[1] for c in comps)
    assert info["bytes"] <= hp.scan_bound_tables(blocks, len(want_offs) - 1) and info["truncated"] == 0
    assert info["out_of_range"] == want_oor
    if want is not None:
        assert info["bytes"] == len(want) and scan.cpu().numpy().tobytes() == want
        assert offs.cpu().numpy().tolist() == want_offs
    return info


@pytest.mark.parametrize("name", OPT)
def test_encode_under_a_files_tables(hp, dev, name):
    """The restatement's blocks of an optimised file, coded under the file's tables, are the file's scan again."""
    data, lay, sampling, shapes, scan, tables, blocks, _ = _fixture(hp, name)
    assert T.encode(blocks, sampling, lay["restart_interval"], tables)[0] == scan
    for order in ("zigzag", "natural"):
        _check_encode(hp, dev, blocks, sampling, lay["restart_interval"], tables, order)
    _check_encode(hp, dev, blocks, sampling, 0, tables)


@pytest.mark.parametrize("sampling", ["grey", "420", "444"])
def test_encode_under_the_built_tables(hp, dev, sampling):
    shapes = {"grey": [(3, 27)], "420": [(4, 6), (2, 3), (2, 3)], "444": [(2, 5)] * 3}[sampling]
    comps = [unscan_corpus.sparse_blocks(s, 60 + i) for i, s in enumerate(shapes)]
    for ri in (0, 1, 4):
        for order in ("zigzag", "natural"):
            info = _check_encode(hp, dev, comps, sampling, ri, T.BUILT, order)
            assert info["out_of_range"] == 0


def test_encode_counts_symbols_without_a_code(hp, dev):
    """Blocks that need symbols a file's small tables lack, and the empty tables: every such symbol is counted."""
    comps = [unscan_corpus.sparse_blocks((3, 27), 61)]
    tables = _fixture(hp, OPT[0])[5]
    info = _check_encode(hp, dev, comps, "grey", 5, tables)
    assert info["out_of_range"] > 0
    info = _check_encode(hp, dev, comps, "grey", 5, [None] * 4)
    assert info["out_of_range"] == int(T.histogram(comps, "grey", 5).sum())
    # a coefficient beyond the categories is counted too, and coded with its low bits as hpdct_encode_scan codes it
    b = comps[0].copy()
    b[0, 0, 5] = 2000
    want = T.encode([b], "grey", 0, T.BUILT)
    assert want[2] == 1
    _check_encode(hp, dev, [b], "grey", 0, T.BUILT)


def test_tables_none_is_annex_k(hp, dev):
    comps = [unscan_corpus.sparse_blocks(s, 70 + i) for i, s in enumerate([(4, 6), (2, 3), (2, 3)])]
    arrays = [_dev(c, dev) for c in comps]
    want, want_offs = J.encode(comps, "420", 2)
    annex = _blob(hp, dev, [hp.huffman_table(k) for k in range(4)])
    for tables in (None, annex):
        scan, info, offs = hp.encode_scan(*arrays, height=32, width=48, subsampling="420", restart_interval=2,
                                          tables=tables)
        assert info == {"bytes": len(want), "truncated": 0, "out_of_range": 0}
        assert scan.cpu().numpy().tobytes() == want and offs.cpu().numpy().tolist() == want_offs
        got, dinfo, st = hp.decode_scan(scan, height=32, width=48, components=3, subsampling="420", restart_interval=2,
                                        tables=tables)
        assert dinfo["bad_intervals"] == 0 and all(np.array_equal(g.cpu().numpy(), c) for g, c in zip(got, comps))


@pytest.mark.parametrize("ones", [False, True])
def test_encode_at_the_buffers_limit(hp, dev, ones):
    """65 blocks in one interval, each of 1665 bits under the built tables: a 16-bit DC code with category 11 and
    63 times a 16-bit AC code with category 10.  ones: every AC extra bit 1 (+1023) and the DC differences
    +2047 / -2047 in turn (a DC cannot rise by 2047 for 65 blocks); else mixed signs."""
    rng = np.random.default_rng(3)
    b = np.zeros((1, 65, 64), np.int16)
    mag = rng.integers(512, 1024, (65, 63))
    b[0, :, 1:] = 1023 if ones else mag * rng.choice([-1, 1], (65, 63))
    b[0, :, 0] = [2047 * (i % 2 == 0) for i in range(65)] if ones else [1500 - 2000 * (i % 2) for i in range(65)]
    want, offs, oor = T.encode([b], "grey", 0, T.BUILT)
    assert oor == 0 and (len(want) - want.count(b"\xff\x00")) * 8 >= 65 * 1665 > (len(want) - want.count(b"\xff\x00") - 1) * 8
    info = _check_encode(hp, dev, [b], "grey", 0, T.BUILT)
    assert info["bytes"] <= hp.scan_bound_tables(65, 1) == 417 * 65 + 4
    print("65 blocks of 1665 bits, ones=%s: %d bytes, bound %d" % (ones, info["bytes"], hp.scan_bound_tables(65, 1)))


# ---------------------------------------------------------------------------
# hpdct_decode_scan_tables
# ---------------------------------------------------------------------------
def _check_decode(hp, dev, scan, sampling, shapes, ri, tables, blob, offsets=None):
    want, status, found, errors = T.decode(scan, sampling, shapes, ri, tables, offsets)
    h, w = 8 * shapes[0][0], 8 * shapes[0][1]
    offs = None if offsets is None else _dev(np.asarray(offsets, np.int64), dev)
    dscan = _dev(np.frombuffer(bytes(scan), np.uint8), dev)
    want_info = {"bad_intervals": int((status != 0).sum()), "markers_found": found, "marker_errors": errors}
    ok = True
    # the serial decoder, and the split one with every interval that has a byte split: bit for bit the same
    for method in ("serial", "split"):
        got, info, st = hp.decode_scan(dscan, height=h, width=w, components=len(shapes),
                                       subsampling="444" if sampling == "grey" else sampling, restart_interval=ri,
                                       offsets=offs, tables=blob, method=method, split_min_bytes=1)
        ok = ok and {k: info[k] for k in want_info} == want_info
        ok = ok and np.array_equal(st.cpu().numpy().astype(np.uint64), status)
        ok = ok and all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got, want))
        if method == "split":
            _memo["split"] = _memo.get("split", 0) + info["split_intervals"]
    return ok


@pytest.mark.parametrize("name", OPT)
def test_decode_optimised_files(hp, dev, name):
    data, lay, sampling, shapes, scan, tables, blocks, found = _fixture(hp, name)
    blob = _blob(hp, dev, tables)
    before = _memo.get("split", 0)
    assert _check_decode(hp, dev, scan, sampling, shapes, lay["restart_interval"], tables, blob)
    assert _memo["split"] > before          # the split walker did decode intervals of the file


def _catalogue():
    """A grey scan, one row of 32 blocks per interval, written symbol by symbol under the built tables until every
    code of both tables has begun at each of the 8 bit positions of a byte: (scan, shapes, ri, blocks written).
    A block is a DC symbol (the sign of its difference keeps the predictor inside int16), one AC symbol with its
    extra bits, and an EOB unless that symbol ended the block."""
    if "catalogue" in _memo:
        return _memo["catalogue"]
    rng = np.random.default_rng(8)
    dc, ac = J.codes_of(T.BUILT_DC), J.codes_of(T.BUILT_AC)
    need = {(0, s, p) for s in dc for p in range(8)} | {(1, s, p) for s in ac for p in range(8)}
    data, rows, per = bytearray(), 0, 32
    while need or rows < 8:
        w, pred = J._Bits(), 0
        for _ in range(per):
            n = int(rng.integers(0, 16))
            s = int(rng.integers(0, 256))
            want = [k for k in need if k[2] == w.n]
            if want:
                pick = want[int(rng.integers(0, len(want)))]
                n, s = (pick[1], s) if pick[0] == 0 else (n, s)
            need.discard((0, n, w.n))
            w.put(*dc[n])
            if n:
                m = int(rng.integers(1 << (n - 1), 1 << n))
                d = -m if pred > 0 else m
                pred += d
                w.put(d if d > 0 else d + (1 << n) - 1, n)
            pend = [k for k in need if k[0] == 1 and k[2] == w.n]
            if pend:
                s = pend[int(rng.integers(0, len(pend)))][1]
            need.discard((1, s, w.n))
            w.put(*ac[s])
            size = s & 15
            if size:
                w.put(int(rng.integers(0, 1 << size)), size)
            if size or s == 0xf0:
                need.discard((1, 0x00, w.n))
                w.put(*ac[0x00])
        rows += 1
        if rows > 1:
            data += bytes([0xff, 0xd0 + ((rows - 2) & 7)])
        data += w.finish()
        assert rows < 400
    _memo["catalogue"] = (bytes(data), [(rows, per)], per)
    return _memo["catalogue"]


def test_decode_every_code_of_the_built_tables_at_every_phase(hp, dev):
    scan, shapes, ri = _catalogue()
    want, status, found, errors = T.decode(scan, "grey", shapes, ri, T.BUILT)
    assert not status.any() and found == shapes[0][0] - 1 and errors == 0
    assert int(np.abs(want[0][..., 1:]).max()) > 16383          # sizes up to 15 were there
    blob = _blob(hp, dev, T.BUILT)
    before = _memo.get("split", 0)
    assert _check_decode(hp, dev, scan, "grey", shapes, ri, T.BUILT, blob)
    assert _memo["split"] > before          # the catalogue went through the split walker too
    print("catalogue: %d blocks, %d bytes" % (shapes[0][0] * shapes[0][1], len(scan)))


def test_decode_corrupt_corpus(hp, dev):
    """Bit flips, truncations and marker edits of the first four catalogue intervals (128 blocks) and of the three
    optimised files' scans, under their own tables, under the wrong tables and under the empty ones."""
    t0 = time.perf_counter()
    rng = np.random.default_rng(9)
    cat, cshapes, cri = _catalogue()
    cut = [p for p in range(len(cat) - 1) if cat[p] == 0xff and 0xd0 <= cat[p + 1] <= 0xd7][3]
    bases = [(cat[:cut], "grey", [(4, 32)], cri, T.BUILT)]
    for name in OPT:
        _, lay, sampling, shapes, scan, tables, _, _ = _fixture(hp, name)
        bases.append((scan, sampling, shapes, lay["restart_interval"], tables))
    cases = wrong = 0
    for scan, sampling, shapes, ri, tables in bases:
        blob = _blob(hp, dev, tables)
        variants = [scan]
        for _ in range(24):
            d = bytearray(scan)
            d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
            variants.append(bytes(d))
        variants += [scan[:int(n)] for n in rng.integers(0, len(scan), 8)]
        for v in (0x00, 0xff, 0xd0, 0xd9):
            d = bytearray(scan)
            d[int(rng.integers(0, len(d)))] = v
            variants.append(bytes(d))
        marks = [p for p in range(len(scan) - 1) if scan[p] == 0xff and 0xd0 <= scan[p + 1] <= 0xd7]
        if marks:
            p = marks[len(marks) // 2]
            variants += [scan[:p] + scan[p + 2:], scan[:p + 1] + bytes([scan[p + 1] ^ 1]) + scan[p + 2:]]
        for v in variants:
            cases += 1
            wrong += not _check_decode(hp, dev, v, sampling, shapes, ri, tables, blob)
        for other in (T.BUILT, [None] * 4):
            if other is not tables:
                cases += 1
                wrong += not _check_decode(hp, dev, scan, sampling, shapes, ri, other, _blob(hp, dev, other))
    print("corrupt corpus under the caller's tables: %d cases in %.2f s" % (cases, time.perf_counter() - t0))
    assert cases >= 150 and wrong == 0


# ---------------------------------------------------------------------------
# the lane dispatch of the serial decoder and of the split decoder's serial launch
# ---------------------------------------------------------------------------
def _encode_unsuffixed(hp, y, h, w, capacity):
    """hpdct_encode_scan itself on grey blocks with restart_interval 1, past the binding (which calls
    hpdct_encode_scan_tables with NULL tables): the scan's bytes."""
    import ctypes
    import torch
    lib, vp = hp.load_library(), ctypes.c_void_p
    ws_bytes = int(lib.hpdct_scan_workspace_bytes(h, w, 1, hp.SUBSAMPLINGS["444"], 1))
    assert ws_bytes > 0
    scan = torch.empty(capacity, dtype=torch.uint8, device=y.device)
    info = torch.empty(2, dtype=torch.int64, device=y.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
    st = lib.hpdct_encode_scan(vp(y.data_ptr()), None, None, h, w, hp.SUBSAMPLINGS["444"], 1, 0, vp(scan.data_ptr()),
                               capacity, vp(info.data_ptr()), None, vp(ws.data_ptr()), ws_bytes,
                               vp(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.hpdct_last_error_string()
    res = hp.scan_info(info)
    assert res["truncated"] == 0
    return scan[:res["bytes"]]


@pytest.mark.parametrize("lanes,h,w", [(1, 8, 512), (4, 8, 65544), (16, 16, 65544), (64, 2048, 2056)],
                         ids=["1-lane", "4-lanes", "16-lanes", "64-lanes"])
def test_lane_dispatch_round_trip(hp, dev, lanes, h, w):
    """Grey frames of one 8x8 block per restart interval, their interval counts (64, 8,193, 16,386, 65,792) on both
    sides of the policy's thresholds (8,192, 16,384, 65,536), so that each of the 1 / 4 / 16 / 64-lane decode kernels
    is the one launched: a kernel picked with the wrong stride leaves intervals undecoded or decodes them twice.
    Seeded blocks, every coefficient within +-1023, three AC positions a block.  encode_scan, then decode_scan and
    decode_scan_split with a split_min_bytes no interval reaches (every interval goes to its serial launch), under
    Annex K's tables (tables=None) and under the optimal tables of the frame's own histogram."""
    import torch
    n = (h // 8) * (w // 8)
    want_lanes = 1 if n <= 8192 else 4 if n <= 16384 else 16 if n <= 65536 else 64
    assert want_lanes == lanes                      # hpdct_policy.hpp's unscan_lanes, restated
    rng = np.random.default_rng(1400 + lanes)
    b = np.zeros((n, 64), np.int16)
    b[:, 0] = rng.integers(-1023, 1024, n)
    np.put_along_axis(b, rng.integers(1, 64, (n, 3)), rng.integers(-1023, 1024, (n, 3)).astype(np.int16), 1)
    y = _dev(b.reshape(h // 8, w // 8, 64), dev)
    counts = hp.scan_histogram(y, restart_interval=1).cpu().numpy()
    optimal = _blob(hp, dev, [hp.huffman_optimal(counts[0]), hp.huffman_optimal(counts[1]), None, None])
    for tables in (None, optimal):
        scan, info, offs = hp.encode_scan(y, restart_interval=1, tables=tables)
        assert info["truncated"] == 0 and info["out_of_range"] == 0
        if tables is None:
            assert torch.equal(scan, _encode_unsuffixed(hp, y, h, w, scan.numel() + 16))
        for method in ("serial", "split"):
            (got,), dinfo, status = hp.decode_scan(scan, height=h, width=w, components=1, restart_interval=1,
                                                   offsets=offs, tables=tables, method=method,
                                                   split_min_bytes=1 << 40)
            assert torch.equal(got, y), (method, tables is not None)
            assert not bool(status.any()) and dinfo["bad_intervals"] == 0
            if method == "split":
                assert dinfo["serial_intervals"] == n and dinfo["split_intervals"] == 0


# ---------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPT)
def test_jpeg_decode_reads_optimised_files(hp, dev, name):
    """A file with Huffman tables of its own (Pillow, optimize=True): refused before this existed."""
    import torch
    data, lay, sampling, shapes, scan, tables, blocks, _ = _fixture(hp, name)
    dblocks = [_dev(b, dev) for b in blocks]
    if lay["components"] == 3:
        img = hp.jpeg_decode(data, device=dev)
        want = hp.inverse_rgb_frame(*dblocks, height=lay["height"], width=lay["width"], subsampling=lay["subsampling"],
                                    q_luma=lay["q_luma"], q_chroma=lay["q_chroma"])
    else:
        hp.set_quant_table(lay["q_luma"])
        try:
            img = hp.jpeg_decode(data, device=dev)
            want = hp.inverse_blocks(dblocks[0], out_dtype=torch.uint8)[:lay["height"], :lay["width"]]
        finally:
            hp.set_quant_table(None)
    assert img.shape == want.shape and torch.equal(img, want)
    if lay["components"] == 3:
        for method in ("serial", "split"):
            assert torch.equal(hp.jpeg_decode(data, device=dev, method=method), want)


def _smooth(h, w, ch):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p = [40 + 150 * xx / w + 50 * yy / h + 25 * np.sin(xx / (3.0 + c) + yy / 5.0) for c in range(ch)]
    a = np.clip(np.rint(np.stack(p, -1)), 0, 255).astype(np.uint8)
    return a[..., 0] if ch == 1 else a


@pytest.mark.parametrize("sampling", ["grey", "420", "444"])
def test_jpeg_encode_optimize_round_trip(hp, oracle, dev, sampling):
    """jpeg_decode(jpeg_encode(x, optimize=True)) is the library's own inverse of its own forward; the file is no
    longer than the plain one, and Pillow opens it at its true size."""
    import torch
    for kind in ("noise", "smooth"):
        if sampling == "grey":
            a = oracle.rand_u8(24 * 56, 9).reshape(24, 56) if kind == "noise" else _smooth(24, 56, 1)
            img = _dev(a, dev)
            fwd = (hp.forward_blocks(img),)
            want = hp.inverse_blocks(fwd[0], out_dtype=torch.uint8)
            kw = {}
        else:
            a = oracle.rand_u8(45 * 70 * 3, 9).reshape(45, 70, 3) if kind == "noise" else _smooth(45, 70, 3)
            img = _dev(a, dev)
            fwd = hp.forward_rgb_frame(img, subsampling=sampling)
            want = hp.inverse_rgb_frame(*fwd, height=45, width=70, subsampling=sampling)
            kw = dict(subsampling=sampling)
        plain, data = hp.jpeg_encode(img, **kw), hp.jpeg_encode(img, optimize=True, **kw)
        assert hp.jpeg_encode(img, optimize=False, **kw) == plain
        # verified on the restatement first: the optimal tables cost no more bits than Annex K's for these inputs
        comps = [c.cpu().numpy() for c in fwd]
        lay = hp.jpeg_parse_tables(data)
        counts = T.histogram(comps, sampling, lay["restart_interval"])
        for k in range(2 if sampling == "grey" else 4):
            assert T.cost(counts[k], lay["tables"][k]) <= T.cost(counts[k], J.TABLES[k])
            assert [list(map(int, x)) for x in lay["tables"][k]] == list(T.optimal(counts[k]))
        want_scan = T.encode(comps, sampling, lay["restart_interval"], lay["tables"])[0]
        assert data[lay["scan_offset"]:lay["scan_offset"] + lay["scan_bytes"]] == want_scan
        print("%s %s: %d bytes optimised, %d plain" % (sampling, kind, len(data), len(plain)))
        assert len(data) <= len(plain)
        got = hp.jpeg_decode(data, device=dev)
        assert got.shape == want.shape and torch.equal(got, want)
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == ((56, 24) if sampling == "grey" else (70, 45))


def test_histogram_and_encode_chain_in_a_graph(hp, dev):
    """bind_scan_histogram and bind_scan(tables=) captured into one graph and replayed: the same counts and bytes."""
    import torch
    comps = [unscan_corpus.sparse_blocks((3, 27), 80)]
    y = _dev(comps[0], dev)
    ri = 27
    blob = _blob(hp, dev, T.BUILT)
    counts = torch.empty((4, 256), dtype=torch.int64, device=dev)
    scan = torch.zeros(hp.scan_bound_tables(81, 3), dtype=torch.uint8, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    offs = torch.empty(4, dtype=torch.int64, device=dev)
    ws = torch.empty(64, dtype=torch.uint8, device=dev)

    def chain():
        hp.bind_scan_histogram(y, None, None, counts, restart_interval=ri)()
        hp.bind_scan(y, None, None, scan, info, offs, ws, restart_interval=ri, tables=blob)()

    chain()
    torch.cuda.synchronize()                        # the kernels are loaded before the capture
    want, want_offs, _ = T.encode(comps, "grey", ri, T.BUILT)
    direct = (counts.cpu().numpy().copy(), scan.cpu().numpy().copy(), info.cpu().numpy().copy())
    assert np.array_equal(direct[0], T.histogram(comps, "grey", ri)) and direct[1][:len(want)].tobytes() == want
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            chain()
    torch.cuda.synchronize()
    counts.fill_(-1)
    scan.fill_(0)
    info.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), direct[0]) and np.array_equal(scan.cpu().numpy(), direct[1])
    assert np.array_equal(info.cpu().numpy(), direct[2]) and offs.cpu().numpy().tolist() == want_offs
