"""hpdct_decode_scan on the GPU, everything compared exactly (blocks, status
array, info) with tests/jpeg_unscan.py, the plain-Python restatement of the
header's rules, or with the blocks hpdct_encode_scan coded:

- small frames of every sampling, restart interval, block order, offsets given
  and located; interval counts around a wave's 64 lanes; every row of the policy
  table and a frame beyond the grid cap;
- the corrupt corpus of test_jpeg_unscan_host.py, grey and colour (which the
  sanitizer program has walked on the CPU), each scan inside a larger buffer of
  0x00, of 0xFF and of 0xD0 bytes, the outputs inside sentinel-filled tensors;
- three Pillow-written files; jpeg_decode(jpeg_encode(frame));
- bound launches on a side stream with reused buffers; a graph capture.
"""
import numpy as np
import pytest

import jpeg_scan as J
import jpeg_unscan as U
import unscan_corpus
from test_jpeg_unscan_host import FIXTURES, fixture_layout, frame_blocks

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scan_dev(data, dev):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(dev)


def _natural(blocks):
    out = np.zeros_like(blocks)
    out[..., J.ZIGZAG] = blocks
    return out


def _check(hp, dev, data, sampling, shapes, ri, offsets, order="zigzag"):
    """One decode_scan call against the restatement: blocks, status and info."""
    want, status, found, errors = U.decode(data, sampling, shapes, ri, offsets)
    h, w = 8 * shapes[0][0], 8 * shapes[0][1]
    offs = None if offsets is None else _dev(np.asarray(offsets, np.uint64).view(np.int64), dev)
    got, info, st = hp.decode_scan(_scan_dev(data, dev), height=h, width=w, components=len(shapes),
                                   subsampling="444" if sampling == "grey" else sampling, restart_interval=ri,
                                   offsets=offs, order=order)
    assert info == {"bad_intervals": int((status != 0).sum()), "markers_found": found, "marker_errors": errors}
    assert np.array_equal(st.cpu().numpy().view(np.uint64), status)
    for g, x in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), _natural(x) if order == "natural" else x)


@pytest.mark.parametrize("sampling", ["grey", "444", "420"])
def test_small_frames_match_the_restatement(hp, dev, sampling):
    """Grey 24 x 56, 4:4:4 16 x 40, 4:2:0 32 x 48 (21, 10 and 6 MCUs): every interval length (some leave a shorter
    last interval), both block orders, offsets given and located."""
    comps, shapes = frame_blocks(sampling, 21)
    nmcu = shapes[-1][0] * shapes[-1][1]
    assert sum(1 for ri in (2, 5, 7) if nmcu % ri != 0) >= 1
    for ri in (0, 1, 2, 5, 7, nmcu):
        data, offs = J.encode(comps, sampling, ri)
        for order in ("zigzag", "natural"):
            for offsets in (None, offs):
                _check(hp, dev, data, sampling, shapes, ri, offsets, order)


@pytest.mark.parametrize("intervals", [63, 64, 65, 129])
def test_interval_counts_around_a_wave(hp, dev, intervals):
    """Grey, 8 rows, one block per interval: the counts cross a wave's 64 lanes and the marker number wraps."""
    shapes = [(1, intervals)]
    blocks = unscan_corpus.sparse_blocks(shapes[0], intervals)
    data, offs = J.encode([blocks], "grey", 1)
    _check(hp, dev, data, "grey", shapes, 1, None)
    _check(hp, dev, data, "grey", shapes, 1, offs, "natural")


def _device_blocks(dev, ty, tx, seed):
    """Sparse int16 blocks in baseline's range, made on the device."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    b = torch.randint(-30, 31, (ty, tx, 64), generator=g, device=dev, dtype=torch.int16)
    keep = torch.rand((ty, tx, 64), generator=g, device=dev) < 0.12
    b = b * keep
    b[..., 0] = torch.randint(-400, 401, (ty, tx), generator=g, device=dev, dtype=torch.int16)
    return b.contiguous()


# lanes per wave the policy gives these interval counts (tests/tools/policy_unscan_check.cpp pins the rows):
# 1,024 -> 1; 9,000 -> 4; 65,536 (a 2048^2 frame) -> 16; 262,144 -> 64; 1,050,625 -> 64, past the grid cap of
# 8,192 workgroups: the decode kernel's stride loop takes a second turn
@pytest.mark.parametrize("ty,tx", [(8, 128), (1, 9000), (256, 256), (512, 512), (1025, 1025)])
def test_policy_rows_round_trip(hp, dev, ty, tx):
    """decode(encode(blocks)) == blocks, one block per interval, the offsets given and the markers located."""
    import torch
    blocks = _device_blocks(dev, ty, tx, ty + tx)
    scan, info, offs = hp.encode_scan(blocks, height=8 * ty, width=8 * tx, restart_interval=1)
    assert info["truncated"] == 0 and info["out_of_range"] == 0
    for located in (False, True):
        (got,), dinfo, status = hp.decode_scan(scan, height=8 * ty, width=8 * tx, restart_interval=1,
                                               offsets=None if located else offs)
        assert dinfo == {"bad_intervals": 0, "markers_found": ty * tx - 1 if located else 0, "marker_errors": 0}
        assert not bool(status.any())
        assert torch.equal(got, blocks)
        del got, status


def test_whole_rows_per_interval_colour(hp, dev):
    """A 4:2:0 512 x 1024 frame at one MCU row per interval and at ri = 0, against the coder."""
    import torch
    y, cb, cr = _device_blocks(dev, 64, 128, 1), _device_blocks(dev, 32, 64, 2), _device_blocks(dev, 32, 64, 3)
    for ri in (64, 0):
        scan, info, offs = hp.encode_scan(y, cb, cr, height=512, width=1024, restart_interval=ri)
        for offsets in (None, offs):
            got, dinfo, status = hp.decode_scan(scan, height=512, width=1024, components=3, restart_interval=ri,
                                                offsets=offsets, order="zigzag")
            assert dinfo["bad_intervals"] == 0 and not bool(status.any())
            assert all(torch.equal(a, b) for a, b in zip(got, (y, cb, cr)))


# ---------------------------------------------------------------------------
# the corrupt corpus
# ---------------------------------------------------------------------------
def test_corrupt_corpus(hp, dev):
    """Every case of the corpus, grey, 4:2:0 and 4:4:4, each scan a slice of one large buffer whose other bytes are
    0x00 in one run, 0xFF in another and 0xD0 in a third (a case may name the byte right after its scan): the
    results are those of the restatement every time, so a read outside the scan shows as a difference -- the
    marker search reading scan[bytes] makes a marker of a final FF in the 0xD0 run.  The block arrays (y, cb, cr
    one after the other), status arrays and infos are slices of sentinel-filled tensors; the sentinels between
    them survive.  All calls of a run are queued, then read back at once."""
    import ctypes
    import time
    import torch
    cases, results = unscan_corpus.cases_and_expected()
    L = hp.load_library()
    n = len(cases)
    pad = 24                                            # bytes around each scan; odd offsets: no alignment rule
    starts, total = [], 7
    for c in cases:
        starts.append(total)
        total += len(c["data"]) + pad + (len(c["data"]) & 1)
    nblk = max(sum(int(np.prod(s)) for s in c["shapes"]) for c in cases)
    nint = max(len(r[1]) for r in results)
    assert {c["sampling"] for c in cases} == {"grey", "420", "444"}
    bstride, sstride = 64 * nblk + 64, (nint + 3) // 2 * 2     # a sentinel block and >= 1 sentinel word between
    offs_all = np.zeros((n, (nint + 3) // 2 * 2), np.uint64)      # rows of a 16-byte multiple
    for i, c in enumerate(cases):
        if c["offsets"] is not None:
            offs_all[i, :len(c["offsets"])] = np.asarray(c["offsets"], np.uint64)
    offs_dev = _dev(offs_all.view(np.int64), dev)
    ws_bytes = max(hp.decode_workspace_bytes(8 * c["shapes"][0][0], 8 * c["shapes"][0][1], components=len(c["shapes"]),
                                             subsampling="420" if c["sampling"] == "420" else "444",
                                             restart_interval=c["ri"], scan_bytes=len(c["data"])) for c in cases)
    # a call is a chain of small launches that wait for one another: four streams, each with a workspace of its own,
    # take the cases in turn so that the chains overlap
    side = [torch.cuda.Stream(device=dev) for _ in range(4)]
    ws = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev) for _ in side]
    vp = ctypes.c_void_p
    for fill in (0x00, 0xff, 0xd0):
        t0 = time.perf_counter()
        host = np.full(total, fill, np.uint8)
        for c, s in zip(cases, starts):
            host[s:s + len(c["data"])] = np.frombuffer(c["data"], np.uint8)
            if "after" in c:
                host[s + len(c["data"])] = c["after"]
        buf = _dev(host, dev)
        blocks = torch.full((n, bstride), SENTINEL, dtype=torch.int16, device=dev)
        status = torch.full((n, sstride), -1, dtype=torch.int64, device=dev)
        info = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
        p_buf, p_offs, p_blk, p_info, p_st = (t.data_ptr() for t in (buf, offs_dev, blocks, info, status))
        torch.cuda.synchronize()                        # the buffers are filled before a side stream reads them
        for i, (c, s) in enumerate(zip(cases, starts)):
            ty, tx = c["shapes"][0]
            p_y = p_blk + 2 * bstride * i
            p_cb = p_cr = None
            if len(c["shapes"]) == 3:                   # cb and cr right behind y: 128-byte multiples
                ny, nc = 64 * ty * tx, 64 * int(np.prod(c["shapes"][1]))
                p_cb, p_cr = vp(p_y + 2 * ny), vp(p_y + 2 * (ny + nc))
            st = L.hpdct_decode_scan(vp(p_buf + s), len(c["data"]),
                                     None if c["offsets"] is None else vp(p_offs + 8 * offs_all.shape[1] * i),
                                     vp(p_y), p_cb, p_cr, 8 * ty, 8 * tx, 1 if c["sampling"] == "420" else 0, c["ri"],
                                     0, vp(p_info + 16 * i), vp(p_st + 8 * sstride * i), vp(ws[i % 4].data_ptr()),
                                     ws_bytes, vp(side[i % 4].cuda_stream))
            assert st == 0, (c["name"], L.hpdct_last_error_string())
        torch.cuda.synchronize()
        got_b, got_s = blocks.cpu().numpy(), status.cpu().numpy().view(np.uint64)
        got_i = info.cpu().numpy().view(np.uint32).reshape(n, 4)
        wrong = []
        for i, (c, (want, wstatus, found, errors)) in enumerate(zip(cases, results)):
            flat = np.concatenate([x.reshape(-1) for x in want])
            k, m = flat.size, len(wstatus)
            ok = (np.array_equal(got_b[i, :k], flat) and np.array_equal(got_s[i, :m], wstatus) and
                  got_i[i].tolist() == [int((wstatus != 0).sum()), found, errors, 0])
            ok = ok and bool((got_b[i, k:] == SENTINEL).all()) and bool((got_s[i, m:] == np.uint64(2 ** 64 - 1)).all())
            if not ok:
                wrong.append(c["name"])
        assert not wrong, (hex(fill), len(wrong), wrong[:10])
        assert np.array_equal(buf.cpu().numpy(), host)
        print("corpus, surroundings %#04x: %d cases in %.2f s" % (fill, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_pillow_files(hp, dev, name):
    """The blocks of a Pillow-written file equal the restatement's; jpeg_decode gives a frame of the file's size."""
    data, lay, sampling, shapes, scan, (hpad, wpad) = fixture_layout(hp, name)
    want, status, found, errors = U.decode(scan, sampling, shapes, lay["restart_interval"])
    got, info, st = hp.decode_scan(_scan_dev(scan, dev), height=hpad, width=wpad, components=lay["components"],
                                   subsampling=lay["subsampling"], restart_interval=lay["restart_interval"])
    assert info == {"bad_intervals": 0, "markers_found": found, "marker_errors": 0} and not bool(st.any())
    for g, x in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), x)
    if lay["components"] == 3:
        img = hp.jpeg_decode(data, device=dev)
        assert tuple(img.shape) == (lay["height"], lay["width"], 3)
        want_img = hp.inverse_rgb_frame(*got, height=lay["height"], width=lay["width"], subsampling=lay["subsampling"],
                                        q_luma=lay["q_luma"], q_chroma=lay["q_chroma"])
        assert bool((img == want_img).all())
    else:
        with pytest.raises(hp.HpdctError, match="set_quant_table"):
            hp.jpeg_decode(data, device=dev)            # quality 60 is not the library table
        hp.set_quant_table(lay["q_luma"])
        try:
            img = hp.jpeg_decode(data, device=dev)
            assert tuple(img.shape) == (43, 61)
            import torch
            assert torch.equal(img, hp.inverse_blocks(got[0], out_dtype=torch.uint8)[:43, :61])
        finally:
            hp.set_quant_table(None)


@pytest.mark.parametrize("sampling", ["420", "444", "grey"])
def test_jpeg_decode_inverts_jpeg_encode(hp, oracle, dev, sampling):
    """jpeg_decode(jpeg_encode(frame)) is the library's own inverse of its own forward, bit for bit."""
    import torch
    if sampling == "grey":
        img = _dev(oracle.rand_u8(24 * 56, 9).reshape(24, 56), dev)
        want = hp.inverse_blocks(hp.forward_blocks(img), out_dtype=torch.uint8)
        data = hp.jpeg_encode(img)
    else:
        img = _dev(oracle.rand_u8(45 * 70 * 3, 9).reshape(45, 70, 3), dev)
        want = hp.inverse_rgb_frame(*hp.forward_rgb_frame(img, subsampling=sampling), height=45, width=70,
                                    subsampling=sampling)
        data = hp.jpeg_encode(img, subsampling=sampling)
    got = hp.jpeg_decode(data, device=dev)
    assert got.shape == want.shape and torch.equal(got, want)
    # a damaged file is reported, not decoded
    lay = hp.jpeg_parse(data)
    scan = data[lay["scan_offset"]:lay["scan_offset"] + lay["scan_bytes"]]
    at = lay["scan_offset"] + U.markers(scan)[-1]       # the last restart marker, cut out: an interval goes missing
    with pytest.raises(hp.HpdctError, match="damaged restart intervals"):
        hp.jpeg_decode(data[:at] + data[at + 2:], device=dev)


# ---------------------------------------------------------------------------
# bound launches: a side stream, reused buffers, a graph
# ---------------------------------------------------------------------------
def _bound_buffers(hp, dev, shapes, ri, scan_bytes):
    import torch
    ty, tx = shapes[0]
    intervals = 1 if ri == 0 else -(-ty * tx // ri)
    y = torch.full((ty, tx, 64), SENTINEL, dtype=torch.int16, device=dev)
    info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    status = torch.full((intervals,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(hp.decode_workspace_bytes(8 * ty, 8 * tx, restart_interval=ri, scan_bytes=scan_bytes),
                     dtype=torch.uint8, device=dev)
    return y, info, status, ws


def test_bound_launch_on_a_side_stream_with_reused_buffers(hp, dev):
    import torch
    shapes, ri = [(3, 7)], 2
    side = torch.cuda.Stream(device=dev)
    first = unscan_corpus.sparse_blocks(shapes[0], 31)
    second = unscan_corpus.sparse_blocks(shapes[0], 32)
    d1, o1 = J.encode([first], "grey", ri)
    d2, _ = J.encode([second], "grey", ri)
    n = max(len(d1), len(d2))
    y, info, status, ws = _bound_buffers(hp, dev, shapes, ri, n)
    s1, s2 = _scan_dev(d1, dev), _scan_dev(d2, dev)
    offs = _dev(np.asarray(o1, np.int64), dev)
    torch.cuda.synchronize()
    c1 = hp.bind_decode_scan(s1, offs, y, None, None, info, status, ws, restart_interval=ri, stream=side)
    c2 = hp.bind_decode_scan(s2, None, y, None, None, info, status, ws, restart_interval=ri, stream=side)
    for call, want, found in ((c1, first, 0), (c2, second, 10), (c1, first, 0)):
        call()
        side.synchronize()
        assert hp.decode_info(info) == {"bad_intervals": 0, "markers_found": found, "marker_errors": 0}
        assert not bool(status.any()) and np.array_equal(y.cpu().numpy(), want)


def test_graph_capture_and_replay(hp, dev):
    """One bind_decode_scan launch (the markers located: four kernels, one chain, no allocation) captured in a
    graph and replayed once gives the same bytes."""
    import torch
    shapes, ri = [(3, 7)], 2
    blocks = unscan_corpus.sparse_blocks(shapes[0], 41)
    data, _ = J.encode([blocks], "grey", ri)
    y, info, status, ws = _bound_buffers(hp, dev, shapes, ri, len(data))
    scan = _scan_dev(data, dev)
    hp.bind_decode_scan(scan, None, y, None, None, info, status, ws, restart_interval=ri)()
    torch.cuda.synchronize()                        # the kernels are loaded before the capture
    direct = (y.cpu().numpy().copy(), status.cpu().numpy().copy(), info.cpu().numpy().copy())
    assert np.array_equal(direct[0], blocks)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            hp.bind_decode_scan(scan, None, y, None, None, info, status, ws, restart_interval=ri)()
    torch.cuda.synchronize()
    y.fill_(SENTINEL)
    status.fill_(-1)
    info.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), direct[0]) and np.array_equal(status.cpu().numpy(), direct[1])
    assert np.array_equal(info.cpu().numpy(), direct[2])
