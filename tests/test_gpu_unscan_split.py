"""hpdct_decode_scan_split on the GPU, everything compared exactly: the blocks,
the status array and all eight words of the info with tests/jpeg_unscan_split.py,
the plain-Python restatement (which test_unscan_split_host.py holds against
jpeg_unscan.decode), or beyond 64 KiB with hpdct_decode_scan on the same bytes.
The segment, the group and the rounds come from hpdct_decode_split_geometry.

- the small frames of test_gpu_unscan.py at every shape, every interval split
  and with the library's threshold, outputs and workspace inside sentinels;
- the corrupt corpus and the built scans, every interval split, inside buffers
  of 00, FF and D0 bytes: each condition of the serial pass is reached;
- interval lengths at the limits of a segment, a group and the rounds: under the
  header's bound nothing is left to the serial walker;
- one feature at each byte offset around a segment boundary; a block that covers
  a segment;
- scans that settle slowly and one that never does; overlapping offsets;
- reused buffers on a side stream, a graph capture, jpeg_decode's methods.
"""
import ctypes

import numpy as np
import pytest

import jpeg_scan as J
import jpeg_unscan as U
import jpeg_unscan_split as S
import unscan_corpus
import unscan_split_inputs as I
from test_jpeg_unscan_host import FIXTURES, fixture_layout, frame_blocks
from test_unscan_split_host import COUNTERS, restated

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a
PAD = 64


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _natural(blocks):
    out = np.zeros_like(blocks)
    out[..., J.ZIGZAG] = blocks
    return out


def _sub(sampling):
    return "444" if sampling == "grey" else sampling


def _call(hp, dev, data, sampling, shapes, ri, offsets, split_min, order="zigzag", fill=0x00, after=None):
    """One hpdct_decode_scan_split call, every buffer a slice of a larger tensor: the scan at an odd offset among
    `fill` bytes, the outputs and the workspace (full of A5 bytes: the call must not count on what it holds) among
    sentinels, which must survive.  -> (components, status uint64, the info's eight words)"""
    import torch
    ty, tx = shapes[0]
    nmcu = int(np.prod(shapes[-1]))
    per = nmcu if ri == 0 else ri
    intervals = -(-nmcu // per)
    sizes = [64 * int(np.prod(s)) for s in shapes]
    host = np.full(len(data) + 2 * PAD + 1, fill, np.uint8)
    host[PAD + 1:PAD + 1 + len(data)] = np.frombuffer(bytes(data), np.uint8)
    if after is not None:
        host[PAD + 1 + len(data)] = after
    buf = _dev(host, dev)
    blocks = torch.full((sum(sizes) + PAD * (len(sizes) + 1),), SENTINEL, dtype=torch.int16, device=dev)
    starts = [PAD + sum(sizes[:i]) + PAD * i for i in range(len(sizes))]
    comps = [blocks[a:a + n].view(s + (64,)) for a, n, s in zip(starts, sizes, shapes)]
    nst = (intervals + 1) // 2 * 2
    status = torch.full((nst + 4,), -1, dtype=torch.int64, device=dev)
    info = torch.full((8,), -1, dtype=torch.int64, device=dev)
    need = hp.decode_split_workspace_bytes(8 * ty, 8 * tx, components=len(shapes), subsampling=_sub(sampling),
                                           restart_interval=ri, scan_bytes=len(data))
    ws = torch.full((need + 2 * PAD,), 0xa5, dtype=torch.uint8, device=dev)
    offs = None if offsets is None else _dev(np.asarray(offsets, np.uint64).view(np.int64), dev)
    y, cb, cr = (comps + [None, None])[:3]
    hp.bind_decode_scan_split(buf[PAD + 1:PAD + 1 + len(data)], offs, y, cb, cr, info[2:6], status[2:2 + intervals],
                              ws[PAD:PAD + need], height=8 * ty, width=8 * tx, subsampling=_sub(sampling),
                              restart_interval=ri, order=order, split_min_bytes=split_min)()
    torch.cuda.synchronize()
    hb, hs, hi, hw = blocks.cpu().numpy(), status.cpu().numpy(), info.cpu().numpy(), ws.cpu().numpy()
    mask = np.ones(hb.size, bool)
    for a, n in zip(starts, sizes):
        mask[a:a + n] = False
    assert (hb[mask] == SENTINEL).all(), "a store outside the block arrays"
    assert (hs[:2] == -1).all() and (hs[2 + intervals:] == -1).all(), "a store outside the status array"
    assert (hi[:2] == -1).all() and (hi[6:] == -1).all(), "a store outside the info"
    assert (hw[:PAD] == 0xa5).all() and (hw[PAD + need:] == 0xa5).all(), "a store outside the workspace"
    assert np.array_equal(buf.cpu().numpy(), host)
    return ([hb[a:a + n].reshape(s + (64,)) for a, n, s in zip(starts, sizes, shapes)],
            hs[2:2 + intervals].view(np.uint64), hi[2:6].view(np.uint32).tolist())


def _check(hp, dev, data, sampling, shapes, ri, offsets, split_min, order="zigzag", want=None, **kw):
    """A call against the restatement: blocks, status and all eight info words."""
    if want is None:
        want = S.decode(data, sampling, shapes, ri, offsets, split_min, hp.decode_split_geometry())
    blocks, status, found, errors, counts = want
    got, st, info = _call(hp, dev, data, sampling, shapes, ri, offsets, split_min, order, **kw)
    assert info == [int((status != 0).sum()), found, errors, 0] + [counts[k] for k in COUNTERS], (info, counts)
    assert np.array_equal(st, status)
    for g, x in zip(got, blocks):
        assert np.array_equal(g, _natural(x) if order == "natural" else x)
    return counts


def _check_case(hp, dev, c, split_min=1, **kw):
    return _check(hp, dev, c["data"], c["sampling"], c["shapes"], c["ri"], c["offsets"], split_min, **kw)


@pytest.mark.parametrize("sampling", ["grey", "444", "420"])
def test_small_frames_match_the_restatement(hp, dev, sampling):
    """The frames of test_gpu_unscan.py's test of this name: every interval length, both block orders, offsets given
    and located; with split_min_bytes = 1 (intervals of one segment take the split path) and with 0 (none does)."""
    comps, shapes = frame_blocks(sampling, 21)
    nmcu = shapes[-1][0] * shapes[-1][1]
    for ri in (0, 1, 2, 5, 7, nmcu):
        data, offs = J.encode(comps, sampling, ri)
        for order in ("zigzag", "natural"):
            for offsets in (None, offs):
                one = _check(hp, dev, data, sampling, shapes, ri, offsets, 1, order)
                zero = _check(hp, dev, data, sampling, shapes, ri, offsets, 0, order)
                intervals = len(offs) - 1
                assert one == dict(split_intervals=intervals, serial_intervals=0, unsettled_intervals=0, rounds=0)
                assert zero == dict(split_intervals=0, serial_intervals=intervals, unsettled_intervals=0, rounds=0)


def test_corrupt_corpus_and_built_scans(hp, dev):
    """Every case of the corrupt corpus, of the built scans and of the split inputs with every interval split, each
    scan a slice of one large buffer whose other bytes are 00 in one run, FF in another and D0 in a third; block
    arrays, status arrays and infos are slices of sentinel-filled tensors.  All calls of a run are queued on four
    streams, each with a workspace of its own, then read back at once.  The restatement's counters say that each of
    the serial pass's conditions is reached."""
    import time
    import torch
    cases, results, counts = restated()
    assert all(v > 0 for v in S.REASONS.values()), S.REASONS
    assert hp.decode_split_geometry() == S.GEOMETRY
    L = hp.load_library()
    n = len(cases)
    pad = 24
    starts, total = [], 7
    for c in cases:
        starts.append(total)
        total += len(c["data"]) + pad + (len(c["data"]) & 1)
    nblk = max(sum(int(np.prod(s)) for s in c["shapes"]) for c in cases)
    nint = max(len(r[1]) for r in results)
    # a sentinel block and >= 1 sentinel word between the cases; the large cases have arenas of their own
    small = [i for i, c in enumerate(cases) if sum(int(np.prod(s)) for s in c["shapes"]) <= 512]
    large = [i for i in range(n) if i not in set(small)]
    nblk = max(sum(int(np.prod(s)) for s in cases[i]["shapes"]) for i in small)
    bstride, sstride = 64 * nblk + 64, (nint + 3) // 2 * 2
    offs_all = np.zeros((n, (nint + 3) // 2 * 2), np.uint64)
    for i, c in enumerate(cases):
        if c["offsets"] is not None:
            offs_all[i, :len(c["offsets"])] = np.asarray(c["offsets"], np.uint64)
    offs_dev = _dev(offs_all.view(np.int64), dev)

    def ws_need(c):
        return hp.decode_split_workspace_bytes(8 * c["shapes"][0][0], 8 * c["shapes"][0][1],
                                               components=len(c["shapes"]), subsampling=_sub(c["sampling"]),
                                               restart_interval=c["ri"], scan_bytes=len(c["data"]))
    ws_bytes = max(ws_need(cases[i]) for i in small)
    side = [torch.cuda.Stream(device=dev) for _ in range(4)]
    ws = [torch.full((ws_bytes + 128,), 0xa5, dtype=torch.uint8, device=dev) for _ in side]
    vp = ctypes.c_void_p
    for fill in (0x00, 0xff, 0xd0):
        t0 = time.perf_counter()
        host = np.full(total, fill, np.uint8)
        for c, s in zip(cases, starts):
            host[s:s + len(c["data"])] = np.frombuffer(c["data"], np.uint8)
            if "after" in c:
                host[s + len(c["data"])] = c["after"]
        buf = _dev(host, dev)
        blocks = torch.full((len(small), bstride), SENTINEL, dtype=torch.int16, device=dev)
        status = torch.full((len(small), sstride), -1, dtype=torch.int64, device=dev)
        info = torch.full((len(small), 4), -1, dtype=torch.int64, device=dev)
        p_buf, p_offs, p_blk, p_info, p_st = (t.data_ptr() for t in (buf, offs_dev, blocks, info, status))
        torch.cuda.synchronize()
        for k, i in enumerate(small):
            c, s = cases[i], starts[i]
            ty, tx = c["shapes"][0]
            p_y = p_blk + 2 * bstride * k
            p_cb = p_cr = None
            if len(c["shapes"]) == 3:
                ny, nc = 64 * ty * tx, 64 * int(np.prod(c["shapes"][1]))
                p_cb, p_cr = vp(p_y + 2 * ny), vp(p_y + 2 * (ny + nc))
            st = L.hpdct_decode_scan_split(vp(p_buf + s), len(c["data"]),
                                           None if c["offsets"] is None else vp(p_offs + 8 * offs_all.shape[1] * i),
                                           vp(p_y), p_cb, p_cr, 8 * ty, 8 * tx, 1 if c["sampling"] == "420" else 0,
                                           c["ri"], 0, 1, vp(p_info + 32 * k), vp(p_st + 8 * sstride * k),
                                           vp(ws[k % 4].data_ptr() + 64), ws_bytes, vp(side[k % 4].cuda_stream))
            assert st == 0, (c["name"], L.hpdct_last_error_string())
        torch.cuda.synchronize()
        got_b, got_s = blocks.cpu().numpy(), status.cpu().numpy().view(np.uint64)
        got_i = info.cpu().numpy().view(np.uint32).reshape(len(small), 8)
        wrong = []
        for k, i in enumerate(small):
            c, (want, wstatus, found, errors) = cases[i], results[i]
            flat = np.concatenate([x.reshape(-1) for x in want])
            m, q = flat.size, len(wstatus)
            ok = (np.array_equal(got_b[k, :m], flat) and np.array_equal(got_s[k, :q], wstatus) and
                  got_i[k].tolist() == [int((wstatus != 0).sum()), found, errors, 0] + [counts[i][x] for x in COUNTERS])
            ok = ok and bool((got_b[k, m:] == SENTINEL).all()) and bool((got_s[k, q:] == np.uint64(2 ** 64 - 1)).all())
            if not ok:
                wrong.append((c["name"], got_i[k].tolist()))
        assert not wrong, (hex(fill), len(wrong), wrong[:10])
        for w in ws:
            h = w.cpu().numpy()
            assert (h[:64] == 0xa5).all() and (h[64 + ws_bytes:] == 0xa5).all()
        assert np.array_equal(buf.cpu().numpy(), host)
        print("corpus, surroundings %#04x: %d cases in %.2f s" % (fill, len(small), time.perf_counter() - t0))
        # the long scans, one call each
        for i in large:
            c = cases[i]
            want = results[i] + (counts[i],)
            if len(c["data"]) <= 65536 or fill == 0x00:
                _check_case(hp, dev, c, want=want, fill=fill)


def _serial_and_split(hp, dev, c, split_min=1):
    """Beyond 64 KiB: hpdct_decode_scan_split against hpdct_decode_scan on the same bytes.  -> the split info"""
    import torch
    ty, tx = c["shapes"][0]
    scan = _dev(np.frombuffer(c["data"], np.uint8).copy(), dev)
    offs = None if c["offsets"] is None else _dev(np.asarray(c["offsets"], np.uint64).view(np.int64), dev)
    kw = dict(height=8 * ty, width=8 * tx, components=len(c["shapes"]), subsampling=_sub(c["sampling"]),
              restart_interval=c["ri"], offsets=offs)
    a, ainfo, ast = hp.decode_scan(scan, **kw)
    b, binfo, bst = hp.decode_scan(scan, method="split", split_min_bytes=split_min, **kw)
    assert all(torch.equal(x, z) for x, z in zip(a, b)) and torch.equal(ast, bst)
    assert all(binfo[k] == v for k, v in ainfo.items())
    assert all(np.array_equal(x.cpu().numpy(), z) for x, z in zip(b, c["blocks"])) or bool(bst.any())
    return binfo


def test_interval_lengths_at_the_limits(hp, dev):
    """Grey, one interval of sparse blocks, lengths within a block's length of a segment, two segments, a group and
    the bound of R + 1 groups on both sides, and one just past R groups.  Up to the bound nothing is left to the
    serial walker and nothing is unsettled: the header's bound guarantees that, no tuning does.  Against the
    restatement up to 64 KiB, against hpdct_decode_scan beyond."""
    s, g, r = hp.decode_split_geometry()
    for c, bounded in I.limits(s, g, r):
        if len(c["data"]) <= 65536:
            k = _check_case(hp, dev, c)
        else:
            k = _serial_and_split(hp, dev, c)
            assert k["bad_intervals"] == 0
        assert k["split_intervals"] == 1
        if bounded:
            assert k["serial_intervals"] == 0 and k["unsettled_intervals"] == 0, (c["name"], k)
        assert len(c["data"]) < hp.SPLIT_MIN_BYTES or _serial_and_split(hp, dev, c, 0)["split_intervals"] == 1   # the threshold


def test_segment_boundaries(hp, dev):
    """An FF 00 pair, a 16-bit code, the longest extra bits, a DC symbol, an EOB, a ZRL and the interval's last byte,
    each at the byte offsets -2 .. +2 around a segment boundary; a block that covers a whole segment."""
    s, g, r = hp.decode_split_geometry()
    for c in I.boundaries(s) + ([I.whole_segment_block(s)] if s <= I.MAX_BLOCK_BYTES else []):
        for order in ("zigzag", "natural"):
            k = _check_case(hp, dev, c, order=order)
            assert k == dict(split_intervals=1, serial_intervals=0, unsettled_intervals=0, rounds=0), c["name"]


def test_slow_convergence(hp, dev):
    """Scans without a single EOB, grey and 4:2:0, longer than the bound; a 4:2:0 scan with half its coefficients
    non-zero; and the scan that never falls into step, which settles in exactly R launches at R + 1 groups and
    cannot at R + 2: the outputs equal hpdct_decode_scan's, the info is the restatement's."""
    s, g, r = hp.decode_split_geometry()
    cases, results, counts = restated()
    want = {c["name"]: k for c, k in zip(cases, counts)}
    for name in ("dense grey", "dense 420", "half 420", "stubborn, settles", "stubborn, does not settle"):
        c = [x for x in cases if x["name"] == name][0]
        info = _serial_and_split(hp, dev, c)
        assert {k: info[k] for k in COUNTERS} == want[name], (name, info)
        assert info["bad_intervals"] == 0
    assert want["stubborn, does not settle"]["unsettled_intervals"] == 1 and want["half 420"]["rounds"] >= 1


def test_untrusted_offsets(hp, dev):
    """Overlapping intervals whose segments exceed the budget: the later ones are walked by one lane, the results
    are jpeg_unscan's, the workspace's sentinels survive."""
    s, g, r = hp.decode_split_geometry()
    c = I.overlapping(s)
    k = _check_case(hp, dev, c)
    n = len(c["offsets"]) - 1
    assert 0 < k["split_intervals"] < n // 2 and k["serial_intervals"] > n // 2
    want = U.decode(c["data"], c["sampling"], c["shapes"], c["ri"], c["offsets"])
    assert (want[1] != 0).sum() >= n // 2


# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------
def _bound_buffers(hp, dev, shapes, ri, scan_bytes):
    import torch
    ty, tx = shapes[0]
    intervals = 1 if ri == 0 else -(-ty * tx // ri)
    y = torch.full((ty, tx, 64), SENTINEL, dtype=torch.int16, device=dev)
    info = torch.full((4,), -1, dtype=torch.int64, device=dev)
    status = torch.full((intervals,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(hp.decode_split_workspace_bytes(8 * ty, 8 * tx, restart_interval=ri, scan_bytes=scan_bytes),
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
    y, info, status, ws = _bound_buffers(hp, dev, shapes, ri, max(len(d1), len(d2)))
    s1, s2 = _dev(np.frombuffer(d1, np.uint8).copy(), dev), _dev(np.frombuffer(d2, np.uint8).copy(), dev)
    offs = _dev(np.asarray(o1, np.int64), dev)
    torch.cuda.synchronize()
    kw = dict(restart_interval=ri, stream=side, split_min_bytes=1)
    c1 = hp.bind_decode_scan_split(s1, offs, y, None, None, info, status, ws, **kw)
    c2 = hp.bind_decode_scan_split(s2, None, y, None, None, info, status, ws, **kw)
    seen = []
    for call, want, found in ((c1, first, 0), (c2, second, 10), (c1, first, 0), (c1, first, 0)):
        call()
        side.synchronize()
        seen.append(hp.decode_split_info(info))
        assert seen[-1] == dict(bad_intervals=0, markers_found=found, marker_errors=0, split_intervals=11,
                                serial_intervals=0, unsettled_intervals=0, rounds=0)
        assert not bool(status.any()) and np.array_equal(y.cpu().numpy(), want)
    assert seen[2] == seen[3]


def test_graph_capture_and_replay(hp, dev):
    """One bind_decode_scan_split launch (thirteen kernels, one chain, no allocation, nothing read back) captured in
    a graph and replayed gives the same bytes."""
    import torch
    shapes, ri = [(3, 7)], 2
    blocks = unscan_corpus.sparse_blocks(shapes[0], 41)
    data, _ = J.encode([blocks], "grey", ri)
    y, info, status, ws = _bound_buffers(hp, dev, shapes, ri, len(data))
    scan = _dev(np.frombuffer(data, np.uint8).copy(), dev)
    hp.bind_decode_scan_split(scan, None, y, None, None, info, status, ws, restart_interval=ri, split_min_bytes=1)()
    torch.cuda.synchronize()                        # the kernels are loaded before the capture
    direct = (y.cpu().numpy().copy(), status.cpu().numpy().copy(), info.cpu().numpy().copy())
    assert np.array_equal(direct[0], blocks) and hp.decode_split_info(info)["split_intervals"] == 11
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            hp.bind_decode_scan_split(scan, None, y, None, None, info, status, ws, restart_interval=ri,
                                      split_min_bytes=1)()
    torch.cuda.synchronize()
    y.fill_(SENTINEL)
    status.fill_(-1)
    info.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), direct[0]) and np.array_equal(status.cpu().numpy(), direct[1])
    assert np.array_equal(info.cpu().numpy(), direct[2])


def test_jpeg_decode_methods_agree(hp, oracle, dev):
    """jpeg_decode(method="split") equals method="serial" on the three Pillow files and on jpeg_encode's output;
    "auto" takes the serial call for these small files and gives the same."""
    import torch
    files = []
    for name in FIXTURES:
        data, lay, _, _, _, _ = fixture_layout(hp, name)
        files.append((data, lay["q_luma"] if lay["components"] == 1 else None))
    img = _dev(oracle.rand_u8(45 * 70 * 3, 9).reshape(45, 70, 3), dev)
    files += [(hp.jpeg_encode(img, subsampling=s), None) for s in ("420", "444")]
    files.append((hp.jpeg_encode(_dev(oracle.rand_u8(24 * 56, 9).reshape(24, 56), dev)), None))
    for data, table in files:
        if table is not None:
            hp.set_quant_table(table)
        try:
            a, b, c = (hp.jpeg_decode(data, device=dev, method=m) for m in ("serial", "split", "auto"))
        finally:
            hp.set_quant_table(None)
        assert torch.equal(a, b) and torch.equal(a, c)
