"""hpdct_decode_scan on the GPU over the scans tests/unscan_built.py builds,
everything compared exactly (blocks, status array, info) with what was built or
with tests/jpeg_unscan.py.  tests/test_unscan_built_host.py proves on the CPU
that the inputs are what they are meant to be:

- the catalogue: every code of the four Annex K tables at every bit phase, both
  extremes of the extra bits; 4:4:4, grey and a 4:2:0 layout of the same blocks,
  both block orders, offsets given and markers located;
- the stuffed scan at the eight addresses mod 8, inside 0xFF and inside 0x00;
- markers written over the edges of the search's 64-byte steps and 4096-byte
  chunks, 3,000 markers in a row, and a 128 MiB scan whose markers only the
  second turn of the locate kernels' loop and a 33-chunk thread of the rank
  kernel can find.
"""
import time

import numpy as np
import pytest

import jpeg_scan as J
import jpeg_unscan as U
import unscan_built as B
import unscan_corpus
from test_gpu_unscan import _check, _dev, _natural

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# A. every code at every bit phase
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["444", "grey", "420"])
def test_catalogue_decodes_to_the_built_blocks(hp, dev, sampling):
    if sampling == "420":
        comps, shapes, ri = B.as_420(B.catalogue("444"))
        data, offs = J.encode(comps, "420", ri)
    else:
        b = B.catalogue(sampling)
        comps, shapes, ri, data, offs = b["components"], b["shapes"], b["ri"], b["data"], b["offsets"]
    scan = _dev(np.frombuffer(data, np.uint8), dev)
    for order in ("zigzag", "natural"):
        for offsets in (None, offs):
            given = None if offsets is None else _dev(np.asarray(offsets, np.int64), dev)
            got, info, st = hp.decode_scan(scan, height=8 * shapes[0][0], width=8 * shapes[0][1],
                                           components=len(shapes), restart_interval=ri, offsets=given, order=order,
                                           subsampling="444" if sampling == "grey" else sampling)
            # against the construction itself, not a decoder
            assert info == {"bad_intervals": 0, "markers_found": 0 if offsets else len(offs) - 2, "marker_errors": 0}
            assert not bool(st.any()) and len(st) == len(offs) - 1
            for g, x in zip(got, comps):
                assert np.array_equal(g.cpu().numpy(), _natural(x) if order == "natural" else x)


# ---------------------------------------------------------------------------
# B. stuffing and the word cache
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xff, 0x00])
def test_stuffed_scan_at_every_address(hp, dev, fill):
    """The scan as a slice of a larger tensor at each address mod 8 (the reader's word cache loads the aligned 8
    bytes around a position only when they lie inside the interval), the other bytes FF or 00."""
    import torch
    blocks, data, offs = B.stuffed()
    n, src = blocks.shape[1], torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    offs_dev = _dev(np.asarray(offs, np.int64), dev)
    for shift in range(8):
        big = torch.full((len(data) + 64,), fill, dtype=torch.uint8, device=dev)
        scan = big[16 + shift:16 + shift + len(data)]
        scan.copy_(src)
        assert scan.data_ptr() % 8 == shift
        for offsets in (None, offs_dev):
            (got,), info, st = hp.decode_scan(scan, height=8, width=8 * n, restart_interval=1, offsets=offsets)
            assert info == {"bad_intervals": 0, "markers_found": 0 if offsets is not None else n - 1,
                            "marker_errors": 0}, shift
            assert not bool(st.any())
            assert np.array_equal(got.cpu().numpy(), blocks), shift
        assert bool((big[:16 + shift] == fill).all()) and bool((big[16 + shift + len(data):] == fill).all())


# ---------------------------------------------------------------------------
# D. the marker search at its edges
# ---------------------------------------------------------------------------
def test_markers_on_the_edges_of_steps_and_chunks(hp, dev):
    """FF Dn written over the last lane of a step, over a chunk's end and at the scan's end, with its number and
    with a wrong one; FF as the last byte; 3,000 markers in a row: blocks, status and info as the restatement."""
    b = B.catalogue("grey")
    for name, data, _ in B.marker_cases(b):
        _check(hp, dev, data, "grey", b["shapes"], 1, None)


def test_markers_in_the_second_turn_of_the_search(hp, dev):
    """128 MiB of zeros, then the grey corpus base: 32,769 chunks for 32,768 waves, 33 chunks per thread of the
    rank kernel; marker 0 lies across chunks 32767 / 32768, the others in the last chunk."""
    import torch
    zeros, blocks, data = B.far_markers()
    want, status, found, errors = B.far_expected(zeros, data)
    t0 = time.perf_counter()
    scan = torch.zeros(zeros + len(data), dtype=torch.uint8, device=dev)
    scan[zeros:] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    ty, tx = unscan_corpus.GREY_SHAPES[0]
    (got,), info, st = hp.decode_scan(scan, height=8 * ty, width=8 * tx, restart_interval=unscan_corpus.GREY_RI)
    torch.cuda.synchronize()
    print("far markers: buffer and decode_scan in %.3f s" % (time.perf_counter() - t0))
    assert info == {"bad_intervals": 1, "markers_found": 10, "marker_errors": 0} and (found, errors) == (10, 0)
    st = st.cpu().numpy().view(np.uint64)
    assert np.array_equal(st, status) and st[0] != 0 and not st[1:].any()
    got = got.cpu().numpy()
    assert np.array_equal(got, want[0])
    assert np.array_equal(got.reshape(-1, 64)[2:], blocks.reshape(-1, 64)[2:])     # intervals 1..10: the base's blocks
    assert U.NAMES[int(status[0]) & 255] == "TAIL"
