"""The inputs of tests/scan_limits.py reach what they claim (no GPU, no kernel
runs): the restatement of tests/jpeg_scan.py alone says how full the coder's
bit buffer gets, that encode_scan's first buffer is too small, that the
offsets kernel's threads own more than one interval, and that the assembled
scan of the 2^20-interval frame is what the restatement codes.  The figures are
those of csrc/hpdct_scan.hpp; tests/test_gpu_scan_limits.py runs the inputs.
"""
import numpy as np
import pytest

import jpeg_scan as J
import scan_limits as S

SAT_IDS = ["%s-%dx%d" % (s, h, w) for s, (h, w) in S.SATURATED_SHAPES]


def _unstuffed(scan):
    return scan.replace(b"\xff\x00", b"\xff")


# ---------------------------------------------------------------------------
# saturated steps
# ---------------------------------------------------------------------------
def test_grey_saturated_block_lengths():
    """18 + 63 * 26 bits for an interval's first block (DC category 10), 20 + 63 * 26 after it (category 11)."""
    comps = S.saturated("grey", (8, 1024), "neg")
    bits, per = S.block_bits(comps, "grey", 0)
    assert per == 128 and bits[0] == 1656 and set(bits[1:]) == {1658}
    bits, per = S.block_bits(comps, "grey", 50)
    assert per == 50
    assert all(b == (1656 if i % 50 == 0 else 1658) for i, b in enumerate(bits))
    assert set(S.block_bits(comps, "grey", 1)[0]) == {1656}
    # the first 64-block step of the one interval: 3317 of the buffer's 3322 words, 137 bits from the most
    fill = S.step_fill(*S.block_bits(comps, "grey", 0))
    assert fill == [106110, 106110 % 8 + 64 * 1658]
    assert S.buffer_words(fill[0]) == 3317 and S.buffer_words(fill[1]) == 3318 <= S.BIT_WORDS
    assert STEP_MAX - fill[0] == 137


STEP_MAX = S.STEP * S.MAX_BLOCK_BITS + 7        # 106,247 bits: what kBitWords is sized for


def test_every_step_fits_the_buffer_and_grey_fills_it():
    """Every step of every input fits the buffer.  No block is longer than a luma block after its interval's first:
    kMaxBlockBits pairs the chroma DC table's 11-bit code with the luma AC table's 16-bit one, and the chroma code
    of a category-10 coefficient is 12 bits, so a saturated chroma block is 22 + 63 * 22 bits."""
    longest, fullest = {}, 0
    for sampling, shape in S.SATURATED_SHAPES:
        for ac in S.SATURATED_AC:
            for ri in (0, 1, S.UNEVEN_INTERVAL[sampling]):
                bits, per = S.block_bits(S.saturated(sampling, shape, ac), sampling, ri)
                assert len(bits) == S.blocks_of(sampling, shape) and max(bits) <= S.MAX_BLOCK_BITS
                fill = S.step_fill(bits, per)
                assert max(fill) <= STEP_MAX and S.buffer_words(max(fill)) <= S.BIT_WORDS
                longest[sampling] = max(longest.get(sampling, 0), max(bits))
                fullest = max(fullest, max(fill))
    assert longest == {"grey": 1658, "444": 1658, "420": 1658}
    bits, _ = S.block_bits(S.saturated("444", (16, 88), "neg"), "444", 0)
    assert bits[:6] == [1656, 20 + 63 * 22, 20 + 63 * 22, 1658, 22 + 63 * 22, 22 + 63 * 22]
    # the fullest step of all: a grey interval's second, 6 carried bits and 64 blocks of 1658
    assert fullest == 6 + 64 * 1658 == 106118 and S.buffer_words(fullest) == 3318


@pytest.mark.parametrize("ac", S.SATURATED_AC)
@pytest.mark.parametrize("sampling,shape", S.SATURATED_SHAPES, ids=SAT_IDS)
def test_saturated_inputs_are_extreme(hp, sampling, shape, ac):
    comps = S.saturated(sampling, shape, ac)
    blocks = S.blocks_of(sampling, shape)
    assert J.out_of_range(comps, sampling, 0) == 0 and J.out_of_range(comps, sampling, 1) == 0
    for c in comps:
        assert (np.abs(c.astype(np.int64)) == 1023).all()
    if ac != "mixed":
        assert all((c[..., 1:] == (1023 if ac == "pos" else -1023)).all() for c in comps)
    else:
        share = np.mean([(c[..., 1:] > 0).mean() for c in comps])
        assert 0.45 < share < 0.55
    scan, offs = S.expected(("sat", shape, ac), comps, sampling, 0)
    assert offs == [0, len(scan)]
    # the bit fill: at least an interval's first luma block, 1656 bits, in every luma block; a saturated chroma
    # block cannot be that long under the Annex K tables (its AC codes are 12 bits): 20 + 63 * 22 = 1406 at least
    luma = comps[0].shape[0] * comps[0].shape[1]
    print("%s %s %s: %d bits unstuffed in %d blocks" % (sampling, shape, ac, 8 * len(_unstuffed(scan)), blocks))
    assert 8 * len(_unstuffed(scan)) >= 1656 * luma + 1406 * (blocks - luma)
    bits, per = S.block_bits(comps, sampling, 0)
    assert len(_unstuffed(scan)) == -(-sum(bits) // 8)           # the lengths above are the restatement's
    # more than encode_scan's first buffer (128 bytes per block and 4 per interval), within the bound
    assert len(scan) > 128 * blocks + 4
    assert len(scan) <= hp.scan_bound(blocks, 1)
    # a full step's whole bytes take every 256-byte pass there can be, 52, in a grey frame; fewer with chroma in it
    fill = S.step_fill(bits, per)
    passes = max(-(-(n // 8) // 256) for n in fill)
    assert passes == {"grey": 52, "444": 47, "420": 50}[sampling] and -(-(STEP_MAX // 8) // 256) == 52
    for ri in (1, S.UNEVEN_INTERVAL[sampling]):
        scan_ri, offs_ri = S.expected(("sat", shape, ac), comps, sampling, ri)
        n = S.intervals_of(sampling, shape, ri)
        assert len(offs_ri) == n + 1
        assert len(scan_ri) > 128 * blocks + 4 * n                  # the retry at every interval tested
        assert len(scan_ri) <= hp.scan_bound(blocks, n)


def test_saturated_sizes():
    """The stuffed sizes at interval 0, as measured when the inputs were written."""
    size = lambda sampling, shape, ac: len(S.expected(("sat", shape, ac), S.saturated(sampling, shape, ac),  # noqa: E731
                                                      sampling, 0)[0])
    assert size("grey", (8, 1024), "neg") == 28609
    pos = S.expected(("sat", (8, 1024), "pos"), S.saturated("grey", (8, 1024), "pos"), "grey", 0)[0]
    assert len(pos) == 40705 and pos.count(b"\xff\x00") == 14177
    assert size("444", (16, 88), "neg") == 13391
    assert size("420", (32, 176), "neg") == 28120


def test_uneven_intervals_cut_a_step():
    for sampling, shape in S.SATURATED_SHAPES:
        ri = S.UNEVEN_INTERVAL[sampling]
        _, per = S.block_bits(S.saturated(sampling, shape, "neg"), sampling, ri)
        assert S.STEP % per != 0 and per % S.STEP != 0 and S.blocks_of(sampling, shape) % per != 0


@pytest.mark.parametrize("sampling,shape", S.SATURATED_SHAPES, ids=SAT_IDS)
def test_saturated_out_of_range_input(sampling, shape):
    comps = S.saturated_out_of_range(sampling, shape)
    blocks = S.blocks_of(sampling, shape)
    for c in comps:
        flat = c.reshape(-1).astype(np.int64)
        assert set(flat.tolist()) == {32767, -32768} and (flat[:-1] != flat[1:]).sum() >= flat.size - blocks
    # every AC coefficient, and every DC difference that has a predecessor in its interval
    assert J.out_of_range(comps, sampling, 0) == 64 * blocks
    assert J.out_of_range(comps, sampling, 1) == 64 * blocks
    with pytest.raises(ValueError):
        J.encode(comps, sampling, 0)


# ---------------------------------------------------------------------------
# more than 1024 intervals
# ---------------------------------------------------------------------------
def test_many_intervals_give_the_offsets_threads_more_than_one():
    assert [S.offsets_chunk(n) for n in S.MANY_GREY] == [1, 1, 2, 3, 3]
    # at 2500 thread 833 owns one interval (2499), the 190 threads after it none
    chunk = S.offsets_chunk(2500)
    assert 2500 - 833 * chunk == 1 and 834 * chunk > 2500
    assert S.intervals_of("420", S.MANY_420, 2) == 1100 and S.offsets_chunk(1100) == 2
    assert S.blocks_of("420", S.MANY_420) == 13200


@pytest.mark.parametrize("n", S.MANY_GREY)
def test_sparse_grey_input(n):
    comps = S.sparse_grey(n)
    x = comps[0].astype(np.int64)
    assert x.shape == (1, n, 64) and np.abs(x).max() <= 1023
    assert 0.08 < (x != 0).mean() < 0.12
    assert J.out_of_range(comps, "grey", 1) == 0
    scan, offs = S.expected(("sparse", n), comps, "grey", 1)
    lens = np.diff(offs)
    assert len(offs) == n + 1 and len(set(lens.tolist())) >= 10            # the interval lengths differ
    back, = J.decode(scan, "grey", [(1, n)], 1)
    assert np.array_equal(back, comps[0])


def test_sparse_unclipped_shares_the_mask():
    clipped, raw = S.sparse_grey(2500)[0], S.sparse_grey(2500, clip=False)[0]
    assert np.array_equal(clipped != 0, raw != 0)
    assert int(np.abs(raw.astype(np.int64)).max()) > 32000
    n = J.out_of_range([raw], "grey", 1)
    per_interval = [J.out_of_range([raw[:, i:i + 1]], "grey", 1) for i in range(2500)]
    assert n == sum(per_interval) > 2500                                   # a sum across every chunk and thread
    chunk = S.offsets_chunk(2500)
    assert all(sum(per_interval[t * chunk:(t + 1) * chunk]) > 0 for t in range(0, 834, 50))


def test_sparse_420_input():
    comps = S.sparse_420()
    assert [c.shape for c in comps] == [(2, 4400, 64), (1, 2200, 64), (1, 2200, 64)]
    assert J.out_of_range(comps, "420", 2) == 0
    scan, offs = S.expected("sparse420", comps, "420", 2)
    assert len(offs) == 1101 and len(set(np.diff(offs).tolist())) >= 10


# ---------------------------------------------------------------------------
# more than 2^20 intervals
# ---------------------------------------------------------------------------
def test_grid_cap_assembly_is_the_restatement(oracle):
    g = S.GridCap(oracle.default_transform())
    assert g.N == 1050625 == S.MAX_WGS + 2049 and len(g.per) == 381
    # the first 3000 intervals against jpeg_scan.encode of the same 3000 blocks (which ends without a marker)
    n = 3000
    blocks = g.blocks[np.arange(n) % 381].reshape(1, n, 64)
    want, want_offs = J.encode([blocks], "grey", 1)
    got, offs = g.scan(n), g.offsets(n)
    assert got.tobytes()[:-2] == want and got.tobytes()[-2:] == bytes([0xff, 0xd0 + ((n - 1) & 7)])
    assert offs[:-1].tolist() == want_offs[:-1] and offs[-1] == want_offs[-1] + 2
    # past one period of blocks and markers (3048 intervals), the tiled assembly against the plain one
    n = g.PERIOD + 500
    plain = b"".join(g.per[i % 381] + bytes([0xff, 0xd0 + (i & 7)]) for i in range(n))
    assert g.scan(n).tobytes() == plain and g.offsets(n)[-1] == len(plain)
    # the whole frame
    scan, offs = g.scan(g.N), g.offsets(g.N)
    assert scan.size == 59323860 == offs[-1] and offs.size == g.N + 1
    assert scan[offs[-2]:].tobytes() == g.per[(g.N - 1) % 381]             # the last interval: no marker
    i = S.MAX_WGS                                # the first interval a wave takes on its second turn
    assert scan[offs[i]:offs[i + 1]].tobytes() == g.per[i % 381] + bytes([0xff, 0xd0 + (i & 7)])
