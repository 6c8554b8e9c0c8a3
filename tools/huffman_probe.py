"""The caller's Huffman tables at 8192^2, grey and 4:2:0, on the
noise and the smooth frame of tools/scan_probe.py: back-to-back calls over
rotating input sets, HIP events on the launch stream, a clock warm-up first,
every case twice (the second pass in reverse order; the two passes' difference
is the run's own spread).

  existing calls (also with a library that lacks the new ones: --pkg DIR takes
  hpdct.py and lib/ from DIR, for runs alternated with another build)
    (a)  encode_scan, one MCU row per interval
    (b)  decode_scan of that scan, offsets given
    (c)  decode_scan_split of it, offsets given
  new calls
    (d)  scan_histogram, one MCU row per interval
    (e)  scan_histogram, restart_interval = 0: the same pass, it does not depend on intervals
    (f)  a device copy of the blocks' own bytes (2 B per coefficient read, as much written)
    (g)  encode_scan under the optimal tables of the frame (tables=)
    (h)  decode_scan of that scan under those tables
  and the sizes of both scans, then jpeg_encode(optimize=False / True) on the
  host clock (forward, the scan, the copies to the host) with the files' sizes.

usage: python tools/huffman_probe.py [--pkg DIR] [size]      (default 8192)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = sys.argv[1:]
PKG = os.path.join(ROOT, "cuda-dct-idct_amd")
if "--pkg" in _args:
    at = _args.index("--pkg")
    PKG = os.path.abspath(_args[at + 1])
    del _args[at:at + 2]
sys.path.insert(0, PKG)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import numpy as np      # noqa: E402
import torch            # noqa: E402
import hpdct            # noqa: E402
from scan_probe import noise, smooth    # noqa: E402

SETS = 4


def main():
    n = int(_args[0]) if _args else 8192
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    new = hasattr(hpdct, "scan_histogram")
    print(f"huffman_probe: {hpdct.version()} from {hpdct.LIB_PATH}; new calls: {new}", flush=True)

    def region(calls, reps):
        for c in calls[:4]:
            c()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for i in range(reps):
            calls[i % len(calls)]()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    warm_in = torch.empty((n, n), dtype=torch.uint8, device=dev)
    warm_out = torch.empty((n // 8, n // 8, 64), dtype=torch.int16, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, warm_out, stream=stream)
    for _ in range(20000):      # clocks up
        warm()
    torch.cuda.synchronize()
    del warm, warm_in, warm_out

    px = n * n
    for layout in ("grey", "420"):
        for kind, make in (("noise", noise), ("smooth", smooth)):
            if layout == "grey":
                frames = [make(s, (n, n), dev) for s in range(SETS)]
                blocks = [(hpdct.forward_blocks(f), None, None) for f in frames]
                ri, sub, comps = n // 8, "444", 1
            else:
                frames = [make(s, (n, n, 3), dev) for s in range(SETS)]
                blocks = [hpdct.forward_rgb_frame(f, subsampling="420") for f in frames]
                ri, sub, comps = n // 16, "420", 3
            intervals = n // (8 if layout == "grey" else 16)
            kw = dict(height=n, width=n, subsampling=sub, restart_interval=ri)
            torch.cuda.synchronize()

            def coder(tables):
                """The bound encode and decode calls of every set under `tables`, and the first scan's length."""
                extra = {} if tables is None else {"tables": tables}
                scans, infos, offs, encs, decs, splits, keep, split_args = [], [], [], [], [], [], [], []
                _, info0, _ = hpdct.encode_scan(*blocks[0], **kw, **extra)
                assert not info0["truncated"] and not info0["out_of_range"], info0
                cap = info0["bytes"] + info0["bytes"] // 8
                for s in range(SETS):
                    scans.append(torch.empty(cap, dtype=torch.uint8, device=dev))
                    infos.append(torch.empty(2, dtype=torch.int64, device=dev))
                    offs.append(torch.empty(intervals + 1, dtype=torch.int64, device=dev))
                    ws = torch.empty(16 * intervals, dtype=torch.uint8, device=dev)
                    keep.append(ws)
                    encs.append(hpdct.bind_scan(*blocks[s], scans[s], infos[s], offs[s], ws, stream=stream, **kw, **extra))
                    encs[s]()
                torch.cuda.synchronize()
                outs = [tuple(torch.empty_like(b) for b in blocks[0] if b is not None) for _ in range(2)]
                for s in range(SETS):
                    k = int(infos[s][0])
                    assert k <= cap
                    o = outs[s % 2] + (None, None) * (comps == 1)
                    dinfo = torch.empty(4, dtype=torch.int64, device=dev)
                    dws = torch.empty(hpdct.decode_split_workspace_bytes(n, n, components=comps, subsampling=sub,
                                                                         restart_interval=ri, scan_bytes=k),
                                      dtype=torch.uint8, device=dev)
                    keep += [dinfo, dws]
                    split_args.append((scans[s][:k], offs[s], *o, dinfo, None, dws))
                    decs.append(hpdct.bind_decode_scan(scans[s][:k], offs[s], *o, dinfo[:2], None, dws, stream=stream,
                                                       **kw, **extra))
                    if tables is None:
                        splits.append(hpdct.bind_decode_scan_split(scans[s][:k], offs[s], *o, dinfo, None, dws,
                                                                   stream=stream, **kw))
                decs[0]()
                torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(outs[0], blocks[0]))
                # a bound call holds pointers, not tensors: the buffers live as long as the caller keeps them
                return info0["bytes"], encs, decs, splits, [split_args] + keep + scans + infos + offs + outs

            nbytes, encs, decs, splits, keep_k = coder(None)
            cases = [("(a) encode_scan", encs), ("(b) decode_scan, offsets given", decs),
                     ("(c) decode_scan_split, offsets given", splits)]
            print(f"\n{n} x {n} {layout}, {kind}: {intervals} intervals of one MCU row, Annex K scan {nbytes} bytes = "
                  f"{nbytes / px:.4f} B/px", flush=True)
            if new:
                counts = [torch.empty((4, 256), dtype=torch.int64, device=dev) for _ in range(2)]
                hist = [hpdct.bind_scan_histogram(*blocks[s], counts[s % 2], stream=stream, **kw) for s in range(SETS)]
                kw0 = dict(kw, restart_interval=0)
                hist0 = [hpdct.bind_scan_histogram(*blocks[s], counts[s % 2], stream=stream, **kw0) for s in range(SETS)]
                dst = [tuple(torch.empty_like(b) for b in blocks[0] if b is not None) for _ in range(2)]

                def copy_of(s):
                    def call():
                        for d, b in zip(dst[s % 2], blocks[s]):
                            d.copy_(b)
                    return call

                # one set of tables for all the sets: of their summed counts, so that every symbol has a code
                c = sum(hpdct.scan_histogram(*blocks[s], **kw).cpu().numpy() for s in range(SETS))
                specs = [hpdct.huffman_optimal(c[k]) if k < 2 or comps == 3 else None for k in range(4)]
                blob = torch.from_numpy(hpdct.huffman_prepare(specs)).to(dev)
                obytes, oencs, odecs, _, keep_o = coder(blob)
                print(f"optimal tables of the sets' summed counts: scan of set 0 {obytes} bytes = {obytes / px:.4f} B/px, "
                      f"{100.0 * (nbytes - obytes) / nbytes:.1f} % smaller; symbols in use "
                      f"{[0 if sp is None else len(sp[1]) for sp in specs]}", flush=True)
                # capacity 0: the measure launch, the offsets launch, and an emit launch that returns at once
                zinfo = torch.empty(2, dtype=torch.int64, device=dev)
                zoffs = torch.empty(intervals + 1, dtype=torch.int64, device=dev)
                zws = torch.empty(16 * intervals, dtype=torch.uint8, device=dev)
                zscan = torch.empty(16, dtype=torch.uint8, device=dev)
                measure = [hpdct.bind_scan(*blocks[s], zscan, zinfo, zoffs, zws, capacity=0, stream=stream, **kw)
                           for s in range(SETS)]
                osplits = [hpdct.bind_decode_scan_split(*a, stream=stream, tables=blob, **kw) for a in keep_o[0]]
                if layout == "grey":
                    fout = [torch.empty_like(blocks[0][0]) for _ in range(2)]
                    fwd = [hpdct.bind_blocks("fwd", frames[s], fout[s % 2], stream=stream) for s in range(SETS)]
                else:
                    fwd = [(lambda f=frames[s]: hpdct.forward_rgb_frame(f, subsampling="420")) for s in range(SETS)]
                cases += [("(i) the forward of the frame (4:2:0: with its allocations)", fwd),
                          ("(m) encode_scan with capacity 0: its measure launch", measure),
                          ("(j) decode_scan_split(tables=optimal)", osplits),
                          ("(d) scan_histogram, one MCU row", hist), ("(e) scan_histogram, restart_interval 0", hist0),
                          ("(f) copy of the blocks", [copy_of(s) for s in range(SETS)]),
                          ("(g) encode_scan(tables=optimal)", oencs), ("(h) decode_scan(tables=optimal)", odecs)]
            reps = 32
            first = [region(calls, reps) for _, calls in cases]
            second = [region(calls, reps) for _, calls in reversed(cases)][::-1]
            print("| case | pass 1 us | pass 2 us | spread us |")
            print("|---|---|---|---|")
            for (name, _), t1, t2 in zip(cases, first, second):
                print(f"| {name} | {t1:.1f} | {t2:.1f} | {abs(t1 - t2):.1f} |", flush=True)
            if new:
                t = {name[:3]: min(t1, t2) for (name, _), t1, t2 in zip(cases, first, second)}
                sizes = [len(hpdct.jpeg_encode(frames[0], subsampling="420", optimize=opt)) for opt in (False, True)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = hpdct.scan_histogram(*blocks[0], **kw).cpu().numpy()
                sp = [hpdct.huffman_optimal(c[k]) if k < 2 or comps == 3 else None for k in range(4)]
                torch.from_numpy(hpdct.huffman_prepare(sp)).to(dev)
                torch.cuda.synchronize()
                host = (time.perf_counter() - t0) * 1e6
                print(f"jpeg_encode device time, the launches' sum: optimize=False (i) + (a) = {t['(i)'] + t['(a)']:.1f} us, "
                      f"file {sizes[0]} bytes; optimize=True (i) + (d) + (g) = {t['(i)'] + t['(d)'] + t['(g)']:.1f} us, "
                      f"file {sizes[1]} bytes; between (d) and (g) the counts go to the host and the tables come back: "
                      f"{host:.0f} us on the host clock with the histogram's launch", flush=True)
            del frames, blocks, encs, decs, splits, cases, keep_k
            keep_o = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
