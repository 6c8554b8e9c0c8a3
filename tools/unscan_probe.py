"""The entropy decoder (decode_scan) at 8192^2, grey and 4:2:0, on the scans
encode_scan makes of a noise frame (nearly incompressible, the worst case) and
of a smooth one (gradient plus low noise), with the method of scan_probe.py:
back-to-back calls over rotating input sets, HIP events on the launch stream, a
clock warm-up first, every case twice (the second pass in reverse order; the
two passes' difference is the run's own spread).

For one MCU row, 64 MCUs and 8 MCUs per restart interval:
  (a)  decode_scan with the coder's offsets (two launches)
  (b)  decode_scan locating the markers itself (four launches)
  (c)  encode_scan of the same blocks (three launches)
  (d)  the copy ceiling with 1 B in and 4 B out per pixel: the decoder reads
       less than 1 B/px and writes its blocks once (2 or 3 B/px)
and, for the grey frames, end to end on the host clock with pinned memory: H2D
copy of the scan + decode_scan against the H2D copy of the blocks.

The time of each launch comes from a kernel trace of `unscan_probe.py --quick`
(a few calls per case, no timing), a run of its own.

`--grey` leaves the 4:2:0 frames out and `--mcus=16,32` replaces the interval
lengths (for A/B runs of the policy's rows against another build named by
HPDCT_LIB).

usage: python tools/unscan_probe.py [--quick] [--grey] [--mcus=a,b] [size]      (default 8192)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np      # noqa: E402
import torch            # noqa: E402
import hpdct            # noqa: E402
from scan_probe import noise, smooth   # noqa: E402

SETS = 4


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mcus = [int(v) for a in sys.argv[1:] if a.startswith("--mcus=") for v in a[7:].split(",")]
    quick = "--quick" in sys.argv[1:]
    layouts = ("grey",) if "--grey" in sys.argv[1:] else ("grey", "420")
    n = int(args[0]) if args else 8192
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()

    def region(calls, reps):
        for c in calls[:2]:
            c()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for i in range(reps):
            calls[i % len(calls)]()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    if not quick:       # clocks up: ~2 s of back-to-back launches
        warm_in = torch.empty((n, n), dtype=torch.uint8, device=dev)
        warm_out = torch.empty((n // 8, n // 8, 64), dtype=torch.int16, device=dev)
        warm = hpdct.bind_blocks("fwd", warm_in, warm_out, stream=stream)
        for _ in range(30000):
            warm()
        torch.cuda.synchronize()
        del warm, warm_in, warm_out

    px = n * n
    for layout in layouts:
        for kind, make in (("noise", noise), ("smooth", smooth)):
            if layout == "grey":
                frames = [make(s, (n, n), dev) for s in range(SETS)]
                blocks = [(hpdct.forward_blocks(f), None, None) for f in frames]
                row, sub, nblk, comps = n // 8, "444", px // 64, 1
            else:
                frames = [make(s, (n, n, 3), dev) for s in range(SETS)]
                blocks = [hpdct.forward_rgb_frame(f, subsampling="420") for f in frames]
                row, sub, nblk, comps = n // 16, "420", px // 64 * 3 // 2, 3
            nmcu = row * row
            del frames
            outs = [tuple(torch.empty_like(b) for b in blocks[0] if b is not None) for _ in range(2)]
            src8 = [torch.empty(px, dtype=torch.uint8, device=dev) for _ in range(4)]
            dst32 = [torch.empty(px, dtype=torch.float32, device=dev) for _ in range(2)]
            copy = [hpdct.bind_copy_ceiling(src8[s % 4], dst32[s % 2], stream=stream) for s in range(SETS)]
            lengths = [(m, f"{m} MCUs") for m in mcus] or [(row, "one MCU row"), (64, "64 MCUs"), (8, "8 MCUs")]
            for ri, what in lengths:
                intervals = -(-nmcu // ri)
                scans, offsets = [], []
                for s in range(SETS):
                    sc, info, of = hpdct.encode_scan(*blocks[s], height=n, width=n, subsampling=sub,
                                                     restart_interval=ri)
                    assert not info["truncated"] and not info["out_of_range"], info
                    scans.append(sc.clone())
                    offsets.append(of)
                nbytes = max(int(s.numel()) for s in scans)
                infos = [torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2)]
                stat = [torch.empty(intervals, dtype=torch.int64, device=dev) for _ in range(2)]
                ws = [torch.empty(hpdct.decode_workspace_bytes(n, n, components=comps, subsampling=sub,
                                                               restart_interval=ri, scan_bytes=nbytes),
                                  dtype=torch.uint8, device=dev) for _ in range(2)]

                def bound(s, located):
                    o = outs[s % 2]
                    return hpdct.bind_decode_scan(scans[s], None if located else offsets[s], o[0],
                                                  o[1] if comps == 3 else None, o[2] if comps == 3 else None,
                                                  infos[s % 2], stat[s % 2], ws[s % 2], height=n, width=n,
                                                  subsampling=sub, restart_interval=ri, stream=stream)

                given = [bound(s, False) for s in range(SETS)]
                located = [bound(s, True) for s in range(SETS)]
                ebuf = [torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, device=dev) for _ in range(2)]
                einfo = [torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2)]
                eoffs = [torch.empty(intervals + 1, dtype=torch.int64, device=dev) for _ in range(2)]
                ews = [torch.empty(16 * intervals, dtype=torch.uint8, device=dev) for _ in range(2)]
                enc = [hpdct.bind_scan(*blocks[s], ebuf[s % 2], einfo[s % 2], eoffs[s % 2], ews[s % 2], height=n,
                                       width=n, subsampling=sub, restart_interval=ri, stream=stream)
                       for s in range(SETS)]
                # the decoder gives the coder's blocks back
                for calls in (given, located):
                    calls[0]()
                    torch.cuda.synchronize()
                    assert hpdct.decode_info(infos[0])["bad_intervals"] == 0
                    assert all(torch.equal(a, b) for a, b in zip(outs[0], [b for b in blocks[0] if b is not None]))
                print(f"\n{n} x {n} {layout}, {kind}, {what} per interval: {nblk} blocks, {intervals} intervals, scan "
                      f"{nbytes} bytes = {nbytes / px:.4f} B/px (blocks: {2 * nblk * 64 / px:.1f} B/px)", flush=True)
                if quick:
                    for c in given[:2] + located[:2]:
                        c()
                    torch.cuda.synchronize()
                    continue
                cases = [("(a) decode_scan, offsets given", given), ("(b) decode_scan, markers located", located),
                         ("(c) encode_scan of the same blocks", enc), ("(d) copy ceiling 1 B in, 4 B out", copy)]
                reps = 8
                first = [region(calls, reps) for _, calls in cases]
                second = [region(calls, reps) for _, calls in reversed(cases)][::-1]
                print("| case | pass 1 us | pass 2 us | spread us |")
                print("|---|---|---|---|")
                for (name, _), t1, t2 in zip(cases, first, second):
                    print(f"| {name} | {t1:.1f} | {t2:.1f} | {abs(t1 - t2):.1f} |", flush=True)
                if layout == "grey":
                    host_scan = scans[0].cpu().pin_memory()
                    host_blocks = blocks[0][0].cpu().pin_memory()
                    dev_scan, dev_blocks = torch.empty_like(scans[0]), torch.empty_like(blocks[0][0])
                    call = hpdct.bind_decode_scan(dev_scan, None, outs[0][0], None, None, infos[0], stat[0], ws[0],
                                                  height=n, width=n, restart_interval=ri, stream=stream)

                    def scan_in():
                        dev_scan.copy_(host_scan, non_blocking=True)
                        call()
                        torch.cuda.synchronize()

                    def blocks_in():
                        dev_blocks.copy_(host_blocks, non_blocking=True)
                        torch.cuda.synchronize()

                    for name, fn in (("H2D of the scan + decode_scan (markers located)", scan_in),
                                     ("H2D of the blocks", blocks_in)):
                        for _ in range(3):
                            fn()
                        times = []
                        for _ in range(12):
                            t0 = time.perf_counter()
                            fn()
                            times.append((time.perf_counter() - t0) * 1e6)
                        print(f"(e) {name}: median {float(np.median(times)):.0f} us, min {min(times):.0f}, "
                              f"max {max(times):.0f} (12 frames, host clock)", flush=True)
                    del host_scan, host_blocks, dev_scan, dev_blocks
                del scans, offsets, given, located, enc, ebuf
            del blocks, outs, src8, dst32, copy
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
