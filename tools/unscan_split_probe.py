"""The split entropy decoder (decode_scan(method="split")) against the serial one
(decode_scan) on the same scans in the same session, with the frames, the
rotation over input sets and the event timing of unscan_probe.py: 8192^2, grey
and 4:2:0, a noise frame and a smooth one, at one MCU row, 64 MCUs and 8 MCUs per
restart interval (the twelve rows of DESIGN.md 4.9), and a 1920 x 1088 grey
frame without restart markers, which is one interval.  Every case twice, the
second pass in reverse order; the two passes' difference is the run's own spread.

  (a)  decode_scan, offsets given            (b)  decode_scan, markers located
  (c)  split, every interval split, offsets  (d)  split, every interval, located
  (e)  split with the library's threshold (split_min_bytes = 0), offsets given
and the split call's counters for (c).

`--grey` leaves the 4:2:0 frames out and `--mcus=16,32` replaces the interval
lengths (for the threshold: the shortest interval at which (c) beats (a)).

usage: python tools/unscan_split_probe.py [--grey] [--mcus=a,b] [--no-restart-only] [size]      (default 8192)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch            # noqa: E402
import hpdct            # noqa: E402
from scan_probe import noise, smooth   # noqa: E402

SETS = 4


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mcus = [int(v) for a in sys.argv[1:] if a.startswith("--mcus=") for v in a[7:].split(",")]
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

    # clocks up: ~2 s of back-to-back launches
    warm_in = torch.empty((2048, 2048), dtype=torch.uint8, device=dev)
    warm_out = torch.empty((256, 256, 64), dtype=torch.int16, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, warm_out, stream=stream)
    for _ in range(30000):
        warm()
    torch.cuda.synchronize()
    del warm, warm_in, warm_out
    print("segment bytes, segments of a group, launches between groups:", hpdct.decode_split_geometry(), flush=True)

    def run(h, w, layout, kind, make, lengths, reps):
        px = h * w
        if layout == "grey":
            frames = [make(s, (h, w), dev) for s in range(SETS)]
            blocks = [(hpdct.forward_blocks(f), None, None) for f in frames]
            sub, nblk, comps, nmcu = "444", px // 64, 1, px // 64
        else:
            frames = [make(s, (h, w, 3), dev) for s in range(SETS)]
            blocks = [hpdct.forward_rgb_frame(f, subsampling="420") for f in frames]
            sub, nblk, comps, nmcu = "420", px // 64 * 3 // 2, 3, px // 256
        del frames
        outs = [tuple(torch.empty_like(b) for b in blocks[0] if b is not None) for _ in range(2)]
        for ri, what in lengths:
            intervals = 1 if ri == 0 else -(-nmcu // ri)
            scans, offsets = [], []
            for s in range(SETS):
                sc, info, of = hpdct.encode_scan(*blocks[s], height=h, width=w, subsampling=sub, restart_interval=ri)
                assert not info["truncated"] and not info["out_of_range"], info
                scans.append(sc.clone())
                offsets.append(of)
            nbytes = max(int(s.numel()) for s in scans)
            infos = [torch.empty(4, dtype=torch.int64, device=dev) for _ in range(2)]
            stat = [torch.empty(intervals, dtype=torch.int64, device=dev) for _ in range(2)]
            ws = [torch.empty(hpdct.decode_split_workspace_bytes(h, w, components=comps, subsampling=sub,
                                                                 restart_interval=ri, scan_bytes=nbytes),
                              dtype=torch.uint8, device=dev) for _ in range(2)]

            def bound(s, located, split_min):
                o = outs[s % 2]
                a = (scans[s], None if located else offsets[s], o[0], o[1] if comps == 3 else None,
                     o[2] if comps == 3 else None)
                kw = dict(height=h, width=w, subsampling=sub, restart_interval=ri, stream=stream)
                if split_min is None:
                    return hpdct.bind_decode_scan(*a, infos[s % 2][:2], stat[s % 2], ws[s % 2], **kw)
                return hpdct.bind_decode_scan_split(*a, infos[s % 2], stat[s % 2], ws[s % 2], split_min_bytes=split_min,
                                                    **kw)

            cases = [("(a) decode_scan, offsets given", [bound(s, False, None) for s in range(SETS)]),
                     ("(b) decode_scan, markers located", [bound(s, True, None) for s in range(SETS)]),
                     ("(c) split, every interval, offsets given", [bound(s, False, 1) for s in range(SETS)]),
                     ("(d) split, every interval, markers located", [bound(s, True, 1) for s in range(SETS)]),
                     ("(e) split, the library's threshold, offsets given", [bound(s, False, 0) for s in range(SETS)])]
            want = [b for b in blocks[0] if b is not None]
            counters = {}
            for name, calls in cases:               # every call gives the coder's blocks back
                for o in outs[0]:
                    o.fill_(0x5a5a)
                calls[0]()
                torch.cuda.synchronize()
                got = hpdct.decode_split_info(infos[0]) if "split" in name else hpdct.decode_info(infos[0][:2])
                assert got["bad_intervals"] == 0 and all(torch.equal(a, b) for a, b in zip(outs[0], want)), name
                counters[name[:3]] = {k: v for k, v in got.items() if k.endswith("intervals") or k == "rounds"}
            print(f"\n{h} x {w} {layout}, {kind}, {what} per interval: {nblk} blocks, {intervals} intervals of "
                  f"{nbytes // intervals} bytes, scan {nbytes} bytes = {nbytes / px:.4f} B/px", flush=True)
            print("counters (c):", counters["(c)"], " (e):", counters["(e)"], flush=True)
            first = [region(calls, reps) for _, calls in cases]
            second = [region(calls, reps) for _, calls in reversed(cases)][::-1]
            print("| case | pass 1 us | pass 2 us | spread us |")
            print("|---|---|---|---|")
            for (name, _), t1, t2 in zip(cases, first, second):
                print(f"| {name} | {t1:.1f} | {t2:.1f} | {abs(t1 - t2):.1f} |", flush=True)
            del scans, offsets, cases
        del blocks, outs
        torch.cuda.empty_cache()

    if "--no-restart-only" not in sys.argv[1:]:
        for layout in layouts:
            row = n // 8 if layout == "grey" else n // 16
            lengths = [(m, f"{m} MCUs") for m in mcus] or [(row, "one MCU row"), (64, "64 MCUs"), (8, "8 MCUs")]
            for kind, make in (("noise", noise), ("smooth", smooth)):
                run(n, n, layout, kind, make, lengths, 8)
    if not mcus:
        for kind, make in (("noise", noise), ("smooth", smooth)):
            run(1088, 1920, "grey", kind, make, [(0, "no restart markers: all MCUs")], 2)


if __name__ == "__main__":
    main()
