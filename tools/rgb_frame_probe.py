"""Colour frames of any size and row pitch (forward_rgb_frame / inverse_rgb_frame)
against the whole-unit calls they extend, in the manner of tools/rgb_probe.py:
back-to-back launches over rotating input sets (>= 1 GiB of RGB, or of blocks
for the inverse; at most 192 frames, which for 667 x 1000 is 366 MiB: still
beyond the 256 MiB Infinity Cache), HIP events on the
launch stream, a clock warm-up first, every case twice (the second pass in
reverse order; the two passes' difference is the run's own spread).

Per direction and subsampling:
  1  8192^2 dense through forward_rgb_blocks / inverse_rgb_blocks
  2  8192^2 dense through the frame call (the same kernel instantiation)
  3  8192^2 with a row pitch of 3 * 8192 + 64 bytes (the same instantiation)
  4  8184 x 8184 dense: whole 8x8 tiles, so 4:4:4 stays on the instantiation of
     1-3; 4:2:0 has half an MCU at the right and bottom edges (kRgbClip: the
     edge units alone leave the 8-byte loads and stores)
  5  8185 x 8190 dense: pitch 24570, not a multiple of 8: every unit moves its
     RGB bytes one at a time
  6  1080 x 1920 and 667 x 1000 (rows x pixels), dense
Cases 4 and 5 are reported as ratios to case 1 (the same padded size).

usage: python tools/rgb_frame_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))

N = 8192
POOL_BUFFERS = 6                              # x N * (3 N + 64) bytes: 1.13 GiB
MAX_SETS = 192


def main():
    import torch
    import hpdct

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

    # the RGB pool every case carves its input frames from, filled once
    buf_bytes = N * (3 * N + 64)
    pool = [torch.empty(buf_bytes, dtype=torch.uint8, device=dev) for _ in range(POOL_BUFFERS)]
    for s, t in enumerate(pool):
        hpdct.fill_hash_u8(t, seed=7 + s)
    out_pool = [torch.empty(buf_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]

    def carve(bufs, h, w, pitch, at_least):
        """(h, w, 3) views with rows `pitch` bytes apart, 256-byte aligned, as many as hold `at_least` bytes."""
        step = -(-(h * pitch) // 256) * 256
        views = []
        for b in bufs:
            for k in range(buf_bytes // step):
                views.append(b.as_strided((h, w, 3), (pitch, 3, 1), k * step))
                if len(views) * 3 * h * w >= at_least or len(views) >= MAX_SETS:
                    return views
        return views

    # clocks up: ~2 s of back-to-back launches
    warm_in = torch.empty((N, N), dtype=torch.uint8, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, torch.empty((N // 8, N // 8, 64), dtype=torch.int16, device=dev),
                             stream=stream)
    for _ in range(30000):
        warm()
    torch.cuda.synchronize()
    del warm, warm_in

    shapes = [("1 8192^2 dense, whole-unit call", N, N, 3 * N, "blocks"),
              ("2 8192^2 dense, frame call", N, N, 3 * N, "frame"),
              ("3 8192^2 pitch 3*8192+64", N, N, 3 * N + 64, "frame"),
              ("4 8184x8184 dense", 8184, 8184, 3 * 8184, "frame"),
              ("5 8185x8190 dense (pitch 24570)", 8185, 8190, 3 * 8190, "frame"),
              ("6 1080x1920 dense", 1080, 1920, 3 * 1920, "frame"),
              ("6 667x1000 dense", 667, 1000, 3000, "frame")]

    for sub in ("420", "444"):
        cases = []
        keep = []
        for name, h, w, pitch, entry in shapes:
            ins = carve(pool, h, w, pitch, 1 << 30)
            outs = carve(out_pool, h, w, pitch, 2 * 3 * h * w)      # two output frames
            assert len(outs) == 2
            hp_, wp_, yb, cbk = hpdct.rgb_frame_geometry(h, w, sub)
            fo = [tuple(torch.empty((n, 64), dtype=torch.int16, device=dev) for n in (yb, cbk, cbk)) for _ in range(2)]
            # the inverse's rotating inputs: >= 1 GiB of blocks
            nb = min(len(ins), max(2, -(-(1 << 30) // (128 * (yb + 2 * cbk)))))
            blocks = [hpdct.forward_rgb_frame(ins[s], subsampling=sub) for s in range(nb)]
            torch.cuda.synchronize()
            if entry == "blocks":
                fwd = [hpdct.bind_rgb_blocks("fwd", ins[s], *fo[s % 2], subsampling=sub, stream=stream)
                       for s in range(len(ins))]
                inv = [hpdct.bind_rgb_blocks("inv", outs[s % 2], *blocks[s], subsampling=sub, stream=stream)
                       for s in range(nb)]
            else:
                fwd = [hpdct.bind_rgb_frame("fwd", ins[s], *fo[s % 2], subsampling=sub, stream=stream)
                       for s in range(len(ins))]
                inv = [hpdct.bind_rgb_frame("inv", outs[s % 2], *blocks[s], subsampling=sub, stream=stream)
                       for s in range(nb)]
            cases.append(("forward " + name, fwd, max(96, 2 * len(fwd))))
            cases.append(("inverse " + name, inv, max(96, 2 * len(inv))))
            keep.append((fo, blocks))
        # the set-up above let the clocks drop: ~0.3 s of the first case again before the timed passes
        region(cases[0][1], 3000)
        first = [region(calls, r) for _, calls, r in cases]
        second = [region(calls, r) for _, calls, r in reversed(cases)][::-1]
        best = [min(a, b) for a, b in zip(first, second)]
        print(f"\n4:{sub[1]}:{sub[2]}")
        print("| case | input sets | pass 1 us | pass 2 us | spread us | case / case 1 |")
        print("|---|---|---|---|---|---|")
        for i, ((name, calls, _), t1, t2) in enumerate(zip(cases, first, second)):
            ratio = f"{best[i] / best[i % 2]:.3f}" if i < 10 else ""
            print(f"| {name} | {len(calls)} | {t1:.2f} | {t2:.2f} | {abs(t1 - t2):.2f} | {ratio} |", flush=True)
        del cases, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
