"""Grey frames of any size and row pitch (forward_grey_frame / inverse_grey_frame)
against the whole-tile calls they extend, in the manner of tools/rgb_frame_probe.py:
back-to-back launches over rotating input sets (>= 1 GiB of pixels, or of blocks
for the inverse; at most 192 frames, which for 667 x 1000 is 122 MiB of pixels:
that case and 1080 x 1920 at 379 MiB are launch-bound, not memory-bound), HIP
events on the launch stream, a clock lead-in first, every case twice (the second
pass in reverse order; the two passes' difference is the run's own spread).

Per direction, us per frame:
  1  8192^2 through forward_blocks / inverse_blocks to uint8: the yardstick, the
     kernels the frame calls are measured against.  Twice (1a, 1b), on two
     different groups of buffers: their difference is what two buffer sets alone
     are worth.
  2  8192^2 dense through the frame calls (the instantiation without edge code)
  3  8192^2 with a row pitch of 8192 + 64 bytes (the same instantiation)
  4  8185 x 8190 with a pitch of 8192: the edge tiles alone run the byte path
  5  8185 x 8190 dense: pitch 8190, not a multiple of 8: every tile by bytes
  6  1080 x 1920 and 667 x 1000, dense
  7  what a caller without the frame calls does for case 4: the frame copied into
     an edge-replicated 8192^2 buffer with torch (three copies) and forward_blocks;
     inverse_blocks into a padded buffer and a cropped copy out of it
Cases 2-5 and 7 are reported as ratios to case 1a (the same padded size).

usage: python tools/grey_frame_probe.py [--log PATH]   (default profiles/r14/grey_frame_probe.log)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))

N = 8192
POOL_BUFFERS = 32                             # x N * (N + 64) bytes: 2.0 GiB, two groups of 16
MAX_SETS = 192


def main():
    import torch
    import hpdct

    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r14", "grey_frame_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    u8 = torch.uint8

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

    # the pixel pool every case carves its input frames from, filled once
    buf_bytes = N * (N + 64)
    pool = [torch.empty(buf_bytes, dtype=u8, device=dev) for _ in range(POOL_BUFFERS)]
    for s, t in enumerate(pool):
        hpdct.fill_hash_u8(t, seed=7 + s)
    out_pool = [torch.empty(buf_bytes, dtype=u8, device=dev) for _ in range(2)]

    def carve(bufs, h, w, pitch, at_least):
        """(h, w) views with rows `pitch` bytes apart, 256-byte aligned, as many as hold `at_least` bytes."""
        step = -(-(h * pitch) // 256) * 256
        views = []
        for b in bufs:
            for k in range(buf_bytes // step):
                views.append(b.as_strided((h, w), (pitch, 1), k * step))
                if len(views) * h * w >= at_least or len(views) >= MAX_SETS:
                    return views
        return views

    # clocks up: ~1 s of back-to-back launches
    warm_in = torch.empty((N, N), dtype=u8, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, torch.empty((N // 8, N // 8, 64), dtype=torch.int16, device=dev),
                             stream=stream)
    for _ in range(30000):
        warm()
    torch.cuda.synchronize()
    del warm, warm_in

    half = POOL_BUFFERS // 2
    shapes = [("1a 8192^2 dense, blocks calls", N, N, N, "blocks", pool[:half]),
              ("1b 8192^2 dense, blocks calls, other buffers", N, N, N, "blocks", pool[half:]),
              ("2 8192^2 dense, frame calls", N, N, N, "frame", pool[:half]),
              ("3 8192^2 pitch 8192+64", N, N, N + 64, "frame", pool),
              ("4 8185x8190 pitch 8192", 8185, 8190, N, "frame", pool[:half]),
              ("5 8185x8190 dense (pitch 8190)", 8185, 8190, 8190, "frame", pool[:half]),
              ("7 8185x8190 pitch 8192: torch pad + blocks calls + crop", 8185, 8190, N, "legacy", pool[:half]),
              ("6 1080x1920 dense", 1080, 1920, 1920, "frame", pool[:half]),
              ("6 667x1000 dense", 667, 1000, 1000, "frame", pool[:half])]
    ratio_rows = 2 * 7                        # the 8192^2-sized cases, forward and inverse each

    cases, keep = [], []
    for name, h, w, pitch, entry, bufs in shapes:
        ins = carve(bufs, h, w, pitch, 1 << 30)
        outs = carve(out_pool, h, w, pitch, 2 * h * w)          # two output frames
        assert len(outs) == 2
        hp_, wp_, nb_blocks = hpdct.grey_frame_geometry(h, w)
        fo = [torch.empty((hp_ // 8, wp_ // 8, 64), dtype=torch.int16, device=dev) for _ in range(2)]
        # the inverse's rotating inputs: >= 1 GiB of blocks
        nb = min(len(ins), max(2, -(-(1 << 30) // (128 * nb_blocks))))
        blocks = [hpdct.forward_grey_frame(ins[s]) for s in range(nb)]
        torch.cuda.synchronize()
        if entry == "blocks":
            fwd = [hpdct.bind_blocks("fwd", ins[s], fo[s % 2], stream=stream) for s in range(len(ins))]
            inv = [hpdct.bind_blocks("inv", blocks[s], outs[s % 2], stream=stream) for s in range(nb)]
        elif entry == "frame":
            fwd = [hpdct.bind_grey_frame("fwd", ins[s], fo[s % 2], stream=stream) for s in range(len(ins))]
            inv = [hpdct.bind_grey_frame("inv", outs[s % 2], blocks[s], stream=stream) for s in range(nb)]
        else:
            padded = torch.empty((hp_, wp_), dtype=u8, device=dev)

            def pad_and_forward(x, o, padded=padded, h=h, w=w):
                run = hpdct.bind_blocks("fwd", padded, o, stream=stream)

                def call():
                    padded[:h, :w].copy_(x)
                    padded[:h, w:] = padded[:h, w - 1:w]
                    padded[h:, :] = padded[h - 1:h, :]
                    run()
                return call

            def inverse_and_crop(b, o, padded=padded, h=h, w=w):
                run = hpdct.bind_blocks("inv", b, padded, stream=stream)

                def call():
                    run()
                    o.copy_(padded[:h, :w])
                return call

            fwd = [pad_and_forward(ins[s], fo[s % 2]) for s in range(len(ins))]
            inv = [inverse_and_crop(blocks[s], outs[s % 2]) for s in range(nb)]
        cases.append(("forward " + name, fwd, max(96, 2 * len(fwd))))
        cases.append(("inverse " + name, inv, max(96, 2 * len(inv))))
        keep.append((fo, blocks))
    # the set-up above let the clocks drop: ~0.3 s of the first case again before the timed passes
    region(cases[0][1], 10000)
    first = [region(calls, r) for _, calls, r in cases]
    second = [region(calls, r) for _, calls, r in reversed(cases)][::-1]
    best = [min(a, b) for a, b in zip(first, second)]
    say(f"{hpdct.version()}  {hpdct.build_info()}")
    say(f"{torch.cuda.get_device_name(0)}")
    say("| case | input sets | pass 1 us | pass 2 us | spread us | case / case 1a |")
    say("|---|---|---|---|---|---|")
    for i, ((name, calls, _), t1, t2) in enumerate(zip(cases, first, second)):
        ratio = f"{best[i] / best[i % 2]:.3f}" if i < ratio_rows else ""
        say(f"| {name} | {len(calls)} | {t1:.2f} | {t2:.2f} | {abs(t1 - t2):.2f} | {ratio} |")
    log.close()


if __name__ == "__main__":
    main()
