"""The entropy coder (encode_scan) at 8192^2, grey and 4:2:0, one MCU row per
restart interval, on a noise frame (rand_u8 and hash noise: nearly
incompressible, the worst case) and on a smooth one (gradient plus low noise):
back-to-back calls over rotating input sets (>= 1 GiB of blocks), HIP events on
the launch stream, a clock warm-up first, every case twice (the second pass in
reverse order; the two passes' difference is the run's own spread).

  (a)  encode_scan, the whole call (three launches), and its bytes per pixel
  (b)  the copy ceiling with 4 B in and 1 B out per pixel: the coder reads its
       blocks twice (4 B/px) and writes less than 1 B/px
  (c)  end to end, host clock around a synchronised pipeline with pinned memory:
       forward_blocks + D2H copy of the blocks, against forward_blocks +
       encode_scan + D2H copy of the 16-byte info, then of the scan's bytes

The time of each of the three launches comes from a kernel trace of
`scan_probe.py --quick` (a few calls per case, no timing), a run of its own.

`scan_probe.py --psnr` instead reports how close a standard decoder's pixels
(Pillow, exact DCT) are to the library's own inverse of the same blocks.

usage: python tools/scan_probe.py [--quick | --psnr] [size]      (default 8192)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402
import hpdct            # noqa: E402

SETS = 8


def noise(s, shape, dev):
    t = torch.empty(shape, dtype=torch.uint8, device=dev)
    if s == 0:          # the reference's own input stream; the other sets are hash noise
        t.copy_(torch.from_numpy(hpdct.fill_rand_u8(t.numel(), 42).reshape(shape)))
    else:
        hpdct.fill_hash_u8(t, seed=7 + s)
    return t


def smooth(s, shape, dev):
    r = torch.arange(shape[0], device=dev, dtype=torch.float32).view(-1, 1, *([1] * (len(shape) - 2)))
    c = torch.arange(shape[1], device=dev, dtype=torch.float32).view(1, -1, *([1] * (len(shape) - 2)))
    g = torch.Generator(device=dev)
    g.manual_seed(100 + s)
    x = (r + c) * (200.0 / (shape[0] + shape[1])) + 20.0 + s
    x = x + torch.randint(-2, 3, shape, device=dev, generator=g, dtype=torch.int32).to(torch.float32)
    return x.clamp_(0, 255).to(torch.uint8)


def psnr(a, b):
    d = a.astype(np.float32) - b.astype(np.float32)
    mse = float(np.mean(d * d, dtype=np.float64))
    return float("inf") if mse == 0.0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def psnr_report(n, dev):
    """--psnr: a standard decoder (Pillow) inverts the file with the exact DCT, the library with the HpApprDCT
    matrix it coded with: how far apart the two reconstructions of the same blocks are."""
    import io
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    for layout in ("grey", "420"):
        for kind, make in (("noise", noise), ("smooth", smooth)):
            if layout == "grey":
                x = make(0, (n, n), dev)
                ours = hpdct.inverse_blocks(hpdct.forward_blocks(x), out_dtype=torch.uint8)
            else:
                x = make(0, (n, n, 3), dev)
                y, cb, cr = hpdct.forward_rgb_frame(x, subsampling="420")
                ours = hpdct.inverse_rgb_frame(y, cb, cr, height=n, width=n, subsampling="420")
            data = hpdct.jpeg_encode(x, subsampling="420")
            theirs = np.asarray(Image.open(io.BytesIO(data)))
            src, ours = x.cpu().numpy(), ours.cpu().numpy()
            print(f"{n} x {n} {layout}, {kind}: file {len(data)} bytes; PSNR Pillow's pixels against the library's "
                  f"inverse {psnr(theirs, ours):.2f} dB; against the frame: Pillow {psnr(theirs, src):.2f} dB, "
                  f"the library's inverse {psnr(ours, src):.2f} dB", flush=True)


def main():
    flags = ("--quick", "--psnr")
    args = [a for a in sys.argv[1:] if a not in flags]
    quick = "--quick" in sys.argv[1:]
    n = int(args[0]) if args else 8192
    dev = torch.device("cuda", 0)
    if "--psnr" in sys.argv[1:]:
        return psnr_report(n, dev)
    stream = torch.cuda.current_stream()

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

    if not quick:       # clocks up: ~2 s of back-to-back launches
        warm_in = torch.empty((n, n), dtype=torch.uint8, device=dev)
        warm_out = torch.empty((n // 8, n // 8, 64), dtype=torch.int16, device=dev)
        warm = hpdct.bind_blocks("fwd", warm_in, warm_out, stream=stream)
        for _ in range(30000):
            warm()
        torch.cuda.synchronize()
        del warm, warm_in, warm_out

    px = n * n
    for layout in ("grey", "420"):
        for kind, make in (("noise", noise), ("smooth", smooth)):
            if layout == "grey":
                frames = [make(s, (n, n), dev) for s in range(SETS)]
                blocks = [(hpdct.forward_blocks(f), None, None) for f in frames]
                ri, sub, nblk = n // 8, "444", px // 64
            else:
                frames = [make(s, (n, n, 3), dev) for s in range(SETS)]
                blocks = [hpdct.forward_rgb_frame(f, subsampling="420") for f in frames]
                ri, sub, nblk = n // 16, "420", px // 64 * 3 // 2
            intervals = n // (8 if layout == "grey" else 16)
            torch.cuda.synchronize()
            scan0, info0, _ = hpdct.encode_scan(*blocks[0], height=n, width=n, subsampling=sub, restart_interval=ri)
            nbytes = info0["bytes"]
            assert not info0["truncated"] and not info0["out_of_range"], info0
            cap = nbytes + nbytes // 8
            outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
            infos = [torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2)]
            offs = [torch.empty(intervals + 1, dtype=torch.int64, device=dev) for _ in range(2)]
            ws = [torch.empty(16 * intervals, dtype=torch.uint8, device=dev) for _ in range(2)]
            enc = [hpdct.bind_scan(*blocks[s], outs[s % 2], infos[s % 2], offs[s % 2], ws[s % 2], height=n, width=n,
                                   subsampling=sub, restart_interval=ri, stream=stream) for s in range(SETS)]
            print(f"\n{n} x {n} {layout}, {kind}: {nblk} blocks, {intervals} intervals of one MCU row, "
                  f"scan {nbytes} bytes = {nbytes / px:.4f} B/px (blocks: {2 * nblk * 64 / px:.1f} B/px)", flush=True)
            if quick:
                for c in enc:
                    c()
                torch.cuda.synchronize()
                del frames, blocks, outs, enc
                torch.cuda.empty_cache()
                continue
            src32 = [torch.empty(px, dtype=torch.float32, device=dev) for _ in range(4)]
            dst8 = [torch.empty(px, dtype=torch.uint8, device=dev) for _ in range(2)]
            cases = [("(a) encode_scan, whole call", enc),
                     ("(b) copy ceiling 4 B in, 1 B out",
                      [hpdct.bind_copy_ceiling(src32[s % 4], dst8[s % 2], stream=stream) for s in range(SETS)])]
            reps = 64
            first = [region(calls, reps) for _, calls in cases]
            second = [region(calls, reps) for _, calls in reversed(cases)][::-1]
            print("| case | pass 1 us | pass 2 us | spread us |")
            print("|---|---|---|---|")
            for (name, _), t1, t2 in zip(cases, first, second):
                print(f"| {name} | {t1:.1f} | {t2:.1f} | {abs(t1 - t2):.1f} |", flush=True)
            t_enc, t_copy = min(first[0], second[0]), min(first[1], second[1])
            print(f"encode_scan = {t_enc / t_copy:.1f} x its copy ceiling; {2 * nblk * 128 / t_enc / 1e6:.3f} TB/s of "
                  f"block reads")
            del src32, dst8, cases
            if layout == "grey":
                # end to end: what leaves the device, with pinned host memory
                host_blocks = torch.empty((n // 8, n // 8, 64), dtype=torch.int16).pin_memory()
                host_scan = torch.empty(cap, dtype=torch.uint8).pin_memory()
                host_info = torch.empty(2, dtype=torch.int64).pin_memory()
                blk_o = [torch.empty((n // 8, n // 8, 64), dtype=torch.int16, device=dev) for _ in range(2)]

                def blocks_out(s):
                    hpdct.forward_blocks(frames[s % SETS], out=blk_o[s % 2])
                    host_blocks.copy_(blk_o[s % 2], non_blocking=True)
                    torch.cuda.synchronize()

                def scan_out(s):
                    hpdct.forward_blocks(frames[s % SETS], out=blk_o[s % 2])
                    hpdct.bind_scan(blk_o[s % 2], None, None, outs[s % 2], infos[s % 2], offs[s % 2], ws[s % 2],
                                    height=n, width=n, restart_interval=ri, stream=stream)()
                    host_info.copy_(infos[s % 2], non_blocking=True)
                    torch.cuda.synchronize()
                    k = int(host_info[0])
                    host_scan[:k].copy_(outs[s % 2][:k], non_blocking=True)
                    torch.cuda.synchronize()

                for name, fn in (("forward_blocks + D2H of the blocks", blocks_out),
                                 ("forward_blocks + encode_scan + D2H of the scan", scan_out)):
                    for s in range(3):
                        fn(s)
                    times = []
                    for s in range(20):
                        t0 = time.perf_counter()
                        fn(s)
                        times.append((time.perf_counter() - t0) * 1e6)
                    print(f"(c) {name}: median {float(np.median(times)):.0f} us, min {min(times):.0f}, "
                          f"max {max(times):.0f} (20 frames, host clock)", flush=True)
                del host_blocks, host_scan, blk_o
            del frames, blocks, outs, enc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
