"""JPEG-style int16 blocks against what they replace, at 8192^2 and 4096^2 in one
run: back-to-back launches over 16 or more rotating input sets (>= 1 GiB of
inputs), HIP events on the launch stream, a clock warm-up first, every case
twice (the second pass in reverse order; the two passes' difference is the
run's own spread).

  (a)  forward u8 -> fp32 plane
  (b)  (a) + the torch permute-and-cast a caller needs today to get int16
       zig-zag blocks: one copy_ that regroups and casts (4 B/px read, 2 written)
       and one int16 gather into zig-zag order; (b nat) stops after the copy_
  (c)  forward u8 -> int8 plane
  (d)  forward_blocks, zig-zag and natural
  (e)  inverse_blocks -> u8 and -> fp32, beside inverse int8 -> u8 and -> fp32
  (f)  the copy ceiling with 1 B in and 1 B + 1 B out per pixel: the 3 B/px of
       (d) (the ceiling tool has no 2-byte type)

usage: python tools/blocks_probe.py [sizes...]      (default 8192 4096)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [8192, 4096]
    import torch
    import hpdct

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    zz = torch.from_numpy(hpdct.zigzag_order().astype("int64")).to(dev)

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

    # clocks up before the first size: ~2 s of back-to-back launches
    n0 = sizes[0]
    warm_in = torch.empty((n0, n0), dtype=torch.uint8, device=dev)
    warm_out = torch.empty((n0 // 8, n0 // 8, 64), dtype=torch.int16, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, warm_out, stream=stream)
    for _ in range(30000):
        warm()
    torch.cuda.synchronize()
    del warm, warm_in, warm_out

    for n in sizes:
        px = n * n
        sets = max(16, -(-(1 << 30) // px))
        reps = max(320, 2 * sets)
        img = [torch.empty((n, n), dtype=torch.uint8, device=dev) for _ in range(sets)]
        for s, t in enumerate(img):
            hpdct.fill_hash_u8(t, seed=7 + s)
        f32 = [torch.empty((n, n), dtype=torch.float32, device=dev) for _ in range(2)]
        i8 = [hpdct.forward(t, out_dtype=torch.int8) for t in img]
        blk = [hpdct.forward_blocks(t) for t in img]
        blk_o = [torch.empty((n // 8, n // 8, 64), dtype=torch.int16, device=dev) for _ in range(2)]
        nat_o = [torch.empty((n // 8, n // 8, 64), dtype=torch.int16, device=dev) for _ in range(2)]
        i8_o = [torch.empty((n, n), dtype=torch.int8, device=dev) for _ in range(2)]
        u8_o = [torch.empty((n, n), dtype=torch.uint8, device=dev) for _ in range(2)]
        u8_o2 = [torch.empty((n, n), dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()

        def fwd_plane(s):
            return hpdct.bind("fwd", img[s], f32[s % 2], stream=stream)

        def today(s, zigzag):
            f = fwd_plane(s)
            src = f32[s % 2].view(n // 8, 8, n // 8, 8).permute(0, 2, 1, 3)
            nat = nat_o[s % 2]
            dst = nat.view(n // 8, n // 8, 8, 8)
            out = blk_o[s % 2]

            def call():
                f()
                dst.copy_(src)                       # regroup + cast: 4 B/px read, 2 written
                if zigzag:
                    torch.index_select(nat, 2, zz, out=out)
            return call

        cases = [
            ("(a) forward u8->fp32", [fwd_plane(s) for s in range(sets)]),
            ("(b) (a) + torch permute/cast/zig-zag", [today(s, True) for s in range(sets)]),
            ("(b nat) (a) + torch permute/cast", [today(s, False) for s in range(sets)]),
            ("(c) forward u8->int8", [hpdct.bind("fwd", img[s], i8_o[s % 2], stream=stream) for s in range(sets)]),
            ("(d) forward_blocks zig-zag",
             [hpdct.bind_blocks("fwd", img[s], blk_o[s % 2], stream=stream) for s in range(sets)]),
            ("(d) forward_blocks natural",
             [hpdct.bind_blocks("fwd", img[s], blk_o[s % 2], order="natural", stream=stream) for s in range(sets)]),
            ("(e) inverse_blocks ->u8",
             [hpdct.bind_blocks("inv", blk[s], u8_o[s % 2], stream=stream) for s in range(sets)]),
            ("(e) inverse int8->u8", [hpdct.bind("inv", i8[s], u8_o[s % 2], stream=stream) for s in range(sets)]),
            ("(e) inverse_blocks ->fp32",
             [hpdct.bind_blocks("inv", blk[s], f32[s % 2], stream=stream) for s in range(sets)]),
            ("(e) inverse int8->fp32", [hpdct.bind("inv", i8[s], f32[s % 2], stream=stream) for s in range(sets)]),
            ("(f) copy ceiling 1 B in, 1+1 B out",
             [hpdct.bind_copy_ceiling(img[s], u8_o[s % 2], u8_o2[s % 2], stream=stream) for s in range(sets)]),
        ]
        first = [region(calls, reps) for _, calls in cases]
        second = [region(calls, reps) for _, calls in reversed(cases)][::-1]
        ceil = min(first[-1], second[-1])
        print(f"\n{n} x {n}, {sets} input sets, {reps} launches per region")
        print("| case | pass 1 us | pass 2 us | spread us | (f) / case |")
        print("|---|---|---|---|---|")
        for (name, _), t1, t2 in zip(cases, first, second):
            print(f"| {name} | {t1:.2f} | {t2:.2f} | {abs(t1 - t2):.2f} | {ceil / min(t1, t2):.2f} |", flush=True)
        a, b, d = (min(first[i], second[i]) for i in (0, 1, 4))
        worst_d, best_b = max(first[4], second[4]), min(first[1], second[1])
        print(f"(d) zig-zag against (b): {worst_d:.2f} us at worst against {best_b:.2f} us at best "
              f"({'faster beyond the spread' if worst_d < best_b else 'NOT faster beyond the spread'}); "
              f"(d) / (a) = {d / a:.2f}")
        del cases, img, f32, i8, blk, blk_o, nat_o, i8_o, u8_o, u8_o2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
