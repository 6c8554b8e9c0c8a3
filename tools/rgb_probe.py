"""Colour frames against what they replace, at 8192^2 and 4096^2 in one run:
back-to-back launches over rotating input sets (>= 1 GiB of RGB, well beyond
the 256 MiB Infinity Cache), HIP events on the launch stream, a clock warm-up
first, every case twice (the second pass in reverse order; the two passes'
difference is the run's own spread).

  (a)   the caller's route before forward_rgb_blocks: the conversion (and the
        2x2 average) in torch integer arithmetic, then set_quant_table(luma),
        forward_blocks(Y), set_quant_table(chroma), forward_blocks(Cb),
        forward_blocks(Cr)
  (a')  the three forward_blocks of (a) alone, on planes made beforehand: what
        (a) costs with a conversion that is free
  (b)   forward_rgb_blocks, 4:2:0 and 4:4:4; 4:2:0 also under the two other
        quotient forms (the same bytes, more arithmetic: a VALU-bound kernel
        slows down with them, a memory-bound one does not)
  (c)   inverse_rgb_blocks, 4:2:0 and 4:4:4
  (d)   the copy ceiling of the same bytes per pixel (hpdct_copy_ceiling):
        3 B in + 3 B out (4:2:0 both ways), 3 in + 3 + 3 out (4:4:4 forward),
        6 in (as fp32 elements) + 1.5 + 1.5 out (4:4:4 inverse)

usage: python tools/rgb_probe.py [sizes...]      (default 8192 4096)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [8192, 4096]
    import torch
    import hpdct

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    q_chroma = hpdct.default_chroma_quant_table()
    # the other quotient forms: libjpeg's quality-75 scaling (integers) and a fractional pair
    q75 = tuple(np.maximum(np.floor((q * 50 + 50) / 100), 1) for q in (hpdct.default_quant_table(), q_chroma))
    x37 = tuple(q * np.float32(0.37) for q in (hpdct.default_quant_table(), q_chroma))

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

    def blocks(h, w, n=1):
        return [torch.empty((h // 8, w // 8, 64), dtype=torch.int16, device=dev) for _ in range(n)]

    # clocks up before the first size: ~2 s of back-to-back launches
    n0 = sizes[0]
    warm_in = torch.empty((n0, n0), dtype=torch.uint8, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, blocks(n0, n0)[0], stream=stream)
    for _ in range(30000):
        warm()
    torch.cuda.synchronize()
    del warm, warm_in

    for n in sizes:
        px = n * n
        sets = max(4, -(-(1 << 30) // (3 * px)))
        reps = max(96, 2 * sets)
        rgb = [torch.empty((n, n, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
        for s, t in enumerate(rgb):
            hpdct.fill_hash_u8(t, seed=7 + s)
        rgb_o = [torch.empty((n, n, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        y_o, cb4_o, cr4_o = blocks(n, n, 2), blocks(n, n, 2), blocks(n, n, 2)
        cb2_o, cr2_o = blocks(n // 2, n // 2, 2), blocks(n // 2, n // 2, 2)
        in420 = [hpdct.forward_rgb_blocks(t, subsampling="420") for t in rgb]
        in444 = [hpdct.forward_rgb_blocks(t, subsampling="444") for t in rgb]
        torch.cuda.synchronize()

        def convert(x, sub):
            r, g, b = x.to(torch.int32).unbind(-1)
            y = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).to(torch.uint8)
            cb = (-11059 * r - 21709 * g + 32768 * b + ((128 << 16) + 32767)) >> 16
            cr = (32768 * r - 27439 * g - 5329 * b + ((128 << 16) + 32767)) >> 16
            if sub == "420":
                cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
            return y, cb.to(torch.uint8).contiguous(), cr.to(torch.uint8).contiguous()

        def today(s, sub, planes=None):
            cb_o, cr_o = (cb2_o, cr2_o) if sub == "420" else (cb4_o, cr4_o)

            def call():
                y, cb, cr = planes if planes is not None else convert(rgb[s], sub)
                hpdct.set_quant_table(None)
                hpdct.forward_blocks(y, out=y_o[s % 2], stream=stream)
                hpdct.set_quant_table(q_chroma)
                hpdct.forward_blocks(cb, out=cb_o[s % 2], stream=stream)
                hpdct.forward_blocks(cr, out=cr_o[s % 2], stream=stream)
                hpdct.set_quant_table(None)
            return call

        # (a'): planes of two input sets per subsampling, made once
        planes = {sub: [convert(rgb[s], sub) for s in range(2)] for sub in ("420", "444")}
        torch.cuda.synchronize()

        def fwd(s, sub, tables=(None, None)):
            cb_o, cr_o = (cb2_o, cr2_o) if sub == "420" else (cb4_o, cr4_o)
            return hpdct.bind_rgb_blocks("fwd", rgb[s], y_o[s % 2], cb_o[s % 2], cr_o[s % 2], subsampling=sub,
                                         q_luma=tables[0], q_chroma=tables[1], stream=stream)

        def inv(s, sub):
            y, cb, cr = (in420 if sub == "420" else in444)[s]
            return hpdct.bind_rgb_blocks("inv", rgb_o[s % 2], y, cb, cr, subsampling=sub, stream=stream)

        flat = [t.view(-1) for t in rgb]
        o8 = [torch.empty(3 * px, dtype=torch.uint8, device=dev) for _ in range(4)]
        f32_in = [torch.empty(3 * px // 2, dtype=torch.float32, device=dev) for _ in range(sets)]
        h8 = [torch.empty(3 * px // 2, dtype=torch.uint8, device=dev) for _ in range(4)]
        few = max(8, sets)
        cases = [
            ("(a) torch conversion + 3 forward_blocks 4:2:0", [today(s, "420") for s in range(sets)], few),
            ("(a) torch conversion + 3 forward_blocks 4:4:4", [today(s, "444") for s in range(sets)], few),
            ("(a') 3 forward_blocks alone 4:2:0", [today(s, "420", planes["420"][s]) for s in range(2)], reps),
            ("(a') 3 forward_blocks alone 4:4:4", [today(s, "444", planes["444"][s]) for s in range(2)], reps),
            ("(b) forward_rgb_blocks 4:2:0", [fwd(s, "420") for s in range(sets)], reps),
            ("(b) forward_rgb_blocks 4:4:4", [fwd(s, "444") for s in range(sets)], reps),
            ("(b q75) 4:2:0, 3-op quotient for Y too", [fwd(s, "420", q75) for s in range(sets)], reps),
            ("(b x0.37) 4:2:0, IEEE division", [fwd(s, "420", x37) for s in range(sets)], reps),
            ("(c) inverse_rgb_blocks 4:2:0", [inv(s, "420") for s in range(sets)], reps),
            ("(c) inverse_rgb_blocks 4:4:4", [inv(s, "444") for s in range(sets)], reps),
            ("(d) copy 3 B in, 3 B out",
             [hpdct.bind_copy_ceiling(flat[s], o8[s % 2], stream=stream) for s in range(sets)], reps),
            ("(d) copy 3 B in, 3 + 3 B out",
             [hpdct.bind_copy_ceiling(flat[s], o8[s % 2], o8[2 + s % 2], stream=stream) for s in range(sets)], reps),
            ("(d) copy 6 B in, 1.5 + 1.5 B out",
             [hpdct.bind_copy_ceiling(f32_in[s], h8[s % 2], h8[2 + s % 2], stream=stream) for s in range(sets)], reps),
        ]
        first = [region(calls, r) for _, calls, r in cases]
        second = [region(calls, r) for _, calls, r in reversed(cases)][::-1]
        best = [min(a, b) for a, b in zip(first, second)]
        # the ceiling of each case: (a), (a') have none
        ceiling = {4: 10, 5: 11, 6: 10, 7: 10, 8: 10, 9: 12}
        print(f"\n{n} x {n}, {sets} input sets, {reps} launches per region ({few} for (a))")
        print("| case | pass 1 us | pass 2 us | spread us | (d) / case |")
        print("|---|---|---|---|---|")
        for i, ((name, _, _), t1, t2) in enumerate(zip(cases, first, second)):
            ratio = f"{best[ceiling[i]] / best[i]:.2f}" if i in ceiling else ""
            print(f"| {name} | {t1:.2f} | {t2:.2f} | {abs(t1 - t2):.2f} | {ratio} |", flush=True)
        for sub, ia, iap, ib in (("4:2:0", 0, 2, 4), ("4:4:4", 1, 3, 5)):
            print(f"{sub}: (a) / (b) = {best[ia] / best[ib]:.2f}, (a') / (b) = {best[iap] / best[ib]:.2f}")
        del cases, rgb, rgb_o, y_o, cb4_o, cr4_o, cb2_o, cr2_o, in420, in444, planes, flat, o8, f32_in, h8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
