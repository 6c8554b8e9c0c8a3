"""The exact DCT on the frame calls (transform="dct", HPDCT_FRAME_DCT) against the
same calls without it, at 8192^2 in one process, in the manner of
tools/grey_frame_probe.py and tools/rgb_probe.py: back-to-back launches over
rotating input sets (>= 1 GiB of pixels, or of blocks for the inverse, well
beyond the 256 MiB Infinity Cache), HIP events on the launch stream, a clock
lead-in first, every case twice (the second pass in reverse order; the two
passes' difference is the run's own spread).

  grey    forward_grey_frame / inverse_grey_frame, dense 8192^2, and 8185 x 8190
          with a pitch of 8192 (the frame's edge tiles on the byte path)
  colour  forward_rgb_frame / inverse_rgb_frame, dense 8192^2, 4:2:0 and 4:4:4
  each    without the flag ("hpappr") and with it ("dct"), under the default
          tables (the per-position quotient forms without the flag, the 3-op
          quotient with it); the grey forward also under the quality-75 table,
          where both run the 3-op quotient
  copy    the copy ceiling of the same bytes per pixel (hpdct_copy_ceiling):
          grey 1 B in + 1 + 1 B out (the inverse moves the same 3 B/px the other
          way), colour 3 in + 3 out (4:2:0 both ways), 3 in + 3 + 3 out (4:4:4
          forward), 6 in (as fp32 elements) + 1.5 + 1.5 out (4:4:4 inverse)
Reported per case: the time, dct / hpappr from the same run, and case / copy.

usage: python tools/dct_probe.py [--log PATH]   (default profiles/r15/dct_probe.log)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-dct-idct_amd"))

N = 8192
TRANSFORMS = ("hpappr", "dct")


def main():
    import torch
    import hpdct

    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r15", "dct_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    u8, i16 = torch.uint8, torch.int16
    q75 = np.maximum(np.floor((hpdct.default_quant_table() * 50 + 50) / 100), 1).astype(np.float32)

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
        return [torch.empty((h // 8, w // 8, 64), dtype=i16, device=dev) for _ in range(n)]

    # clocks up: ~1 s of back-to-back launches
    warm_in = torch.empty((N, N), dtype=u8, device=dev)
    warm = hpdct.bind_blocks("fwd", warm_in, blocks(N, N)[0], stream=stream)
    for _ in range(30000):
        warm()
    torch.cuda.synchronize()
    del warm, warm_in

    say(f"{hpdct.version()}  {hpdct.build_info()}")
    say(f"{torch.cuda.get_device_name(0)}")

    def report(title, cases, pairs, ceilings):
        """cases: (name, calls, reps); pairs: {dct case: hpappr case}; ceilings: {case: its copy case}."""
        region(cases[0][1], 2000)               # the set-up let the clocks drop
        first = [region(calls, r) for _, calls, r in cases]
        second = [region(calls, r) for _, calls, r in reversed(cases)][::-1]
        best = [min(a, b) for a, b in zip(first, second)]
        say()
        say(title)
        say("| case | input sets | pass 1 us | pass 2 us | spread us | dct / hpappr | case / copy |")
        say("|---|---|---|---|---|---|---|")
        for i, ((name, calls, _), t1, t2) in enumerate(zip(cases, first, second)):
            rel = f"{best[i] / best[pairs[i]]:.3f}" if i in pairs else ""
            cop = f"{best[i] / best[ceilings[i]]:.2f}" if i in ceilings else ""
            say(f"| {name} | {len(calls)} | {t1:.2f} | {t2:.2f} | {abs(t1 - t2):.2f} | {rel} | {cop} |")

    # ---- grey ---------------------------------------------------------------
    sets = 16                                   # x 64 MiB: 1 GiB of pixels
    reps = 96
    pix = [torch.empty(N * N, dtype=u8, device=dev) for _ in range(sets)]
    for s, t in enumerate(pix):
        hpdct.fill_hash_u8(t, seed=7 + s)
    out = [torch.empty(N * N, dtype=u8, device=dev) for _ in range(4)]
    fo = blocks(N, N, 2)
    nb = 8                                      # x 128 MiB: 1 GiB of blocks
    cases, pairs, ceilings = [], {}, {}
    geometries = [("8192^2 dense", N, N, N), ("8185x8190 pitch 8192", 8185, 8190, N)]
    grey_keep = []
    for gname, h, w, pitch in geometries:
        ins = [t.as_strided((h, w), (pitch, 1), 0) for t in pix]
        outs = [t.as_strided((h, w), (pitch, 1), 0) for t in out[:2]]
        for table, q in (("default table", None), ("quality-75 table", q75)):
            if q is not None and h != N:
                continue
            for tr in TRANSFORMS:
                b = [hpdct.forward_grey_frame(ins[s], q=q, transform=tr) for s in range(nb)]
                torch.cuda.synchronize()
                grey_keep.append(b)
                fwd = [hpdct.bind_grey_frame("fwd", ins[s], fo[s % 2], q=q, stream=stream, transform=tr)
                       for s in range(sets)]
                cases.append((f"grey forward {gname}, {table}, {tr}", fwd, reps))
                if tr == "dct":
                    pairs[len(cases) - 1] = len(cases) - (3 if q is None else 2)
                if q is None:
                    inv = [hpdct.bind_grey_frame("inv", outs[s % 2], b[s], stream=stream, transform=tr)
                           for s in range(nb)]
                    cases.append((f"grey inverse {gname}, {table}, {tr}", inv, reps))
                    if tr == "dct":
                        pairs[len(cases) - 1] = len(cases) - 3
    cases.append(("copy 1 B in, 1 + 1 B out",
                  [hpdct.bind_copy_ceiling(pix[s], out[s % 2], out[2 + s % 2], stream=stream) for s in range(sets)],
                  reps))
    ceilings = {i: len(cases) - 1 for i in range(len(cases) - 1)}
    report(f"grey frames, {sets} input sets of pixels, {nb} of blocks, {reps} launches per region", cases, pairs,
           ceilings)
    del cases, grey_keep, pix, out, fo
    torch.cuda.empty_cache()

    # ---- colour -------------------------------------------------------------
    px = N * N
    sets = max(4, -(-(1 << 30) // (3 * px)))
    reps = max(96, 2 * sets)
    rgb = [torch.empty((N, N, 3), dtype=u8, device=dev) for _ in range(sets)]
    for s, t in enumerate(rgb):
        hpdct.fill_hash_u8(t, seed=7 + s)
    rgb_o = [torch.empty((N, N, 3), dtype=u8, device=dev) for _ in range(2)]
    y_o, cb4_o, cr4_o = blocks(N, N, 2), blocks(N, N, 2), blocks(N, N, 2)
    cb2_o, cr2_o = blocks(N // 2, N // 2, 2), blocks(N // 2, N // 2, 2)
    cases, pairs, ceilings, keep = [], {}, {}, []
    kinds = []
    for sub in ("420", "444"):
        cb_o, cr_o = (cb2_o, cr2_o) if sub == "420" else (cb4_o, cr4_o)
        for tr in TRANSFORMS:
            b = [hpdct.forward_rgb_frame(t, subsampling=sub, transform=tr) for t in rgb]
            torch.cuda.synchronize()
            keep.append(b)
            fwd = [hpdct.bind_rgb_frame("fwd", rgb[s], y_o[s % 2], cb_o[s % 2], cr_o[s % 2], subsampling=sub,
                                        stream=stream, transform=tr) for s in range(sets)]
            inv = [hpdct.bind_rgb_frame("inv", rgb_o[s % 2], *b[s], subsampling=sub, stream=stream, transform=tr)
                   for s in range(sets)]
            cases.append((f"rgb forward {sub}, {tr}", fwd, reps))
            cases.append((f"rgb inverse {sub}, {tr}", inv, reps))
            kinds += [("fwd", sub), ("inv", sub)]
            if tr == "dct":
                pairs[len(cases) - 2] = len(cases) - 4
                pairs[len(cases) - 1] = len(cases) - 3
    flat = [t.view(-1) for t in rgb]
    o8 = [torch.empty(3 * px, dtype=u8, device=dev) for _ in range(4)]
    f32_in = [torch.empty(3 * px // 2, dtype=torch.float32, device=dev) for _ in range(sets)]
    h8 = [torch.empty(3 * px // 2, dtype=u8, device=dev) for _ in range(4)]
    first_copy = len(cases)
    cases += [("copy 3 B in, 3 B out",
               [hpdct.bind_copy_ceiling(flat[s], o8[s % 2], stream=stream) for s in range(sets)], reps),
              ("copy 3 B in, 3 + 3 B out",
               [hpdct.bind_copy_ceiling(flat[s], o8[s % 2], o8[2 + s % 2], stream=stream) for s in range(sets)], reps),
              ("copy 6 B in, 1.5 + 1.5 B out",
               [hpdct.bind_copy_ceiling(f32_in[s], h8[s % 2], h8[2 + s % 2], stream=stream) for s in range(sets)],
               reps)]
    copy_of = {("fwd", "420"): 0, ("inv", "420"): 0, ("fwd", "444"): 1, ("inv", "444"): 2}
    ceilings = {i: first_copy + copy_of[k] for i, k in enumerate(kinds)}
    report(f"colour frames, {sets} input sets, {reps} launches per region", cases, pairs, ceilings)
    log.close()


if __name__ == "__main__":
    main()
