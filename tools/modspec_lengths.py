"""Times the three routes of the float64 modulation-spectrum entries at DFT lengths that are no power of two (a measuring tool,
not a test): per n and per mode (spectrum with phase, inverse, smoothing, backward) on a 256 x min(n, 1000) x 60 float64 batch,

    chirp_ms    the chirp-z route (csrc/modspec_chirp.hip; table kernels included: they are part of every call),
    direct_ms   the direct transform of the same n (mlpg_hip_modspec_set_direct(1): the code every such n ran before chirp-z),
    fft_ms      the in-LDS FFT route at n = M = 2^ceil(log2(2n - 1)) with the same T -- the transform length chirp-z runs twice,

one JSON line each.  Device events around `--reps` calls; the three routes alternate within each of `--rounds` rounds and the
median round is reported, so that a drift of the clocks hits all three alike.  Needs a GPU; there is no fallback.

    python tools/modspec_lengths.py [--lengths 100,1000,1025,2000,2047] [--reps 5] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ("spectrum", "inverse", "smoothing", "backward")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="100,1000,1025,2000,2047")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from nnmnkwii_amd import _hip
    if not torch.cuda.is_available():
        raise SystemExit("modspec_lengths.py measures on the GPU and found none")
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for n in [int(v) for v in args.lengths.split(",")]:
        if L.mlpg_hip_modspec_route(n) != 2:
            raise SystemExit("n = %d is not on the chirp-z route" % n)
        M = 1
        while M < 2 * n - 1:
            M <<= 1
        B, T, D = args.batch, min(n, args.frames), args.dim
        x = 0.1 * torch.cumsum(torch.randn(B, T, D, dtype=torch.float64, device=dev, generator=gen), dim=1) + \
            torch.rand(B, T, D, dtype=torch.float64, device=dev, generator=gen)

        def problem(length):
            ms, ph = _hip.modspec(x, length, want_phase=True)
            g = torch.rand(B, length // 2 + 1, D, dtype=torch.float64, device=dev, generator=gen)
            out_inv = torch.empty(B, length, D, dtype=torch.float64, device=dev)

            def inverse():  # the C entry at the length itself (the Python wrapper derives an even n from the bin count)
                rc = L.mlpg_hip_inv_modspec(0, _hip._stream(dev), _hip._p(ms), _hip._p(ph), B, length, D, 0, _hip._p(out_inv))
                assert rc == 0, L.mlpg_hip_last_error()
            return {"spectrum": lambda: _hip.modspec(x, length, want_phase=True), "inverse": inverse,
                    "smoothing": lambda: _hip.modspec_smoothing(x, length, length // 8, log_domain=True),
                    "backward": lambda: _hip.modspec_backward(x, g, length)}

        at_n, at_M = problem(n), problem(M)
        for mode in MODES:
            def direct():
                L.mlpg_hip_modspec_set_direct(1)
                try:
                    at_n[mode]()
                finally:
                    L.mlpg_hip_modspec_set_direct(0)
            routes = {"chirp_ms": at_n[mode], "direct_ms": direct, "fft_ms": at_M[mode]}
            c0 = L.mlpg_hip_launch_count(20)
            for fn in routes.values():                       # warm-up: code objects, scratch, the allocator's blocks
                fn()
                fn()
            assert L.mlpg_hip_launch_count(20) == c0 + 2, "the chirp-z route did not serve n = %d" % n
            torch.cuda.synchronize()
            rounds = {k: [] for k in routes}
            for _ in range(args.rounds):
                for k, fn in routes.items():
                    rounds[k].append(timed(fn, args.reps))
            rec = {"n": n, "M": M, "mode": mode, "shape": [B, T, D], "dtype": "float64", "reps": args.reps, "rounds": args.rounds}
            for k, v in rounds.items():
                rec[k] = round(statistics.median(v), 4)
                rec[k.replace("_ms", "_min_ms")] = round(min(v), 4)
                rec[k.replace("_ms", "_max_ms")] = round(max(v), 4)
            rec["direct_over_chirp"] = round(rec["direct_ms"] / rec["chirp_ms"], 2)
            rec["chirp_over_fft"] = round(rec["chirp_ms"] / rec["fft_ms"], 2)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
