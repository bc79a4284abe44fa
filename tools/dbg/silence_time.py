"""Times of silence removal on the device: one kept-frame expansion of a 64 x ~1000-frame x 425-column float32
batch against ``frame_features_batch`` followed by a boolean-index compaction and re-padding in torch, and the row gather of a
187-column acoustic batch against the same compaction.  Medians of 7 windows of back-to-back calls between two events, the two
sides alternating; the outputs of both sides are compared first.  Prints one JSON line (and writes it to argv[1] if given).

    python tools/dbg/silence_time.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nnmnkwii_amd import preprocessing as PP  # noqa: E402
from nnmnkwii_amd.frontend import merlin as fe  # noqa: E402

B, NMAX, S, DL, DY, WINDOWS, CALLS = 64, 60, 5, 416, 187, 7, 1000


def inputs():
    rng = np.random.RandomState(18)
    dur = rng.randint(1, 6, size=(B, NMAX, S)).astype(np.int64)              # 3 frames per state on average: 900 per utterance
    dur[:, 0] = rng.randint(4, 12, size=(B, S))                              # long silences at both ends
    dur[:, -1] = rng.randint(4, 12, size=(B, S))
    sil = rng.rand(B, NMAX) < 0.08                                           # and short pauses inside
    sil[:, 0] = sil[:, -1] = True
    P = (rng.rand(B, NMAX, DL) < 0.1).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (P, dur, sil))


def composed_mask(dur, sil, T):
    """keep (B, T) from the flags: each frame's phone by searchsorted on the running frame counts."""
    ends = dur.sum(2).cumsum(1)                                               # (B, Nmax)
    t = torch.arange(T, device=dur.device).expand(B, T).contiguous()
    phone = torch.searchsorted(ends, t, right=True).clamp_(max=NMAX - 1)
    keep = ~sil.gather(1, phone) & (t < ends[:, -1:])
    return keep


def compact(X, keep, Tcap):
    """Boolean-index compaction and re-padding: the kept rows of every utterance to the front of a zeroed (B, Tcap, D)."""
    pos = keep.cumsum(1) - 1
    rows = X[keep]                                                            # (the synchronisation: the shape is data)
    b = torch.arange(B, device=X.device).view(B, 1).expand_as(keep)[keep]
    out = torch.zeros((B, Tcap, X.shape[2]), dtype=X.dtype, device=X.device)
    out[b, pos[keep]] = rows
    return out, keep.sum(1).to(torch.int32)


def windows(fns):
    """Median and range of the per-call time of each function, in ms: WINDOWS windows of CALLS calls each, alternating."""
    for f in fns:
        for _ in range(10):
            f()
    times = [[] for _ in fns]
    for _ in range(WINDOWS):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / CALLS)
    return [dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)) for t in times]


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    P, dur, sil = inputs()
    T = int(dur.sum((1, 2)).max().item())
    counts = torch.where(sil, torch.zeros_like(dur.sum(2)), dur.sum(2)).sum(1)
    K = int(counts.max().item())
    W = DL + 9
    out = torch.empty((B, K, W), dtype=torch.float32, device="cuda")
    full = torch.empty((B, T, W), dtype=torch.float32, device="cuda")

    def ours():
        return fe.kept_frame_features_batch(P, dur, sil, None, "full", out=out, strict=False)

    def theirs():
        X, _ = fe.frame_features_batch(P, dur, None, "full", out=full, strict=False)
        return compact(X, composed_mask(dur, sil, T), K)

    def expand_alone():
        return fe.frame_features_batch(P, dur, None, "full", out=full, strict=False)

    a, la = ours()
    b, lb = theirs()
    assert torch.equal(a, b) and torch.equal(la, lb), "the two sides differ"
    Y = torch.randn((B, T, DY), dtype=torch.float32, device="cuda")
    ylen = dur.sum((1, 2)).to(torch.int32)
    yout = torch.empty((B, K, DY), dtype=torch.float32, device="cuda")

    def gather_ours():
        return PP.remove_silence_frames_batch(Y, dur, sil, ylen, out=yout, strict=False)

    def gather_theirs():
        return compact(Y, composed_mask(dur, sil, T), K)

    c, lc = gather_ours()
    e, le = gather_theirs()
    assert torch.equal(c, e) and torch.equal(lc, le), "the two gathers differ"
    r = windows([ours, theirs, expand_alone, gather_ours, gather_theirs])
    res = dict(shape=dict(B=B, Nmax=NMAX, S=S, Dl=DL, W=W, Dy=DY, Tmax=T, Kmax=K, frames=int(dur.sum().item()), kept=int(counts.sum().item())),
               protocol="medians of %d windows of %d back-to-back calls between two events, sides alternating; outputs compared first" % (WINDOWS, CALLS),
               kept_frame_features_batch=r[0], frame_features_batch_then_torch_compaction=r[1], frame_features_batch_alone=r[2],
               remove_silence_frames_batch=r[3], torch_compaction_alone=r[4],
               bytes_written_expand=B * K * W * 4, bytes_moved_gather=int(counts.sum().item()) * DY * 4 + B * K * DY * 4,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
