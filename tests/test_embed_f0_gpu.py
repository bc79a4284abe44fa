"""GPU tests (-m gpu): nnmk_f0_interp on buffers at odd element offsets between guard bands (tests/embed.py).  x, lengths, y and
vuv each start an odd number of elements into a byte buffer filled with one value, so no pointer is aligned beyond its element;
after the call the inputs hold their bits, every guard holds its fill byte, and the results equal tools/f0_model.py bit for
bit."""
import numpy as np
import pytest

import embed
import f0_cases as FC
from f0_cases import F0

pytestmark = pytest.mark.gpu

DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
CASES = [c for c in FC.cases() if c["name"] in ("lengths-slinear", "lengths-linear", "structural-nearest-up-both", "structural-previous-both",
                                               "no-lengths", "clamped-lengths")]


@pytest.mark.parametrize("offsets", [(1, 3, 5, 7), (3, 1, 1, 1)], ids=["1-3-5-7", "3-1-1-1"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_offset_buffers_between_guard_bands(case, offsets):
    import torch
    from nnmnkwii_amd import _f0_hip as FH
    L = FH.lib()
    dx, dy, dv = (np.dtype(t) for t in case["dtypes"])
    in_place = case["mode"] == "inplace"
    X = case["X"].astype(dx)
    B, Tmax, C = X.shape
    ox, ol, oy, ov = offsets
    x = embed.embedded(X, ox)
    lengths = embed.embedded(case["lengths"], ol)
    y = None if in_place else embed.Embedded(X.shape, dy, oy)
    v = embed.Embedded(X.shape, dv, ov)
    assert x.ptr() % 16 and v.ptr() % 16 and x.ptr() % dx.itemsize == 0
    want_y, want_v = FC.expected(case)
    n0 = L.nnmk_f0_launch_count()
    dev = torch.device("cuda", torch.cuda.current_device())
    rc = L.nnmk_f0_interp(dev.index, None, DT_CODE[dx], x.ptr(), C, embed.ptr(lengths), B, Tmax, C, F0.kind_of(case["kind"]),
                          DT_CODE[dx if in_place else dy], x.ptr() if in_place else y.ptr(), C, DT_CODE[dv], v.ptr(), C)
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert L.nnmk_f0_launch_count() == n0 + 1
    if in_place:
        assert embed.failed(inputs=dict(lengths=lengths), outputs=dict(x=x, vuv=v)) == []
        assert FC.same_bits(x.host(), want_y)
    else:
        assert embed.failed(inputs=dict(x=x, lengths=lengths), outputs=dict(y=y, vuv=v)) == []
        assert FC.same_bits(y.host(), want_y)
    assert FC.same_bits(v.host(), want_v)
