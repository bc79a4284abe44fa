"""GPU tests (-m gpu): nnmk_wave_encode and nnmk_wave_decode on buffers at odd element offsets between guard bands
(tests/embed.py).  x, lengths, the table and y each start an odd number of elements into a byte buffer filled with one value, so
no pointer is aligned beyond its element and the 16-byte accesses must not be taken; after the call the inputs hold their bits,
every guard holds its fill byte, and the results equal tools/wave_model.py (bit for bit where no transcendental is involved).
The class dtypes here are uint8, int32 and int64: tests/embed.py has no int16 (tests/test_wave_gpu.py covers it)."""
import numpy as np
import pytest

import embed
import wave_cases as WC
from wave_cases import WM

pytestmark = pytest.mark.gpu

CASES = [c for c in WC.cases() if c["name"] in ("deemph-none-f32", "deemph-seg2048-f64", "deemph-auto-f64-f32", "table-uint8", "table-deemph-int32",
                                                "table-int64", "preemph-f32", "preemph-quantize-u8-wide", "preemph-quantize-i32", "preemph-quantize-i64",
                                                "mulaw-f32", "inplace-quantize-f32-i32")]


@pytest.mark.parametrize("offsets", [(1, 3, 5, 7), (3, 1, 1, 1)], ids=["1-3-5-7", "3-1-1-1"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_offset_buffers_between_guard_bands(case, offsets):
    import torch
    from nnmnkwii_amd import _wave_hip as WH
    L = WH.lib()
    dx, dy = (np.dtype(t) for t in case["dtypes"])
    in_place = case["mode"] == "inplace"
    X = case["X"].astype(dx)
    B, Lmax = X.shape
    ox, ol, ot, oy = offsets
    x = embed.embedded(X, ox)
    lengths = embed.embedded(case["lengths"], ol)
    table = embed.embedded(WM.inv_mulaw_table(case["mu"]), ot) if case["op"] == "decode" and case["stage"] == WM.QUANTIZE else None
    y = None if in_place else embed.Embedded(X.shape, dy, oy)
    assert x.ptr() % dx.itemsize == 0 and (dx.itemsize == 1 or x.ptr() % 16)
    want = WC.expected(case)
    n0 = L.nnmk_wave_launch_count()
    dev = torch.device("cuda", torch.cuda.current_device())
    yp = x.ptr() if in_place else y.ptr()
    if case["op"] == "encode":
        rc = L.nnmk_wave_encode(dev.index, None, WM.CODE[dx], x.ptr(), Lmax, embed.ptr(lengths), B, Lmax, case["coef"] is not None,
                                case["coef"] or 0.0, case["stage"], case["mu"], WM.CODE[dy], yp, Lmax)
    else:
        rc = L.nnmk_wave_decode(dev.index, None, WM.CODE[dx], x.ptr(), Lmax, embed.ptr(lengths), B, Lmax, case["stage"], case["mu"], embed.ptr(table),
                                case["coef"] is not None, case["coef"] or 0.0, min(case["segment"], 1 << 40), WM.CODE[dy], yp, Lmax)
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert L.nnmk_wave_launch_count() == n0 + 1
    if in_place:
        assert embed.failed(inputs=dict(lengths=lengths, table=table), outputs=dict(x=x)) == []
        got = x.host().view(dy)
    else:
        assert embed.failed(inputs=dict(x=x, lengths=lengths, table=table), outputs=dict(y=y)) == []
        got = y.host()
    assert WC.compare(case, got, want) == []
